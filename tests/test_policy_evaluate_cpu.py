"""CPU: the policy evaluator's surface (header, library, Python functions) and the numpy reference's
own checks: its forward equals the sampler reference's, its gradient matches finite differences, its
bad rows behave as include/cog.h states, and its float32 mode agrees with float64 within the
tolerance tests/test_gpu_policy_evaluate.py allows the kernels."""
import ctypes
import os
import re

import numpy as np

import policy_eval_ref as per
import policy_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gym-eldorado_amd", "city_of_gold", "libcog_hip.so")
TOL = 1e-5


def sampled(rng, n, seed=99):
    logits, masks = pr.random_logits(rng, n), pr.random_masks(rng, n)
    ref = pr.sample(logits, masks, pr.sampler_states(seed, n))
    return logits, masks, ref


def test_header_declares_the_policy_evaluator():
    src = open(os.path.join(ROOT, "include", "cog.h")).read()
    for name in ("cog_policy_evaluate", "cog_policy_evaluate_backward"):
        assert re.search(rf"COG_API\s+int\s+{name}\s*\(\s*const\s+cog_policy_eval_args\s*\*", src), name
    m = re.search(r"typedef struct cog_policy_eval_args \{(.*?)\} cog_policy_eval_args;", src, re.S)
    assert m
    for field in ("size_t n;", "const void *d_logits;", "int logits_dtype;", "size_t ld;", "const uint8_t *d_actions;",
                  "size_t action_stride;", "const void *d_masks;", "float *d_logp;", "float *d_entropy;",
                  "const float *d_grad_logp;", "const float *d_grad_entropy;", "void *d_grad_logits;", "int device;",
                  "void *stream;"):
        assert field in m.group(1), field
    assert re.search(r"#define\s+COG_ABI_VERSION\s+1\b", src)


def test_null_arguments_are_invalid():
    lib = ctypes.CDLL(LIB)
    lib.cog_last_error.restype = ctypes.c_char_p
    for name in ("cog_policy_evaluate", "cog_policy_evaluate_backward"):
        fn = getattr(lib, name)
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p]
        assert fn(None) == -1, name                                     # COG_ERR_INVALID
        assert b"NULL" in lib.cog_last_error()


def test_python_functions_exist(cg):
    for name in ("policy_evaluate", "mask_records"):
        assert callable(getattr(cg, name)), name
        assert name in cg.__all__ and name in cg.__doc__, name
    assert callable(cg._C.policy_evaluate_raw)


def test_reference_forward_equals_the_sampler_reference():
    rng = np.random.default_rng(31)
    logits, masks, ref = sampled(rng, 4000)
    ev = per.evaluate(logits, ref["actions"], masks)
    assert not ev["bad"].any()
    assert np.abs(ev["logp"] - ref["logp"]).max() <= 1e-12
    assert np.abs(ev["entropy"] - ref["entropy"]).max() <= 1e-12


def test_reference_gradient_matches_finite_differences():
    """Central differences in float64 of sum(g_lp logp + g_en entropy) on 30 rows x 92 columns."""
    rng = np.random.default_rng(37)
    n, h = 30, 1e-5
    logits, masks, ref = sampled(rng, n)
    logits = logits.astype(np.float64)
    g_lp, g_en = rng.normal(size=n), rng.normal(size=n)
    grad = per.evaluate(logits, ref["actions"], masks, g_lp, g_en)["grad"]

    def f(x):
        ev = per.evaluate(x, ref["actions"], masks)
        return g_lp * ev["logp"] + g_en * ev["entropy"]                 # (per row: rows are independent)
    fd = np.zeros_like(grad)
    for c in range(per.COLS):
        e = np.zeros(per.COLS)
        e[c] = h
        fd[:, c] = (f(logits + e) - f(logits - e)) / (2 * h)
    valid = masks[:, :per.COLS] != 0
    assert np.abs(fd[~valid]).max() == 0 and np.abs(grad[~valid]).max() == 0
    assert np.abs(grad - fd).max() <= 1e-7, np.abs(grad - fd).max()
    only_lp = per.evaluate(logits, ref["actions"], masks, g_lp, None)["grad"]
    only_en = per.evaluate(logits, ref["actions"], masks, None, g_en)["grad"]
    assert np.abs(only_lp + only_en - grad).max() <= 1e-14


def plant_bad_rows(logits, masks, actions):
    """Rows 3, 10, 17, 24 made bad in the four ways (head 0 non-empty there); returns them."""
    masks[[3, 10, 17, 24], :22] = 0
    masks[[3, 10, 17, 24], 2:9] = 1
    actions[[3, 10, 17, 24], 0] = 4
    logits[3, 6] = np.inf                                               # +inf on a valid entry
    logits[10, 2:9] = -np.inf                                           # nothing but -inf / NaN
    logits[10, 5] = np.nan
    masks[17, 4] = 0                                                    # the action's mask byte is 0
    actions[24, 0] = 200                                                # an action byte past the head
    return np.array([3, 10, 17, 24])


def test_reference_bad_rows():
    rng = np.random.default_rng(41)
    n = 40
    logits, masks, ref = sampled(rng, n)
    actions = ref["actions"].copy()
    clean = per.evaluate(logits, actions, masks, np.ones(n), np.ones(n))
    bad = plant_bad_rows(logits, masks, actions)
    g = np.ones(n)
    g[bad] = np.nan
    ev = per.evaluate(logits, actions, masks, g, g)
    assert np.array_equal(np.flatnonzero(ev["bad"]), bad)
    assert np.isnan(ev["logp"][bad]).all() and np.isnan(ev["entropy"][bad]).all()
    assert not ev["grad"][bad].any()
    good = np.setdiff1d(np.arange(n), bad)
    for k in ("logp", "entropy", "grad"):
        assert np.array_equal(ev[k][good], clean[k][good]), k
    # an empty head ignores its action byte; a valid -inf entry that is not alone is no bad row
    masks2, actions2, logits2 = masks.copy(), actions.copy(), logits.copy()
    masks2[0, 66:73] = 0
    actions2[0, 3] = 250
    masks2[1, 22:44] = 1
    logits2[1, 30] = -np.inf
    actions2[1, 1] = 3
    ev2 = per.evaluate(logits2, actions2, masks2, np.ones(n), np.ones(n))
    assert not ev2["bad"][[0, 1]].any() and np.isfinite(ev2["grad"][[0, 1]]).all()
    assert not ev2["grad"][0, 66:73].any() and ev2["grad"][1, 30] == 0


def test_float32_mode_pins_the_gpu_tolerance():
    """The same formulas in float32 over 20,000 rows: gradient within 1e-5 (|g_lp| + |g_en|) per row,
    logp and entropy within 1e-5 of float64."""
    rng = np.random.default_rng(43)
    n = 20000
    logits, masks, ref = sampled(rng, n)
    g_lp, g_en = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    e64 = per.evaluate(logits, ref["actions"], masks, g_lp, g_en)
    e32 = per.evaluate(logits, ref["actions"], masks, g_lp, g_en, dtype=np.float32)
    assert e32["grad"].dtype == np.float32 and e32["logp"].dtype == np.float32
    scale = (np.abs(g_lp) + np.abs(g_en)).astype(np.float64)
    err_g = (np.abs(e64["grad"] - e32["grad"]).max(1) / scale).max()
    err_lp = np.abs(e64["logp"] - e32["logp"]).max()
    err_en = np.abs(e64["entropy"] - e32["entropy"]).max()
    print(f"float32 against float64: grad {err_g:.3g} (relative to |g_lp| + |g_en|), logp {err_lp:.3g}, entropy {err_en:.3g}")
    assert err_g <= TOL and err_lp <= TOL and err_en <= TOL
