"""CPU: the policy sampler's surface (header, library, Python class) and the numpy reference's own
float32-against-float64 agreement, which pins the band tests/test_gpu_policy_sampler.py allows."""
import ctypes
import os
import re

import numpy as np

import policy_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gym-eldorado_amd", "city_of_gold", "libcog_hip.so")


def test_header_declares_the_policy_sampler():
    src = open(os.path.join(ROOT, "include", "cog.h")).read()
    assert re.search(r"COG_API\s+int\s+cog_sampler_sample_policy\s*\(\s*cog_sampler\s*\*\s*\w+\s*,\s*const\s+cog_policy_args\s*\*", src)
    assert "typedef struct cog_policy_args" in src
    expect = {"COG_LOGITS_F32": "0", "COG_LOGITS_BF16": "1", "COG_MASKS_SELECTED": "0", "COG_MASKS_STORED": "1",
              "COG_MASKS_POINTER": "2", "COG_POLICY_GREEDY": "0x1u", "COG_ABI_VERSION": "1"}
    for name, value in expect.items():
        m = re.search(rf"#define\s+{name}\s+(\S+)", src)
        assert m and m.group(1) == value, name


def test_null_arguments_are_invalid():
    lib = ctypes.CDLL(LIB)
    lib.cog_sampler_sample_policy.restype = ctypes.c_int
    lib.cog_sampler_sample_policy.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.cog_last_error.restype = ctypes.c_char_p
    assert lib.cog_sampler_sample_policy(None, None) == -1          # COG_ERR_INVALID
    assert b"NULL" in lib.cog_last_error()


def test_python_method_exists(cg):
    cls = cg.vec.get_vec_sampler(64)
    assert callable(getattr(cls, "sample_policy"))
    assert "sample_policy_raw" in dir(cls)
    assert "sample_policy" in cg.__doc__


def test_reference_rng_matches_the_engine_header():
    """x <- 16807 x mod (2^31 - 1) from mr_seed(seed + i); u = ((x - 1) >> 7) 2^-24 in [0, 1)."""
    x = pr.sampler_states(0xFFFFFFFF, 3)
    assert [int(v) for v in x] == [0xFFFFFFFF % pr.MINSTD_M, 2, 3]          # (the sum is not wrapped)
    assert pr.mr_seed(pr.MINSTD_M) == 1
    assert int(pr.mr_next(np.array([1], dtype=np.uint64))[0]) == 16807
    y = np.array([1], dtype=np.uint64)
    for _ in range(10000):
        y = pr.mr_next(y)
    assert int(y[0]) == 1043618065                                          # minstd_rand0's 10000th value


def test_float32_index_agrees_with_float64_outside_the_band():
    """The same formulas in float32 pick the float64 index whenever no valid prefix sum lies within
    1e-5 Z of u Z; the band takes a small share of the cases; logp and entropy agree to 1e-5."""
    rng = np.random.default_rng(2024)
    n = 50000
    logits = pr.random_logits(rng, n)
    masks = pr.random_masks(rng, n)
    states = pr.sampler_states(12345, n)
    r64 = pr.sample(logits, masks, states)
    r32 = pr.sample(logits, masks, states, dtype=np.float32)
    differ = r64["actions"] != r32["actions"]
    assert not (differ & ~r64["near"]).any(), f"{int((differ & ~r64['near']).sum())} disagreements outside the band"
    assert r64["near"].mean() <= 0.01
    assert pr.legal(r64["actions"], masks).all() and pr.legal(r32["actions"], masks).all()
    same = ~differ.any(1)
    assert np.abs(r64["logp"] - r32["logp"])[same].max() <= 1e-5
    assert np.abs(r64["entropy"] - r32["entropy"]).max() <= 1e-5
    assert np.array_equal(r64["states"], r32["states"])
    g = pr.sample(logits, masks, greedy=True)
    assert pr.legal(g["actions"], masks).all()
