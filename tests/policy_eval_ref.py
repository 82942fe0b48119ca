"""TEST INFRASTRUCTURE ONLY -- the numpy form of the policy evaluator's semantics (include/cog.h
cog_policy_evaluate / cog_policy_evaluate_backward), shared by tests/test_policy_evaluate_cpu.py and
tests/test_gpu_policy_evaluate.py: the joint log-probability of recorded actions and the entropy of
the five masked heads, their gradient with respect to the logits, and the bad rows.

Float64 by default; dtype=np.float32 evaluates the same formulas in float32 (sequential sums), which
is how the CPU test pins the tolerance of the GPU test."""
import numpy as np

from policy_ref import COLS, HEADS, random_logits, random_masks, sample  # noqa: F401  (re-exported for the tests)


def evaluate(logits, actions, masks, g_lp=None, g_en=None, dtype=np.float64):
    """logits: (n, 92) float array (the float32 / widened bfloat16 values); actions: (n, >= 5) ints, the
    recorded action of each head; masks: (n, >= 92), non-zero = valid; g_lp, g_en: (n,) incoming
    gradients (None = zeros).
    Returns dict(logp, entropy (n,) dtype: NaN for a bad row; grad (n, 92) dtype: zeros for a bad row;
    bad (n,) bool; nonempty (n, 5) bool).  A recorded action on a valid -inf entry beside finite valid
    ones is no bad row: logp is -inf and the gradient entry at the action is g_lp."""
    logits = np.asarray(logits)
    actions = np.asarray(actions)
    n = logits.shape[0]
    valid_all = np.asarray(masks)[:, :COLS] != 0
    g_lp = np.zeros(n, dtype=dtype) if g_lp is None else np.asarray(g_lp).astype(dtype)
    g_en = np.zeros(n, dtype=dtype) if g_en is None else np.asarray(g_en).astype(dtype)
    logp = np.zeros(n, dtype=dtype)
    ent = np.zeros(n, dtype=dtype)
    grad = np.zeros((n, COLS), dtype=dtype)
    bad = np.zeros(n, dtype=bool)
    nonempty = np.zeros((n, 5), dtype=bool)
    rows = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for h, (off, k) in enumerate(HEADS):
            valid = valid_all[:, off:off + k]
            some = valid.any(1)
            nonempty[:, h] = some
            l = logits[:, off:off + k].astype(dtype)
            lv = np.where(valid & ~np.isnan(l), l, -np.inf).astype(dtype)
            m = lv.max(1)
            a = actions[:, h].astype(np.int64)
            ac = np.minimum(a, k - 1)
            illegal = (a >= k) | ~valid[rows, ac]
            bad |= some & (~np.isfinite(m) | illegal)
            ok = some & np.isfinite(m) & ~illegal
            m0 = np.where(ok, m, 0).astype(dtype)
            d = lv - m0[:, None]
            w = np.exp(d).astype(dtype)
            dz = np.where(np.isfinite(d), d, 0).astype(dtype)           # (w is 0 there: 0 * d counts as 0)
            if dtype == np.float32:
                Z = np.cumsum(w, axis=1, dtype=np.float32)[:, -1]
                S = np.cumsum(w * dz, axis=1, dtype=np.float32)[:, -1]
            else:
                Z, S = w.sum(1), (w * dz).sum(1)
            Z1 = np.where(ok, Z, 1).astype(dtype)
            logZ = np.log(Z1).astype(dtype)
            H = (logZ - S / Z1).astype(dtype)
            logp += np.where(ok, d[rows, ac] - logZ, 0).astype(dtype)
            ent += np.where(ok, H, 0).astype(dtype)
            p = (w / Z1[:, None]).astype(dtype)
            onehot = (np.arange(k)[None, :] == ac[:, None]).astype(dtype)
            # log p_j + H = d_j - S / Z; the entropy term is 0 where p_j = 0
            t = np.where(p > 0, p * (dz - (S / Z1)[:, None]), 0).astype(dtype)
            g = g_lp[:, None] * (onehot - p) - g_en[:, None] * t
            grad[:, off:off + k] = np.where(valid & ok[:, None], g, 0).astype(dtype)
    logp[bad] = np.nan
    ent[bad] = np.nan
    grad[bad] = 0
    return {"logp": logp, "entropy": ent, "grad": grad, "bad": bad, "nonempty": nonempty}


def bf16_round(x):
    """float32 values rounded to the nearest bfloat16 (ties to even), as float32."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)
    return r.view(np.float32)
