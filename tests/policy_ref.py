"""TEST INFRASTRUCTURE ONLY -- the numpy form of the policy sampler's semantics (include/cog.h
cog_sampler_sample_policy), shared by tests/test_policy_cpu.py and tests/test_gpu_policy_sampler.py.

Float64 by default; dtype=np.float32 evaluates the same formulas in float32 (sequential prefix
sums), which is how the CPU test pins the width of the band in which a float32 sampler may pick a
neighbouring index."""
import numpy as np

HEADS = ((0, 22), (22, 22), (44, 22), (66, 7), (73, 19))   # (offset, size) in ActionMask byte order
COLS = 92
MINSTD_M = 2147483647
BAND = 1e-5            # |u Z - C_j| <= BAND * Z: the index may differ from the float64 one


def mr_seed(s):
    x = int(s) % MINSTD_M
    return 1 if x == 0 else x


def sampler_states(seed, n, first=0):
    """minstd_rand0 states of a fresh sampler: sampler i is seeded seed + first + i."""
    return np.array([mr_seed((seed & 0xFFFFFFFF) + first + i) for i in range(n)], dtype=np.uint64)


def mr_next(x):
    return x * np.uint64(16807) % np.uint64(MINSTD_M)


def sample(logits, masks, states=None, greedy=False, dtype=np.float64, strict=True):
    """logits: (n, 92) float array (the float32 / widened bfloat16 values); masks: (n, >= 92), non-zero
    = valid; states: (n,) uint64 sampler states (None with greedy).  strict=False is the wrong rule
    C_j >= u Z, kept so that a test can show that its cases tell the two apart.
    Returns dict(actions (n, 5) int, logp, entropy (n,) dtype, near (n, 5) bool: some valid prefix sum
    lies within the band of u Z, states: the states after the call)."""
    logits = np.asarray(logits)
    n = logits.shape[0]
    valid_all = np.asarray(masks)[:, :COLS] != 0
    actions = np.zeros((n, 5), dtype=np.int64)
    near = np.zeros((n, 5), dtype=bool)
    logp = np.zeros(n, dtype=dtype)
    ent = np.zeros(n, dtype=dtype)
    bad = np.zeros(n, dtype=bool)
    x = None if greedy else np.array(states, dtype=np.uint64)
    rows = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for h, (off, k) in enumerate(HEADS):
            valid = valid_all[:, off:off + k]
            some = valid.any(1)
            l = logits[:, off:off + k].astype(dtype)
            lv = np.where(valid & ~np.isnan(l), l, -np.inf).astype(dtype)
            m = lv.max(1)
            degen = some & ~np.isfinite(m)
            best = ((lv == m[:, None]) & valid).argmax(1)          # largest logit, lowest index
            ok = some & ~degen
            m0 = np.where(ok, m, 0).astype(dtype)
            d = lv - m0[:, None]
            w = np.exp(d).astype(dtype)
            if dtype == np.float32:                                # a sequential float32 sum, as a scan has it
                C = np.cumsum(w, axis=1, dtype=np.float32)
            else:
                C = np.cumsum(w, axis=1)
            Z = C[:, -1]
            if greedy:
                a = best
            else:
                x = mr_next(x)
                u = (((x - np.uint64(1)) >> np.uint64(7)).astype(np.float64) * 2.0 ** -24).astype(dtype)
                t = (u * Z).astype(dtype)
                over = ((C > t[:, None]) if strict else (C >= t[:, None])) & valid
                last = k - 1 - valid[:, ::-1].argmax(1)
                a = np.where(over.any(1), over.argmax(1), last)
                a = np.where(degen, best, a)
                near[:, h] = ok & ((np.abs(t[:, None] - C) <= BAND * Z[:, None]) & valid).any(1)
            a = np.where(some, a, 0)
            actions[:, h] = a
            da = np.where(greedy, 0, d[rows, a])
            wd = np.where(w > 0, w * np.where(np.isfinite(d), d, 0), 0)
            logZ = np.log(np.where(ok, Z, 1)).astype(dtype)
            logp += np.where(ok, da - logZ, 0).astype(dtype)
            ent += np.where(ok, logZ - wd.sum(1) / np.where(ok, Z, 1), 0).astype(dtype)
            bad |= degen
    logp[bad] = np.nan
    ent[bad] = np.nan
    return {"actions": actions, "logp": logp, "entropy": ent, "near": near, "states": x}


def legal(actions, masks):
    """(n, 5) bool: the action lies inside its head's mask (0 for a head with no valid entry)."""
    valid_all = np.asarray(masks)[:, :COLS] != 0
    out = np.zeros(actions.shape, dtype=bool)
    rows = np.arange(actions.shape[0])
    for h, (off, k) in enumerate(HEADS):
        valid = valid_all[:, off:off + k]
        a = actions[:, h].astype(np.int64)
        inside = a < k
        out[:, h] = np.where(valid.any(1), inside & valid[rows, np.minimum(a, k - 1)], a == 0)
    return out


def random_masks(rng, n):
    """(n, 128) uint8 ActionMask records: random 0/1 bytes with empty, full and single-entry heads,
    a byte value 2 here and there, and junk in the 36 padding bytes."""
    m = (rng.random((n, 128)) < 0.5).astype(np.uint8)
    for h, (off, k) in enumerate(HEADS):
        kind = rng.integers(0, 8, n)
        m[kind == 0, off:off + k] = 0
        m[kind == 1, off:off + k] = 1
        one = np.flatnonzero(kind == 2)
        m[one, off:off + k] = 0
        m[one, off + rng.integers(0, k, one.size)] = 1
    m[(rng.random((n, 128)) < 0.05) & (m != 0)] = 2
    m[:, COLS:] = rng.integers(0, 256, (n, 128 - COLS))
    return m


def random_logits(rng, n):
    return np.clip(rng.normal(0.0, 3.0, (n, COLS)), -8.0, 8.0).astype(np.float32)
