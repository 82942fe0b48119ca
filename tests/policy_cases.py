"""TEST INFRASTRUCTURE ONLY -- inputs at the edges of the policy kernels (csrc/cog_policy.hip) that
random_logits / random_masks / consecutive seeds never reach, shared by tests/test_policy_edges_cpu.py
and tests/test_gpu_policy_edges.py: logit families far outside [-8, 8], flat heads whose sampled
index has a closed form, sampler states with a planted draw, unlikely legal actions, arbitrary
non-zero mask bytes; and the allowances both files hold results to."""
import numpy as np

import policy_ref as pr
from policy_ref import COLS, HEADS, MINSTD_M

TOL = 1e-5                                                  # entropy; gradient relative to |g_lp| + |g_en|
FAMILIES = ("offset", "spread", "peaked", "premasked", "tiny")
ORDINARY = -1e8                                             # a logit above it is no mask of the network's own
FLAT_CONSTANTS = np.array([0.0, -0.0, 1000.5, -3e5, 3e38, -3e38, 1e-40, 7.25], dtype=np.float32)


def logp_allowance(ref):
    """About eight float32 roundings of magnitude up to |ref| (x - m, - log Z, the adds into the wave's
    sum, three cross-wave adds) on top of the project's 1e-5."""
    return TOL + 8 * 2.0 ** -24 * np.abs(ref)


def logit_family(rng, n, name):
    """(n, 92) float32 of the named family."""
    base = rng.normal(0.0, 3.0, (n, COLS))
    if name == "offset":
        base = base + rng.choice([-1e4, 1e4, 3e5, -2.5e3], n)[:, None]
    elif name == "spread":
        base = np.clip(rng.normal(0.0, 40.0, (n, COLS)), -150.0, 150.0)
    elif name == "peaked":
        for off, k in HEADS:
            base[np.arange(n), off + rng.integers(0, k, n)] += rng.choice([20.0, 50.0, 120.0], n)
    elif name == "premasked":
        fill = np.array([-np.inf, np.finfo(np.float32).min, -1e9, -1e30])
        hit = rng.random((n, COLS)) < 0.4
        base = np.where(hit, fill[rng.integers(0, 4, (n, COLS))], base)
    elif name == "tiny":
        with np.errstate(under="ignore"):
            return (base.astype(np.float32) * np.float32(1e-40)).astype(np.float32)
    else:
        raise ValueError(name)
    return base.astype(np.float32)


def ordinary(logits):
    with np.errstate(invalid="ignore"):
        return np.isfinite(logits) & (logits > ORDINARY)


def give_ordinary_entry(rng, logits, masks):
    """Every non-empty head without a valid ordinary logit gets N(0, 3) on one of its valid entries
    (in place), so that no row is degenerate."""
    valid_all = masks[:, :COLS] != 0
    for off, k in HEADS:
        valid = valid_all[:, off:off + k]
        need = np.flatnonzero(valid.any(1) & ~(valid & ordinary(logits[:, off:off + k])).any(1))
        for i in need:
            logits[i, off + rng.choice(np.flatnonzero(valid[i]))] = rng.normal(0.0, 3.0)
    return logits


def family_case(rng, n, name):
    """(logits, masks) of a family, masks from random_masks, no degenerate head."""
    logits, masks = logit_family(rng, n, name), pr.random_masks(rng, n)
    return give_ordinary_entry(rng, logits, masks), masks


def uniform_legal_actions(rng, masks, logits):
    """(n, 5) uint8: per head a uniformly chosen valid entry with an ordinary logit, 0 for an empty head."""
    n = logits.shape[0]
    valid_all = masks[:, :COLS] != 0
    out = np.zeros((n, 5), dtype=np.uint8)
    for h, (off, k) in enumerate(HEADS):
        valid = valid_all[:, off:off + k]
        can = valid & ordinary(logits[:, off:off + k])
        assert (can.any(1) == valid.any(1)).all(), "a non-empty head without an ordinary valid logit"
        score = np.where(can, rng.random((n, k)), -1.0)
        out[:, h] = np.where(valid.any(1), score.argmax(1), 0)
    return out


# ---- flat heads: every head of a row holds one constant, and the index has a closed form ----

def flat_logits(rng, n):
    idx = rng.integers(0, FLAT_CONSTANTS.size, (n, 5))
    return np.repeat(FLAT_CONSTANTS[idx], [k for _, k in HEADS], axis=1)


def entry_number(valid, number):
    """Column of the valid entry number `number` (counted from 0) of each row of valid (n, k)."""
    return ((np.cumsum(valid, axis=1) == (number + 1)[:, None]) & valid).argmax(1)


def flat_expected(masks, states):
    """For flat heads all d are 0 and all w are 1, the prefix sums over the K valid entries are the
    integers 1..K and t = fl32(u K) is one IEEE multiply: the action is the valid entry number
    floor(t) (the last one should t reach K), logp = -sum log K, entropy = +sum log K.
    Returns (actions (n, 5), sum log K (n,) float64, first valid entries (n, 5), the states after)."""
    valid_all = masks[:, :COLS] != 0
    n = masks.shape[0]
    x = np.array(states, dtype=np.uint64)
    actions, first = np.zeros((n, 5), dtype=np.int64), np.zeros((n, 5), dtype=np.int64)
    logk = np.zeros(n)
    for h, (off, k) in enumerate(HEADS):
        valid = valid_all[:, off:off + k]
        K = valid.sum(1)
        x = pr.mr_next(x)
        u = (((x - np.uint64(1)) >> np.uint64(7)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
        t = u * K.astype(np.float32)                        # float32 x float32: one rounding
        assert t.dtype == np.float32
        number = np.minimum(np.floor(t).astype(np.int64), K - 1)
        actions[:, h] = np.where(K > 0, entry_number(valid, number), 0)
        first[:, h] = np.where(K > 0, valid.argmax(1), 0)
        logk += np.log(np.maximum(K, 1))
    return actions, logk, first, x


# ---- planted draws ----

def state_for(head, r):
    """The sampler state for which head `head`'s draw (the state advanced head + 1 times) has
    x_new - 1 == r, so that u = (r >> 7) 2^-24.  r in 0 .. 2^31 - 3."""
    assert 0 <= r <= MINSTD_M - 2
    inv = pow(16807, -1, MINSTD_M)
    return (r + 1) * pow(inv, head + 1, MINSTD_M) % MINSTD_M


# (r, u, which of the four equally likely valid entries the draw selects under C_j > u Z)
PLANTED_DRAWS = [(0, 0.0, 0), (127, 0.0, 0), (1 << 29, 0.25, 1), (2 << 29, 0.5, 2), (3 << 29, 0.75, 3),
                 (MINSTD_M - 2, 1.0 - 2.0 ** -24, 3)]
# The last bit of u: on three equally likely entries u = 11184811 2^-24 (odd) gives u Z = 2 + 2^-24, which
# float32 rounds to 2: not below C_1 = 2, so entry 2.  Without its last bit u Z = 2 - 2^-23: entry 1.
LAST_BIT_DRAW = (11184811 << 7, 11184811 * 2.0 ** -24, 2)


def equal_row(rng, head, count=4):
    """One row (logits (1, 92), masks (1, 128), the `count` columns within the head): head `head` has
    exactly `count` (3 or 4) valid entries with equal logits, spread over the head with its last
    column among them and its first column invalid; the logits under its zero mask bytes are larger;
    the other heads are random."""
    logits, masks = pr.random_logits(rng, 1), pr.random_masks(rng, 1)
    off, k = HEADS[head]
    cols = np.array([1, k // 3 + 1, 2 * k // 3, k - 1][4 - count:])
    masks[0, off:off + k] = 0
    masks[0, off + cols] = 1
    logits[0, off:off + k] = 6.0
    logits[0, off + cols] = np.float32(rng.normal(0.0, 3.0))
    return logits, masks, cols


# ---- mask bytes ----

def any_nonzero_bytes(rng, masks):
    """The same records with every non-zero byte of the 92 used ones replaced by a value from 1..255;
    the first rows hold 0x80, 0x7f, 0xff and 0 next to one another within one dword."""
    out = masks.copy()
    used = out[:, :COLS]
    used[...] = np.where(used != 0, rng.integers(1, 256, used.shape), 0).astype(np.uint8)
    pattern = np.array([[0x80, 0x00, 0x7f, 0xff], [0x00, 0x80, 0x00, 0x7f], [0xff, 0x80, 0x80, 0x00], [0x7f, 0xff, 0x00, 0x80],
                        [0x00, 0x00, 0x00, 0x80], [0x7f, 0x00, 0x00, 0x00], [0x80, 0x80, 0x80, 0x80], [0x01, 0xfe, 0x00, 0x40]],
                       dtype=np.uint8)
    for i in range(min(len(pattern), out.shape[0])):
        used[i] = np.resize(np.roll(pattern, i, axis=0).ravel(), COLS)
    return out


def as_ones(masks):
    """The same records with every non-zero used byte set to 1."""
    out = masks.copy()
    out[:, :COLS] = out[:, :COLS] != 0
    return out
