"""CPU: the claims tests/test_gpu_policy_edges.py rests on, pinned with the two numpy references alone:
the closed form of a flat head's index, the planted sampler states, the float32 modes inside the
allowances on every logit family, the share of cases inside the band, and the counts that show a
family still makes its point."""
import numpy as np
import pytest

import policy_cases as pc
import policy_eval_ref as per
import policy_ref as pr

SEED = 20250


def test_flat_closed_form_equals_the_float32_reference():
    """4096 rows x 5 heads, two calls: the action is the valid entry number floor(fl32(u K)); logp and
    entropy are -+ sum log K; greedy takes the first valid entry."""
    rng = np.random.default_rng(1)
    n = 4096
    states = pr.sampler_states(SEED, n)
    counts = set()
    for call in range(2):
        logits, masks = pc.flat_logits(rng, n), pr.random_masks(rng, n)
        want, logk, first, after = pc.flat_expected(masks, states)
        r32 = pr.sample(logits, masks, states, dtype=np.float32)
        r64 = pr.sample(logits, masks, states)
        assert np.array_equal(r32["actions"], want), f"call {call}: {int((r32['actions'] != want).sum())} differ"
        assert np.array_equal(r32["states"], after)
        assert pr.legal(want, masks).all()
        assert np.abs(r64["logp"] + logk).max() <= 1e-12 and np.abs(r64["entropy"] - logk).max() <= 1e-12
        assert np.abs(r32["logp"] + logk).max() <= pc.TOL and np.abs(r32["entropy"] - logk).max() <= pc.TOL
        assert np.array_equal(pr.sample(logits, masks, greedy=True)["actions"], first)
        states = after
        for off, k in pr.HEADS:
            counts |= set((masks[:, off:off + k] != 0).sum(1).tolist())
    assert counts >= set(range(20)) | {22}, "random_masks no longer covers the valid counts 0..19 and 22"
    for h, (off, k) in enumerate(pr.HEADS):                 # every head of a row is one constant
        assert (logits[:, off:off + k] == logits[:, off:off + 1]).all()
    assert set(np.unique(logits).tolist()) <= set(pc.FLAT_CONSTANTS.tolist())


def test_state_for_gives_the_intended_draw():
    for head in range(5):
        for r, u, _ in pc.PLANTED_DRAWS + [pc.LAST_BIT_DRAW]:
            x = np.array([pc.state_for(head, r)], dtype=np.uint64)
            assert 1 <= int(x[0]) < pr.MINSTD_M and pr.mr_seed(int(x[0])) == int(x[0])
            for _ in range(head + 1):
                x = pr.mr_next(x)
            assert int(x[0]) - 1 == r, (head, r)
            assert ((int(x[0]) - 1) >> 7) * 2.0 ** -24 == u, (head, r)
    assert [u for _, u, _ in pc.PLANTED_DRAWS] == [0.0, 0.0, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -24]
    assert np.float32(1.0 - 2.0 ** -24) < 1.0               # (the top of the range is a float32 below 1)


def test_planted_draws_separate_the_strict_comparison():
    """On four equally likely entries u = j / 4 meets the prefix sum j exactly: C_j > u Z selects entry
    j, C_j >= u Z entry j - 1.  Both float modes; the other draws give both rules the same entry."""
    rng = np.random.default_rng(2)
    for head in range(5):
        logits, masks, cols = pc.equal_row(rng, head)
        assert (masks[0, pr.HEADS[head][0]:][:pr.HEADS[head][1]] != 0).sum() == 4
        for r, u, entry in pc.PLANTED_DRAWS:
            states = np.array([pc.state_for(head, r)], dtype=np.uint64)
            for dtype in (np.float64, np.float32):
                strict = pr.sample(logits, masks, states, dtype=dtype)["actions"][0, head]
                loose = pr.sample(logits, masks, states, dtype=dtype, strict=False)["actions"][0, head]
                assert strict == cols[entry], (head, r, dtype)
                if u in (0.25, 0.5, 0.75):
                    assert loose == cols[entry - 1] != strict, (head, r, dtype)
                else:
                    assert loose == strict, (head, r, dtype)


def test_last_bit_draw_needs_every_bit_of_u():
    """Three equally likely entries, u = 11184811 2^-24: u Z = 2 + 2^-24 is 2 in float32 and entry 2 in
    both float modes; the same u without its last bit gives 2 - 2^-23 and entry 1."""
    r, u, entry = pc.LAST_BIT_DRAW
    assert (r >> 7) & 1 and (r >> 7) * 2.0 ** -24 == u and np.float32(u) == u
    assert np.float32(u) * np.float32(3) == 2 and u * 3 == 2 + 2.0 ** -24
    short = np.float32(((r >> 8) << 1) * 2.0 ** -24)
    assert short * np.float32(3) == np.float32(2 - 2.0 ** -23) < 2
    rng = np.random.default_rng(5)
    for head in range(5):
        logits, masks, cols = pc.equal_row(rng, head, 3)
        assert len(cols) == 3 and cols[-1] == pr.HEADS[head][1] - 1
        states = np.array([pc.state_for(head, r)], dtype=np.uint64)
        for dtype in (np.float64, np.float32):
            assert pr.sample(logits, masks, states, dtype=dtype)["actions"][0, head] == cols[entry]


@pytest.mark.parametrize("name", pc.FAMILIES)
def test_float32_mode_stays_inside_the_allowances(name):
    """20,000 rows of a family: no bad row; the float32 index is the float64 one outside the band and
    the band holds at most 1 % of the cases; entropy within 1e-5, logp within 1e-5 + 8 2^-24 |ref|,
    the gradient within 1e-5 (|g_lp| + |g_en|), under the sampled actions and under uniformly drawn
    legal ones; and the family still makes its point."""
    rng = np.random.default_rng(100 + pc.FAMILIES.index(name))
    n = 20000
    logits, masks = pc.family_case(rng, n, name)
    states = pr.sampler_states(SEED, n)
    r64 = pr.sample(logits, masks, states)
    r32 = pr.sample(logits, masks, states, dtype=np.float32)
    assert not np.isnan(r64["logp"]).any() and not np.isnan(r32["logp"]).any() and not np.isnan(r32["entropy"]).any()
    differ = r64["actions"] != r32["actions"]
    assert not (differ & ~r64["near"]).any(), f"{int((differ & ~r64['near']).sum())} disagreements outside the band"
    assert r64["near"].mean() <= 0.01
    assert pr.legal(r64["actions"], masks).all() and pr.legal(r32["actions"], masks).all()
    same = ~differ.any(1)
    over_lp = (np.abs(r64["logp"] - r32["logp"]) - pc.logp_allowance(r64["logp"]))[same].max()
    err_en = np.abs(r64["entropy"] - r32["entropy"]).max()
    print(f"{name} sampler: in the band {int(r64['near'].sum())}/{differ.size}, logp over allowance {over_lp:.3g}, entropy {err_en:.3g}")
    assert over_lp <= 0 and err_en <= pc.TOL

    g_lp, g_en = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    scale = (np.abs(g_lp) + np.abs(g_en)).astype(np.float64)
    uniform = pc.uniform_legal_actions(rng, masks, logits)
    assert pr.legal(uniform.astype(np.int64), masks).all()
    for label, actions in (("sampled", r64["actions"]), ("uniform", uniform)):
        e64 = per.evaluate(logits, actions, masks, g_lp, g_en)
        e32 = per.evaluate(logits, actions, masks, g_lp, g_en, dtype=np.float32)
        assert not e64["bad"].any() and not e32["bad"].any()
        assert np.isfinite(e64["logp"]).all() and np.isfinite(e32["logp"]).all()
        assert np.isfinite(e32["grad"]).all() and np.isfinite(e32["entropy"]).all()
        over_lp = (np.abs(e64["logp"] - e32["logp"]) - pc.logp_allowance(e64["logp"])).max()
        err_en = np.abs(e64["entropy"] - e32["entropy"]).max()
        err_g = (np.abs(e64["grad"] - e32["grad"]).max(1) / scale).max()
        print(f"{name} evaluator, {label} actions: max |logp| {np.abs(e64['logp']).max():.4g}, logp over allowance {over_lp:.3g}, "
              f"entropy {err_en:.3g}, grad {err_g:.3g}")
        assert over_lp <= 0 and err_en <= pc.TOL and err_g <= pc.TOL
        if label == "uniform" and name == "spread":
            assert (np.abs(e64["logp"]) > 100).sum() >= n // 10, "spread has lost its unlikely recorded actions"
            assert (e32["logp"] < -104).any()               # p_a underflows to 0 in float32
    if name == "premasked":
        valid = masks[:, :pr.COLS] != 0
        assert (valid & ~np.isfinite(logits)).any(1).sum() >= n // 2, "premasked has lost its non-finite valid entries"
        for v in (-np.inf, np.finfo(np.float32).min, np.float32(-1e9), np.float32(-1e30)):
            assert (valid & (logits == v)).any()
    if name == "peaked":
        assert (r64["entropy"] < 1e-3).sum() >= n // 100, "peaked has lost its rows of entropy near 0"
    if name == "tiny":
        assert (np.abs(logits[logits != 0]) < np.finfo(np.float32).tiny).all()
    if name == "offset":
        assert (np.abs(logits).min(1) > 2000).all()


def test_recorded_action_on_a_valid_minus_inf_entry():
    """Such an action has probability 0: logp is -inf (not NaN), the row is not bad, the entropy is
    that of the other entries and the gradient is finite, g_lp (1[j = a] - p_j) - g_en p_j (...) with
    p_a = 0.  Both float modes."""
    rng = np.random.default_rng(3)
    n = 8
    logits, masks = pr.random_logits(rng, n), pr.random_masks(rng, n)
    actions = pr.sample(logits, masks, pr.sampler_states(SEED, n))["actions"]
    masks[:, 22:44] = 0
    masks[:, [24, 27, 31, 43]] = 1
    actions[:, 1] = 2
    g_lp, g_en = rng.normal(size=n), rng.normal(size=n)
    clean = per.evaluate(logits, actions, masks, g_lp, g_en)
    logits[:, 31] = -np.inf
    actions[:, 1] = 9
    for dtype in (np.float64, np.float32):
        ev = per.evaluate(logits, actions, masks, g_lp, g_en, dtype=dtype)
        assert not ev["bad"].any()
        assert (ev["logp"] == -np.inf).all() and np.isfinite(ev["entropy"]).all() and np.isfinite(ev["grad"]).all()
        assert np.abs(ev["grad"][:, 31] - g_lp).max() <= 1e-6
        other = np.setdiff1d(np.arange(92), np.arange(22, 44))
        assert np.abs(ev["grad"][:, other] - clean["grad"][:, other]).max() <= 1e-6
    smp = pr.sample(logits, masks, pr.sampler_states(SEED, n))
    assert (smp["actions"][:, 1] != 9).all() and np.isfinite(smp["logp"]).all()


def test_mask_byte_helpers():
    rng = np.random.default_rng(4)
    masks = pr.random_masks(rng, 257)
    alt = pc.any_nonzero_bytes(rng, masks)
    ones = pc.as_ones(alt)
    assert np.array_equal(alt[:, :92] != 0, ones[:, :92] != 0) and np.array_equal(alt[:, 92:], ones[:, 92:])
    assert set(np.unique(ones[:, :92]).tolist()) == {0, 1}
    assert set(np.unique(alt[:, :92]).tolist()) == set(range(256))
    words = alt[:, :92].reshape(-1, 4)
    for a, b in ((0x80, 0x7f), (0x80, 0xff), (0x7f, 0xff), (0x80, 0x00)):
        assert ((words == a).any(1) & (words == b).any(1)).any(), (a, b)
    assert np.array_equal(alt[8:, :92] != 0, masks[8:, :92] != 0)
