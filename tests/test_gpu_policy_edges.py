"""GPU: the policy sampler and evaluator (csrc/cog_policy.hip) at the edges the random cases of
tests/test_gpu_policy_sampler.py and tests/test_gpu_policy_evaluate.py never reach: sampled indices
known exactly (flat heads, planted draws at u = 0, j / 4 and 1 - 2^-24), logits far outside [-8, 8],
unlikely recorded actions, a recorded action on a valid -inf entry, arbitrary non-zero mask bytes,
and the stored masks of 1, 2 and 3 players.  The inputs and the allowances come from
tests/policy_cases.py; tests/test_policy_edges_cpu.py pins them with the numpy references alone.

Allowances: entropy 1e-5; logp 1e-5 + 8 2^-24 |ref|; a float32 gradient row 1e-5 (|g_lp| + |g_en|); a
bfloat16 gradient entry the rounded reference plus 2^-8 |ref| plus the float32 allowance."""
import numpy as np
import pytest

import policy_cases as pc
import policy_eval_ref as per
import policy_ref as pr

pytestmark = pytest.mark.gpu

SEED = 9091
N = 257                                                     # four full tiles and one row
KINDS = [("f32", 92), ("f32", 93), ("bf16", 92)]            # 16-B loads, the element-wise path, bfloat16
HEAD_SIZES = [k for _, k in pr.HEADS]


def kind_id(kind):
    return f"{kind[0]}-ld{kind[1]}"


def to_device(logits, kind, requires_grad=False):
    """kind: (dtype name, ld).  Returns (the leaf buffer, its (n, 92) view, the float32 values it holds
    as read back from the device)."""
    import torch
    dt, ld = kind
    n = logits.shape[0]
    t = torch.from_numpy(logits).cuda()
    if dt == "bf16":
        t = t.to(torch.bfloat16)
    buf = torch.full((n * ld + 8,), float("nan"), dtype=t.dtype, device="cuda")
    with torch.no_grad():
        buf[:n * ld].view(n, ld)[:, :92].copy_(t)
    buf.requires_grad_(requires_grad)
    view = buf[:n * ld].view(n, ld)[:, :92]
    return buf, view, view.detach().float().cpu().numpy()


def run_sampler(smp, view, masks_np, **kw):
    import torch
    actions, logp, ent = smp.sample_policy(view, None, torch.from_numpy(masks_np).cuda(), **kw)
    return actions.cpu().numpy(), logp.cpu().numpy(), ent.cpu().numpy()


def run_evaluator(cg, logits, kind, actions, masks, g_lp, g_en):
    """Forward and backward; returns (values, logp, entropy, grad (n, 92) widened to float32)."""
    import torch
    n, ld = logits.shape[0], kind[1]
    buf, view, values = to_device(logits, kind, requires_grad=True)
    lp, en = cg.policy_evaluate(view, torch.from_numpy(np.ascontiguousarray(actions, dtype=np.uint8)).cuda(),
                                torch.from_numpy(masks).cuda())
    torch.autograd.backward([lp, en], [torch.from_numpy(g_lp).cuda(), torch.from_numpy(g_en).cuda()])
    assert buf.grad.dtype == buf.dtype
    g = buf.grad[:n * ld].view(n, ld).float().cpu().numpy()
    assert not g[:, 92:].any() and not buf.grad[n * ld:].any()
    return values, lp.detach().cpu().numpy(), en.detach().cpu().numpy(), g[:, :92]


def check_sampler(ref, acts, logp, ent, label):
    """The index rule of tests/test_gpu_policy_sampler.py with the logp allowance of this file; returns
    (cases inside the band, cases)."""
    differ = acts[:, :5].astype(np.int64) != ref["actions"]
    outside = differ & ~ref["near"]
    assert not outside.any(), f"{label}: {int(outside.sum())} indices differ outside the band, first at {np.argwhere(outside)[0]}"
    assert not np.isnan(logp).any() and not np.isnan(ent).any(), f"{label}: NaN in a good row"
    same = ~differ.any(1)
    err_lp = np.abs(logp.astype(np.float64) - ref["logp"])
    over_lp = (err_lp - pc.logp_allowance(ref["logp"]))[same].max()
    err_en = np.abs(ent.astype(np.float64) - ref["entropy"]).max()
    print(f"{label}: in the band {int(ref['near'].sum())}/{differ.size}, max |logp| {np.abs(ref['logp']).max():.4g}, "
          f"max |dlogp| {err_lp[same].max():.3g} (over allowance {over_lp:.3g}), max |dentropy| {err_en:.3g}")
    assert over_lp <= 0, f"{label}: logp over its allowance by {over_lp}"
    assert err_en <= pc.TOL, f"{label}: entropy off by {err_en}"
    return int(ref["near"].sum()), differ.size


def check_evaluator(kind, ref, masks, g_lp, g_en, logp, ent, grad, label):
    """logp, ent, grad against the float64 reference `ref` (finite or -inf logp) under the allowances."""
    assert not ref["bad"].any()
    assert not np.isnan(logp).any() and not np.isnan(ent).any() and not np.isnan(grad).any(), f"{label}: NaN in a good row"
    inf = np.isinf(ref["logp"])
    assert np.array_equal(logp[inf], ref["logp"][inf].astype(np.float32)), f"{label}: an infinite logp differs"
    err_lp = np.where(inf, 0, np.abs(logp.astype(np.float64) - np.where(inf, 0, ref["logp"])))
    over_lp = (err_lp - pc.logp_allowance(np.where(inf, 0, ref["logp"])))[~inf].max()
    err_en = np.abs(ent.astype(np.float64) - ref["entropy"]).max()
    scale = np.abs(g_lp).astype(np.float64) + np.abs(g_en)
    want = ref["grad"]
    allow = pc.TOL * scale[:, None] * np.ones_like(want)
    if kind[0] == "bf16":
        want = per.bf16_round(want.astype(np.float32)).astype(np.float64)
        allow = allow + 2.0 ** -8 * np.abs(want)
    over_g = (np.abs(grad - want) - allow).max()
    used = (np.abs(grad - want) / allow)[allow > 0].max()
    print(f"{label}: max |logp| {np.abs(ref['logp'][~inf]).max():.4g}, max |dlogp| {err_lp.max():.3g} (over allowance {over_lp:.3g}), "
          f"max |dentropy| {err_en:.3g}, grad error over allowance {over_g:.3g} (at most {used:.3g} of it used)")
    assert over_lp <= 0, f"{label}: logp over its allowance by {over_lp}"
    assert err_en <= pc.TOL, f"{label}: entropy off by {err_en}"
    assert over_g <= 0, f"{label}: gradient over its allowance by {over_g}"
    zero = ~((masks[:, :92] != 0) & np.repeat(ref["nonempty"], HEAD_SIZES, axis=1))
    assert not grad[zero].any(), f"{label}: a column of an invalid entry or an empty head is not exactly 0"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_flat_heads_are_exact(cg, dt):
    """Every head of a row holds one constant (0, -0, 1000.5, -3e5, 3e38, -3e38, 1e-40, 7.25; the
    bfloat16 ones as the device holds them): all w are 1, so the sampled action is the valid entry
    number floor(fl32(u K)) on every one of the 2 x 257 x 5 cases, with no band and no skip; logp and
    entropy are -+ sum log K within 1e-5; greedy mode takes the first valid entry.

    Measured on the MI355X: all 2,570 indices of either type equal the closed form, so __expf(0.0f) is
    1.0f on gfx950 and u Z is one IEEE multiply there; logp and entropy are at most 1.7e-6 off."""
    rng = np.random.default_rng(31)
    kind = (dt, 92)
    smp = cg.vec.get_vec_sampler(N)(SEED)
    states = pr.sampler_states(SEED, N)
    for call in range(2):
        logits, masks = pc.flat_logits(rng, N), pr.random_masks(rng, N)
        _, view, values = to_device(logits, kind)
        for off, k in pr.HEADS:                             # still one finite constant per head
            assert np.isfinite(values).all() and (values[:, off:off + k] == values[:, off:off + 1]).all()
        want, logk, first, states = pc.flat_expected(masks, states)
        acts, logp, ent = run_sampler(smp, view, masks)
        wrong = acts[:, :5] != want
        err_lp, err_en = np.abs(logp + logk).max(), np.abs(ent - logk).max()
        print(f"flat {dt} call {call}: {int(wrong.sum())}/{wrong.size} indices off the closed form, "
              f"max |dlogp| {err_lp:.3g}, max |dentropy| {err_en:.3g}")
        assert not wrong.any(), f"call {call}: first at {np.argwhere(wrong)[0]}"
        assert not acts[:, 5:8].any()
        assert err_lp <= pc.TOL and err_en <= pc.TOL
    g = cg.vec.get_vec_sampler(N)(SEED)
    acts, logp, ent = run_sampler(g, view, masks, greedy=True)
    assert np.array_equal(acts[:, :5], first)
    assert np.abs(logp + logk).max() <= pc.TOL and np.abs(ent - logk).max() <= pc.TOL


@pytest.mark.parametrize("head", range(5))
def test_planted_draws(cg, head):
    """One-env samplers whose state makes head `head`'s draw u = 0 (x_new - 1 = 0 and 127), 1/4, 1/2,
    3/4 and 1 - 2^-24, on a head of four equally likely valid entries (prefix sums 1, 2, 3, 4, u Z
    exact): the first entry, entry j at u = j / 4 (C_j >= u Z would give entry j - 1, the draw of the
    next head a random entry), the last entry.  Then three equally likely entries at the odd
    u = 11184811 2^-24, where u Z = 2 + 2^-24 rounds to 2 and selects entry 2; a u short of its last
    bit gives entry 1.  The other heads of the same samplers follow the band rule against the float64
    reference.

    Measured on the MI355X: all 35 planted entries are the expected ones.  A build of the kernel with
    C_j >= u Z, and one with u short of its last bit, pass tests/test_gpu_policy_sampler.py and fail
    here."""
    rng = np.random.default_rng(50 + head)
    others = [h for h in range(5) if h != head]
    for (r, u, entry), count in [(d, 4) for d in pc.PLANTED_DRAWS] + [(pc.LAST_BIT_DRAW, 3)]:
        logits, masks, cols = pc.equal_row(rng, head, count)
        x = pc.state_for(head, r)
        smp = cg.vec.get_vec_sampler(1)(x)
        _, view, values = to_device(logits, ("f32", 92))
        acts, logp, ent = run_sampler(smp, view, masks)
        ref = pr.sample(values, masks, np.array([x], dtype=np.uint64))
        assert acts[0, head] == cols[entry], f"head {head}, u = {u}: entry {acts[0, head]}, not {cols[entry]} of {cols}"
        assert pr.legal(acts[:, :5], masks).all()
        differ = acts[:, :5].astype(np.int64) != ref["actions"]
        assert not (differ & ~ref["near"])[:, others].any(), f"head {head}, u = {u}: another head differs outside the band"
        if not differ.any():
            assert abs(logp[0] - ref["logp"][0]) <= pc.logp_allowance(ref["logp"][0])
        assert abs(ent[0] - ref["entropy"][0]) <= pc.TOL


@pytest.mark.parametrize("kind", KINDS, ids=kind_id)
@pytest.mark.parametrize("name", pc.FAMILIES)
def test_wide_families_sampler(cg, name, kind):
    """Two calls on one sampler per family and layout against the float64 reference: the index rule
    with its cap on the cases inside the band, legal actions, no NaN, the allowances above.

    Measured on the MI355X over the 15 cases: 3 of 38,550 indices inside the band, at most 1 of 1,285
    in a call; logp at most 1.9e-6 off (|logp| up to 16.6), entropy at most 1.9e-6."""
    rng = np.random.default_rng(1000 * pc.FAMILIES.index(name) + kind[1])
    smp = cg.vec.get_vec_sampler(N)(SEED)
    states = pr.sampler_states(SEED, N)
    skipped = cases = 0
    for call in range(2):
        logits, masks = pc.family_case(rng, N, name)
        _, view, values = to_device(logits, kind)
        acts, logp, ent = run_sampler(smp, view, masks)
        ref = pr.sample(values, masks, states)
        states = ref["states"]
        assert not np.isnan(ref["logp"]).any(), "a bad row in the reference"
        assert pr.legal(acts[:, :5], masks).all(), f"call {call}: illegal action"
        assert not acts[:, 5:8].any()
        s, c = check_sampler(ref, acts, logp, ent, f"{name} {kind_id(kind)} call {call}")
        skipped, cases = skipped + s, cases + c
    assert skipped <= max(1, cases // 100), f"{skipped} of {cases} cases fell inside the band"


@pytest.mark.parametrize("kind", KINDS, ids=kind_id)
@pytest.mark.parametrize("name", pc.FAMILIES)
def test_wide_families_evaluator(cg, name, kind):
    """Forward and backward with random incoming gradients, once with the sampler reference's actions
    and once with uniformly drawn legal ones (|logp| in the hundreds, p_a underflowed to 0 in float32),
    against the float64 reference: the allowances above, exact zeros in the columns of invalid entries
    and empty heads, no NaN.

    Measured on the MI355X over the 15 cases: logp at most 3.7e-5 off where |logp| reaches 629 (its
    allowance there: 3.1e-4) and at most 4.2e-6 where |logp| stays under 100; entropy at most 1.7e-6; a
    float32 gradient entry uses at most 2.5 % of its allowance, and every bfloat16 gradient entry
    equals the rounded reference."""
    rng = np.random.default_rng(2000 * pc.FAMILIES.index(name) + kind[1])
    logits, masks = pc.family_case(rng, N, name)
    g_lp, g_en = rng.normal(size=N).astype(np.float32), rng.normal(size=N).astype(np.float32)
    uniform = pc.uniform_legal_actions(rng, masks, logits)
    for label in ("sampled", "uniform"):
        if label == "sampled":
            actions = pr.sample(to_device(logits, kind)[2], masks, pr.sampler_states(SEED, N))["actions"]
        else:
            actions = uniform
        values, logp, ent, grad = run_evaluator(cg, logits, kind, actions, masks, g_lp, g_en)
        ref = per.evaluate(values, actions, masks, g_lp, g_en)
        assert np.isfinite(ref["logp"]).all()
        check_evaluator(kind, ref, masks, g_lp, g_en, logp, ent, grad, f"{name} {kind_id(kind)} {label} actions")
    if name == "spread":
        assert (np.abs(ref["logp"]) > 100).any(), "spread has lost its unlikely recorded actions"


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_recorded_action_on_a_valid_minus_inf_entry(cg, dt):
    """Rows at both ends of a tile whose recorded action of head 1 is a valid entry holding -inf, beside
    three finite valid entries: logp is -inf exactly (not NaN), the row is not bad, entropy and the
    gradient row follow the reference (g_lp at the action, finite everywhere); the other rows are
    bit-equal to a run without the planted entries.

    Measured on the MI355X: logp is -inf on the six rows in both types; entropy at most 8.4e-7 off; a
    float32 gradient entry uses at most 1.9 % of its allowance, every bfloat16 one equals the rounded
    reference."""
    rng = np.random.default_rng(61)
    kind = (dt, 92)
    rows = np.array([0, 63, 64, 127, 128, 256])
    logits, masks = pr.random_logits(rng, N), pr.random_masks(rng, N)
    actions = pr.sample(to_device(logits, kind)[2], masks, pr.sampler_states(SEED, N))["actions"]
    masks[rows, 22:44] = 0
    masks[rows[:, None], [24, 27, 31, 43]] = 1
    actions[rows, 1] = 2
    g_lp, g_en = rng.normal(size=N).astype(np.float32), rng.normal(size=N).astype(np.float32)
    _, lp0, en0, g0 = run_evaluator(cg, logits, kind, actions, masks, g_lp, g_en)
    assert np.isfinite(lp0).all()
    logits[rows, 31] = -np.inf
    actions[rows, 1] = 9
    values, lp1, en1, g1 = run_evaluator(cg, logits, kind, actions, masks, g_lp, g_en)
    ref = per.evaluate(values, actions, masks, g_lp, g_en)
    assert not ref["bad"].any() and (ref["logp"][rows] == -np.inf).all()
    assert (lp1[rows] == -np.inf).all(), f"logp of the planted rows: {lp1[rows]}"
    check_evaluator(kind, ref, masks, g_lp, g_en, lp1, en1, g1, f"-inf action {dt}")
    assert np.isfinite(g1).all() and np.isfinite(en1).all()
    # p_a is exactly 0 there, so the entry is g_lp (1 - 0) - g_en (0 (d_a - c)) = g_lp with no rounding
    assert np.array_equal(ref["grad"][rows, 31], g_lp[rows].astype(np.float64))
    assert np.array_equal(g1[rows, 31], per.bf16_round(g_lp[rows]) if dt == "bf16" else g_lp[rows])
    good = np.setdiff1d(np.arange(N), rows)
    assert np.array_equal(lp0[good], lp1[good]) and np.array_equal(en0[good], en1[good]) and np.array_equal(g0[good], g1[good])


def test_any_non_zero_mask_byte_is_valid(cg):
    """Every non-zero mask byte replaced by a value from 1..255, with 0x80, 0x7f, 0xff and 0 next to
    one another within a dword: the sampler (same seed) and the evaluator (forward and gradient) are
    bit-equal to the run with those bytes set to 1, for float32 and bfloat16.

    Measured on the MI355X: bit-equal.  A build of nonzero_bytes without its top-bit term passes the
    two older policy test files and fails here."""
    rng = np.random.default_rng(71)
    logits = pr.random_logits(rng, N)
    alt = pc.any_nonzero_bytes(rng, pr.random_masks(rng, N))
    ones = pc.as_ones(alt)
    assert (alt[:, :92] != ones[:, :92]).any() and np.array_equal(alt[:, :92] != 0, ones[:, :92] != 0)
    g_lp, g_en = rng.normal(size=N).astype(np.float32), rng.normal(size=N).astype(np.float32)
    for kind in (("f32", 92), ("bf16", 92)):
        out = []
        for masks in (ones, alt):
            smp = cg.vec.get_vec_sampler(N)(SEED)
            _, view, values = to_device(logits, kind)
            acts, logp, ent = run_sampler(smp, view, masks)
            assert pr.legal(acts[:, :5], masks).all()
            ev = run_evaluator(cg, logits, kind, acts[:, :5], masks, g_lp, g_en)
            out.append((acts[:, :8], logp, ent) + ev[1:])
        for a, b in zip(*out):
            assert np.array_equal(a, b, equal_nan=True), kind
        ref = pr.sample(values, ones, pr.sampler_states(SEED, N))
        check_sampler(ref, *out[1][:3], f"mask bytes {kind_id(kind)}")


@pytest.mark.parametrize("players", [2, 3, 1])
def test_stored_masks_of_fewer_players(cg, players):
    """20 steps of sample_policy(logits, env, "stored") -> step_device with 2, 3 and 1 players: the actions
    are legal under the current agent's stored mask as it was before the step and follow the index
    rule; every player takes a turn within the 20 steps.

    Measured on the MI355X: agents 0..players-1 all seen, none of the 6,400 indices inside the band."""
    import torch

    import pyoracle as po
    n, seed, steps = 64, 37 + players, 20
    env = cg.vec.get_vec_env(n)()
    smp = cg.vec.get_vec_sampler(n)(SEED)
    env.reset(seed, players, 3, cg.HARD, 100000, False)
    gen = torch.Generator(device="cuda").manual_seed(players)
    states = pr.sampler_states(SEED, n)
    skipped = cases = 0
    agents = set()
    for t in range(steps):
        agents |= set(np.asarray(env.agent_selection).astype(np.int64).tolist())
        before = po.stored_masks(env).view(np.uint8).reshape(n, 128)
        logits = torch.randn((n, 92), generator=gen, device="cuda") * 3
        actions, logp, ent = smp.sample_policy(logits, env, "stored")
        env.step_device(actions.data_ptr())
        env.sync_host()
        acts = actions.cpu().numpy()
        assert pr.legal(acts[:, :5], before).all(), f"step {t}: illegal action"
        ref = pr.sample(logits.cpu().numpy(), before, states)
        states = ref["states"]
        differ = (acts[:, :5] != ref["actions"]) & ~ref["near"]
        assert not differ.any(), f"step {t}: index differs outside the band at {np.argwhere(differ)[0]}"
        same = ~(acts[:, :5] != ref["actions"]).any(1)
        assert (np.abs(logp.cpu().numpy() - ref["logp"]) <= pc.logp_allowance(ref["logp"]))[same].all()
        skipped, cases = skipped + int(ref["near"].sum()), cases + differ.size
    print(f"{players} players: agents {sorted(agents)}, in the band {skipped}/{cases}")
    assert skipped <= max(1, cases // 100)
    assert agents == set(range(players)), f"agents seen: {sorted(agents)}: the test lost its case"
