"""GPU: the policy sampler (samplers.sample_policy, cog_sampler_sample_policy): masked categorical
actions, joint log-probability and entropy from logits, against the float64 numpy reference in
tests/policy_ref.py.

Index rule: for every (env, head) the kernel's index equals the float64 reference's unless some valid
prefix sum C_j lies within 1e-5 Z of u Z (float32 prefix-sum and exp rounding; the CPU test pins the
band); such cases are skipped and must stay under 1 % of all cases.  logp / entropy: 1e-5 absolute
for logits in [-8, 8] (float32 exp / log at 1-2 ulp plus the exponent's argument scaling over a
16-wide range: about 2e-6)."""
import numpy as np
import pytest

import policy_ref as pr

pytestmark = pytest.mark.gpu

TOL = 1e-5
SEED = 4242


def to_device(logits, kind):
    """kind: (dtype name, ld, element offset of the base).  Returns (the (n, 92) device view, the
    float32 values it holds)."""
    import torch
    dt, ld, off = kind
    n = logits.shape[0]
    t = torch.from_numpy(logits).cuda()
    if dt == "bf16":
        t = t.to(torch.bfloat16)
    buf = torch.full((off + n * ld + 8,), float("nan"), dtype=t.dtype, device="cuda")
    view = buf[off:off + n * ld].view(n, ld)[:, :92]
    view.copy_(t)
    return view, t.float().cpu().numpy()


def run(smp, view, masks_np, **kw):
    import torch
    d_masks = torch.from_numpy(masks_np).cuda()
    actions, logp, ent = smp.sample_policy(view, None, d_masks, **kw)
    return actions.cpu().numpy(), logp.cpu().numpy(), ent.cpu().numpy()


def check_against(ref, acts, logp, ent, label):
    """The index rule and the logp / entropy tolerance; returns (skipped, cases)."""
    differ = acts[:, :5].astype(np.int64) != ref["actions"]
    outside = differ & ~ref["near"]
    assert not outside.any(), f"{label}: {int(outside.sum())} indices differ outside the band, first at {np.argwhere(outside)[0]}"
    same = ~differ.any(1)
    err_lp = np.abs(logp.astype(np.float64) - ref["logp"])[same]
    err_en = np.abs(ent.astype(np.float64) - ref["entropy"])
    print(f"{label}: skipped {int(ref['near'].sum())}/{differ.size}, max |dlogp| {err_lp.max():.3g}, max |dentropy| {err_en.max():.3g}")
    assert err_lp.max() <= TOL, f"{label}: logp off by {err_lp.max()}"
    assert err_en.max() <= TOL, f"{label}: entropy off by {err_en.max()}"
    return int(ref["near"].sum()), differ.size


KINDS = [("f32", 92, 0), ("f32", 93, 0), ("f32", 128, 0), ("bf16", 92, 0)]


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: f"{k[0]}-ld{k[1]}")
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4096])
def test_sampled_index_logp_entropy(cg, n, kind):
    """Tests 1 and 2: two consecutive calls on one sampler (draws 1..5, then 6..10) against the
    float64 reference; the actions are legal; bytes 5..7 of each record are zero."""
    rng = np.random.default_rng(1000 * n + kind[1])
    smp = cg.vec.get_vec_sampler(n)(SEED)
    states = pr.sampler_states(SEED, n)
    skipped = cases = 0
    for call in range(2):
        logits, masks = pr.random_logits(rng, n), pr.random_masks(rng, n)
        view, values = to_device(logits, kind)
        acts, logp, ent = run(smp, view, masks)
        ref = pr.sample(values, masks, states)
        states = ref["states"]
        assert pr.legal(acts[:, :5], masks).all(), f"call {call}: illegal action"
        assert not acts[:, 5:8].any()
        s, c = check_against(ref, acts, logp, ent, f"n={n} {kind} call {call}")
        skipped, cases = skipped + s, cases + c
    assert skipped <= max(1, cases // 100), f"{skipped} of {cases} cases fell inside the band"


@pytest.mark.parametrize("kind", [("f32", 92, 0), ("bf16", 92, 0), ("bf16", 96, 0), ("f32", 92, 1), ("bf16", 92, 1)],
                         ids=lambda k: f"{k[0]}-ld{k[1]}-off{k[2]}")
def test_other_layouts_match(cg, kind):
    """Every staging path gives the same result: 16-B aligned bfloat16 rows (ld 96) and bases that
    are not 16-B aligned (the element-wise path), at a size with a partial tile."""
    n = 1000 + 37
    rng = np.random.default_rng(5)
    logits, masks = pr.random_logits(rng, n), pr.random_masks(rng, n)
    smp = cg.vec.get_vec_sampler(n)(SEED)
    view, values = to_device(logits, kind)
    acts, logp, ent = run(smp, view, masks)
    ref = pr.sample(values, masks, pr.sampler_states(SEED, n))
    assert pr.legal(acts[:, :5], masks).all()
    check_against(ref, acts, logp, ent, f"layout {kind}")


def test_greedy_is_exact_and_keeps_the_state(cg):
    """Test 3: argmax over the valid entries of the float32 values, ties to the lowest index (planted);
    no draw is consumed: a following sampling call uses draws 1..5."""
    n = 1000
    rng = np.random.default_rng(7)
    logits, masks = pr.random_logits(rng, n), pr.random_masks(rng, n)
    for off, k in pr.HEADS:                                  # ties: copy the head's maximum elsewhere
        rows = np.arange(0, n, 3)
        top = logits[rows, off:off + k].max(1)
        logits[rows, off + rng.integers(0, k, rows.size)] = top
        logits[rows, off + rng.integers(0, k, rows.size)] = top
    smp = cg.vec.get_vec_sampler(n)(SEED)
    for kind in (("f32", 92, 0), ("bf16", 92, 0)):
        view, values = to_device(logits, kind)
        acts, logp, ent = run(smp, view, masks, greedy=True)
        ref = pr.sample(values, masks, greedy=True)
        assert np.array_equal(acts[:, :5], ref["actions"]), kind
        for (off, k), h in zip(pr.HEADS, range(5)):          # numpy argmax on the float32 values
            lv = np.where(masks[:, off:off + k] != 0, values[:, off:off + k], -np.inf)
            some = (masks[:, off:off + k] != 0).any(1)
            assert np.array_equal(acts[:, h], np.where(some, lv.argmax(1), 0)), (kind, h)
        assert np.abs(logp - ref["logp"]).max() <= TOL and np.abs(ent - ref["entropy"]).max() <= TOL
    view, values = to_device(logits, ("f32", 92, 0))
    acts, logp, ent = run(smp, view, masks)
    ref = pr.sample(values, masks, pr.sampler_states(SEED, n))
    check_against(ref, acts, logp, ent, "sampling after greedy")


def test_non_finite_rows(cg):
    """Test 4: all-NaN, a +inf, all -inf on the valid entries: a legal action by the greedy rule, NaN
    logp and entropy for that env, its neighbours as in a run without the planted rows."""
    n = 300
    rng = np.random.default_rng(11)
    logits, masks = pr.random_logits(rng, n), pr.random_masks(rng, n)
    masks[:, :22] |= (rng.random((n, 22)) < 0.3).astype(np.uint8)
    masks[:, 5] = 1                                          # head 0 has valid entries everywhere
    planted = logits.copy()
    rows = {"nan": np.array([3, 64, 130]), "inf": np.array([10, 65, 200]), "ninf": np.array([17, 127, 299])}
    planted[rows["nan"]] = np.nan
    planted[rows["ninf"]] = -np.inf
    for i in rows["inf"]:
        valid = np.flatnonzero(masks[i, :22])
        planted[i, valid[-1]] = np.inf                       # (not the first valid entry)
    bad = np.concatenate(list(rows.values()))
    for kind in (("f32", 92, 0), ("bf16", 92, 0), ("f32", 93, 0)):
        out = []
        for lg in (logits, planted):
            smp = cg.vec.get_vec_sampler(n)(SEED)
            view, values = to_device(lg, kind)
            out.append(run(smp, view, masks) + (values,))
        (a0, lp0, en0, _), (a1, lp1, en1, values) = out
        assert pr.legal(a1[:, :5], masks).all(), kind
        ref = pr.sample(values, masks, pr.sampler_states(SEED, n))
        assert np.array_equal(a1[bad, 0], ref["actions"][bad, 0])
        greedy = pr.sample(values, masks, greedy=True)["actions"]
        assert np.array_equal(a1[rows["nan"], :5], greedy[rows["nan"]])       # every head degenerate
        assert np.array_equal(a1[rows["ninf"], :5], greedy[rows["ninf"]])
        assert np.array_equal(a1[rows["inf"], 0], greedy[rows["inf"], 0])
        assert np.isnan(lp1[bad]).all() and np.isnan(en1[bad]).all()
        good = np.setdiff1d(np.arange(n), bad)
        assert np.array_equal(a0[good], a1[good]) and np.array_equal(lp0[good], lp1[good])
        assert np.array_equal(en0[good], en1[good])
        assert not np.isnan(lp0).any() and not np.isnan(en0).any()
        g = cg.vec.get_vec_sampler(n)(SEED)                 # greedy mode on the same rows
        view, values = to_device(planted, kind)
        ag, lpg, eng = run(g, view, masks, greedy=True)
        assert np.array_equal(ag[:, :5], greedy) and np.isnan(lpg[bad]).all() and not np.isnan(lpg[good]).any()


def test_untouched_memory(cg):
    """Test 5: outputs inside the mask; record bytes past the first 8 unchanged; NaN in columns >= 92 of
    an ld = 128 buffer (to_device fills them) changes nothing against ld = 92."""
    import torch
    n = 777
    rng = np.random.default_rng(13)
    logits, masks = pr.random_logits(rng, n), pr.random_masks(rng, n)
    res = []
    for kind in (("f32", 92, 0), ("f32", 128, 0)):
        smp = cg.vec.get_vec_sampler(n)(SEED)
        rec = torch.from_dlpack(smp.dlpack())
        rec.fill_(0xAB)
        torch.cuda.synchronize()
        view, _ = to_device(logits, kind)
        actions, logp, ent = smp.sample_policy(view, None, torch.from_numpy(masks).cuda())
        assert actions.data_ptr() == rec.data_ptr() == smp.device_actions() and actions.shape == (n, 64)
        assert logp.shape == (n,) and logp.dtype == torch.float32 and ent.shape == (n,)
        a = actions.cpu().numpy()
        assert (a[:, 8:] == 0xAB).all() and not a[:, 5:8].any()
        assert pr.legal(a[:, :5], masks).all()
        res.append((a, logp.cpu().numpy(), ent.cpu().numpy()))
    for x, y in zip(res[0], res[1]):
        assert np.array_equal(x, y)
    assert not np.isnan(res[1][1]).any() and not np.isnan(res[1][2]).any()


def as_actions(po, rec):
    return np.ascontiguousarray(rec).view(po.ACTION).reshape(rec.shape[0])


@pytest.mark.parametrize("source,steps", [("stored", 140), ("selected", 30)])
def test_env_mask_sources(cg, source, steps):
    """Test 6: logits -> sample_policy(env's masks) -> step_device with no synchronize in the loop; the
    actions are legal under the masks as they were before the step and follow the index rule; an
    oracle stepped with the read-back actions stays equal to the engine.  140 steps with the stored
    masks: with max_steps 30 the first episodes of such a policy end between steps 90 and 130 (the
    same loop on the CPU oracle), and the auto-reset is part of what is checked."""
    import torch

    import pyoracle as po
    n, seed = 256, 31
    env = cg.vec.get_vec_env(n)()
    smp = cg.vec.get_vec_sampler(n)(SEED)
    orc = po.OracleVec(n)
    env.reset(seed, 4, 3, cg.HARD, 30, False)
    orc.reset(seed, 4, 3, 2, 30)
    gen = torch.Generator(device="cuda").manual_seed(1)
    states = pr.sampler_states(SEED, n)
    resets = skipped = cases = 0
    for t in range(steps):
        before = (po.stored_masks(env) if source == "stored" else env.selected_action_masks.copy())
        before = before.view(np.uint8).reshape(n, 128)
        logits = torch.randn((n, 92), generator=gen, device="cuda") * 3
        actions, logp, ent = smp.sample_policy(logits, env, source)
        env.step_device(actions.data_ptr())
        env.sync_host()
        acts = actions.cpu().numpy()
        assert pr.legal(acts[:, :5], before).all(), f"step {t}: illegal action"
        ref = pr.sample(logits.cpu().numpy(), before, states)
        states = ref["states"]
        differ = (acts[:, :5] != ref["actions"]) & ~ref["near"]
        assert not differ.any(), f"step {t}: index differs outside the band at {np.argwhere(differ)[0]}"
        skipped, cases = skipped + int(ref["near"].sum()), cases + differ.size
        orc.step(as_actions(po, acts))
        for nm in ("observations", "selected_action_masks", "infos"):
            bad = po.named_equal(getattr(env, nm), getattr(orc, nm))
            assert bad is None, f"{nm}.{bad} differs from the oracle at step {t}"
        resets += int(env.dones.sum())
    assert skipped <= max(1, cases // 100)
    if source == "stored":
        assert resets > 0, "no auto-reset: the test lost a case"


def test_orders_after_torch_stream(cg):
    """Test 7: the logits are overwritten on torch's stream behind a long matmul chain and
    sample_policy(greedy=True) is called at once; logp is read with no explicit synchronize."""
    import torch
    n = 4096
    rng = np.random.default_rng(17)
    new = pr.random_logits(rng, n)
    masks = np.ones((n, 128), dtype=np.uint8)
    smp = cg.vec.get_vec_sampler(n)(SEED)
    src = torch.from_numpy(new).pin_memory()
    d_logits = torch.zeros((n, 92), dtype=torch.float32, device="cuda")
    d_masks = torch.from_numpy(masks).cuda()
    m = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    for _ in range(30):                                    # ~tens of ms of work on torch's stream
        m = torch.tanh(m @ m)
    d_logits.copy_(src, non_blocking=True)                # queued behind the matmuls
    actions, logp, ent = smp.sample_policy(d_logits, None, d_masks, greedy=True)
    lp = logp.cpu().numpy()
    ref = pr.sample(new, masks, greedy=True)
    assert np.array_equal(actions.cpu().numpy()[:, :5], ref["actions"])
    assert np.abs(lp - ref["logp"]).max() <= TOL
    del m


def test_voids_a_speculative_sample(cg):
    """Test 8: after env.step(smp.get_actions()) has speculated the next uniform sample, sample_policy
    makes it stale: the next sample() launches afresh (no new hit) and its actions are legal."""
    import torch
    n = 256
    env = cg.vec.get_vec_env(n)()
    smp = cg.vec.get_vec_sampler(n)(SEED)
    env.reset(3, 4, 3, cg.HARD, 100000, False)
    masks, acts = env.selected_action_masks, smp.get_actions()
    for _ in range(6):
        smp.sample(masks)
        env.step(acts)
    samples, hits = smp.spec_stats()
    assert hits > 0, "the host loop never speculated: the test lost its case"
    logits = torch.zeros((n, 92), device="cuda")
    actions, _, _ = smp.sample_policy(logits, env)
    assert pr.legal(actions.cpu().numpy()[:, :5], masks.view(np.uint8).reshape(n, 128)).all()
    smp.sample(masks)
    assert smp.spec_stats() == (samples + 2, hits)
    assert pr.legal(np.ascontiguousarray(acts).view(np.uint8).reshape(n, 64)[:, :5], masks.view(np.uint8).reshape(n, 128)).all()
    env.step(acts)                                         # (and no speculation from now on: the device
    smp.sample(masks)                                      # actions are handed out)
    assert smp.spec_stats() == (samples + 3, hits)


def test_errors_name_the_cause(cg):
    """Test 9."""
    import torch
    n = 64
    smp = cg.vec.get_vec_sampler(n)(1)
    ok = torch.zeros((n, 92), device="cuda")
    d_masks = torch.ones((n, 128), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="shape"):
        smp.sample_policy(torch.zeros((n, 91), device="cuda"), None, d_masks)
    with pytest.raises(ValueError, match="shape"):
        smp.sample_policy(torch.zeros((n + 1, 92), device="cuda"), None, d_masks)
    with pytest.raises(ValueError, match="dtype"):
        smp.sample_policy(ok.half(), None, d_masks)
    with pytest.raises(ValueError, match="stride"):
        smp.sample_policy(torch.zeros((92, n), device="cuda").t(), None, d_masks)
    with pytest.raises(ValueError, match="stride"):
        smp.sample_policy(torch.zeros((n, 184), device="cuda")[:, ::2], None, d_masks)
    with pytest.raises(ValueError, match="device"):
        smp.sample_policy(torch.zeros((n, 92)), None, d_masks)
    with pytest.raises(ValueError, match="ld"):
        smp.sample_policy_raw(ok.data_ptr(), 0, 91, 2, None, d_masks.data_ptr())
    with pytest.raises(ValueError, match="dtype"):
        smp.sample_policy_raw(ok.data_ptr(), 7, 92, 2, None, d_masks.data_ptr())
    with pytest.raises(ValueError, match="mask source"):
        smp.sample_policy_raw(ok.data_ptr(), 0, 92, 5, None, d_masks.data_ptr())
    with pytest.raises(ValueError, match="NULL"):
        smp.sample_policy_raw(0, 0, 92, 2, None, d_masks.data_ptr())
    with pytest.raises(ValueError, match="NULL"):
        smp.sample_policy_raw(ok.data_ptr(), 0, 92, 2, None, 0)
    with pytest.raises(ValueError, match="needs"):
        smp.sample_policy(ok, None, "stored")
    with pytest.raises(ValueError, match="env"):
        smp.sample_policy_raw(ok.data_ptr(), 0, 92, 1, None, 0)
    with pytest.raises(ValueError, match="batch sizes"):
        smp.sample_policy(ok, cg.vec.get_vec_env(32)(), "selected")
    with pytest.raises(ValueError, match="shard"):
        cg.vec.get_vec_sampler(n)(1, device=[0, 0]).sample_policy(ok, None, d_masks)
    with pytest.raises(ValueError, match="shard"):
        cg.vec.get_vec_sampler(n)(1, device=[0, 0]).sample_policy_raw(ok.data_ptr(), 0, 92, 2, None, d_masks.data_ptr())
    with pytest.raises(ValueError, match="shard"):
        smp.sample_policy(ok, cg.vec.get_vec_env(n)(device=[0, 0]), "selected")
    assert smp.spec_stats()[0] == 0                        # no failed call counted as a sample
