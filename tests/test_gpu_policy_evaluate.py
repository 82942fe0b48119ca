"""GPU: the policy evaluator (city_of_gold.policy_evaluate, cog_policy_evaluate and its backward) and
city_of_gold.mask_records, against the float64 numpy reference in tests/policy_eval_ref.py.

Tolerances: float32 logits: 1e-5 on logp and entropy and 1e-5 (|g_lp| + |g_en|) on a gradient row
(tests/test_policy_evaluate_cpu.py pins them with the reference's own float32 mode).  bfloat16 logits:
the reference is taken from the widened logits and its gradient rounded to bfloat16; the allowance is
2^-8 |ref| (one rounding step of a neighbouring float32 value) plus the float32 tolerance."""
import numpy as np
import pytest

import policy_eval_ref as per
import policy_ref as pr

pytestmark = pytest.mark.gpu

TOL = 1e-5
SEED = 777


def to_device(logits, kind, requires_grad=True):
    """kind: (dtype name, ld, element offset of the base).  Returns (the leaf buffer, its (n, 92) view,
    the float32 values the view holds)."""
    import torch
    dt, ld, off = kind
    n = logits.shape[0]
    t = torch.from_numpy(logits).cuda()
    if dt == "bf16":
        t = t.to(torch.bfloat16)
    buf = torch.full((off + n * ld + 8,), float("nan"), dtype=t.dtype, device="cuda")
    with torch.no_grad():
        buf[off:off + n * ld].view(n, ld)[:, :92].copy_(t)
    buf.requires_grad_(requires_grad)
    view = buf[off:off + n * ld].view(n, ld)[:, :92]
    return buf, view, t.float().cpu().numpy()


def case(n, seed):
    """Random masks and logits, legal actions from the sampler reference, random incoming gradients."""
    rng = np.random.default_rng(seed)
    logits, masks = pr.random_logits(rng, n), pr.random_masks(rng, n)
    actions = pr.sample(logits, masks, pr.sampler_states(SEED, n))["actions"].astype(np.uint8)
    g_lp, g_en = rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)
    return logits, masks, actions, g_lp, g_en


def check(kind, n, values, masks, actions, g_lp, g_en, logp, ent, grad, label):
    """logp, ent, grad: numpy float32 results (grad (n, 92), widened when bfloat16)."""
    ref = per.evaluate(values, actions, masks, g_lp, g_en)
    assert not ref["bad"].any()
    err_lp, err_en = np.abs(logp - ref["logp"]).max(), np.abs(ent - ref["entropy"]).max()
    scale = np.zeros(n) if g_lp is None else np.abs(g_lp).astype(np.float64)
    scale = scale + (0 if g_en is None else np.abs(g_en))
    want = ref["grad"]
    allow = TOL * scale[:, None] * np.ones_like(want)
    if kind[0] == "bf16":
        want = per.bf16_round(want.astype(np.float32)).astype(np.float64)
        allow = allow + 2.0 ** -8 * np.abs(want)
    over = np.abs(grad - want) - allow
    print(f"{label}: max |dlogp| {err_lp:.3g}, |dentropy| {err_en:.3g}, grad error over allowance {over.max():.3g}")
    assert err_lp <= TOL and err_en <= TOL
    assert over.max() <= 0, f"{label}: gradient off at {np.unravel_index(over.argmax(), over.shape)}"
    zero = ~((masks[:, :92] != 0) & np.repeat(ref["nonempty"], [k for _, k in pr.HEADS], axis=1))
    assert not grad[zero].any(), f"{label}: a column of an invalid entry or an empty head is not exactly 0"
    return ref


KINDS = [("f32", 92, 0), ("f32", 96, 0), ("f32", 93, 0), ("f32", 92, 1), ("bf16", 92, 0), ("bf16", 96, 0), ("bf16", 93, 0)]


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: f"{k[0]}-ld{k[1]}-off{k[2]}")
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_forward_and_gradient(cg, n, kind):
    """Partial tiles, one full tile and more than one workgroup; the vector and the element-wise load
    forms; both incoming gradients, then each alone (logp.sum() and entropy.sum()).

    Measured on the MI355X: at most 1.4e-6 in logp, 7.6e-7 in entropy, and every float32 gradient
    entry at least 5.1e-7 inside its allowance.  A bfloat16 gradient entry that differs from the
    rounded reference at all is a whole bfloat16 step off, between 2^-8 and 2^-7 of |ref|, which the
    allowance of 2^-8 |ref| does not cover: the kernel has to round the same way as the reference,
    also where the exact value lies within 1e-7 of the midpoint of two bfloat16 values (5 of
    162,729 entries here, which a gradient computed in float32 got wrong).  It computes a bfloat16
    gradient in double, and every bfloat16 entry of these cases equals the rounded reference."""
    import torch
    logits, masks, actions, g_lp, g_en = case(n, 100 * n + kind[1] + kind[2])
    d_masks, d_actions = torch.from_numpy(masks).cuda(), torch.from_numpy(actions).cuda()
    buf, view, values = to_device(logits, kind)
    logp, ent = cg.policy_evaluate(view, d_actions, d_masks)
    assert logp.shape == (n,) and ent.shape == (n,) and logp.dtype == torch.float32 and ent.dtype == torch.float32
    torch.autograd.backward([logp, ent], [torch.from_numpy(g_lp).cuda(), torch.from_numpy(g_en).cuda()])
    off, ld = kind[2], kind[1]

    def grad_rows():
        g = buf.grad[off:off + n * ld].view(n, ld).float().cpu().numpy()
        assert not g[:, 92:].any() and not buf.grad[:off].any() and not buf.grad[off + n * ld:].any()
        return g[:, :92]
    assert buf.grad.dtype == buf.dtype
    check(kind, n, values, masks, actions, g_lp, g_en, logp.detach().cpu().numpy(), ent.detach().cpu().numpy(), grad_rows(),
          f"n={n} {kind}")
    ones = np.ones(n, dtype=np.float32)
    for which in ("logp", "entropy"):
        buf.grad = None
        lp, en = cg.policy_evaluate(view, d_actions, d_masks)
        (lp if which == "logp" else en).sum().backward()
        check(kind, n, values, masks, actions, ones if which == "logp" else None, ones if which == "entropy" else None,
              lp.detach().cpu().numpy(), en.detach().cpu().numpy(), grad_rows(), f"n={n} {kind} {which} alone")


def test_no_grad_runs_the_forward_only(cg):
    import torch
    n = 130
    logits, masks, actions, _, _ = case(n, 5)
    d_masks, d_actions = torch.from_numpy(masks).cuda(), torch.from_numpy(actions).cuda()
    x = torch.from_numpy(logits).cuda()
    lp0, en0 = cg.policy_evaluate(x, d_actions, d_masks)
    assert not lp0.requires_grad and not en0.requires_grad
    x.requires_grad_(True)
    with torch.no_grad():
        lp1, en1 = cg.policy_evaluate(x, d_actions, d_masks)
    assert not lp1.requires_grad
    lp2, en2 = cg.policy_evaluate(x, d_actions, d_masks)
    assert lp2.requires_grad and en2.requires_grad
    assert torch.equal(lp0, lp1) and torch.equal(lp0, lp2.detach()) and torch.equal(en0, en2.detach())
    lp2.mean().backward()                                  # (an expanded incoming gradient)
    g0 = x.grad.clone()
    x.grad = None
    lp3, _ = cg.policy_evaluate(x, d_actions, d_masks)
    lp3.mean().backward()
    assert torch.equal(g0, x.grad), "the gradient differs from run to run"


def test_against_torch_autograd(cg):
    """An independent check of the formula: masked log_softmax per head and gather in float64 torch
    ops, differentiated by torch."""
    import torch
    n = 257
    logits, masks, actions, g_lp, g_en = case(n, 7)
    d_masks, d_actions = torch.from_numpy(masks).cuda(), torch.from_numpy(actions).cuda()
    x = torch.from_numpy(logits).cuda().requires_grad_(True)
    logp, ent = cg.policy_evaluate(x, d_actions, d_masks)
    t_lp, t_en = torch.from_numpy(g_lp).cuda(), torch.from_numpy(g_en).cuda()
    torch.autograd.backward([logp, ent], [t_lp, t_en])
    x64 = torch.from_numpy(logits).cuda().double().requires_grad_(True)
    valid = d_masks[:, :92] != 0
    lp64 = torch.zeros(n, dtype=torch.float64, device="cuda")
    en64 = torch.zeros(n, dtype=torch.float64, device="cuda")
    for h, (off, k) in enumerate(pr.HEADS):
        v = valid[:, off:off + k]
        some = v.any(1)
        lh = x64[:, off:off + k].masked_fill(~v, float("-inf"))
        lh = torch.where(some[:, None], lh, torch.zeros_like(lh))
        lsm = torch.log_softmax(lh, 1)
        p = lsm.exp()
        a = d_actions[:, h].long()
        lp64 = lp64 + torch.where(some, lsm.gather(1, a[:, None]).squeeze(1), torch.zeros_like(lp64))
        plogp = torch.where(v & some[:, None], p * lsm.masked_fill(~v, 0.0), torch.zeros_like(p))
        en64 = en64 - plogp.sum(1)
    torch.autograd.backward([lp64, en64], [t_lp.double(), t_en.double()])
    assert (logp.double() - lp64).abs().max().item() <= TOL and (ent.double() - en64).abs().max().item() <= TOL
    scale = (t_lp.abs() + t_en.abs()).double()[:, None]
    assert ((x.grad.double() - x64.grad).abs() <= TOL * scale).all()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_agrees_with_the_sampler(cg, dt):
    """sample_policy then policy_evaluate on the same tensors: the sampler's own logp and entropy, with
    the (n, 64) action tensor itself, its [:, :5] view and a contiguous copy of that."""
    import torch
    n = 1000
    rng = np.random.default_rng(19)
    logits = torch.from_numpy(pr.random_logits(rng, n)).cuda()
    if dt == "bf16":
        logits = logits.to(torch.bfloat16)
    d_masks = torch.from_numpy(pr.random_masks(rng, n)).cuda()
    smp = cg.vec.get_vec_sampler(n)(SEED)
    actions, logp, ent = smp.sample_policy(logits, None, d_masks)
    for acts in (actions, actions[:, :5], actions[:, :5].contiguous()):
        lp, en = cg.policy_evaluate(logits, acts, d_masks)
        assert (lp - logp).abs().max().item() <= TOL and (en - ent).abs().max().item() <= TOL


@pytest.mark.parametrize("kind", [("f32", 92, 0), ("bf16", 92, 0), ("f32", 93, 0)], ids=lambda k: f"{k[0]}-ld{k[1]}")
def test_bad_rows(cg, kind):
    """+inf on a valid entry, a head of nothing but -inf / NaN, an action under a zero mask byte, an
    action byte past the head: NaN logp and entropy, an all-zero gradient row even with a NaN incoming
    gradient; the other rows as in a run without the planted rows."""
    import torch
    n = 150
    logits, masks, actions, g_lp, g_en = case(n, 23)
    rows = np.array([3, 10, 17, 24, 64, 127, 128, 149])
    masks[rows, :22] = 0
    masks[rows, 2:9] = 1
    actions[rows, 0] = 4
    out = []
    for planted in (False, True):
        lg, mk, ac, gl, ge = logits.copy(), masks.copy(), actions.copy(), g_lp.copy(), g_en.copy()
        if planted:
            lg[[3, 64], 6] = np.inf
            lg[[10, 127], 2:9] = -np.inf
            lg[[10, 127], 5] = np.nan
            mk[[17, 128], 4] = 0
            ac[[24, 149], 0] = 200
            gl[[3, 17, 127]] = np.nan
            ge[[10, 24, 64]] = np.nan
        buf, view, values = to_device(lg, kind)
        lp, en = cg.policy_evaluate(view, torch.from_numpy(ac).cuda(), torch.from_numpy(mk).cuda())
        torch.autograd.backward([lp, en], [torch.from_numpy(gl).cuda(), torch.from_numpy(ge).cuda()])
        g = buf.grad[:n * kind[1]].view(n, kind[1])[:, :92].float().cpu().numpy()
        out.append((lp.detach().cpu().numpy(), en.detach().cpu().numpy(), g))
        if planted:
            ref = per.evaluate(values, ac, mk, gl, ge)
            assert np.array_equal(np.flatnonzero(ref["bad"]), rows)
    (lp0, en0, g0), (lp1, en1, g1) = out
    assert np.isnan(lp1[rows]).all() and np.isnan(en1[rows]).all()
    assert not g1[rows].any() and not np.isnan(g1).any()
    good = np.setdiff1d(np.arange(n), rows)
    assert not np.isnan(lp0).any() and not np.isnan(en0).any()
    assert np.array_equal(lp0[good], lp1[good]) and np.array_equal(en0[good], en1[good])
    assert np.array_equal(g0[good], g1[good])


def test_padded_logits_leave_the_padding_zero(cg):
    import torch
    n = 100
    logits, masks, actions, g_lp, g_en = case(n, 29)
    leaf = torch.randn((n, 96), device="cuda")
    with torch.no_grad():
        leaf[:, :92] = torch.from_numpy(logits).cuda()
    leaf.requires_grad_(True)
    lp, en = cg.policy_evaluate(leaf[:, :92], torch.from_numpy(actions).cuda(), torch.from_numpy(masks).cuda())
    torch.autograd.backward([lp, en], [torch.from_numpy(g_lp).cuda(), torch.from_numpy(g_en).cuda()])
    assert leaf.grad.shape == (n, 96) and not leaf.grad[:, 92:].any().item()
    ref = per.evaluate(logits, actions, masks, g_lp, g_en)
    scale = (np.abs(g_lp) + np.abs(g_en)).astype(np.float64)[:, None]
    assert (np.abs(leaf.grad[:, :92].cpu().numpy() - ref["grad"]) <= TOL * scale).all()


def test_orders_on_a_side_stream(cg):
    """Logits produced by a torch op on a side stream, policy_evaluate and backward() inside the same
    block; the results are read with no explicit synchronize."""
    import torch
    n = 4096
    logits, masks, actions, g_lp, g_en = case(n, 31)
    d_masks, d_actions = torch.from_numpy(masks).cuda(), torch.from_numpy(actions).cuda()
    src = torch.from_numpy(logits).cuda().requires_grad_(True)
    m = torch.randn(2048, 2048, device="cuda")
    t_lp, t_en = torch.from_numpy(g_lp).cuda(), torch.from_numpy(g_en).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(20):                                # work ahead of the logits on the side stream
            m = torch.tanh(m @ m)
        x = src + m[0, 0] * 0.0                            # (queued behind the matmuls; the same values)
        lp, en = cg.policy_evaluate(x, d_actions, d_masks)
        torch.autograd.backward([lp, en], [t_lp, t_en])
        got = lp.detach().cpu().numpy(), en.detach().cpu().numpy(), src.grad.cpu().numpy()
    ref = per.evaluate(logits, actions, masks, g_lp, g_en)
    assert np.abs(got[0] - ref["logp"]).max() <= TOL and np.abs(got[1] - ref["entropy"]).max() <= TOL
    scale = (np.abs(g_lp) + np.abs(g_en)).astype(np.float64)[:, None]
    assert (np.abs(got[2] - ref["grad"]) <= TOL * scale).all()
    torch.cuda.synchronize()


def stored_masks_host(env, n):
    """observations[i].player_data[agent_selection[i]].action_mask as (n, 128) bytes, from the host views."""
    obs = np.ascontiguousarray(env.observations).view(np.uint8).reshape(n, 17216)
    agent = np.asarray(env.agent_selection).astype(np.int64)
    out = np.zeros((n, 128), dtype=np.uint8)
    for i in range(n):
        o = 16192 + 256 * agent[i] + 128
        out[i] = obs[i, o:o + 128]
    return out


def test_mask_records(cg):
    import pyoracle as po
    n = 64
    env = cg.vec.get_vec_env(n)()
    smp = cg.vec.get_vec_sampler(n)(SEED)
    env.reset(11, 4, 3, cg.HARD, 100000, False)
    masks, acts = env.selected_action_masks, smp.get_actions()
    for _ in range(6):
        smp.sample(masks)
        env.step(acts)
        sel = cg.mask_records(env, "selected")
        sto = cg.mask_records(env, "stored")
        assert sel.shape == (n, 128) and sel.dtype.is_floating_point is False and sel.is_contiguous() and sel.is_cuda
        assert sto.shape == (n, 128) and sto.is_contiguous()
        assert np.array_equal(sel.cpu().numpy(), np.ascontiguousarray(masks).view(np.uint8).reshape(n, 128))
        want = stored_masks_host(env, n)
        # (the oracle helper's copy of the same records: their 92 used bytes; a structured copy drops the padding)
        assert np.array_equal(want[:, :92], po.stored_masks(env).view(np.uint8).reshape(n, 128)[:, :92])
        assert np.array_equal(sto.cpu().numpy(), want)
    assert sel.data_ptr() != env.device_pointers(0)["selected_action_masks"]       # a copy
    with pytest.raises(ValueError, match="source"):
        cg.mask_records(env, "other")
    with pytest.raises(ValueError, match="shard"):
        cg.mask_records(cg.vec.get_vec_env(n)(device=[0, 0]))


def test_end_to_end_ratio_is_one(cg):
    """20 steps of mask_records -> sample_policy -> step_device on the stored masks, then one
    policy_evaluate over the 1,280 recorded rows with the same logits: the recorded logp (ratio 1 on
    the first epoch) and a finite gradient that sums to 0 over every non-empty head."""
    import torch
    n, steps = 64, 20
    env = cg.vec.get_vec_env(n)()
    smp = cg.vec.get_vec_sampler(n)(SEED)
    env.reset(5, 4, 3, cg.HARD, 100000, False)
    gen = torch.Generator(device="cuda").manual_seed(3)
    buf_l = torch.zeros((steps, n, 92), device="cuda")
    buf_m = torch.zeros((steps, n, 128), dtype=torch.uint8, device="cuda")
    buf_a = torch.zeros((steps, n, 5), dtype=torch.uint8, device="cuda")
    buf_lp = torch.zeros((steps, n), device="cuda")
    for t in range(steps):
        buf_l[t] = torch.randn((n, 92), generator=gen, device="cuda") * 3
        buf_m[t] = cg.mask_records(env, "stored")
        actions, logp, _ = smp.sample_policy(buf_l[t], env, "stored")
        buf_a[t], buf_lp[t] = actions[:, :5], logp
        env.step_device(actions.data_ptr())
    x = buf_l.view(-1, 92).clone().requires_grad_(True)
    a, m, old = buf_a.view(-1, 5), buf_m.view(-1, 128), buf_lp.view(-1)
    lp, en = cg.policy_evaluate(x, a, m)
    assert not torch.isnan(old).any() and (lp.detach() - old).abs().max().item() <= TOL
    assert ((lp.detach() - old).exp() - 1).abs().max().item() <= 2 * TOL
    g_lp = torch.randn(steps * n, generator=gen, device="cuda")
    g_en = torch.randn(steps * n, generator=gen, device="cuda")
    torch.autograd.backward([lp, en], [g_lp, g_en])
    assert torch.isfinite(x.grad).all()
    scale = (g_lp.abs() + g_en.abs()).double()
    valid = (m[:, :92] != 0)
    assert not x.grad[~valid].any()
    heads_seen = 0
    for off, k in pr.HEADS:
        s = x.grad[:, off:off + k].double().sum(1)
        assert (s.abs() <= TOL * scale).all()
        heads_seen += int(valid[:, off:off + k].any(1).sum())
    assert heads_seen > steps * n, "hardly a non-empty head: the test lost its case"


def test_errors_name_the_cause(cg):
    import torch
    n = 64
    ok = torch.zeros((n, 92), device="cuda")
    acts = torch.zeros((n, 5), dtype=torch.uint8, device="cuda")
    masks = torch.ones((n, 128), dtype=torch.uint8, device="cuda")
    ev = cg.policy_evaluate
    with pytest.raises(ValueError, match="shape"):
        ev(torch.zeros((n, 91), device="cuda"), acts, masks)
    with pytest.raises(ValueError, match="shape"):
        ev(torch.zeros((n, 2, 46), device="cuda"), acts, masks)
    with pytest.raises(ValueError, match="dtype"):
        ev(ok.half(), acts, masks)
    with pytest.raises(ValueError, match="stride"):
        ev(torch.zeros((92, n), device="cuda").t(), acts, masks)
    with pytest.raises(ValueError, match="stride"):
        ev(torch.zeros((n, 184), device="cuda")[:, ::2], acts, masks)
    with pytest.raises(ValueError, match="device"):
        ev(torch.zeros((n, 92)), acts, masks)
    with pytest.raises(ValueError, match="device"):
        ev(ok, acts.cpu(), masks)
    with pytest.raises(ValueError, match="device"):
        ev(ok, acts, masks.cpu())
    with pytest.raises(ValueError, match="shape"):
        ev(ok, acts[:, :4], masks)
    with pytest.raises(ValueError, match="shape"):
        ev(ok, acts[:-1], masks)
    with pytest.raises(ValueError, match="dtype"):
        ev(ok, acts.to(torch.int32), masks)
    with pytest.raises(ValueError, match="stride"):
        ev(ok, torch.zeros((n, 10), dtype=torch.uint8, device="cuda")[:, ::2], masks)
    with pytest.raises(ValueError, match="shape"):
        ev(ok, acts, masks[:, :127])
    with pytest.raises(ValueError, match="contiguous"):
        ev(ok, acts, torch.ones((n, 256), dtype=torch.uint8, device="cuda")[:, :128])
    with pytest.raises(ValueError, match="dtype"):
        ev(ok, acts, masks.to(torch.int8))
    with pytest.raises(ValueError, match="tensor"):
        ev(ok.cpu().numpy(), acts, masks)
    raw = cg._C.policy_evaluate_raw
    lp = torch.zeros(n, device="cuda")
    args = (acts.data_ptr(), 5, masks.data_ptr(), lp.data_ptr())
    with pytest.raises(ValueError, match="dtype"):
        raw(n, ok.data_ptr(), 7, 92, *args)
    with pytest.raises(ValueError, match="ld"):
        raw(n, ok.data_ptr(), 0, 91, *args)
    with pytest.raises(ValueError, match="NULL"):
        raw(n, 0, 0, 92, *args)
    with pytest.raises(ValueError, match="NULL"):
        raw(n, ok.data_ptr(), 0, 92, 0, 5, masks.data_ptr())
    with pytest.raises(ValueError, match="NULL"):
        raw(n, ok.data_ptr(), 0, 92, acts.data_ptr(), 5, 0)
    with pytest.raises(ValueError, match="action_stride"):
        raw(n, ok.data_ptr(), 0, 92, acts.data_ptr(), 4, masks.data_ptr())
    with pytest.raises(ValueError, match="aligned"):
        raw(n, ok.data_ptr(), 0, 92, acts.data_ptr(), 5, masks.data_ptr() + 8)
    with pytest.raises(ValueError, match="aligned"):
        raw(n, ok.data_ptr() + 2, 0, 92, *args)
    with pytest.raises(ValueError, match="NO_STREAM"):
        raw(n, ok.data_ptr(), 0, 92, *args, stream=-1)
    with pytest.raises(ValueError, match="NULL"):            # backward without a gradient output
        raw(n, ok.data_ptr(), 0, 92, acts.data_ptr(), 5, masks.data_ptr(), backward=True)
    with pytest.raises(ValueError, match="aligned"):
        raw(n, ok.data_ptr(), 0, 92, acts.data_ptr(), 5, masks.data_ptr(), d_grad_logits=ok.data_ptr() + 4, backward=True)
    raw(0, 0, 0, 92, 0, 5, 0)                                # n == 0: nothing launched, nothing to refuse
    e = torch.zeros((0, 92), device="cuda", requires_grad=True)
    lp0, en0 = ev(e, acts[:0], masks[:0])
    assert lp0.shape == (0,) and en0.shape == (0,)
    lp0.sum().backward()
    assert e.grad.shape == (0, 92)
