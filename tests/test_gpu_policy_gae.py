"""GPU: the per-seat advantage estimator (city_of_gold.turn_gae, cog_policy_gae, k_turn_gae) against
the float64 recursion in tests/gae_ref.py.

TOL is gae_ref.TOL: 4 times the largest |float32 - float64| of the recursion over this file's own
inputs, measured and pinned by tests/test_policy_gae_cpu.py (the factor covers the kernel contracting
to FMAs and associating differently from numpy)."""
import numpy as np
import pytest

import gae_ref as gr

pytestmark = pytest.mark.gpu

TOL = gr.TOL


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run(cg, values, agents, rewards, dones, last_values=None, **kw):
    """turn_gae on numpy inputs: (advantages, returns) as numpy."""
    a, r = cg.turn_gae(dev(values), dev(agents), dev(rewards), dev(dones),
                       None if last_values is None else dev(last_values), **kw)
    assert a.shape == values.shape and r.shape == values.shape and a.is_contiguous() and r.is_contiguous()
    assert str(a.dtype) == "torch.float32" and str(r.dtype) == "torch.float32" and not a.requires_grad
    return a.cpu().numpy(), r.cpu().numpy()


def assert_close(got, want, label):
    err = max(np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max())
    print(f"{label}: max error {err:.3g} (TOL {TOL:.3g}), max |adv| {np.abs(want[0]).max():.3g}")
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all(), label
    assert err <= TOL, label


@pytest.mark.parametrize("params", gr.PARAMS, ids=lambda p: f"gamma{p[0]}-lam{p[1]}")
@pytest.mark.parametrize("shape", gr.SHAPES, ids=lambda s: f"T{s[0]}-n{s[1]}")
def test_random_windows(cg, shape, params):
    w = gr.case(*shape)
    gamma, lam = params
    assert np.isnan(w["rewards"][w["dones"] == 0]).all()
    got = run(cg, *gr.arrays(w), w["last_values"], gamma=gamma, lam=lam)
    assert_close(got, gr.scan(*gr.arrays(w), w["last_values"], gamma, lam), f"T={shape[0]} n={shape[1]} {params}")


def test_random_windows_hold_their_cases():
    seen = {}
    for T, n in gr.SHAPES:
        for k, v in gr.features(gr.case(T, n)).items():
            seen[k] = seen.get(k, False) or v
    assert all(seen.values()), seen


@pytest.mark.parametrize("shape", ((512, 64), (128, 300), (9, 65)), ids=lambda s: f"T{s[0]}-n{s[1]}")
def test_exact_on_small_integers(cg, shape):
    """gamma = lam = 1, integers in [-8, 8]: every float32 operation is exact, so the kernel gives the
    float64 reference's values bit for bit."""
    w = gr.case(*shape, integers=True)
    got = run(cg, *gr.arrays(w), w["last_values"], gamma=1.0, lam=1.0)
    want = gr.scan(*gr.arrays(w), w["last_values"], 1.0, 1.0)
    assert max(np.abs(want[0]).max(), np.abs(want[1]).max()) < 2 ** 24
    assert np.array_equal(got[0], want[0].astype(np.float32)) and np.array_equal(got[0].astype(np.float64), want[0])
    assert np.array_equal(got[1].astype(np.float64), want[1])


def test_hand_written_window(cg):
    """One env.  Rows 4 and 5 (seat 1) bootstrap from last_values[0, 1] = 8; the done at row 3 gives
    seat 0 its reward 10 at row 3 and seat 1 its reward 20 at row 2, both with nothing behind them;
    rows 1 and 0 (seat 0) chain to row 3.  gamma = lam = 0.5, so gamma lam = 0.25:
      t=5: delta = 0.5 * 8 - 6 = -2                     A = -2
      t=4: delta = 0.5 * 6 - 5 = -2                     A = -2 + 0.25 * -2 = -2.5
      t=3: delta = 10 - 4 = 6                           A = 6
      t=2: delta = 20 - 3 = 17                          A = 17
      t=1: delta = 0.5 * 4 - 2 = 0                      A = 0.25 * 6 = 1.5
      t=0: delta = 0.5 * 2 - 1 = 0                      A = 0.25 * 1.5 = 0.375"""
    values = np.array([1, 2, 3, 4, 5, 6], dtype=np.float32)[:, None]
    agents = np.array([0, 0, 1, 0, 1, 1], dtype=np.uint8)[:, None]
    dones = np.array([0, 0, 0, 1, 0, 0], dtype=np.uint8)[:, None]
    rewards = np.full((6, 1, 4), np.nan, dtype=np.float32)
    rewards[3, 0] = (10, 20, 30, 40)
    last = np.array([[7, 8, 9, 10]], dtype=np.float32)
    a, r = run(cg, values, agents, rewards, dones, last, gamma=0.5, lam=0.5)
    assert a[:, 0].tolist() == [0.375, 1.5, 17.0, 6.0, -2.5, -2.0]
    assert r[:, 0].tolist() == [1.375, 3.5, 20.0, 10.0, 2.5, 4.0]


def test_last_values(cg):
    w = gr.case(128, 300)
    T, n = w["values"].shape
    base = run(cg, *gr.arrays(w), w["last_values"])
    none = run(cg, *gr.arrays(w), None)
    zeros = run(cg, *gr.arrays(w), np.zeros((n, 4), dtype=np.float32))
    assert np.array_equal(none[0], zeros[0]) and np.array_equal(none[1], zeros[1])
    last_done = gr.last_done_row(w["dones"])
    seat = w["agents"] & 3
    rows = np.arange(T)[:, None]
    changed_some, absent_some = 0, 0
    for i, p in ((0, 0), (7, 1), (63, 0), (64, 1), (150, 2), (299, 0), (299, 3), (10, 3), (11, 2)):
        lv = w["last_values"].copy()
        lv[i, p] += 3.0
        got = run(cg, *gr.arrays(w), lv)
        diff = (got[0] != base[0]) | (got[1] != base[1])
        want = np.zeros((T, n), dtype=bool)
        want[:, i] = (seat[:, i] == p) & (rows[:, 0] > last_done[i])
        assert np.array_equal(diff, want), f"last_values[{i}, {p}]: the rows that change are not seat {p}'s tail rows"
        changed_some += int(want.any())
        absent_some += int(not want.any())
    assert changed_some >= 3 and absent_some >= 1, "the test lost its cases (a seat in the tail / a seat absent from it)"


def test_strided_inputs(cg):
    """[:, :n] views of (T, n + 5) buffers, rewards with a row stride of 4 n + 8 floats, dones as bool,
    agent bytes with high bits set: the contiguous call's bits, the padding untouched."""
    import torch
    w = gr.case(33, 200)
    T, n = w["values"].shape
    lv = dev(w["last_values"])
    base = cg.turn_gae(dev(w["values"]), dev(w["agents"]), dev(w["rewards"]), dev(w["dones"]), lv)
    vbuf = torch.full((T, n + 5), float("nan"), device="cuda")
    abuf = torch.full((T, n + 5), 0xEE, dtype=torch.uint8, device="cuda")
    dbuf = torch.full((T, n + 5), 1, dtype=torch.uint8, device="cuda")
    rbuf = torch.full((T + 2, 4 * n + 8), float("inf"), device="cuda")
    vbuf[:, :n], abuf[:, :n], dbuf[:, :n] = dev(w["values"]), dev(w["agents"]), dev(w["dones"])
    rbuf[:T, :4 * n] = dev(w["rewards"]).view(T, 4 * n)
    rview = rbuf[:T, :4 * n].view(T, n, 4)
    assert rview.stride() == (4 * n + 8, 4, 1) and vbuf[:, :n].stride() == (n + 5, 1)
    keep = [b.clone() for b in (vbuf, abuf, dbuf, rbuf)]
    got = cg.turn_gae(vbuf[:, :n], abuf[:, :n], rview, dbuf[:, :n], lv)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    for b, k in zip((vbuf, abuf, dbuf, rbuf), keep):
        assert torch.equal(b.view(torch.uint8), k.view(torch.uint8))
    as_bool = cg.turn_gae(vbuf[:, :n], abuf[:, :n], rview, dbuf[:, :n] != 0, lv)
    assert (dbuf[:, :n] != 0).dtype == torch.bool
    assert torch.equal(as_bool[0], base[0]) and torch.equal(as_bool[1], base[1])
    high = cg.turn_gae(vbuf[:, :n], abuf[:, :n] | 0x40, rview, dbuf[:, :n], lv)
    assert torch.equal(high[0], base[0]) and torch.equal(high[1], base[1])
    done_bytes = cg.turn_gae(dev(w["values"]), dev(w["agents"]), dev(w["rewards"]), dev(w["dones"]) * 0x80, lv)
    assert torch.equal(done_bytes[0], base[0])                          # any non-zero byte is a done
    assert_close((got[0].cpu().numpy(), got[1].cpu().numpy()), gr.scan(*gr.arrays(w), w["last_values"]), "strided")


def test_deterministic_and_ordered_on_a_side_stream(cg):
    """Two calls give the same bits; a call queued on a side stream behind a kernel that writes
    `values` on that stream sees the written values, with no explicit synchronize."""
    import torch
    w = gr.case(128, 300)
    args = [dev(x) for x in gr.arrays(w)]
    lv = dev(w["last_values"])
    one, two = cg.turn_gae(*args, lv), cg.turn_gae(*args, lv)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    m = torch.randn(2048, 2048, device="cuda")
    values = torch.zeros_like(args[0])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(20):                                # work ahead of the values on the side stream
            m = torch.tanh(m @ m)
        values.copy_(args[0] + m[0, 0] * 0.0)              # (queued behind the matmuls; the same values)
        got = cg.turn_gae(values, *args[1:], lv)
        got = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.array_equal(got[0], one[0].cpu().numpy()) and np.array_equal(got[1], one[1].cpu().numpy())
    torch.cuda.synchronize()


def record_engine(cg, players):
    """T steps of the engine, one per runner call, under the full dynamics: agent_selection before
    each step, dones and rewards after it, as clones of the device views."""
    import torch
    n, T = gr.REC["n"], gr.REC["T"]
    env = cg.vec.get_vec_env(n)()
    smp = cg.vec.get_vec_sampler(n)(gr.REC["sampler_seed"])
    env.reset(gr.rec(players)["reset_seed"], players, gr.REC["pieces"], cg.HARD, gr.rec(players)["max_steps"], False)
    runner = cg.vec.get_runner(n)(env, smp, None, device_views=True, stored_masks=True)
    views = cg.device_tensors(env)
    agents, dones, rewards = [], [], []
    for _ in range(T):
        agents.append(views["agent_selection"].clone())
        torch.cuda.synchronize()                           # (the step overwrites the views on the engine's stream)
        runner.rollout(1)
        runner.sync()
        dones.append(views["dones"].clone())
        rewards.append(views["rewards"].clone())
    torch.cuda.synchronize()
    return torch.stack(agents), torch.stack(dones), torch.stack(rewards)


@pytest.mark.parametrize("players", (4, 3, 2, 1))
def test_recorded_from_the_engine(cg, players):
    import torch
    orc = gr.oracle_window(players)
    gr.check_oracle_window(orc, players)
    agents, dones, rewards = record_engine(cg, players)
    n, T = gr.REC["n"], gr.REC["T"]
    assert agents.shape == (T, n) and agents.dtype == torch.uint8 and dones.shape == (T, n) and rewards.shape == (T, n, 4)
    assert np.array_equal(agents.cpu().numpy(), orc["agents"]) and np.array_equal(dones.cpu().numpy() != 0, orc["dones"] != 0)
    assert np.array_equal(rewards.cpu().numpy(), orc["rewards"])
    c = gr.recorded_case(players)
    values, lv = dev(c["values"]), dev(c["last_values"])
    # (a) the rewards as recorded (all zero): a bootstrapped value crosses a done only through a bug
    a, r = cg.turn_gae(values, agents, rewards, dones, lv)
    want = gr.scan(c["values"], orc["agents"], orc["rewards"], orc["dones"], c["last_values"])
    err = max(np.abs(a.cpu().numpy() - want[0]).max(), np.abs(r.cpu().numpy() - want[1]).max())
    assert err <= TOL, err
    a100, r100 = cg.turn_gae(values, agents, rewards, dones, lv * 100)
    before = dev(np.arange(T)[:, None] <= gr.last_done_row(orc["dones"])[None, :])
    assert before.any(1).all() and not before.all()
    assert torch.equal(a100[before], a[before]) and torch.equal(r100[before], r[before])
    assert not torch.equal(a100, a)
    # (b) random rewards on the done rows, NaN elsewhere
    got = cg.turn_gae(values, agents, dev(c["planted"]), dones, lv)
    assert_close((got[0].cpu().numpy(), got[1].cpu().numpy()),
                 gr.scan(c["values"], c["agents"], c["planted"], c["dones"], c["last_values"]), f"recorded, {players} players")


def test_errors_name_the_cause(cg):
    import torch
    T, n = 6, 64
    v = torch.zeros((T, n), device="cuda")
    a = torch.zeros((T, n), dtype=torch.uint8, device="cuda")
    d = torch.zeros((T, n), dtype=torch.uint8, device="cuda")
    r = torch.zeros((T, n, 4), device="cuda")
    lv = torch.zeros((n, 4), device="cuda")
    gae = cg.turn_gae
    gae(v, a, r, d, lv)
    for bad in (v[0], v[:, :, None], v[:, :-1]):
        with pytest.raises(ValueError, match="shape"):
            gae(bad, a, r, d, lv)
    for bad in (a[:-1], a[:, :-1], a[0]):
        with pytest.raises(ValueError, match="shape"):
            gae(v, bad, r, d, lv)
    for bad in (r[:, :, :3], r[:-1], r[:, :, 0], r.view(T, n * 4)):
        with pytest.raises(ValueError, match="shape"):
            gae(v, a, bad, d, lv)
    for bad in (d[:-1], d[:, :-1], d[:, :, None]):
        with pytest.raises(ValueError, match="shape"):
            gae(v, a, r, bad, lv)
    for bad in (lv[:, 0], lv[:-1], lv[:, :3], torch.zeros(n, device="cuda")):
        with pytest.raises(ValueError, match="shape"):
            gae(v, a, r, d, bad)
    for bad in (v.double(), v.half(), v.bfloat16()):
        with pytest.raises(ValueError, match="dtype"):
            gae(bad, a, r, d, lv)
    with pytest.raises(ValueError, match="dtype"):
        gae(v, a.to(torch.int32), r, d, lv)
    with pytest.raises(ValueError, match="dtype"):
        gae(v, a, r.double(), d, lv)
    with pytest.raises(ValueError, match="dtype"):
        gae(v, a, r, d.float(), lv)
    with pytest.raises(ValueError, match="dtype"):
        gae(v, a, r, d, lv.double())
    with pytest.raises(ValueError, match="stride"):
        gae(torch.zeros((n, T), device="cuda").t(), a, r, d, lv)
    with pytest.raises(ValueError, match="stride"):
        gae(v, torch.zeros((T, 2 * n), dtype=torch.uint8, device="cuda")[:, ::2], r, d, lv)
    with pytest.raises(ValueError, match="stride"):
        gae(v, a, r, torch.zeros((n, T), dtype=torch.uint8, device="cuda").t(), lv)
    with pytest.raises(ValueError, match="stride"):
        gae(v, a, torch.zeros((T, n, 8), device="cuda")[:, :, ::2], d, lv)
    with pytest.raises(ValueError, match="stride"):
        gae(v, a, torch.zeros((T, n, 8), device="cuda")[:, :, :4], d, lv)
    with pytest.raises(ValueError, match="aligned"):                    # rows 4 n + 2 floats apart
        gae(v, a, torch.zeros((T, 4 * n + 2), device="cuda")[:, :4 * n].view(T, n, 4), d, lv)
    with pytest.raises(ValueError, match="stride"):
        gae(v, a, r, d, torch.zeros((n, 8), device="cuda")[:, :4])
    with pytest.raises(ValueError, match="device"):
        gae(v.cpu(), a, r, d, lv)
    for k in range(1, 5):
        args = [v, a, r, d, lv]
        args[k] = args[k].cpu()
        with pytest.raises(ValueError, match="device"):
            gae(*args)
    if cg.device_count() > 1:
        with pytest.raises(ValueError, match="device"):
            gae(v, a.to("cuda:1"), r, d, lv)
        with pytest.raises(ValueError, match="device"):
            gae(v, a, r, d, lv.to("cuda:1"))
    with pytest.raises(ValueError, match="tensor"):
        gae(v.cpu().numpy(), a, r, d, lv)
    raw = cg._C.policy_gae_raw
    out = torch.zeros((2, T, n), device="cuda")
    ptrs = dict(d_values=v.data_ptr(), d_agents=a.data_ptr(), d_rewards=r.data_ptr(), d_dones=d.data_ptr(),
                d_advantages=out[0].data_ptr(), d_returns=out[1].data_ptr())
    lds = dict(values_ld=n, agents_ld=n, rewards_ld=4 * n, dones_ld=n)
    raw(T, n, **ptrs, **lds)
    for name in ptrs:
        with pytest.raises(ValueError, match="NULL"):
            raw(T, n, **{**ptrs, name: 0}, **lds)
    for name in lds:
        with pytest.raises(ValueError, match=name):
            raw(T, n, **ptrs, **{**lds, name: lds[name] - 1})
    with pytest.raises(ValueError, match="aligned"):
        raw(T, n, **ptrs, **{**lds, "rewards_ld": 4 * n + 2})
    with pytest.raises(ValueError, match="aligned"):
        raw(T, n, **{**ptrs, "d_rewards": r.data_ptr() + 4}, **lds)
    with pytest.raises(ValueError, match="aligned"):
        raw(T, n, **{**ptrs, "d_values": v.data_ptr() + 2}, **lds)
    with pytest.raises(ValueError, match="NO_STREAM"):
        raw(T, n, **ptrs, **lds, stream=-1)
    with pytest.raises(ValueError, match="device"):
        raw(T, n, **ptrs, **lds, device=cg.device_count())


def test_empty_windows_launch_nothing(cg):
    import torch
    raw = cg._C.policy_gae_raw
    raw(0, 64, 0, 64, 0, 64, 0, 256, 0, 64)                             # nothing launched, nothing to refuse
    raw(6, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    for T, n in ((0, 64), (6, 0), (0, 0)):
        a, r = cg.turn_gae(torch.zeros((T, n), device="cuda"), torch.zeros((T, n), dtype=torch.uint8, device="cuda"),
                           torch.zeros((T, n, 4), device="cuda"), torch.zeros((T, n), dtype=torch.bool, device="cuda"),
                           torch.zeros((n, 4), device="cuda"))
        assert a.shape == (T, n) and r.shape == (T, n) and a.dtype == torch.float32 and a.is_cuda
