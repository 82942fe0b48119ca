"""GPU: city_of_gold.policy_features (cog_env_policy_features, k_policy_features) against the numpy
reference in tests/policy_features_ref.py, bit for bit in float32 and in bfloat16.  The reference is
computed from a C oracle driven in step with the engine (same seeds, the same masks sampled), from
the oracle's published records and player cells; tests/test_policy_features_cpu.py asserts from the
oracle that these runs reach what the cases need."""
import ctypes as C
import os

import numpy as np
import pytest

import driver_cases as dc
import policy_features_ref as fr
import pyoracle as po

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gym-eldorado_amd", "city_of_gold", "libcog_hip.so")
FIELDS, PLAIN = dc.FIELDS, dc.PLAIN


def dtypes():
    import torch
    return (torch.float32, torch.bfloat16)


def bits(t):
    """A result tensor's bit patterns as numpy (uint32 for float32, uint16 for bfloat16)."""
    import torch
    if t.dtype == torch.float32:
        return t.detach().cpu().numpy().view(np.uint32)
    return t.detach().view(torch.int16).cpu().numpy().view(np.uint16)


def want_bits(x, dtype):
    import torch
    return np.ascontiguousarray(x).view(np.uint32) if dtype == torch.float32 else fr.to_bf16_bits(x)


def assert_equal(got, want, dtype, label):
    """got: the (vec, local) tensors; want: the float32 reference pair."""
    n, W = want[0].shape[0], want[1].shape[-1]
    assert tuple(got[0].shape) == (n, fr.VEC) and tuple(got[1].shape) == (n, fr.CHANNELS, W, W), label
    for name, g, w in zip(("vec", "local"), got, want):
        assert g.dtype == dtype and g.is_contiguous() and g.is_cuda, (label, name)
        gb, wb = bits(g), want_bits(w, dtype)
        if not np.array_equal(gb, wb):
            i = np.argwhere(gb != wb)[0]
            raise AssertionError(f"{label}: {name} {dtype} differs from the reference, first at {tuple(int(k) for k in i)}: "
                                 f"bits {int(gb[tuple(i)]):#x}, reference {int(wb[tuple(i)]):#x} ({float(w[tuple(i)])})")


def check(cg, env, want, radius, label, **kw):
    for dtype in dtypes():
        assert_equal(cg.policy_features(env, radius, dtype=dtype, **kw), want, dtype, label)


def make(cg, run, n=None, players=None):
    """An engine (env, sampler) and the oracle pair, reset alike."""
    n = run["n"] if n is None else n
    players = run["players"] if players is None else players
    env, smp = cg.vec.get_vec_env(n)(device=0), cg.vec.get_vec_sampler(n)(run["sampler_seed"], device=0)
    env.reset(run["seed"], players, run["pieces"], cg.Difficulty(run["difficulty"]), 100000, False)
    orc, osm = fr.oracle_pair(run, n, players)
    return env, smp, orc, osm


def host_step(env, smp, orc, osm):
    smp.sample(po.stored_masks(env))
    env.step(smp.get_actions())
    osm.sample(po.stored_masks(orc))
    orc.step(osm.actions)


def assert_views(env, orc, label):
    for nm in FIELDS:
        bad = po.named_equal(getattr(env, nm), getattr(orc, nm))
        assert bad is None, f"{label}: {nm}.{bad} differs from the oracle"
    for nm in PLAIN:
        assert np.array_equal(np.asarray(getattr(env, nm)), np.asarray(getattr(orc, nm))), f"{label}: {nm} differs"


@pytest.mark.parametrize("n", (1, 3, 65, 130))
@pytest.mark.parametrize("players", (4, 3, 2, 1))
def test_after_reset(cg, players, n):
    env, _, orc, _ = make(cg, fr.RUN_A, n, players)
    for radius in (0, 1, 4):
        check(cg, env, fr.oracle_features(orc, players, radius), radius, f"{players} players, n {n}, radius {radius}")


def test_along_run_a_host_loop(cg):
    env, smp, orc, osm = make(cg, fr.RUN_A)
    for t in range(max(fr.RUN_A_CHECKS) + 1):
        if t:
            host_step(env, smp, orc, osm)
        if t in fr.RUN_A_CHECKS:
            for radius in (1, 4):
                check(cg, env, fr.oracle_features(orc, 4, radius), radius, f"run A step {t}, radius {radius}")
    assert_views(env, orc, "run A")


def test_along_run_a_device_loop(cg):
    """sample_policy on the stored masks -> step_device -> policy_features with no host
    synchronisation between them, the next step queued behind the kernel; every result is read at the
    end.  The oracle takes the numpy mirror of the greedy choice (tests/driver_cases.py, driver G)."""
    import torch
    env, smp, orc, _ = make(cg, fr.RUN_A)
    n = fr.RUN_A["n"]
    logits_np = dc.logits_table(n)
    logits = torch.from_numpy(logits_np).cuda()
    pending = []

    def features(t):
        want = fr.oracle_features(orc, 4, 4)
        for dtype in dtypes():
            pending.append((t, dtype, cg.policy_features(env, 4, dtype=dtype), want))
    features(0)
    for t in range(1, max(fr.RUN_A_CHECKS) + 1):
        acts, _, _ = smp.sample_policy(logits, env, "stored", greedy=True)
        env.step_device(acts.data_ptr())
        orc.step(dc.greedy_actions(logits_np, po.stored_masks(orc)))
        if t in fr.RUN_A_CHECKS:
            features(t)
    torch.cuda.synchronize()
    for t, dtype, got, want in pending:
        assert_equal(got, want, dtype, f"device loop step {t}")
    env.sync_host()
    assert_views(env, orc, "device loop")


def test_after_a_stored_mask_rollout(cg):
    env, smp, orc, osm = make(cg, fr.RUN_A)
    runner = cg.vec.get_runner(fr.RUN_A["n"])(env, smp, None, device_views=True, stored_masks=True)
    runner.rollout(60)
    got = [cg.policy_features(env, 4, dtype=d) for d in dtypes()]       # (queued behind the rollout)
    runner.sync()
    for _ in range(60):
        fr.oracle_step(orc, osm)
    want = fr.oracle_features(orc, 4, 4)
    for d, g in zip(dtypes(), got):
        assert_equal(g, want, d, "after rollout(60), stored masks")
    check(cg, env, want, 4, "after the sync")


def test_after_a_trio_rollout(cg):
    """20 selected-mask steps of 4 players in launches of 5: the trio kernel, whose launches hand the
    decks over through the compact image."""
    env, smp, orc, osm = make(cg, fr.RUN_A)
    n = fr.RUN_A["n"]
    assert cg._C.rollout_kind(n, 4, False) == "trio"
    runner = cg.vec.get_runner(n)(env, smp, None, device_views=True)
    runner.set_chunk(5)
    runner.rollout(20)
    runner.sync()
    for _ in range(20):
        osm.sample(orc.selected_action_masks)
        orc.step(osm.actions)
    check(cg, env, fr.oracle_features(orc, 4, 4), 4, "after a trio rollout of 20")
    check(cg, env, fr.oracle_features(orc, 4, 2, seats=2), 2, "after a trio rollout of 20, seat 2", seat=2)


def test_radius_24_on_run_b(cg):
    env, smp, orc, osm = make(cg, fr.RUN_B)
    for _ in range(fr.RUN_B_STEPS):
        host_step(env, smp, orc, osm)
    cells = orc.player_cells()[0]
    assert int((cells.max(axis=(1, 2)) >= fr.GRID - fr.MAX_RADIUS).sum()) >= 3, "run B lost its high-edge envs"
    assert not (orc.flags() & (po.F_MAPGEN_FAIL | po.F_GRID_OVER)).any()
    want = fr.oracle_features(orc, 4, fr.MAX_RADIUS)
    assert (want[1][:, 9].reshape(orc.n, -1).min(axis=1) == 0).all()    # every window leaves the grid
    check(cg, env, want, fr.MAX_RADIUS, "run B, radius 24")
    for seat in range(4):                                               # every player's window
        check(cg, env, fr.oracle_features(orc, 4, fr.MAX_RADIUS, seats=seat), fr.MAX_RADIUS, f"run B, seat {seat}", seat=seat)


def test_seats(cg):
    import torch
    env, smp, orc, osm = make(cg, fr.RUN_A, players=3)
    n = fr.RUN_A["n"]
    for _ in range(20):
        host_step(env, smp, orc, osm)
    for seat in range(4):
        want = fr.oracle_features(orc, 3, 4, seats=seat)
        check(cg, env, want, 4, f"seat {seat}", seat=seat)
        if seat == 3:
            assert not want[0].any() and not want[1].any()
            for dtype in dtypes():
                vec, loc = cg.policy_features(env, 4, seat=3, dtype=dtype)
                assert not vec.any() and not loc.any()
    mixed = (np.arange(n) * 7 // 3 % 4).astype(np.uint8)
    assert set(mixed.tolist()) == {0, 1, 2, 3}
    check(cg, env, fr.oracle_features(orc, 3, 4, seats=mixed), 4, "mixed seats", seat=torch.from_numpy(mixed).cuda())
    high = mixed | np.uint8(0xA4)                                       # only the low two bits count
    check(cg, env, fr.oracle_features(orc, 3, 4, seats=mixed), 4, "seat bytes with high bits", seat=torch.from_numpy(high).cuda())
    agent = torch.from_numpy(np.array(orc.agent_selection, copy=True)).cuda()
    assert len(set(orc.agent_selection.tolist())) > 1
    for dtype in dtypes():
        a, b = cg.policy_features(env, 4, dtype=dtype), cg.policy_features(env, 4, seat=agent, dtype=dtype)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    check(cg, env, fr.oracle_features(orc, 3, 4), 4, "the acting seat")


@pytest.mark.parametrize("side_stream", (False, True), ids=("current_stream", "side_stream"))
def test_out_slices_of_a_rollout_buffer(cg, side_stream):
    """out = (buf_vec[1], buf_loc[1]) of time-major buffers with n = 3, radius 4: the local slice starts
    12 (bfloat16) or 8 (float32) bytes past a 16-byte boundary; a second pair of buffers is shifted by
    one element, so that the vec slice is unaligned too.  Rows 0 and 2 keep their fill."""
    import torch
    n, T, radius, W = 3, 3, 4, 9
    env, smp, orc, osm = make(cg, fr.RUN_A, n)
    for _ in range(5):
        host_step(env, smp, orc, osm)
    want = fr.oracle_features(orc, 4, radius)
    stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
    for dtype in dtypes():
        for shift in (0, 1):
            flat_v = torch.full((T * n * fr.VEC + shift,), 77.0, dtype=dtype, device="cuda")
            flat_l = torch.full((T * n * fr.CHANNELS * W * W + shift,), 77.0, dtype=dtype, device="cuda")
            buf_vec = flat_v[shift:].view(T, n, fr.VEC)
            buf_loc = flat_l[shift:].view(T, n, fr.CHANNELS, W, W)
            assert buf_loc[1].data_ptr() % 16 != 0 and (shift == 0 or buf_vec[1].data_ptr() % 16 != 0)
            torch.cuda.synchronize()
            with torch.cuda.stream(stream):
                out = (buf_vec[1], buf_loc[1])
                got = cg.policy_features(env, radius, dtype=dtype, out=out)
            stream.synchronize()
            assert got[0] is out[0] and got[1] is out[1]
            assert_equal((buf_vec[1], buf_loc[1]), want, dtype, f"out=, shift {shift}")
            for t in (0, 2):
                assert (buf_vec[t] == 77).all() and (buf_loc[t] == 77).all(), f"row {t} was written"
            assert (flat_v[:shift] == 77).all() and (flat_l[:shift] == 77).all()


def test_no_side_effects(cg):
    import torch
    env, smp, orc, osm = make(cg, fr.RUN_A)
    for _ in range(20):
        host_step(env, smp, orc, osm)
    views = cg.device_tensors(env)
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in views.items()}
    host_before = {nm: np.array(getattr(env, nm), copy=True) for nm in FIELDS + PLAIN}
    for dtype in dtypes():
        for seat in (None, 2):
            cg.policy_features(env, 4, seat=seat, dtype=dtype)
    torch.cuda.synchronize()
    for k, v in views.items():
        assert torch.equal(v, before[k]), f"device view {k} changed"
    for nm in FIELDS:
        assert po.named_equal(getattr(env, nm), host_before[nm]) is None, f"host view {nm} changed"
    for nm in PLAIN:
        assert np.array_equal(np.asarray(getattr(env, nm)), host_before[nm]), f"host view {nm} changed"
    for t in range(10):
        host_step(env, smp, orc, osm)
        if t % 3 == 0:
            cg.policy_features(env, 4)                                  # (between steps, as a policy loop calls it)
        assert_views(env, orc, f"step {t} after the call")
    check(cg, env, fr.oracle_features(orc, 4, 4), 4, "ten steps later")


def test_refusals(cg):
    import torch
    n, radius, W = 8, 4, 9
    env = cg.vec.get_vec_env(n)(device=0)
    env.reset(7, 4, 3, cg.EASY, 100000, False)
    f = cg.policy_features
    vec, loc = f(env, radius)
    assert vec.dtype == torch.bfloat16 and tuple(loc.shape) == (n, 10, W, W)          # the defaults
    two = cg.vec.get_vec_env(n)(device=[0, 0])
    two.reset(7, 4, 3, cg.EASY, 100000, False)
    with pytest.raises(ValueError, match="shard"):
        f(two, radius)
    for bad in (-1, 25, 4.0, True, None):
        with pytest.raises(ValueError, match="radius"):
            f(env, bad)
    for bad in (torch.float16, torch.float64, torch.uint8, "bfloat16"):
        with pytest.raises(ValueError, match="dtype"):
            f(env, radius, dtype=bad)
    for bad in (4, -1, 1.0, "0"):
        with pytest.raises(ValueError, match="seat"):
            f(env, radius, seat=bad)
    seats = torch.zeros(n, dtype=torch.uint8, device="cuda")
    f(env, radius, seat=seats)
    for bad in (seats[:-1], torch.zeros(n + 1, dtype=torch.uint8, device="cuda"), seats.to(torch.int32), seats.long(),
                seats.cpu(), seats[:, None], torch.zeros(2 * n, dtype=torch.uint8, device="cuda")[::2]):
        with pytest.raises(ValueError, match="seat"):
            f(env, radius, seat=bad)

    def outs(dtype=torch.bfloat16, vshape=(n, 208), lshape=(n, 10, W, W), device="cuda"):
        return (torch.full(vshape, 77.0, dtype=dtype, device=device), torch.full(lshape, 77.0, dtype=dtype, device=device))
    good = outs()
    assert f(env, radius, out=good)[0] is good[0] and torch.equal(good[0], vec) and torch.equal(good[1], loc)
    wide_v, wide_l = torch.full((n, 416), 77.0, dtype=torch.bfloat16, device="cuda"), outs(lshape=(n, 10, W, 2 * W))[1]
    cases = [("shape", outs(vshape=(n, 207))), ("shape", outs(lshape=(n, 10, W, W + 1))), ("shape", outs(lshape=(n, 10, 7, 7))),
             ("shape", outs(vshape=(n + 1, 208))), ("shape", outs(lshape=(n, W, W, 10))), ("dtype", outs(dtype=torch.float32)),
             ("dtype", (outs()[0], outs(dtype=torch.float32)[1])), ("device", outs(device="cpu")),
             ("contiguous", (wide_v[:, ::2], outs()[1])), ("contiguous", (outs()[0], wide_l[:, :, :, ::2]))]
    for match, bad in cases:
        keep = [t.clone() for t in bad]
        with pytest.raises(ValueError, match=match):
            f(env, radius, out=bad)
        torch.cuda.synchronize()
        assert all(torch.equal(t, k) for t, k in zip(bad, keep)), f"a refused call wrote its out ({match})"
    for bad in (good[0], (good[0],), (good[0], good[1], good[1]), (good[0], None)):
        with pytest.raises(ValueError, match="pair"):
            f(env, radius, out=bad)
    # refusals with a good out leave it alone
    fresh = outs()
    for kw in (dict(radius=25), dict(radius=4, seat=4), dict(radius=4, dtype=torch.float16), dict(radius=4, seat=seats[:-1])):
        with pytest.raises(ValueError):
            f(env, out=fresh, **kw)
    with pytest.raises(ValueError, match="shard"):
        f(two, radius, out=fresh)
    torch.cuda.synchronize()
    assert (fresh[0] == 77).all() and (fresh[1] == 77).all()
    # the raw entry validates what the Python layer validates
    raw = cg._C.VecEnvBase.policy_features_raw
    ptrs = dict(d_vec=fresh[0].data_ptr(), d_local=fresh[1].data_ptr())
    for kw, match in ((dict(radius=25, dtype=1), "radius"), (dict(radius=-1, dtype=1), "radius"), (dict(radius=4, dtype=2), "dtype"),
                      (dict(radius=4, dtype=1, seat_mode=3), "seat mode"), (dict(radius=4, dtype=1, seat_mode=1, seat=4), "seat"),
                      (dict(radius=4, dtype=1, seat_mode=2, d_seats=0), "NULL")):
        with pytest.raises(ValueError, match=match):
            raw(env, **kw, **ptrs)
    with pytest.raises(ValueError, match="NULL"):
        raw(env, 4, 1, d_vec=0, d_local=ptrs["d_local"])
    with pytest.raises(ValueError, match="aligned"):
        raw(env, 4, 0, d_vec=ptrs["d_vec"] + 2, d_local=ptrs["d_local"])
    with pytest.raises(ValueError, match="shard"):
        raw(two, 4, 1, **ptrs)
    torch.cuda.synchronize()
    assert (fresh[0] == 77).all() and (fresh[1] == 77).all()


def test_no_envs(cg):
    import torch
    env = cg.vec.get_vec_env(0)(device=0)
    for dtype in dtypes():
        vec, loc = cg.policy_features(env, 4, dtype=dtype)
        assert tuple(vec.shape) == (0, 208) and tuple(loc.shape) == (0, 10, 9, 9) and vec.dtype == dtype and loc.is_cuda
    out = (torch.empty((0, 208), dtype=torch.float32, device="cuda"), torch.empty((0, 10, 1, 1), dtype=torch.float32, device="cuda"))
    assert cg.policy_features(env, 0, dtype=torch.float32, out=out)[1] is out[1]
    cg._C.VecEnvBase.policy_features_raw(env, 4, 1)                     # nothing launched, nothing to refuse


class Views(C.Structure):                                  # cog_env_views (include/cog.h)
    _fields_ = [("n_envs", C.c_size_t)] + [(f, C.c_void_p) for f in (
        "observations", "selected_action_masks", "rewards", "dones", "agent_selection", "infos",
        "d_observations", "d_selected_action_masks", "d_rewards", "d_dones", "d_agent_selection", "d_infos")]


class FeaturesArgs(C.Structure):                           # cog_features_args (include/cog.h)
    _fields_ = [("radius", C.c_int), ("dtype", C.c_int), ("seat_mode", C.c_int), ("seat", C.c_int), ("d_seats", C.c_void_p),
                ("d_vec", C.c_void_p), ("d_local", C.c_void_p), ("stream", C.c_void_p)]


def test_c_abi_through_ctypes(cg):
    """cog_env_policy_features on a handle made through the C ABI alone, against the Python call on an
    env reset alike, and the oracle's reference; a NULL output pointer is COG_ERR_INVALID."""
    import torch
    n, radius, W = 65, 4, 9
    L = C.CDLL(LIB)
    L.cog_last_error.restype = C.c_char_p
    L.cog_env_create.argtypes = [C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]
    L.cog_env_reset.argtypes = [C.c_void_p, C.c_uint32, C.c_uint8, C.c_uint8, C.c_int, C.c_uint32, C.c_int]
    L.cog_env_policy_features.argtypes = [C.c_void_p, C.POINTER(FeaturesArgs)]
    L.cog_env_destroy.argtypes = [C.c_void_p]
    NO_STREAM = C.c_void_p(2 ** 64 - 1)                                 # COG_NO_STREAM
    env, _, orc, _ = make(cg, fr.RUN_A, n, 3)
    h = C.c_void_p()
    assert L.cog_env_create(n, 0, C.byref(h)) == 0, L.cog_last_error()
    assert L.cog_env_reset(h, fr.RUN_A["seed"], 3, fr.RUN_A["pieces"], fr.RUN_A["difficulty"], 100000, 0) == 0, L.cog_last_error()
    seats = torch.from_numpy((np.arange(n) % 4).astype(np.uint8)).cuda()
    for code, dtype in enumerate(dtypes()):
        for mode, seat, kw, ref_seats in ((0, 0, dict(), None), (1, 1, dict(seat=1), 1), (2, 0, dict(seat=seats), np.arange(n) % 4)):
            vec = torch.full((n, 208), 77.0, dtype=dtype, device="cuda")
            loc = torch.full((n, 10, W, W), 77.0, dtype=dtype, device="cuda")
            torch.cuda.synchronize()
            a = FeaturesArgs(radius, code, mode, seat, seats.data_ptr() if mode == 2 else None, vec.data_ptr(), loc.data_ptr(), NO_STREAM)
            assert L.cog_env_policy_features(h, C.byref(a)) == 0, L.cog_last_error()
            torch.cuda.synchronize()
            want = cg.policy_features(env, radius, dtype=dtype, **kw)
            assert torch.equal(vec, want[0]) and torch.equal(loc, want[1]), (dtype, mode)
            assert_equal((vec, loc), fr.oracle_features(orc, 3, radius, seats=ref_seats), dtype, f"ctypes, seat mode {mode}")
    keep = loc.clone()
    for a in (FeaturesArgs(radius, 1, 0, 0, None, None, loc.data_ptr(), NO_STREAM),
              FeaturesArgs(radius, 1, 0, 0, None, vec.data_ptr(), None, NO_STREAM),
              FeaturesArgs(25, 1, 0, 0, None, vec.data_ptr(), loc.data_ptr(), NO_STREAM),
              FeaturesArgs(radius, 1, 1, 4, None, vec.data_ptr(), loc.data_ptr(), NO_STREAM)):
        assert L.cog_env_policy_features(h, C.byref(a)) == -1           # COG_ERR_INVALID
        assert b"policy_features" in L.cog_last_error()
    assert L.cog_env_policy_features(h, None) == -1
    torch.cuda.synchronize()
    assert torch.equal(loc, keep)
    L.cog_env_destroy(h)
