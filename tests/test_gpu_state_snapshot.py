"""GPU: envs.snapshot() / envs.restore(snap, src) -- state save, restore and fork on the device
(cog.h "state snapshots", csrc/engine/state_copy.h), held to the oracle bit for bit.

The oracle cannot load a state, so its side of a restore is a replay and a fork's twin is a 1-env
oracle fed the source env's recorded actions (tests/snapshot_cases.py; the method and what each case
reaches are asserted on the oracle alone in tests/test_state_snapshot_cpu.py).  Both sides walk the
ops of tests/driver_cases.py; all six host views (the map included) are compared over named fields
after every op, the device views against the host views after every restore.

  undo       X (max_steps 8), 10 steps, snapshot, 30 steps under A, restore, 30 steps under B, for
             every ordered pair of H, G, T20, S20, L, Rr at 70 envs: each kind of kernel follows a
             restore, the trio with cdeck_ok false and its fix-up; the 30 steps in between cross
             auto-resets, so every map a restore leaves differs from the one it found
  players    the same with 3, 2 and 1 players and at 33 and 1 envs; a restore that brings back 4
             players and max_steps 8 after a reset with 2 and 40; wide decks at the snapshot point
  fork       a 70-env snapshot into handles of 70 and 33, a 1-env snapshot into 70: random src with
             repeats, one index, reversed; int32, int64 and uint32; into a handle never reset and one
             that holds other maps; then 40 host-loop steps and a T20 rollout of 30 against
             per-destination 1-env twins, across auto-resets (a fork regenerates its map where its
             source would)
  shards     130 envs over device=[0, 0]: snapshot, T20, restore, T20, H; src= is refused
  reuse      snapshot(out=) twice into one object, one snapshot restored twice, a snapshot between two
             rollout launches with no sync, src from a torch op on a side stream
  around     policy_features after a restore, hazards() per env from a snapshot that holds off-mask
             flags, no speculative hit across a restore, invalidate_device() after a restore, refused
             calls leave every view untouched, a snapshot outlives its handle
  ctypes     create / snapshot / step / restore / info / destroy through the C ABI

Every one fails on a build without the feature (envs.snapshot does not exist).
"""
import ctypes as C
import gc
import os

import numpy as np
import pytest

import driver_cases as dc
import policy_features_ref as pf
import pyoracle as po
import snapshot_cases as sc

pytestmark = pytest.mark.gpu

DRIVERS = dc.REDUCED_DRIVERS
RESET4 = sc.reset_op()


def prefix(cg, n, reset=RESET4, steps=sc.PREFIX, driver="H", device=None):
    h = dc.Harness(cg, n, sc.SAMPLER_SEED, device=device)
    return h, sc.record_prefix(h, reset, steps, driver)


def device_views_equal_host(cg, env, what):
    import torch
    t = cg.device_tensors(env)
    torch.cuda.synchronize()
    for nm in sc.VIEWS:
        dev = t[nm].cpu().numpy().view(np.uint8).reshape(-1)
        host = np.ascontiguousarray(getattr(env, nm)).view(np.uint8).reshape(-1)
        assert np.array_equal(dev, host), f"{what}: the device view {nm} differs from the host view"


def restore_checked(cg, h, snap, reset, acts, what="restore"):
    """env.restore(snap) on the engine, the replay on the oracle; every view and flag compared."""
    h.env.restore(snap)
    sc.after_restore(h, sc.replay(h.n, reset, acts), reset[2], reset[5])
    h.compare(what)
    h.compare_hazards(what)
    if h.env.num_shards == 1:
        device_views_equal_host(cg, h.env, what)


def undo(cg, n, reset, a, b, driver="H", steps=sc.PREFIX, device=None):
    h, acts = prefix(cg, n, reset, steps, driver, device)
    snap = h.env.snapshot()
    assert (snap.n, snap.n_players, snap.max_steps) == (n, reset[2], reset[5])
    dc.run(h, [(a, sc.BETWEEN)])
    ends = h.op_ends[-1]
    restore_checked(cg, h, snap, reset, acts)
    dc.run(h, sc.per_step(b, sc.AFTER))
    h.compare_hazards("at the end")
    return h, ends


@pytest.mark.parametrize("b", DRIVERS)
@pytest.mark.parametrize("a", DRIVERS)
def test_undo(cg, a, b):
    h, ends = undo(cg, sc.SIZES[0], RESET4, a, b)
    assert ends >= 1, "no episode end between snapshot and restore"


@pytest.mark.parametrize("a,b", [("T20", "H"), ("H", "T20"), ("S20", "L"), ("G", "S20"), ("Rr", "T20")])
@pytest.mark.parametrize("players", [3, 2, 1])
def test_undo_players(cg, players, a, b):
    undo(cg, sc.SIZES[0], sc.reset_op(players), a, b)


@pytest.mark.parametrize("a,b", [("T20", "T20"), ("H", "S20"), ("S20", "H"), ("L", "T20")])
@pytest.mark.parametrize("n", sc.SIZES[1:])
def test_undo_sizes(cg, n, a, b):
    undo(cg, n, RESET4, a, b)


@pytest.mark.parametrize("b", ["T20", "S20", "H"])
def test_undo_wide_decks(cg, b):
    w = sc.WIDE
    undo(cg, w["n"], sc.reset_op(w["players"], w["seed"], w["max_steps"]), "T20", b, w["driver"], w["prefix"])


def test_restore_brings_back_players_and_max_steps(cg):
    h, acts = prefix(cg, sc.SIZES[0])
    snap = h.env.snapshot()
    dc.run(h, [sc.OTHER_RESET, ("T20", sc.BETWEEN)])         # (2 players: the duo)
    restore_checked(cg, h, snap, RESET4, acts)
    dc.run(h, [("T20", sc.AFTER), ("T20", sc.AFTER)])        # 4 players again: the trio, with its fix-up
    h.compare_hazards("at the end")


# ---- fork ---------------------------------------------------------------------------------------
def torch_src(cg, env, src, dtype):
    import torch
    dev = torch.device("cuda", env.shard_info(0)[2])
    if dtype == "uint32":
        return torch.from_numpy(src.astype(np.uint32)).to(dev)
    return torch.from_numpy(src.astype(np.int64)).to(dev).to(getattr(torch, dtype))


def fork_and_run(cg, n_dst, n_src, kind, dtype, dirty):
    hs, acts = prefix(cg, n_src)
    snap = hs.env.snapshot()
    want = sc.views_of(hs.orc)
    dst = cg.vec.get_vec_env(n_dst)()
    smp = cg.vec.get_vec_sampler(n_dst)(sc.SAMPLER_SEED + 1)
    if dirty:                                                # other maps, players and counters in the way
        dst.reset(sc.SEED + 99, 3, sc.PIECES, cg.Difficulty(0), 5, False)
        for _ in range(12):
            smp.sample(dst.selected_action_masks)
            dst.step(smp.get_actions())
        smp = cg.vec.get_vec_sampler(n_dst)(sc.SAMPLER_SEED + 1)
    else:
        dst.observations                                     # (host views before the restore)
    src = sc.fork_sources(n_dst, n_src)[kind]
    dst.restore(snap, torch_src(cg, dst, src, dtype))
    bad = sc.views_differ(dst, {nm: v[src] for nm, v in want.items()})
    assert bad is None, f"after the fork: {bad} differs from the gathered snapshot views"
    device_views_equal_host(cg, dst, "after the fork")
    tw = sc.Twins(RESET4, acts, src)
    osm = po.OracleSampler(n_dst, sc.SAMPLER_SEED + 1)
    for t in range(sc.FORK_STEPS):
        smp.sample(dst.selected_action_masks)
        osm.sample(tw.view("selected_action_masks"))
        assert po.named_equal(smp.get_actions(), osm.actions) is None, f"fork step {t}: the sampled actions differ"
        dst.step(smp.get_actions())
        tw.step(osm.actions.copy())
        bad = sc.views_differ(dst, tw.views())
        assert bad is None, f"fork step {t}: {bad} differs from the twins"
    r = cg.vec.get_runner(n_dst)(dst, smp, None, device_views=True)
    r.set_chunk(20)
    r.rollout(sc.FORK_ROLLOUT)
    r.sync()
    dst.sync_host()
    for _ in range(sc.FORK_ROLLOUT):
        osm.sample(tw.view("selected_action_masks"))
        tw.step(osm.actions.copy())
    bad = sc.views_differ(dst, tw.views())
    assert bad is None, f"after the fork's rollout: {bad} differs from the twins"
    assert np.array_equal(dst.hazards()[1], tw.flags())
    assert tw.ends >= 1
    # the source handle is none the wiser
    dc.run(hs, [("H", 3)])


@pytest.mark.parametrize("dirty", [False, True], ids=["fresh", "dirty"])
@pytest.mark.parametrize("kind", ["random", "one", "reversed"])
def test_fork(cg, kind, dirty):
    fork_and_run(cg, 70, 70, kind, "int32", dirty)


@pytest.mark.parametrize("dtype", ["int64", "uint32"])
def test_fork_src_dtypes(cg, dtype):
    fork_and_run(cg, 70, 70, "random", dtype, True)


@pytest.mark.parametrize("n_dst,n_src", [(33, 70), (70, 1)])
@pytest.mark.parametrize("dtype", ["int32", "int64"])
def test_fork_sizes(cg, n_dst, n_src, dtype):
    fork_and_run(cg, n_dst, n_src, "random", dtype, True)


# ---- two shards ---------------------------------------------------------------------------------
def test_two_shards(cg):
    import torch
    n = sc.SHARD_N
    h, acts = prefix(cg, n, device=sc.SHARD_DEVICES)
    assert h.env.num_shards == 2
    snap = h.env.snapshot()
    assert snap.devices == sc.SHARD_DEVICES and sum(snap.counts) == n and snap.nbytes >= 4000 * n
    dc.run(h, [("T20", sc.BETWEEN)])
    assert h.op_ends[-1] >= 1
    before = sc.views_of(h.env)
    src = torch.arange(n, dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError, match="single-shard"):
        h.env.restore(snap, src)
    assert sc.views_differ(h.env, before) is None
    one = cg.vec.get_vec_env(n)()                            # the same envs on one shard: another layout
    with pytest.raises(ValueError, match="layout"):
        one.restore(snap)
    with pytest.raises(ValueError, match="layout"):
        one.snapshot(out=snap)
    restore_checked(cg, h, snap, RESET4, acts)
    dc.run(h, [("T20", sc.AFTER)] + sc.per_step("H", 10))
    h.compare_hazards("at the end")


# ---- reuse and ordering -------------------------------------------------------------------------
def test_snapshot_out_twice_and_restored_twice(cg):
    h, acts = prefix(cg, sc.SIZES[0])
    snap = h.env.snapshot()
    for _ in range(5):
        dc.run(h, [("H", 1)])
        acts.append(h.last.copy())
    assert h.env.snapshot(out=snap) is snap                  # the later point, into the same object
    dc.run(h, [("T20", sc.BETWEEN)])
    restore_checked(cg, h, snap, RESET4, acts, "first restore")
    dc.run(h, [("S20", sc.AFTER)])
    restore_checked(cg, h, snap, RESET4, acts, "second restore")
    dc.run(h, [("T20", sc.AFTER)] + sc.per_step("H", 5))
    with pytest.raises(ValueError):
        h.env.snapshot(out=object())


def test_snapshot_between_two_rollout_launches_without_a_sync(cg):
    n = sc.SIZES[0]
    h, acts = prefix(cg, n)
    r = h.runner(False, True)                                # selected masks, device views
    r.set_chunk(20)
    r.rollout(20)
    snap = h.env.snapshot()                                  # enqueued behind the first launch: no sync
    r.rollout(20)
    r.sync()
    for t in range(40):
        h.osm.sample(h.orc.selected_action_masks)
        h.last = h.osm.actions.copy()
        h.orc.step(h.last)
        if t < 20:
            acts.append(h.last)
    h.env.sync_host()
    h.acts_fresh = False
    h.compare("after the two launches")
    restore_checked(cg, h, snap, RESET4, acts)
    dc.run(h, [("T20", sc.AFTER)])


def test_src_from_a_torch_op_on_a_side_stream(cg):
    import torch
    n_src, n_dst = 70, 70
    hs, acts = prefix(cg, n_src)
    snap = hs.env.snapshot()
    want = sc.views_of(hs.orc)
    dst = cg.vec.get_vec_env(n_dst)()
    dst.observations
    dev = torch.device("cuda", dst.shard_info(0)[2])
    side = torch.cuda.Stream(device=dev)
    big = torch.ones((2048, 2048), device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        pad = (big @ big).sum()                              # work ahead of src on the side stream
        src = ((torch.arange(n_dst, device=dev) * 7 + (pad * 0).long()) % n_src).to(torch.int32)
        dst.restore(snap, src)                               # ordered after the current (side) stream
    idx = (np.arange(n_dst) * 7) % n_src
    bad = sc.views_differ(dst, {nm: v[idx] for nm, v in want.items()})
    assert bad is None, f"{bad} differs from the gathered snapshot views"


# ---- around a restore ---------------------------------------------------------------------------
def test_policy_features_after_a_restore(cg):
    import torch
    h, acts = prefix(cg, sc.SIZES[0], driver="Hs", steps=20)
    snap = h.env.snapshot()
    dc.run(h, [("S20", sc.BETWEEN)])
    restore_checked(cg, h, snap, RESET4, acts)
    vec, loc = cg.policy_features(h.env, 4, dtype=torch.float32)
    want_vec, want_loc = pf.oracle_features(h.orc, 4, 4)
    torch.cuda.synchronize()
    assert np.array_equal(vec.cpu().numpy(), want_vec)
    assert np.array_equal(loc.cpu().numpy(), want_loc)


def offmask_prefix(cg, n):
    """Ten recorded host steps of which half the envs take an action their mask need not allow
    (driver_cases' M op, kind `all`): hazard flags on some envs at the snapshot point."""
    h = dc.Harness(cg, n, sc.SAMPLER_SEED)
    reset = sc.reset_op(4, sc.SEED, 100000)
    dc.run(h, [reset])
    acts = []
    for j in range(sc.PREFIX):
        dc.run(h, [("M", "step", 1, 800 + j, "all", 0.5)])
        acts.append(h.last.copy())
    return h, reset, acts


def test_hazards_per_env_from_a_snapshot_with_offmask_flags(cg):
    h, reset, acts = offmask_prefix(cg, sc.SIZES[0])
    flagged = h.orc.flags() != 0
    assert 0 < flagged.sum() < h.n, f"{int(flagged.sum())} of {h.n} envs hold a flag at the snapshot point"
    snap = h.env.snapshot()
    dc.run(h, ["C", ("H", sc.BETWEEN)])                      # flags compared and cleared, then other states
    restore_checked(cg, h, snap, reset, acts)                # (compares hazards() per env with the replay's)
    assert np.array_equal(h.env.hazards()[1] != 0, flagged)
    dc.run(h, [("T20", sc.AFTER), "C"])


def test_no_speculative_hit_across_a_restore(cg):
    h, acts = prefix(cg, sc.SIZES[0])
    snap = h.env.snapshot()
    dc.run(h, [("H", 20)])
    assert h.smp.spec_stats()[1] > 0, "the host loop never took a speculative sample: the case shows nothing"
    restore_checked(cg, h, snap, RESET4, acts)
    hits = h.smp.spec_stats()[1]
    dc.run(h, [("H", 1)])                                    # its sample reads the restored masks
    assert h.smp.spec_stats()[1] == hits, "a sample speculated before the restore was taken after it"
    dc.run(h, [("H", 10)])


def test_invalidate_device_after_a_restore_changes_nothing(cg):
    h, acts = prefix(cg, sc.SIZES[0])
    snap = h.env.snapshot()
    dc.run(h, [("T20", sc.BETWEEN)])
    restore_checked(cg, h, snap, RESET4, acts)
    dc.run(h, ["I"])
    device_views_equal_host(cg, h.env, "after invalidate_device")
    dc.run(h, [("T20", sc.AFTER)] + sc.per_step("H", 5))


def test_refused_calls_leave_every_view_untouched(cg):
    import torch
    n = sc.SIZES[0]
    h, acts = prefix(cg, n)
    snap = h.env.snapshot()
    dc.run(h, [("H", 5)])
    before = sc.views_of(h.env)
    t = cg.device_tensors(h.env)
    torch.cuda.synchronize()
    dev_before = {nm: t[nm].clone() for nm in sc.VIEWS}
    dev = t["dones"].device
    good = torch.arange(n, dtype=torch.int32, device=dev)
    over, under = good.clone(), good.clone().to(torch.int64)
    over[n - 1] = n
    under[3] = -1
    small = cg.vec.get_vec_env(sc.SIZES[1])()
    refused = [
        ("an index past the snapshot", lambda: h.env.restore(snap, over)),
        ("a negative index", lambda: h.env.restore(snap, under)),
        ("src on the host", lambda: h.env.restore(snap, good.cpu())),
        ("a float src", lambda: h.env.restore(snap, good.float())),
        ("an int16 src", lambda: h.env.restore(snap, good.to(torch.int16))),
        ("a short src", lambda: h.env.restore(snap, good[:n - 1])),
        ("a strided src", lambda: h.env.restore(snap, torch.arange(2 * n, dtype=torch.int32, device=dev)[::2])),
        ("a numpy src", lambda: h.env.restore(snap, np.arange(n, dtype=np.int32))),
        ("not a snapshot", lambda: h.env.restore(object())),
        ("another layout into the handle", lambda: h.env.restore(small.snapshot())),
        ("the handle into another layout", lambda: h.env.snapshot(out=cg.EnvSnapshot(small))),
        ("an empty snapshot", lambda: h.env.restore(cg.EnvSnapshot(h.env))),
    ]
    for what, call in refused:
        with pytest.raises(ValueError):
            call()
        assert sc.views_differ(h.env, before) is None, f"{what}: a host view changed"
        torch.cuda.synchronize()
        for nm in sc.VIEWS:
            assert torch.equal(t[nm], dev_before[nm]), f"{what}: the device view {nm} changed"
    h.compare("after the refused calls")
    dc.run(h, [("H", 3), ("T20", 20)])                       # and the handle goes on
    restore_checked(cg, h, snap, RESET4, acts)               # the snapshot is as it was


def test_a_snapshot_outlives_its_handle(cg):
    n = sc.SIZES[0]
    h, acts = prefix(cg, n)
    snap = h.env.snapshot()
    want = sc.views_of(h.orc)
    del h
    gc.collect()
    h2 = dc.Harness(cg, n, sc.SAMPLER_SEED + 5)
    dc.run(h2, [sc.OTHER_RESET, ("H", 5)])
    h2.env.restore(snap)
    assert sc.views_differ(h2.env, want) is None
    sc.after_restore(h2, sc.replay(n, RESET4, acts), RESET4[2], RESET4[5])
    dc.run(h2, [("T20", sc.AFTER)])


# ---- the C ABI through ctypes -------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gym-eldorado_amd", "city_of_gold", "libcog_hip.so")
NO_STREAM = C.c_void_p(-1)


def test_ctypes_round_trip():
    from test_gpu_ctypes_abi import Views, lib, view
    L = lib()
    L.cog_env_snapshot_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.cog_env_snapshot.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.cog_env_restore.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    L.cog_snapshot_info.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_size_t),
                                    C.POINTER(C.c_int), C.POINTER(C.c_uint32)]
    L.cog_snapshot_destroy.argtypes = [C.c_void_p]
    L.cog_snapshot_destroy.restype = None
    n, seed = sc.SIZES[0], sc.SEED
    env, smp, snap = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.cog_env_create(n, 0, C.byref(env)) == 0, L.cog_last_error()
    assert L.cog_env_reset(env, seed, 4, sc.PIECES, sc.DIFFICULTY, sc.MAX_STEPS, 0) == 0, L.cog_last_error()
    assert L.cog_sampler_create(n, sc.SAMPLER_SEED, 0, C.byref(smp)) == 0, L.cog_last_error()
    v = Views()
    assert L.cog_env_get_views(env, C.byref(v)) == 0
    views = {"observations": view(v.observations, po.OBS, (n,)),
             "selected_action_masks": view(v.selected_action_masks, po.MASK, (n,)),
             "infos": view(v.infos, po.INFO, (n,)), "rewards": view(v.rewards, np.dtype("<f4"), (n, 4)),
             "dones": view(v.dones, np.dtype("?"), (n,)), "agent_selection": view(v.agent_selection, np.dtype("u1"), (n,))}
    orc, osm = po.OracleVec(n), po.OracleSampler(n, sc.SAMPLER_SEED)
    orc.reset(seed, 4, sc.PIECES, sc.DIFFICULTY, sc.MAX_STEPS)

    rec = []

    def steps(k, oracle, rec=None):
        for _ in range(k):
            assert L.cog_sampler_sample(smp, v.selected_action_masks, n) == 0, L.cog_last_error()
            assert L.cog_env_step(env, L.cog_sampler_actions(smp), n) == 0, L.cog_last_error()
            osm.sample(oracle.selected_action_masks)
            oracle.step(osm.actions)
            if rec is not None:
                rec.append(osm.actions.copy())
    steps(sc.PREFIX, orc, rec)
    assert L.cog_env_restore(env, None, None, 0, 0, NO_STREAM) == -1                  # COG_ERR_INVALID
    assert L.cog_env_snapshot_create(env, C.byref(snap)) == 0, L.cog_last_error()
    assert L.cog_env_restore(env, snap, None, 0, 0, NO_STREAM) == -1 and b"nothing was saved" in L.cog_last_error()
    assert L.cog_env_snapshot(env, snap, NO_STREAM) == 0, L.cog_last_error()
    nn, ns, nb, npl, ms = C.c_size_t(), C.c_int(), C.c_size_t(), C.c_int(), C.c_uint32()
    assert L.cog_snapshot_info(snap, C.byref(nn), C.byref(ns), C.byref(nb), C.byref(npl), C.byref(ms)) == 0
    assert (nn.value, ns.value, npl.value, ms.value) == (n, 1, 4, sc.MAX_STEPS) and 4000 * n <= nb.value <= 4400 * n
    at_snap = sc.views_of(orc)
    steps(sc.BETWEEN, orc)                                   # both sides go on, across episode ends
    assert sc.views_differ(views, orc) is None
    assert L.cog_env_restore(env, snap, None, 0, 0, NO_STREAM) == 0, L.cog_last_error()
    assert sc.views_differ(views, at_snap) is None
    orc = sc.replay(n, ("X", seed, 4, sc.PIECES, sc.DIFFICULTY, sc.MAX_STEPS), rec)
    for t in range(sc.AFTER):
        steps(1, orc)
        bad = sc.views_differ(views, orc)
        assert bad is None, f"step {t} after the restore: {bad} differs from the oracle"
    L.cog_snapshot_destroy(snap)
    L.cog_sampler_destroy(smp)
    L.cog_env_destroy(env)
