"""GPU: map generation and stepping on big maps (2 to 10 map pieces, boxes up to the 48x48 limit)
against the oracle, bit-exact over every named field.  tests/bigmap_cases.py names the cases and
tests/test_bigmap_cpu.py shows, on the oracle alone, what each reaches: a third and a fourth
candidate batch in add_random_piece, boxes of 47 cells and more, start pieces in a corner of the
box, moves on its outermost cells, auto-resets that generate such maps inside every rollout kernel.

  reset grid   130 envs at {2, 4, 5, 6, 7, 8, 9} pieces x {MEDIUM, HARD}, 2 and 3 players at 6 and 7
               pieces, EASY at 1-3 pieces, 1 and 65 envs at 7 pieces, 10 pieces HARD: all six views
               and the hazard flags
  reference    tests/golden/ref_maps_big.json (the unmodified reference core) on the engine
  overflow     one env of 130 overflows the observation grid: the reset raises, the flags equal
               the oracle's, every other env equals the oracle, the handle recovers
  failures     0 pieces, EASY with 4 pieces, 255 pieces: the reset raises, every env is flagged
  host loop    300 steps with every step checked, selected and stored masks
  rollouts     the trio (selected masks) and, with stored masks and 20-turn episodes, the duo, one
               launch per step, the pipe and the one-wave kernel (the last two at 5 pieces MEDIUM:
               bigmap_cases.RUNS says why), at checkpoints; the fix-up pass completes the episodes
               that end inside the launches
  auto-reset   an auto-reset inside a duo launch overflows the observation grid: runner.sync()
               raises, the flag is on that env alone, the handle recovers
  off-lattice  maps on which the reference places pieces half a cell off the hex lattice, against
               the oracle and against the reference's own digests

No env is left unchecked but those the oracle itself flags (the overflow case: 1 of 130, capped at
2 % of the batch and asserted); of the pipe and wave batches the first and the last 128 envs are
checked, as in tests/test_gpu_lategame.py.
"""
import json
import os

import numpy as np
import pytest

import bigmap_cases as bc
import pyoracle as po

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
VIEWS = ("observations", "selected_action_masks", "rewards", "dones", "agent_selection", "infos")


def assert_same(env, orc, tag, pick=None):
    """Every named field of all six views, of all envs or of the envs `pick` (a bool array)."""
    for nm in VIEWS:
        a, b = getattr(env, nm), getattr(orc, nm)
        if pick is not None:
            a, b = a[pick], b[pick]
        if a.dtype.names:
            d = po.named_equal(a, b)
            if d is not None:
                bad = [i for i in range(len(a)) if po.named_equal(a[i:i + 1], b[i:i + 1]) is not None]
                raise AssertionError(f"{tag}: {nm}.{d} differs from the oracle (rows {bad[:10]})")
        else:
            assert np.array_equal(a, b), f"{tag}: {nm} differs from the oracle at {np.nonzero(np.asarray(a) != b)[0][:10]}"


def reset(cg, env, case, seed=None, pieces=None, max_steps=100000):
    env.reset(case.seed if seed is None else seed, case.players, case.pieces if pieces is None else pieces,
              cg.Difficulty(case.difficulty), max_steps, False)


# ---- resets -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bc.RESET_GRID, ids=[c.id for c in bc.RESET_GRID])
def test_reset_grid_against_oracle(cg, case):
    orc, g, raised = bc.reset_reference(case)
    assert not raised and not (g["flags"] & bc.ERR).any()  # the window is clean (tests/test_bigmap_cpu.py)
    env = cg.vec.get_vec_env(case.n)()
    reset(cg, env, case)
    assert_same(env, orc, f"reset {case.id} seed {case.seed}")
    assert np.array_equal(env.hazards()[1], g["flags"]), f"reset {case.id}: hazard flags differ"


def digest_env(e, actions, i):
    s = slice(i, i + 1)
    return po.step_digest(e.observations[s], e.selected_action_masks[s], e.rewards[s], e.dones[s],
                          e.agent_selection[s], e.infos[s], actions[s])


def test_engine_matches_reference_big_maps(cg):
    with open(os.path.join(GOLD, "ref_maps_big.json")) as f:
        gold = json.load(f)
    w = gold["window"]
    zero = np.zeros(w, dtype=po.ACTION)
    groups = {}
    for diff, npc, seed, hexd, players in gold["entries"]:
        groups.setdefault((diff, npc, players, seed // w * w), {})[seed] = hexd
    assert len(groups) == 24 and sum(len(v) for v in groups.values()) >= 250
    for (diff, npc, players, lo), by_seed in groups.items():
        env = cg.vec.get_vec_env(w)()                      # (a fresh handle: Info and n_in_market survive a reset)
        env.reset(lo, players, npc, cg.Difficulty(diff), 100000, False)
        for seed, hexd in by_seed.items():
            assert digest_env(env, zero, seed - lo).hex() == hexd, f"map seed={seed} diff={diff} n_pieces={npc} players={players}"


def test_reset_off_lattice_against_oracle(cg):
    """In env 57 of the window (seed 141707, 6 pieces HARD) a travel piece finds no free placement
    and stays reset at the origin, still named by the list of placed pieces; the recursion connects
    pieces to it there, half a cell off the map's lattice (bigmap_cases.OFF_LATTICE): 59 hexes at
    half-integer coordinates, box 26 x 26.  The engine keeps such hexes in a list beside its grid.
    (Before it did, its generation gave up here: 3 of the 32,770 seeds 140000 + i at 6 pieces HARD
    raised on the MI355X, envs 1707, 9887 and 22857.)"""
    case = bc.OFF_LATTICE
    orc, g, raised = bc.reset_reference(case)
    assert not raised and not (g["flags"] & bc.ERR).any() and tuple(np.nonzero(g["offlat"])[0]) == bc.OFF_LATTICE_ENVS
    env = cg.vec.get_vec_env(case.n)()
    reset(cg, env, case)
    assert_same(env, orc, f"reset {case.id} seed {case.seed}")
    assert np.array_equal(env.hazards()[1], g["flags"]), "hazard flags differ"


def test_engine_matches_reference_off_lattice_maps(cg):
    """Four maps of 4 pieces HARD with pieces half a cell off the lattice, recorded from the
    unmodified reference core (ref_maps_big.json, "off_lattice")."""
    with open(os.path.join(GOLD, "ref_maps_big.json")) as f:
        off = json.load(f)["off_lattice"]
    assert len(off) == 4
    zero = np.zeros(1, dtype=po.ACTION)
    for diff, npc, seed, hexd, players in off:
        env = cg.vec.get_vec_env(1)()
        env.reset(seed, players, npc, cg.Difficulty(diff), 100000, False)
        assert digest_env(env, zero, 0).hex() == hexd, f"map seed={seed} diff={diff} n_pieces={npc}"


def test_overflow_at_reset(cg):
    """One env of the batch generates a map wider than the observation.  The reset raises; the
    flags are the oracle's (GRID_OVER on that env alone, no MAPGEN_FAIL beside it); every other env
    holds what the oracle holds; a following reset regenerates every env, the flagged one too (its
    sticky flag decides nothing), and 50 steps of the host loop equal the oracle."""
    case = bc.OVERFLOW
    n = case.n
    orc, osm = po.OracleVec(n), po.OracleSampler(n, 77)
    orc.reset(case.seed, case.players, case.pieces, case.difficulty, 100000)   # (the oracle only flags)
    flags = orc.flags()
    flagged = (flags & bc.ERR) != 0
    assert tuple(np.nonzero(flagged)[0]) == bc.OVERFLOW_ENVS and 1 <= flagged.sum() <= bc.MAX_FLAGGED_SHARE * n
    env, smp = cg.vec.get_vec_env(n)(), cg.vec.get_vec_sampler(n)(77)
    with pytest.raises(RuntimeError, match="48x48"):
        reset(cg, env, case)
    assert np.array_equal(env.hazards()[1], flags), "hazard flags differ"
    assert_same(env, orc, "overflow: the unflagged envs", pick=~flagged)

    reset(cg, env, case, seed=4242, pieces=3, max_steps=40)
    orc.reset(4242, case.players, 3, case.difficulty, 40)
    assert_same(env, orc, "after the overflow, reset")
    for t in range(50):
        smp.sample(po.stored_masks(env))
        osm.sample(po.stored_masks(orc))
        env.step(smp.get_actions())
        orc.step(osm.actions)
        assert_same(env, orc, f"after the overflow, step {t}")
    assert np.array_equal(env.hazards()[1], orc.flags()), "hazard flags differ after the recovery"


@pytest.mark.parametrize("case", bc.FAILURES, ids=[c.id for c in bc.FAILURES])
def test_failures_at_reset(cg, case):
    """Generation gives up in every env: the reset raises, MAPGEN_FAIL (and no GRID_OVER) is on
    every env as on the oracle's, env by env, and the handle recovers.  At 255 pieces the oracle
    places hexes up to 70 cells from the origin before it gives up; the engine gives up at its
    coordinate bound (62), with the same report."""
    n = case.n
    ref, g, raised = bc.reset_reference(case)
    assert raised and (g["flags"] & bc.ERR == po.F_MAPGEN_FAIL).all()
    env, smp = cg.vec.get_vec_env(n)(), cg.vec.get_vec_sampler(n)(5)
    with pytest.raises(RuntimeError, match="generate map"):
        reset(cg, env, case)
    per = env.hazards()[1]
    assert np.array_equal(per & bc.ERR, g["flags"] & bc.ERR), f"flags {per} against the oracle's {g['flags']}"

    orc, osm = po.OracleVec(n), po.OracleSampler(n, 5)     # the handle recovers
    if case.pieces != 255:                                 # (the oracle's own failed reset first, where it is quick)
        with pytest.raises(RuntimeError):
            orc.reset_threaded(case.seed, case.players, case.pieces, case.difficulty, 100000)
    env.reset(1000, 4, 3, cg.HARD, 40, False)
    orc.reset(1000, 4, 3, 2, 40)
    assert_same(env, orc, "after the failure, reset")
    for t in range(50):
        smp.sample(po.stored_masks(env))
        osm.sample(po.stored_masks(orc))
        env.step(smp.get_actions())
        orc.step(osm.actions)
        assert_same(env, orc, f"after the failure, step {t}")


# ---- the host loop, every step ------------------------------------------------------------------
@pytest.mark.parametrize("rid", [r.id for r in bc.RUNS.values() if r.kind == "host"])
def test_host_loop_every_step(cg, rid):
    run = bc.RUNS[rid]
    env, smp = cg.vec.get_vec_env(run.n)(), cg.vec.get_vec_sampler(run.n)(run.seed)
    env.reset(run.seed, run.players, run.pieces, cg.Difficulty(run.difficulty), run.max_steps, False)
    orun = bc.OracleRun(run)
    orc, osm = orun.parts[0]
    assert_same(env, orc, f"{rid} reset")
    acts = smp.get_actions()
    resets = 0
    for t in range(run.steps):
        smp.sample(po.stored_masks(env) if run.stored else env.selected_action_masks)
        env.step(acts)
        orun.step()
        assert po.named_equal(acts, osm.actions) is None, f"{rid}: actions differ at step {t}"
        assert_same(env, orc, f"{rid} step {t}")
        resets += int(env.dones.sum())
    assert resets >= run.min_resets, f"{rid}: {resets} auto-resets: the test lost its case"
    assert np.array_equal(env.hazards()[1], orc.flags()), f"{rid}: hazard flags differ"


# ---- rollouts -----------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", [r.id for r in bc.RUNS.values() if r.kind != "host"])
def test_rollout_against_oracle(cg, rid):
    run = bc.RUNS[rid]
    if run.kind is not None:
        assert cg._city_of_gold.rollout_kind(run.n, run.players, run.stored) == run.kind
    ref = bc.run_reference(rid)
    bc.check_run(run, ref)                                 # the case is there
    env, smp = cg.vec.get_vec_env(run.n)(), cg.vec.get_vec_sampler(run.n)(run.seed)
    env.reset(run.seed, run.players, run.pieces, cg.Difficulty(run.difficulty), run.max_steps, False)
    runner = cg.vec.get_runner(run.n)(env, smp, None, device_views=True, stored_masks=run.stored)
    if run.chunk:
        runner.set_chunk(run.chunk)
    done = 0
    for k in run.checkpoints:
        runner.rollout(k - done)
        runner.sync()
        env.sync_host()
        done = k
        bad = ref.snapshots[k].differences(env, rid)
        assert not bad, "\n".join(bad)
    per = env.hazards()[1]
    assert not (per & bc.ERR).any(), f"{rid}: error flags on envs {np.nonzero(per & bc.ERR)[0][:10]}"
    got = np.concatenate([per[lo:hi] for lo, hi in run.blocks])
    assert np.array_equal(got, ref.flags), f"{rid}: hazard flags differ"


def test_overflow_at_autoreset_inside_rollout(cg):
    """An auto-reset inside a launch generates a map wider than the observation (env 102, step 132
    of a stored-mask duo rollout at 8 pieces).  The run equals the oracle at 120 steps; the launches
    past the overflow raise at runner.sync(); GRID_OVER is on that env alone (its record is
    unspecified until the next reset); the handle recovers with a reset."""
    c = bc.AUTORESET_OVERFLOW
    n, seed = c["n"], c["seed"]
    run = bc.Run("auto", "duo", n, c["players"], c["pieces"], c["difficulty"], seed, c["max_steps"],
                 c["checkpoint"] + c["past"], True)
    assert cg._city_of_gold.rollout_kind(n, c["players"], True) == "duo"
    env, smp = cg.vec.get_vec_env(n)(), cg.vec.get_vec_sampler(n)(seed)
    env.reset(seed, c["players"], c["pieces"], cg.Difficulty(c["difficulty"]), c["max_steps"], False)
    runner = cg.vec.get_runner(n)(env, smp, None, device_views=True, stored_masks=True)
    runner.set_chunk(c["chunk"])
    orun = bc.OracleRun(run)
    orc, _ = orun.parts[0]
    for _ in range(c["checkpoint"]):
        orun.step()
    runner.rollout(c["checkpoint"])
    runner.sync()
    env.sync_host()
    bad = bc.lc.snapshot(orun).differences(env, "before the overflow")
    assert not bad, "\n".join(bad)
    assert not (env.hazards()[1] & bc.ERR).any() and not (orc.flags() & bc.ERR).any()

    for _ in range(c["past"]):
        orun.step()                                        # (the oracle only flags)
    assert list(np.nonzero(orc.flags() & bc.ERR)[0]) == [c["fail_env"]]
    runner.rollout(c["past"])
    with pytest.raises(RuntimeError, match="48x48"):
        runner.sync()
    per = env.hazards()[1]
    assert list(np.nonzero(per & bc.ERR)[0]) == [c["fail_env"]]
    assert per[c["fail_env"]] & bc.ERR == po.F_GRID_OVER == orc.flags(c["fail_env"]) & bc.ERR
    others = np.arange(n) != c["fail_env"]
    assert np.array_equal(per[others], orc.flags()[others]), "hazard flags of the other envs differ"

    seed2 = 4321                                           # the handle recovers
    smp2 = cg.vec.get_vec_sampler(n)(seed2)
    env.reset(seed2, c["players"], 3, cg.Difficulty(c["difficulty"]), c["max_steps"], False)
    runner2 = cg.vec.get_runner(n)(env, smp2, None, device_views=True, stored_masks=True)
    runner2.set_chunk(c["chunk"])
    runner2.rollout(100)
    runner2.sync()
    env.sync_host()
    orc.reset(seed2, c["players"], 3, c["difficulty"], c["max_steps"])
    orun.parts = [(orc, po.OracleSampler(n, seed2))]
    for _ in range(100):
        orun.step()
    # (a reset leaves Info alone, and the oracle went on stepping the flagged env where the engine
    # held it: that env's Info stays unspecified until its next episode end writes it)
    st = bc.lc.snapshot(orun).state[0]
    for nm in bc.lc.FIELDS:
        rows = others if nm == "infos" else slice(None)
        d = po.named_equal(getattr(env, nm)[rows], st[nm][rows])
        assert d is None, f"after the reset: {nm}.{d} differs from the oracle"
    for nm in bc.lc.PLAIN:
        assert np.array_equal(getattr(env, nm), st[nm]), f"after the reset: {nm} differs from the oracle"
