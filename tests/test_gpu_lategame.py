"""GPU: the full-dynamics rollout kernels (k_env_rollout_duo, k_env_rollout_pipe, the one-wave
k_env_rollout, k_env_fixup, and k_env_step / k_env_step_pub under the runner) in the late game:
thousands of steps on one-piece maps with max_steps 100,000, where episodes end because a
player reaches the end hex and the uniform sampler plays every special and the remove path.
tests/lategame_cases.py names the configurations and counts what each of them reaches on the
oracle (tests/test_lategame_cpu.py asserts the minima: >= 10 natural ends, each special >= 100
times, >= 100 removes).  Bit-exact over named fields.

  rollout       configurations A-F against the oracle after the step of the first natural end
                (its dones, rewards and terminal infos, the auto-reset in the same step) and after
                2,000, 4,000, 6,000 and 8,000 steps, hazard flags at the end
  host loop     F through sampler.sample(stored masks); env.step(actions), every step checked from
                the reset to 200 steps past the first natural end
  interleave    A: chunked launches, the host loop, runner host-view steps, chunked again
  reference     the engine against tests/golden/ref_lategame_digests.npz (the unmodified reference
                core): the host loop at every step, chunk-37 launches at every 500th step
  mapgen        a map-generation failure at an auto-reset inside a launch is reported at the next
                sync, flagged on that env alone, and the handle recovers with a reset

Durations on the MI355X (pytest --durations=0, the oracle's census included; the census of A and F
is shared with the tests that follow them): rollout A 0.33 s, B 0.31 s, C 0.33 s, C' 0.32 s,
D 0.69 s, E 0.77 s, F 0.34 s; host loop 0.44 s; interleave 0.06 s; reference host loop 2.22 s;
reference rollout 0.04 s; mapgen 0.28 s.  6.1 s together.
"""
import json
import os

import numpy as np
import pytest

import lategame_cases as lc
import pyoracle as po

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def make(cg, cfg, device_views=True):
    env = cg.vec.get_vec_env(cfg.n)()
    smp = cg.vec.get_vec_sampler(cfg.n)(cfg.seed)
    env.reset(cfg.seed, cfg.players, cfg.pieces, cg.Difficulty(cfg.difficulty), lc.MAX_STEPS, False)
    runner = cg.vec.get_runner(cfg.n)(env, smp, None, device_views=device_views, stored_masks=True)
    if cfg.chunk:
        runner.set_chunk(cfg.chunk)
    return env, smp, runner


def advance(env, runner, steps):
    runner.rollout(steps)
    runner.sync()
    env.sync_host()


def assert_flags(env, snap, what):
    per = env.hazards()[1]
    for (lo, hi), st in zip(snap.blocks, snap.state):
        assert np.array_equal(per[lo:hi], st["flags"]), f"{what}: hazard flags of envs [{lo}, {hi}) differ"


def assert_terminal_step(env, snap, cfg):
    """The checkpoint after the step of the first natural end: the env that ended shows dones and
    the oracle's non-zero rewards, terminal infos, and the state of its auto-reset (same step)."""
    ended = 0
    for (lo, hi), st in zip(snap.blocks, snap.state):
        for j in np.nonzero(st["dones"] & (st["rewards"] > 0).any(1))[0]:
            i = lo + int(j)
            ended += 1
            assert env.dones[i], f"config {cfg.id}: env {i} does not show its end"
            assert (env.rewards[i] > 0).any() and np.array_equal(env.rewards[i], st["rewards"][j])
            info = env.infos[i]
            assert info["total_length"] == st["infos"][j]["total_length"] > 0
            assert np.array_equal(info["agent_infos"]["returns"][:cfg.players], env.rewards[i][:cfg.players])
            assert env.agent_selection[i] == 0                         # reset in the same step (Q16)
            assert env.observations["shared"]["phase"][i] == st["observations"]["shared"]["phase"][j]
    assert ended >= 1, f"config {cfg.id}: the oracle shows no natural end at this step"


@pytest.mark.parametrize("cid", lc.IDS)
def test_lategame_rollout_against_oracle(cg, cid):
    cfg = lc.CONFIGS[cid]
    if cfg.kind is not None:
        assert cg._city_of_gold.rollout_kind(cfg.n, cfg.players, True) == cfg.kind
    ref = lc.reference(cid)
    lc.check_conditions(cfg, ref)                          # the case is there
    first = ref.t_star + 1
    env, smp, runner = make(cg, cfg)
    done = 0
    for k in sorted({first, *lc.CHECKPOINTS}):
        advance(env, runner, k - done)
        done = k
        bad = ref.snapshots[k].differences(env, f"config {cid}")
        assert not bad, "\n".join(bad)
        if k == first:
            assert_terminal_step(env, ref.snapshots[k], cfg)
    assert_flags(env, ref.snapshots[lc.HORIZON], f"config {cid}")


def test_lategame_host_loop_every_step(cg):
    """Config F through the host loop, every output of all 130 envs at every step, from the reset
    to 200 steps past the first natural end: the end, its rewards and its auto-reset under a
    per-step check, on envs that diverge within their waves."""
    cfg = lc.CONFIGS["F"]
    steps = lc.reference("F").t_star + 1 + 200
    env = cg.vec.get_vec_env(cfg.n)()
    smp = cg.vec.get_vec_sampler(cfg.n)(cfg.seed)
    env.reset(cfg.seed, cfg.players, cfg.pieces, cg.Difficulty(cfg.difficulty), lc.MAX_STEPS, False)
    run = lc.OracleRun.of(cfg)
    orc, osm = run.parts[0]
    acts = smp.get_actions()
    ends = 0
    for t in range(steps):
        smp.sample(po.stored_masks(env))
        env.step(acts)
        run.step()
        assert po.named_equal(acts, osm.actions) is None, f"F host loop: actions differ at step {t}"
        for nm in lc.FIELDS:
            bad = po.named_equal(getattr(env, nm), getattr(orc, nm))
            assert bad is None, f"F host loop: {nm}.{bad} differs from the oracle at step {t}"
        for nm in lc.PLAIN:
            assert np.array_equal(getattr(env, nm), getattr(orc, nm)), f"F host loop: {nm} differs at step {t}"
        ends += int((env.dones & (env.rewards > 0).any(1)).sum())
    assert ends >= 1, "no natural end: the test lost its case"
    assert np.array_equal(env.hazards()[1], orc.flags())


def test_lategame_rollout_interleaves_with_host_steps(cg):
    """Config A: 3,000 steps of chunked launches, 50 of the host loop, 50 host-view runner steps
    (runner.sample(); runner.step_sync(): the step that publishes itself), chunked launches again
    to 8,000: one consistent state, the oracle's."""
    cfg = lc.CONFIGS["A"]
    ref = lc.reference("A")
    env, smp, runner = make(cg, cfg)
    advance(env, runner, 3000)
    for _ in range(50):
        smp.sample(po.stored_masks(env))
        env.step(smp.get_actions())
    host = cg.vec.get_runner(cfg.n)(env, smp, None, stored_masks=True)
    for _ in range(50):
        host.sample()
        host.step_sync()
    advance(env, runner, lc.HORIZON - 3100)
    snap = ref.snapshots[lc.HORIZON]
    bad = snap.differences(env, "config A interleaved")
    assert not bad, "\n".join(bad)
    assert_flags(env, snap, "config A interleaved")


# ---- against the reference core's recorded late game ------------------------------------------
with open(os.path.join(GOLD, "ref_lategame.json")) as _f:
    META = json.load(_f)
DIGESTS = np.load(os.path.join(GOLD, "ref_lategame_digests.npz"))
SEEDS = [e["seed"] for e in META["envs"]]
BASE, IDX = min(SEEDS), [s - min(SEEDS) for s in SEEDS]   # one batch whose envs BASE + i hold the seeds
REF = [DIGESTS[f"{META['name']}__{k}"] for k in range(len(SEEDS))]


def digest_env(e, actions, i):
    s = slice(i, i + 1)
    return po.step_digest(e.observations[s], e.selected_action_masks[s], e.rewards[s], e.dones[s],
                          e.agent_selection[s], e.infos[s], actions[s])


def make_fixture_batch(cg):
    n = max(IDX) + 1
    env = cg.vec.get_vec_env(n)()
    smp = cg.vec.get_vec_sampler(n)(BASE)
    env.reset(BASE, META["n_players"], META["n_pieces"], cg.Difficulty(META["difficulty"]), META["max_steps"], False)
    return n, env, smp


def test_lategame_host_loop_matches_reference_digests(cg):
    n, env, smp = make_fixture_batch(cg)
    acts = smp.get_actions()
    for t in range(META["steps"] + 1):
        for k, i in enumerate(IDX):
            assert digest_env(env, acts, i) == REF[k][t].tobytes(), \
                f"seed {SEEDS[k]} (env {i}) differs from the reference after {t} steps"
        if t < META["steps"]:
            smp.sample(po.stored_masks(env))
            env.step(acts)


def test_lategame_rollout_matches_reference_digests(cg):
    """The same seeds through launches of 37 steps (ends fall at every position of a launch),
    against the reference's digests at every 500th step."""
    n, env, smp = make_fixture_batch(cg)
    assert cg._city_of_gold.rollout_kind(n, META["n_players"], True) == "duo"
    runner = cg.vec.get_runner(n)(env, smp, None, stored_masks=True)   # host views: sync() publishes
    runner.set_chunk(37)
    acts = runner.get_actions()
    for t in range(500, META["steps"] + 1, 500):
        runner.rollout(500)
        runner.sync()
        for k, i in enumerate(IDX):
            assert digest_env(env, acts, i) == REF[k][t].tobytes(), \
                f"seed {SEEDS[k]} (env {i}) differs from the reference after {t} steps"


# ---- a map-generation failure at an auto-reset inside a launch --------------------------------
def test_mapgen_failure_at_autoreset_inside_rollout(cg):
    """Map generation gives up after its bounded attempts (an error report by design).  At
    env.reset() that raises; here it happens at the auto-reset of env 105 in step 7,326 of a
    rollout: the run equals the oracle at 7,000 steps, the launch past the failure raises at
    runner.sync(), F_MAPGEN_FAIL is on that env alone, and the handle recovers with a reset (the
    oracle goes on from its own state: a reset leaves Info and the players' counters alone)."""
    c = lc.MAPGEN_CASE
    n, seed = c["n"], c["seed"]
    env = cg.vec.get_vec_env(n)()
    smp = cg.vec.get_vec_sampler(n)(seed)
    env.reset(seed, c["players"], c["pieces"], cg.Difficulty(c["difficulty"]), c["max_steps"], False)
    runner = cg.vec.get_runner(n)(env, smp, None, device_views=True, stored_masks=True)
    runner.set_chunk(c["chunk"])
    run = lc.OracleRun(((0, n),), seed, c["players"], c["pieces"], c["difficulty"], c["max_steps"])
    orc, osm = run.parts[0]
    for _ in range(c["checkpoint"]):
        run.step()
    advance(env, runner, c["checkpoint"])
    bad = lc.snapshot(run).differences(env, "before the failure")
    assert not bad, "\n".join(bad)
    assert not (env.hazards()[1] & po.F_MAPGEN_FAIL).any()

    past = 500                                             # to 7,500 steps: past the failing step
    first = None
    for t in range(c["checkpoint"], c["checkpoint"] + past):
        try:
            run.step()
        except RuntimeError:
            first = t if first is None else first
            run.steps_done += 1                            # (the oracle finished the step for every other env)
    assert first == c["fail_step"] and list(np.nonzero(orc.flags() & po.F_MAPGEN_FAIL)[0]) == [c["fail_env"]]
    runner.rollout(past)
    with pytest.raises(RuntimeError, match="generate map"):
        runner.sync()
    failed = np.nonzero(env.hazards()[1] & po.F_MAPGEN_FAIL)[0]
    assert list(failed) == [c["fail_env"]]

    seed2 = 4321                                           # the handle recovers
    smp2 = cg.vec.get_vec_sampler(n)(seed2)
    env.reset(seed2, c["players"], c["pieces"], cg.Difficulty(c["difficulty"]), c["max_steps"], False)
    runner2 = cg.vec.get_runner(n)(env, smp2, None, device_views=True, stored_masks=True)
    runner2.set_chunk(c["chunk"])
    advance(env, runner2, 100)
    orc.reset(seed2, c["players"], c["pieces"], c["difficulty"], c["max_steps"])
    run.parts = [(orc, po.OracleSampler(n, seed2))]
    for _ in range(100):
        run.step()
    bad = lc.snapshot(run).differences(env, "after the reset")
    assert not bad, "\n".join(bad)
