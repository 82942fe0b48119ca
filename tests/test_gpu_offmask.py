"""GPU: host actions inside their heads that the mask does not allow, through env.step,
env.step_device and runner.step(), and every rollout kernel started from the state they leave
(tests/offmask_cases.py has the cases; tests/test_offmask_cpu.py asserts on the oracle alone what
each reaches, and holds the oracle to the unmodified reference on such streams).

The reference's step never reads the mask (environment.cpp:91-181), so such an action is executed
as it stands: u8 counters wrap, moves leave the map.  The engine restates the step on registers and
is held to the oracle bit for bit: both sides walk the same list of ops (driver_cases.Harness), all
six views are compared over named fields after every op -- an M op is one step -- and the hazard
flags per env at the end of every case.  COG_HAZ_BAD_ACTION must stay clear: no index leaves its head.

  kinds x paths    single, replace, all, play, special, remove, move, shop (200 envs) and sweep (261:
                   every (head, value) pair three times a step) through each of the three paths; 60 to
                   90 steps, 4 players, HARD, max_steps 100000, so that the wrapped state lives on
  players / ends   single and all with 3, 2, 1 players, and with 4 to 1 players at max_steps 12
                   (finish_episode's Info counters and rewards, the auto-reset out of wrapped states)
  auto-reset off   every env ended, then 15 steps of arbitrary bytes: the dead step changes nothing
  hand-overs       X, 30 M steps, driver(30), 30 M steps, driver(30) for each of the 18 step drivers at
                   max_steps 100000 and 40; runner.step() is the last path before each driver (no
                   compact deck image may survive it into a trio launch)
  two shards       the same for T20 and S20 on a handle of two shards (301 envs; M through env.step there)
  big batches      16,385 (pipe) and 32,769 (one-wave) envs: M(15) S50 M(15) T20, the oracle threaded
  policy_features  after 60 `all` steps, float32 and bfloat16 bit for bit against
                   tests/policy_features_ref.py (records with bytes of 255, sums past 256)
  reference        the 27 streams of tests/golden/ref_offmask.json on the engine against the
                   reference's own digests, every step
(The rows under the launcher's switches are tests/launch_form_cases.py's offmask-* rows.)

Durations on the MI355X and which cases fail on two value-only mutations of step_regs: DESIGN.md
section 5, "Off-mask host actions".
"""
import json
import os

import numpy as np
import pytest

import driver_cases as dc
import offmask_cases as oc
import policy_features_ref as fr
import pyoracle as po

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def walk(cg, n, seq, **kw):
    """Every case ends with C, which compares the hazard flags per env (COG_HAZ_BAD_ACTION among them:
    on no env, since no index leaves its head) before it clears them."""
    assert seq[-1] == "C"
    return dc.run(dc.Harness(cg, n, oc.SEED, **kw), seq)


@pytest.mark.parametrize("name", list(oc.KIND_CASES))
def test_every_kind_through_every_path(cg, name):
    n, seq = oc.KIND_CASES[name]
    walk(cg, n, seq)


@pytest.mark.parametrize("name", list(oc.PLAYER_CASES))
def test_players_and_episode_ends(cg, name):
    n, seq = oc.PLAYER_CASES[name]
    h = walk(cg, n, seq)
    if seq[0][5] == 12:
        assert h.ends >= 50, h.ends


def test_autoreset_off_dead_steps_change_nothing(cg):
    n, seq = oc.AUTORESET_OFF_CASE
    h = dc.Harness(cg, n, oc.SEED)
    before = None
    for k, op in enumerate(seq):
        try:
            h.apply(op)
        except AssertionError as e:
            raise AssertionError(f"{e}\n  after the sequence {seq[:k + 1]!r}") from None
        if k + 1 == oc.AUTORESET_OFF_ALL_DONE_AT:
            assert np.asarray(h.env.dones).all()
            before = {nm: np.array(getattr(h.env, nm), copy=True) for nm in dc.FIELDS + dc.PLAIN}
        elif before is not None and op[0] == "M" and k < oc.AUTORESET_OFF_ALL_DONE_AT + 15:
            for nm in dc.FIELDS:
                assert po.named_equal(getattr(h.env, nm), before[nm]) is None, f"a dead step changed {nm} (op {k})"
            for nm in dc.PLAIN:
                assert np.array_equal(getattr(h.env, nm), before[nm]), f"a dead step changed {nm} (op {k})"


@pytest.mark.parametrize("name", list(oc.HANDOVER_CASES))
def test_handover_to_every_driver(cg, name):
    n, seq = oc.HANDOVER_CASES[name]
    walk(cg, n, seq)


@pytest.mark.parametrize("driver", list(oc.SHARD_CASES))
def test_handover_on_two_shards(cg, driver):
    n, seq = oc.SHARD_CASES[driver]
    h = dc.Harness(cg, n, oc.SEED, device=[0, 0])
    assert h.env.num_shards == 2
    assert seq[-1] == "C"                                    # (the flags per env, compared before the clear)
    dc.run(h, seq)


@pytest.mark.parametrize("kind", list(dc.BIG_SIZES))
def test_handover_at_the_big_batches(cg, kind):
    n = dc.BIG_SIZES[kind]
    assert cg._city_of_gold.rollout_kind(n, 4, True) == kind
    walk(cg, n, oc.BIG_HANDOVER, threads=po.host_threads())


def test_policy_features_after_offmask_steps(cg):
    import torch
    n, seq = oc.FEATURES_CASE
    h = dc.run(dc.Harness(cg, n, oc.SEED), seq)
    h.compare_hazards("after the 60 steps")
    piles = np.ascontiguousarray(h.orc.observations["player_data"]["obs"]).view(np.uint8).reshape(n, 4, 5, 21).astype(int)
    assert (piles == 255).any() and (piles.sum(2) > 255).any(), "no byte of 255, or no card total past 255"
    for radius in (1, 4):
        want = fr.oracle_features(h.orc, 4, radius)
        for dtype in (torch.float32, torch.bfloat16):
            got = cg.policy_features(h.env, radius, dtype=dtype)
            for nm, g, w in zip(("vec", "local"), got, want):
                if dtype == torch.float32:
                    gb, wb = g.cpu().numpy().view(np.uint32), np.ascontiguousarray(w).view(np.uint32)
                else:
                    gb, wb = g.view(torch.int16).cpu().numpy().view(np.uint16), fr.to_bf16_bits(w)
                if not np.array_equal(gb, wb):
                    i = tuple(int(k) for k in np.argwhere(gb != wb)[0])
                    raise AssertionError(f"radius {radius}, {dtype}: {nm} differs from the reference, first at {i}: "
                                         f"bits {int(gb[i]):#x}, reference {int(wb[i]):#x} ({float(w[i])})")


with open(os.path.join(GOLD, "ref_offmask.json")) as _f:
    GROUPS = json.load(_f)["groups"]
DIGESTS = np.load(os.path.join(GOLD, "ref_offmask_digests.npz"))["digests"]
_AT = np.concatenate([[0], np.cumsum([s + 1 for g in GROUPS for s in g["steps"]])])


@pytest.mark.parametrize("gi", range(len(GROUPS)), ids=[f"{g['kind']}-{g['n_players']}p" for g in GROUPS])
def test_engine_matches_the_reference_on_offmask_streams(cg, gi):
    """The group as one batch: env i is the stream of index i (its seed, its sampler, its own generator
    of altered actions); the kept ones are compared with the reference's digests at every step they hold."""
    g = GROUPS[gi]
    first = sum(len(q["index"]) for q in GROUPS[:gi])
    ref = [DIGESTS[_AT[first + k]:_AT[first + k + 1]] for k in range(len(g["index"]))]
    n = max(g["index"]) + 1
    env, smp = cg.vec.get_vec_env(n)(), cg.vec.get_vec_sampler(n)(g["seed"])
    env.reset(g["seed"], g["n_players"], 3, cg.HARD, 100000, False)
    streams = [oc.Stream(g["kind"], g["n_players"], i) for i in range(n)]
    acts = np.zeros(n, dtype=po.ACTION)
    for t in range(max(g["steps"]) + 1):
        for k, i in enumerate(g["index"]):
            if t <= g["steps"][k]:
                s = slice(i, i + 1)
                d = po.step_digest(env.observations[s], env.selected_action_masks[s], env.rewards[s], env.dones[s],
                                   env.agent_selection[s], env.infos[s], acts[s])
                assert d == ref[k][t].tobytes(), f"{g['kind']}, {g['n_players']} players: env {i} leaves the reference at step {t}"
        smp.sample(env.selected_action_masks)
        legal = np.array(smp.get_actions(), copy=True)
        for i in range(n):
            acts[i:i + 1] = streams[i].next_actions(legal[i:i + 1])[0]
        env.step(acts)
