"""CPU: what the late-game configurations (tests/lategame_cases.py) reach on the oracle, and the
oracle against the reference core in the late game.

  census      per configuration A-F, the oracle alone over the whole horizon: natural ends (a player
              reaches the end hex), ends by number of winners, specials played per card, remove
              actions, hazard flags -- with the minima every configuration must keep, so that a
              reader without a GPU sees what each test of tests/test_gpu_lategame.py reaches
  fixture     the oracle against tests/golden/ref_lategame_digests.npz (the unmodified reference
              core: 8 seeds, HARD, 4 players, 1 piece, stored masks, 6,000 steps, every step)
  live        where the reference library is built: the oracle against the reference itself, every
              named field at every step, on the fixture's seeds and on seeds 2000..2023
"""
import json
import os

import numpy as np
import pytest

import lategame_cases as lc
import pyoracle as po

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def load_fixture():
    with open(os.path.join(GOLD, "ref_lategame.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLD, "ref_lategame_digests.npz"))


META, DIGESTS = load_fixture()


@pytest.mark.parametrize("cid", lc.IDS)
def test_census_conditions(cid):
    cfg = lc.CONFIGS[cid]
    c = lc.reference(cid)                                  # (raises if the oracle raises)
    print(f"config {cid}: {c.row()}")
    for (lo, hi), b in zip(cfg.blocks, c.per_block):
        print(f"  envs [{lo}, {hi}): {b.row()}")
    lc.check_conditions(cfg, c)
    assert c.t_star is not None and c.t_star + 1 in c.snapshots
    assert all(k in c.snapshots for k in lc.CHECKPOINTS)


def test_census_counts_by_effective_action():
    """The census on hand-made steps: the action counted is the one the step takes (play >
    play_special > move > get_from_shop > remove), an end is natural when a reward is positive."""
    a = np.zeros((1, 6), dtype=po.ACTION)
    a["play_special"][0] = [16, 21, 17, 0, 0, 3]           # cards 15, 20, 16; a non-special card last
    a["play"][0, 2] = 1                                    # a play hides the special
    a["remove"][0] = [5, 0, 0, 4, 4, 0]                    # hidden by the special; counted; hidden by a move
    a["move"][0, 4] = 2
    dones = np.array([[True, True, False, True, False, False]])
    rew = np.zeros((1, 6, 4), dtype=np.float32)
    rew[0, 0] = [3, -1, -1, -1]                            # one winner
    rew[0, 1] = [2, 2, -2, -2]                             # two winners
    rew[0, 2] = [3, -1, -1, -1]                            # no done: stale rewards
    ends, first, by_winners, specials, removes = lc._count(a, dones, rew, 4)   # (env 3: done at max_steps)
    assert ends == 2 and by_winners == {1: 1, 2: 1}
    assert list(first) == [0, 0, -1, -1, -1, -1]
    assert specials == {15: 1, 16: 0, 17: 0, 18: 0, 19: 0, 20: 1}
    assert removes == 1


def test_lategame_fixture_counts():
    """The fixture itself keeps its case: 8 seeds with a natural end each, every special >= 20
    times in all, digests for every step."""
    envs = META["envs"]
    assert len(envs) == 8 and META["steps"] == 6000
    assert (META["n_players"], META["n_pieces"], META["difficulty"], META["mode"]) == (4, 1, 2, "sto")
    assert all(len(e["natural_ends"]) >= 1 for e in envs)
    for c in lc.SPECIALS:
        assert sum(e["specials"][str(c)] for e in envs) >= 20, c
    for k in range(8):
        assert DIGESTS[f"{META['name']}__{k}"].shape == (6001, 8)


@pytest.mark.parametrize("k", range(8))
def test_oracle_matches_lategame_fixture(k):
    """Every recorded reference digest equals the oracle's, and the counts recorded beside them
    are what the oracle does."""
    e = META["envs"][k]
    ref = DIGESTS[f"{META['name']}__{k}"]
    run = lc.OracleRun(((0, 1),), e["seed"], META["n_players"], META["n_pieces"], META["difficulty"],
                       META["max_steps"])
    orc, osm = run.parts[0]
    ends = []
    for t in range(META["steps"] + 1):
        got = po.step_digest(orc.observations, orc.selected_action_masks, orc.rewards, orc.dones,
                             orc.agent_selection, orc.infos, osm.actions)
        assert got == ref[t].tobytes(), f"seed {e['seed']}: the oracle differs from the reference after {t} steps"
        if t and orc.dones[0] and (orc.rewards[0] > 0).any():
            ends.append(t - 1)
        if t < META["steps"]:
            run.step()
    assert ends == e["natural_ends"]
    assert not orc.flags(0) & po.REF_UNSAFE


LIVE_SEEDS = [e["seed"] for e in META["envs"]] + list(range(2000, 2024))


@pytest.mark.skipif(not po.ref_available(), reason="the reference library is not built here")
@pytest.mark.parametrize("seed", LIVE_SEEDS)
def test_oracle_matches_live_reference(seed):
    """HARD, 4 players, 1 piece, stored masks, 6,000 steps: every named field of every output and
    the sampled actions at every step.  The oracle steps first: the reference built against
    libstdc++ 11 cannot survive a REF_UNSAFE hazard, so the seed stops before the reference would
    meet one."""
    steps = 6000
    ref, rsm = po.RefVec1(), po.RefSampler1(seed)
    orc, osm = po.OracleVec(1), po.OracleSampler(1, seed)
    orc.reset(seed, 4, 1, 2, lc.MAX_STEPS)
    assert not orc.flags(0) & po.REF_UNSAFE, f"seed {seed}: the reference cannot generate this map"
    ref.reset(seed, 4, 1, 2, lc.MAX_STEPS)
    for t in range(steps):
        osm.sample(po.stored_masks(orc))
        orc.step(osm.actions)
        if orc.flags(0) & po.REF_UNSAFE:
            break
        rsm.sample(po.stored_masks(ref))
        ref.step(rsm.actions)
        assert po.named_equal(rsm.actions, osm.actions) is None, f"seed {seed}: actions differ at step {t}"
        for nm in lc.FIELDS:
            a, b = getattr(ref, nm), getattr(orc, nm)
            if a.tobytes() != b.tobytes():                 # (equal records: equal named fields; else the padding may differ)
                bad = po.named_equal(a, b)
                assert bad is None, f"seed {seed}: {nm}.{bad} differs from the reference at step {t}"
        for nm in lc.PLAIN:
            assert np.array_equal(getattr(ref, nm), getattr(orc, nm)), f"seed {seed}: {nm} differs at step {t}"
