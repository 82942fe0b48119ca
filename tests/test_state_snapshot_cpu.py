"""CPU: the method behind tests/test_gpu_state_snapshot.py, on the oracle alone (tests/snapshot_cases.py).

The oracle has no state setter, so the GPU tests hold a restore to a replay and a fork to 1-env
twins.  Here: a replayed oracle equals the original at the snapshot point in every view; env i of
an OracleVec(n) equals an OracleVec(1) seeded seed + i across auto-resets; and every GPU case
reaches what it is for -- episode ends between snapshot and restore, maps that differ between the
two points, decks with a card type >= 8 at the snapshot point of the wide case.
"""
import numpy as np
import pytest

import driver_cases as dc
import pyoracle as po
import snapshot_cases as sc


def oracle_prefix(n, reset, steps, sampler_seed=sc.SAMPLER_SEED, driver="H"):
    h = dc.Harness(None, n, sampler_seed)
    acts = sc.record_prefix(h, reset, steps, driver)
    return h, acts


@pytest.mark.parametrize("players", [4, 3, 2, 1])
def test_replay_equals_the_original_at_the_snapshot_point(players):
    reset = sc.reset_op(players)
    h, acts = oracle_prefix(sc.SIZES[0], reset, sc.PREFIX)
    assert len(acts) == sc.PREFIX
    orc = sc.replay(sc.SIZES[0], reset, acts)
    assert sc.views_differ(orc, h.orc) is None
    assert np.array_equal(orc.flags(), h.orc.flags())
    # and it goes on alike: the original's further actions give the same views, auto-resets included
    ends0 = h.ends
    for t in range(sc.AFTER):
        dc.run(h, [("H", 1)])
        orc.step(h.last)
        bad = sc.views_differ(orc, h.orc)
        assert bad is None, f"step {t} after the snapshot point: {bad} differs"
    assert h.ends > ends0


@pytest.mark.parametrize("players", [4, 2])
def test_env_i_of_a_batch_is_the_one_env_batch_seeded_seed_plus_i(players):
    n, steps = sc.SIZES[0], sc.TWIN_STEPS
    seed = 0xFFFFFFFF - 20                                   # (seed + i wraps inside the batch)
    reset = ("X", seed, players, sc.PIECES, sc.DIFFICULTY, sc.MAX_STEPS)
    h = dc.Harness(None, n, sc.SAMPLER_SEED)
    dc.run(h, [reset])
    src = np.arange(n)
    tw = sc.Twins(reset, [], src)
    assert sc.views_differ(tw.views(), h.orc) is None
    ends = np.zeros(n, dtype=np.int64)
    for t in range(steps):
        dc.run(h, [("H", 1)])
        tw.step(h.last)
        ends += np.asarray(h.orc.dones, dtype=np.int64)
        bad = sc.views_differ(tw.views(), h.orc)
        assert bad is None, f"step {t}: {bad} of the twins differs from the batch"
    assert np.array_equal(tw.flags(), h.orc.flags())
    assert ends.min() >= 2, f"an env crossed {int(ends.min())} auto-resets, the case needs two"


def maps_of(orc):
    return np.array(orc.observations["shared"]["map"], copy=True)


@pytest.mark.parametrize("players", [4, 3, 2, 1])
@pytest.mark.parametrize("n", sc.SIZES + (sc.SHARD_N,))
def test_undo_case_crosses_episode_ends_and_changes_maps(n, players):
    reset = sc.reset_op(players)
    h, _ = oracle_prefix(n, reset, sc.PREFIX)
    maps0, ends0 = maps_of(h.orc), h.ends
    dc.run(h, [("H", sc.BETWEEN)])
    assert h.ends - ends0 >= 1, "no episode end between snapshot and restore"
    changed = (maps_of(h.orc) != maps0).reshape(n, -1).any(1)
    assert changed.all() if n == 1 else changed.sum() >= n // 2, f"{int(changed.sum())} of {n} maps differ at restore time"
    ends1 = h.ends
    dc.run(h, [("H", sc.AFTER)])
    assert h.ends - ends1 >= 1, "no episode end after the restore"


def test_other_reset_changes_what_the_handle_remembers():
    assert sc.OTHER_RESET[2] != 4 and sc.OTHER_RESET[5] != sc.MAX_STEPS
    # 2 players never take the trio (cog_abi.cpp trio_ok): the restore has to bring 4 back for T20
    assert sc.OTHER_RESET[2] < 3


def test_wide_case_holds_wide_decks_at_the_snapshot_point():
    w = sc.WIDE
    reset = sc.reset_op(w["players"], w["seed"], w["max_steps"])
    h, acts = oracle_prefix(w["n"], reset, w["prefix"], driver=w["driver"])
    wide = dc.wide_envs(h.orc)
    assert w["n"] // 4 <= wide < w["n"], f"{wide} envs hold a card of type >= 8: the case needs wide and narrow decks"
    assert sc.views_differ(sc.replay(w["n"], reset, acts), h.orc) is None


@pytest.mark.parametrize("n_dst,n_src", [(70, 70), (33, 70), (70, 1)])
def test_fork_case_sources_and_episode_ends(n_dst, n_src):
    reset = sc.reset_op()
    h, acts = oracle_prefix(n_src, reset, sc.PREFIX)
    for name, src in sc.fork_sources(n_dst, n_src).items():
        assert src.shape == (n_dst,) and src.min() >= 0 and src.max() < n_src
        if name == "random" and n_src > 1:
            assert len(set(src.tolist())) < n_dst, "no index repeats"
        if name == "one":
            assert len(set(src.tolist())) == 1
    src = sc.fork_sources(n_dst, n_src)["random"]
    tw = sc.Twins(reset, acts, src)
    want = {nm: np.asarray(getattr(h.orc, nm))[src] for nm in sc.VIEWS}
    assert sc.views_differ(tw.views(), want) is None, "a replayed twin is not the snapshot's source env"
    osm = po.OracleSampler(n_dst, sc.SAMPLER_SEED + 1)
    for _ in range(sc.FORK_STEPS + sc.FORK_ROLLOUT):
        osm.sample(tw.view("selected_action_masks"))
        tw.step(osm.actions.copy())
    assert tw.ends >= n_dst, f"{tw.ends} episode ends in {n_dst} forks"
    if n_src > 1:                                            # forks of one source diverge through their samplers
        one = sc.Twins(reset, acts, sc.fork_sources(n_dst, n_src)["one"])
        osm = po.OracleSampler(n_dst, sc.SAMPLER_SEED + 1)
        for _ in range(5):
            osm.sample(one.view("selected_action_masks"))
            one.step(osm.actions.copy())
        obs = np.ascontiguousarray(one.view("observations")).view(np.uint8).reshape(n_dst, -1)
        assert len({r.tobytes() for r in obs}) > 1, "forks of one env did not diverge"
