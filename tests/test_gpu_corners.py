"""GPU: the corners of the reset parameters (tests/corner_cases.py has the tables,
tests/test_corners_cpu.py counts on the oracle alone what each row relies on and pins the oracle to
the reference there).  cog_env_reset takes 1..4 players and any max_steps; the rest of the suite
runs 2..4 players and a max_steps of 8 and more.  Every row walks a driver_cases.Harness: all six
views bit-exact against the oracle after every op, the hazard flags per env at the end, a mismatch
names the sequence up to the failing op.

  solo          one player, max_steps 8: the next agent is the acting agent, which every step kernel
                special-cases.  X d H d for each of the 18 step drivers and X a b a for all 36 pairs
                of H, G, T20, S20, L, Rr, at 200 and 33 envs (selected and stored masks are both the
                duo at these sizes)
  solo_long     one player, one piece, max_steps 100,000, stored masks under Hs, S20, S1000, Ls and
                Hs(200) G(100): 300 steps without an episode end, the solo player moves, buys and
                plays specials (171 of 200 envs hold a card type >= 8 at the end)
  tiny          max_steps 0, 1, 2, 3 with 4, 3, 2, 1 players, X d H d: all 18 drivers at (4p, 0),
                (4p, 1), (1p, 0), (1p, 2), the six above elsewhere; 200 and 33 envs, at max_steps 0
                70 (a full workgroup and one of 6) and 33 with 24 steps per op: every env ends, parks
                and regenerates its map at every step of every launch (k_env_fixup, the park list,
                the dirty-map list and its overflow branch, the speculative sample, the staged publish)
  state         lean_clock and cdeck_ok across 4p/8 -> 1p/8 -> 4p/0 -> 3p/1 -> reset_default ->
                4p/40; auto-reset off at max_steps 0 (every env done after one step, dead steps
                after), back on after a reset_default; invalidate_device and a hazard clear between
                launches at max_steps 0; two shards (301 envs) at (1p, 8) and (4p, 0); host views
                first touched after device work at (4p, 0)
  big           the hand-overs of driver_cases.BIG_CASES at 16,385 envs (k_env_rollout_pipe) and
                32,769 (the one-wave k_env_rollout) with one player: both mask sources take them
  refused       resets cog_env_reset refuses before any launch (0 and 5 players, a difficulty out of
                range) and a reset with no map piece (map generation fails for the whole batch, as on
                the oracle) leave a handle that goes on as the oracle does

What these rows found: 19 of them (every T and Th driver of tiny at (4p, 0), T20 at (3p, 0), the
three state rows, two-shards-4p-ms0 and lazy-views-4p-ms0) differed from the oracle at their first
trio launch, observations.shared.map first.  The trio's lean step checks turn_counter >= max_steps
at turn ends alone; at max_steps 0 the first step after a reset, which ends no turn, ends the
episode.  cog_abi.cpp's trio_ok now keeps a batch reset with max_steps 0 off the trio (the duo /
pipe / wave run the full step); the kernels are unchanged.  One player needed no fix.

Durations on the MI355X (pytest --durations=0, the oracle side included; the oracle's resets with
map generation, 0.34 ms each, are most of a tiny row): solo 0.02-0.35 s (108 rows, 9.9 s together);
solo_long 0.02-0.05 s; tiny 0.03-1.12 s (288 rows, 123 s together; the longest are the max_steps 1
rows at 200 envs, about 4,400 oracle resets each); state 0.6-1.3 s; two shards 0.3 and 2.75 s
(12,040 oracle resets); views first touched 1.3 s; big pipe 1.3-1.6 s, wave 2.6-3.0 s (17 s
together); refused resets 0.13 and 0.04 s; no map piece 0.01 s.  418 cases, 159 s together.

That the cases bite, tried on five scratch builds of cog_engine.hip (never committed; every edit keeps its
addresses in range), the whole GPU suite (1,265 tests) run against each:
  build 1, step_regs' load_actionmask taking the else branch with one player (`R.sel = R.stn`
    although na == ag): 182 fail, the other 1,083 GPU tests pass -- 100 of the 108 solo rows (all but
    the pairs of G and Rr), the 5 solo_long rows, the 48 tiny rows at (1p, 2) and (1p, 3) (at
    max_steps 0 and 1 no episode outlives its first turn end), the 8 big rows, state[players-and-ms0],
    two-shards-1p-ms8, the refused resets through the C ABI (a 1-player batch), the 16 corners-* launch-form
    rows, the 1-player GAE window and the 1-player cog_env loop
  build 2, step_regs without `if (na == ag) R.cells_n = R.cells_a`: nothing fails, neither a new case nor an
    old one (1,265 pass).  The edit cannot give a wrong byte: cells_n is read only where the current
    player is not the acting one (`cur_is_ag` false, which the branch before it rules out when na == ag)
    and by the duo stepper at a turn change (ag1 != ag: never with one player); no store writes it.  The
    line keeps a register tidy and decides nothing; it is reported as such, not as a gap of the rows.
  build 3a, store_outputs and store_private storing the next player's stored mask although na == ag.
    Dropping `na != ag` alone stores nothing there (with one player the step never writes R.stn, so
    its difference from the step-start image is empty); the edit tried compares it with the acting
    player's new mask instead (`mask_diff_granules(bn, na != ag ? S.stn : ba)`), so that the stale
    mask lands on the record and the head just stored: 198 fail, the other 1,067 pass --
    106 of the 108 solo rows (all but Rr-Rr), 3 solo_long rows, the 60 tiny rows at (1p, 1), (1p, 2) and (1p, 3),
    the 8 big rows, state[players-and-ms0], two-shards-1p-ms8, the refused resets through the C ABI, the 16
    corners-* launch-form rows, the 1-player GAE window and the 1-player cog_env loop: the one-player branch of
    k_env_step's, k_env_step_pub's and the lane drivers' stores is seen
  build 3b, the duo storer's `if (na != ag)` dropped (it compares with its own image of the record,
    which the acting player's store has just updated): 91 fail, the other 1,174 pass -- the 58 solo rows
    with a T, Th or S driver, 2 solo_long rows, 17 one-player tiny rows at max_steps 1 to 3, state[players-and-ms0],
    two-shards-1p-ms8 and the 12 corners-* launch-form rows other than pipe and wave
  build 4, the fix-up's reload after an auto-reset skipped when the ended episode's turn counter is 0
    (`if (S.g0.w != 0u) load_env(...)` in rollout_pass<FIX>): 74 fail, the other 1,191 pass -- the 44
    tiny rows of the T, Th and S drivers at max_steps 0 (all players; the other drivers launch one step at a
    time: no fix-up), the
    three state rows, two-shards-4p-ms0, lazy-views-4p-ms0, the 16 corners-* launch-form rows, and the 8
    big rows: among 16,385 one-player envs a few end at their first step after a reset too (2 within 60 steps on
    the oracle: maps flagged Q9_OOB / B_START_LT4, a player standing on an end hex).  One old test sees it as well, test_gpu_lategame's
    test_lategame_rollout_against_oracle[B]: such ends were not wholly new to the suite
"""
import numpy as np
import pytest

import corner_cases as cc
import driver_cases as dc
import pyoracle as po

pytestmark = pytest.mark.gpu


def walk(cg, table, case, **kw):
    n, seq = cc.TABLES[table][case]
    h = dc.run(dc.Harness(cg, n, cc.SAMPLER_SEED, **cc.KINDS[table], **kw), seq)
    h.compare_hazards("at the end")
    return h, seq


def check_ends(h, seq, skip=()):
    """Every step op holds an episode end; with auto-reset on at max_steps 0 every env ends at every step."""
    at = cc.ms_at(seq)
    for k in cc.step_ops(seq):
        ms, on = at[k]
        if ms == 0 and on:
            assert h.op_ends[k] == h.n * seq[k][1], f"op {k} {seq[k]!r}: {h.op_ends[k]} ends, not n x steps"
        elif k not in skip:
            assert h.op_ends[k] >= 1, f"op {k} {seq[k]!r} holds no episode end: {h.op_ends}"


@pytest.mark.parametrize("case", list(cc.SOLO))
def test_solo(cg, case):
    h, seq = walk(cg, "solo", case)
    assert cg._city_of_gold.rollout_kind(h.n, 1, False) == cg._city_of_gold.rollout_kind(h.n, 1, True) == "duo"
    check_ends(h, seq)


@pytest.mark.parametrize("case", list(cc.SOLO_LONG))
def test_solo_long(cg, case):
    h, seq = walk(cg, "solo_long", case)
    assert h.ends == 0 and dc.wide_envs(h.orc) >= cc.SOLO_LONG_WIDE, (h.op_ends, dc.wide_envs(h.orc))


@pytest.mark.parametrize("case", list(cc.TINY))
def test_tiny(cg, case):
    h, seq = walk(cg, "tiny", case)
    check_ends(h, seq)


@pytest.mark.parametrize("case", list(cc.STATE))
def test_state(cg, case):
    h, seq = walk(cg, "state", case)
    check_ends(h, seq, cc.STATE_NO_END_OPS.get(case, ()))


@pytest.mark.parametrize("case", list(cc.TWO_SHARD))
def test_two_shards(cg, case):
    n, seq = cc.TWO_SHARD[case]
    assert not any(o[0] in dc.SINGLE_SHARD_ONLY for o in seq)
    h, seq = walk(cg, "two_shard", case)
    assert h.env.num_shards == 2 and 0 < h.env.shard_info(0)[1] < n
    check_ends(h, seq)


@pytest.mark.parametrize("case", list(cc.LAZY))
def test_views_first_touched_at_max_steps_0(cg, case):
    h, seq = walk(cg, "lazy", case)
    assert h.views
    check_ends(h, seq)


@pytest.mark.parametrize("case", list(cc.BIG))
def test_big_solo(cg, case):
    n, seq = cc.BIG[case]
    kind = case.split("-")[0]
    assert cg._city_of_gold.rollout_kind(n, 1, True) == cg._city_of_gold.rollout_kind(n, 1, False) == kind
    walk(cg, "big", case, threads=po.host_threads())


# ---- resets that do not take place -----------------------------------------------------------------
def go_on(h, steps=5):
    """All six views and the hazards now, then `steps` host steps, equal the oracle's."""
    h.compare("after the refused reset")
    h.compare_hazards("after the refused reset")
    dc.run(h, [("H", steps)])
    h.compare_hazards("after the host steps")


def test_refused_resets_leave_the_handle_alone(cg):
    """0 players, 5 players and a difficulty out of range are refused before any launch: each raises,
    and the handle goes on as the oracle, which was never reset, does (the players and max_steps of
    the last reset that took place included: the next steps end episodes at max_steps 8).
    cg.Difficulty(3) constructs (the binding's enum takes any int), so the value reaches
    cog_env_reset, whose message the test matches."""
    h = dc.run(dc.Harness(cg, 33, cc.SAMPLER_SEED), [cc.X(77, 3, 8), ("T20", cc.P)])
    for players in (0, 5):
        with pytest.raises(ValueError, match="n_players"):
            h.env.reset(5, players, 3, cg.HARD, 0, False)
        go_on(h)
    bad = cg.Difficulty(3)                                   # (no ValueError here: the engine's check is the one met)
    with pytest.raises(ValueError, match="difficulty"):
        h.env.reset(5, 4, 3, bad, 0, False)
    go_on(h)
    assert h.ends >= 1
    dc.run(h, [("T20", cc.P), ("S20", cc.P)])                # (3 players still: the trio, then the duo)
    h.compare_hazards("at the end")


def test_refused_resets_through_the_c_abi():
    """The same through include/cog.h, where a difficulty out of range reaches cog_env_reset:
    COG_ERR_INVALID with its message, then the views, the hazard flags per env and 5 host steps equal
    the oracle's."""
    import ctypes as C
    import test_gpu_ctypes_abi as abi
    L = abi.lib()
    n, seed = 33, 77
    env, smp = C.c_void_p(), C.c_void_p()
    assert L.cog_env_create(n, 0, C.byref(env)) == 0, L.cog_last_error()
    assert L.cog_sampler_create(n, seed, 0, C.byref(smp)) == 0, L.cog_last_error()
    assert L.cog_env_reset(env, seed, 1, 3, 2, 2, 0) == 0, L.cog_last_error()
    orc, osm = po.OracleVec(n), po.OracleSampler(n, seed)
    orc.reset(seed, 1, 3, 2, 2)
    v = abi.Views()
    assert L.cog_env_get_views(env, C.byref(v)) == 0
    got = dict(observations=abi.view(v.observations, po.OBS, (n,)), selected_action_masks=abi.view(v.selected_action_masks, po.MASK, (n,)),
               infos=abi.view(v.infos, po.INFO, (n,)), rewards=abi.view(v.rewards, np.dtype("<f4"), (n, 4)),
               dones=abi.view(v.dones, np.dtype("?"), (n,)), agent_selection=abi.view(v.agent_selection, np.dtype("u1"), (n,)))
    acts = abi.view(L.cog_sampler_actions(smp), po.ACTION, (n,))
    L.cog_env_hazards.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]

    def same(what):
        acc, per = C.c_uint32(0), (C.c_uint32 * n)()
        assert L.cog_env_hazards(env, C.byref(acc), per) == 0, L.cog_last_error()
        want = orc.flags()
        assert np.array_equal(np.array(per[:], dtype=np.uint32), want), f"{what}: hazard flags differ from the oracle's"
        assert acc.value == int(np.bitwise_or.reduce(want))
        for nm in dc.FIELDS:
            bad = po.named_equal(got[nm], getattr(orc, nm))
            assert bad is None, f"{what}: {nm}.{bad} differs from the oracle"
        for nm in dc.PLAIN:
            assert np.array_equal(got[nm], getattr(orc, nm)), f"{what}: {nm} differs from the oracle"

    ends = 0
    for players, difficulty, word in ((0, 2, b"n_players"), (5, 2, b"n_players"), (4, 3, b"difficulty"), (4, -1, b"difficulty")):
        assert L.cog_env_reset(env, 5, players, 3, difficulty, 0, 0) == -1          # COG_ERR_INVALID
        assert word in L.cog_last_error()
        same(f"after the refused reset ({players} players, difficulty {difficulty})")
        for t in range(5):
            assert L.cog_sampler_sample(smp, v.selected_action_masks, n) == 0, L.cog_last_error()
            osm.sample(orc.selected_action_masks)
            assert L.cog_env_step(env, L.cog_sampler_actions(smp), n) == 0, L.cog_last_error()
            orc.step(osm.actions)
            ends += int(orc.dones.sum())
            same(f"step {t} after the refused reset")
        assert po.named_equal(acts, osm.actions) is None
    assert ends >= 1
    L.cog_sampler_destroy(smp)
    L.cog_env_destroy(env)


def test_reset_without_a_map_piece_fails_as_on_the_oracle(cg):
    """n_pieces = 0: the end piece has nothing to attach to, generation exhausts its attempts for every
    env.  The reset raises on both sides, the flags agree per env, and a valid reset with a trio
    rollout after it matches the oracle."""
    n = 33
    h = dc.Harness(cg, n, cc.SAMPLER_SEED)
    with pytest.raises(RuntimeError, match="[Ff]ailed to generate map"):
        h.orc.reset_threaded(77, 4, 0, 2, 100, 2)             # (the threaded reset goes on past a failed env, as the
    with pytest.raises(RuntimeError, match="[Ff]ailed to generate map"):
        h.env.reset(77, 4, 0, cg.HARD, 100, False)            # engine does: every env is flagged)
    assert (h.orc.flags() & po.F_MAPGEN_FAIL).all()
    h.compare_hazards("after the failed reset")
    dc.run(h, ["C", cc.X(78, 4, 8), ("T20", cc.P)])
    assert h.op_ends[-1] >= 1
    h.compare_hazards("at the end")
