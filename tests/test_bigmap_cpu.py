"""CPU: what the big-map cases (tests/bigmap_cases.py) reach on the oracle, and the oracle against
the reference core on big maps.

  reset grid   every window of the grid is free of error flags; the candidate totals, extents and
               start-piece positions each claims (more than 128 and more than 192 candidates, a box
               of 47 cells or more, a start piece within 2 cells of the box's edge)
  overflow     the overflow window holds its GRID_OVER env and no more than 2 % of the batch
  failures     0 pieces, EASY with 4 pieces and 255 pieces give up in every env
  stepping     per case: auto-resets, moves, moves onto the box's outermost cells, no error flag
  sweep        3,072 seeds at 7-12 pieces, MEDIUM and HARD: the largest placed count and
               |coordinate| against the engine's own limits (kMaxPlaced 96, kMaxCoord 62)
  reference    the oracle against tests/golden/ref_maps_big.json (the unmodified reference core:
               2, 4, 6 and 7 pieces, MEDIUM and HARD, 2 to 4 players)

Run with -s to read the counts.
"""
import json
import os

import numpy as np
import pytest

import bigmap_cases as bc
import pyoracle as po

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("case", bc.RESET_GRID, ids=[c.id for c in bc.RESET_GRID])
def test_reset_grid_window(case):
    orc, g, raised = bc.reset_reference(case)
    over128, over192, wide = int((g["total"] > 128).sum()), int((g["total"] > 192).sum()), int((g["dim"] >= 47).sum())
    print(f"{case.id}: candidates max {g['total'].max()} (> 128 in {over128} envs, > 192 in {over192}), placed max "
          f"{g['placed'].max()}, depth max {g['depth'].max()}, extent max {g['dim'].max()} (>= 47 in {wide}), start "
          f"piece within 2 cells of the edge in {int((g['edge'] <= 2).sum())}, flags {int(np.bitwise_or.reduce(g['flags'])):#04x}")
    assert not raised and not (g["flags"] & bc.ERR).any(), f"{case.id}: the oracle flags {np.nonzero(g['flags'] & bc.ERR)[0]}"
    assert not g["offlat"].any(), f"{case.id}: envs {np.nonzero(g['offlat'])[0]} leave the hex lattice"
    want = bc.REACHES.get(case.id)
    if want:
        assert over128 >= want[0] and over192 >= want[1] and wide >= want[2], \
            f"{case.id} reaches {(over128, over192, wide)}, claimed {want}"


def test_reset_grid_reaches_what_it_claims():
    """Over the grid: a third and a fourth candidate batch, an unflagged box of 47 cells or more,
    a start piece within 2 cells of the box's edge (on a box of 40 cells or more too: the corner
    case), every piece count of the issue."""
    over128 = over192 = wide = corner = far_corner = 0
    for case in bc.RESET_GRID:
        _, g, _ = bc.reset_reference(case)
        ok = (g["flags"] & bc.ERR) == 0
        over128 += int((g["total"] > 128).sum())
        over192 += int((g["total"] > 192).sum())
        wide += int((ok & (g["dim"] >= 47)).sum())
        corner += int((ok & (g["edge"] <= 2)).sum())
        far_corner += int((ok & (g["edge"] <= 2) & (g["dim"] >= 40)).sum())
    print(f"reset grid: {over128} envs past 128 candidates, {over192} past 192, {wide} unflagged boxes of >= 47 cells, "
          f"{corner} start pieces within 2 cells of the edge ({far_corner} of them on boxes of >= 40 cells)")
    assert over128 >= 100 and over192 >= 2
    assert wide >= 3
    assert corner >= 500 and far_corner >= 10
    have = {(c.pieces, c.difficulty, c.players) for c in bc.RESET_GRID if c.n == bc.N}
    assert {(pc, d, 4) for pc in (2, 4, 5, 6, 7, 8, 9) for d in (1, 2)} <= have
    assert {(pc, d, pl) for pc in (6, 7) for d in (1, 2) for pl in (2, 3)} <= have
    assert {(pc, 0, 4) for pc in (1, 2, 3)} <= have
    assert {c.n for c in bc.RESET_GRID if c.pieces == 7} >= {1, 65, bc.N}


def test_overflow_window():
    case = bc.OVERFLOW
    orc, g, raised = bc.reset_reference(case)
    flagged = np.nonzero(g["flags"] & bc.ERR)[0]
    print(f"overflow {case.id} seed {case.seed}: flagged envs {list(flagged)}, their boxes "
          f"{[(int(g['dimx'][i]), int(g['dimy'][i])) for i in flagged]}")
    assert not raised                                      # the oracle only sets the flag and goes on
    assert tuple(flagged) == bc.OVERFLOW_ENVS
    assert 1 <= flagged.size <= bc.MAX_FLAGGED_SHARE * case.n
    assert all(g["flags"][i] & bc.ERR == po.F_GRID_OVER for i in flagged)
    assert all(max(g["dimx"][i], g["dimy"][i]) > 49 for i in flagged)


def test_off_lattice_window():
    """The window holds its env whose generation leaves the hex lattice after a failed travel
    placement (recursion depth >= 1), and the oracle finishes every map of it without a flag."""
    case = bc.OFF_LATTICE
    orc, g, raised = bc.reset_reference(case)
    off = np.nonzero(g["offlat"])[0]
    print(f"off-lattice {case.id} seed {case.seed}: envs {list(off)}, {list(g['offlat'][off])} hexes off the lattice, "
          f"depth {list(g['depth'][off])}, placed {list(g['placed'][off])}, boxes "
          f"{[(int(g['dimx'][i]), int(g['dimy'][i])) for i in off]}")
    assert not raised and not (g["flags"] & bc.ERR).any()
    assert tuple(off) == bc.OFF_LATTICE_ENVS and (g["depth"][off] >= 1).all()


@pytest.mark.parametrize("case", bc.FAILURES, ids=[c.id for c in bc.FAILURES])
def test_failures_in_every_env(case):
    """Env by env (the threaded reset goes on past a failure, the serial one stops at the first)."""
    orc, g, raised = bc.reset_reference(case)
    print(f"failure {case.id}: placed max {g['placed'].max()}, |coordinate| {g['absc'].min()}..{g['absc'].max()}, "
          f"depth {g['depth'].min()}..{g['depth'].max()}, candidates max {g['total'].max()}")
    assert raised and (g["flags"] & bc.ERR == po.F_MAPGEN_FAIL).all()
    o = po.OracleVec(1)
    with pytest.raises(RuntimeError):
        o.reset(case.seed, case.players, case.pieces, case.difficulty, 100000)
    assert o.flags(0) == g["flags"][0]
    if case.pieces == 255:                                 # the oracle gives up past the engine's coordinate bound
        assert (g["absc"] > bc.K_MAX_COORD).sum() >= 6 and (g["placed"] <= bc.K_MAX_PLACED).all()
        assert (g["depth"] == 4).all()


@pytest.mark.parametrize("rid", tuple(bc.RUNS))
def test_stepping_case(rid):
    run = bc.RUNS[rid]
    c = bc.run_census(run)
    print(f"{rid} ({run.n} envs, blocks {run.blocks}): {c.row()}")
    bc.check_run(run, c)
    assert c.edge_moves >= run.min_edge_moves, f"{rid}: {c.edge_moves} moves onto the outermost cells"
    if run.stored:
        assert c.moves >= 500
    assert c.flags.size <= run.n and (c.flags & bc.ERR).sum() <= bc.MAX_FLAGGED_SHARE * run.n


def test_sweep_for_the_engines_own_limits():
    """The engine gives up as soon as a hex leaves +-62 or a 97th piece is placed; the oracle (and
    the reference) have no such bound and only judge the finished map.  A seed on which the oracle
    succeeds past either limit would show the engine's early exit to be wrong: this sweep finds
    none, and fails if an edit of the oracle or the tables makes one appear (make it a case then)."""
    sw = bc.SWEEP
    seeds = placed = absc = total = depth = 0
    early = []
    for diff in sw["difficulties"]:
        for pieces in sw["pieces"]:
            o = po.OracleVec(sw["n"])
            try:
                o.reset_threaded(sw["seed"], sw["players"], pieces, diff, 100000, threads=min(16, po.host_threads()))
            except RuntimeError:
                pass
            g = bc.gen_census(o)
            ok = (g["flags"] & bc.ERR) == 0
            seeds += sw["n"]
            placed, absc = max(placed, int(g["placed"].max())), max(absc, int(g["absc"].max()))
            total, depth = max(total, int(g["total"].max())), max(depth, int(g["depth"].max()))
            early += [(diff, pieces, sw["seed"] + int(i)) for i in np.nonzero(ok & ((g["absc"] > bc.K_MAX_COORD) | (g["placed"] > bc.K_MAX_PLACED)))[0]]
            print(f"sweep diff {diff}, {pieces} pieces: {int((g['flags'] & po.F_GRID_OVER != 0).sum())} GRID_OVER, "
                  f"{int((g['flags'] & po.F_MAPGEN_FAIL != 0).sum())} MAPGEN_FAIL of {sw['n']}; placed max {g['placed'].max()}, "
                  f"|coordinate| max {g['absc'].max()}, candidates max {g['total'].max()}, depth max {g['depth'].max()}")
    print(f"sweep: {seeds} seeds; placed max {placed} (limit {bc.K_MAX_PLACED}), |coordinate| max {absc} (limit "
          f"{bc.K_MAX_COORD}), candidates max {total}, depth max {depth}")
    assert seeds >= 3000
    assert not early, f"the oracle succeeds past the engine's limits on (difficulty, pieces, seed) {early}"
    assert depth >= 1 and total > 256                      # recursion with the pieces kept is in the sweep


def test_gen_stats_agree_with_the_state():
    """The counters against what the oracle shows elsewhere: dims as in debug_state, the start
    piece's 37 cells inside the box and holding the players' start cells, placed >= pieces + 2."""
    case = bc.Reset(7, bc.HARD)
    orc, g, _ = bc.reset_reference(case)
    cells, dims = orc.player_cells()
    assert np.array_equal(dims[:, 0], g["dimx"]) and np.array_equal(dims[:, 1], g["dimy"])
    assert (g["sx0"] >= 1).all() and (g["sx1"] <= g["dimx"] - 2).all()
    assert (g["sy0"] >= 1).all() and (g["sy1"] <= g["dimy"] - 2).all()
    assert (g["sx1"] - g["sx0"] == 6).all() and (g["sy1"] - g["sy0"] == 6).all()
    for p in range(4):
        assert ((cells[:, p, 0] >= g["sx0"]) & (cells[:, p, 0] <= g["sx1"])).all()
        assert ((cells[:, p, 1] >= g["sy0"]) & (cells[:, p, 1] <= g["sy1"])).all()
    assert (g["placed"] >= case.pieces + 2).all() and (g["total"] >= 14).all()
    assert (g["cmin"] <= -3).all() and (g["cmax"] >= 3).all()
    assert (g["dimx"] <= 3 + g["cmax"] - g["cmin"]).all()


def test_oracle_matches_reference_big_maps():
    with open(os.path.join(GOLD, "ref_maps_big.json")) as f:
        gold = json.load(f)
    entries = gold["entries"] + gold["off_lattice"]
    assert len(gold["entries"]) >= 250 and len(gold["off_lattice"]) == 4
    assert {(d, pc) for d, pc, *_ in entries} == {(d, pc) for d in (1, 2) for pc in (2, 4, 6, 7)}
    assert {pl for *_, pl in entries} == {2, 3, 4}
    zero = np.zeros(1, dtype=po.ACTION)
    o = po.OracleVec(1)
    for diff, npc, seed, hexd, players in entries:
        o = po.OracleVec(1)
        o.reset(seed, players, npc, diff, 100000)
        got = po.step_digest(o.observations, o.selected_action_masks, o.rewards, o.dones, o.agent_selection,
                             o.infos, zero).hex()
        assert got == hexd, f"map seed={seed} diff={diff} n_pieces={npc} players={players}"
        assert not o.flags(0) & po.REF_UNSAFE
        assert (o.gen_stats()["offlat"][0] > 0) == ([diff, npc, seed, hexd, players] in gold["off_lattice"])


def test_autoreset_overflow_case():
    """The stored-mask run whose auto-reset generates a map wider than the observation: env 102 in
    step 132, alone in 200 steps; the oracle flags it and goes on."""
    c = bc.AUTORESET_OVERFLOW
    run = bc.Run("auto", None, c["n"], c["players"], c["pieces"], c["difficulty"], c["seed"], c["max_steps"],
                 c["checkpoint"] + c["past"], True)
    orun = bc.OracleRun(run)
    orc, _ = orun.parts[0]
    first = None
    for t in range(run.steps):
        orun.step()
        if first is None and (orc.flags() & bc.ERR).any():
            first = t
    assert first == c["fail_step"] and c["checkpoint"] <= first < c["checkpoint"] + c["chunk"]
    assert list(np.nonzero(orc.flags() & bc.ERR)[0]) == [c["fail_env"]]
    assert orc.flags(c["fail_env"]) & bc.ERR == po.F_GRID_OVER
