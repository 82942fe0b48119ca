"""Big-map cases (tests/test_bigmap_cpu.py, tests/test_gpu_bigmap.py): map generation and stepping
with 2 to 10 map pieces, on maps up to the 48x48 observation limit.

With 1 and 3 pieces (every other engine test) map generation never enumerates more than 64
candidate placements, the map stays within 31 cells and the start piece stays near the middle of
the box.  The cases here were searched on the CPU oracle (seeds 1000 + i and their neighbours) for
what those tests never reach; census functions below count it again on every run, so that an edit
of a seed that loses a case fails tests/test_bigmap_cpu.py, without a GPU:

  candidates   add_random_piece enumerates more than 128 candidates (the engine's wave recomputes
               its third ballot) from 7 pieces on, more than 192 (a fourth) from 10 pieces on
  extent       maps whose bounding box is 47 or 48 cells wide (dimx or dimy 47..49) from 8 pieces on
  corner       the start piece within 2 cells of the box's edge: the board grows away from it
  overflow     a batch in which one env's map is wider than the observation (GRID_OVER)
  stepping     players moving on the box's outermost cells, auto-resets that generate big maps

Seeds: env i of a batch is seeded seed + i (and its sampler seed + i), so a block [lo, hi) of a
large batch is a batch of its own seeded seed + lo (lategame_cases.OracleRun).
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import lategame_cases as lc
import pyoracle as po

EASY, MEDIUM, HARD = 0, 1, 2
ERR = po.F_GRID_OVER | po.F_MAPGEN_FAIL       # the flags with which the engine raises
MAX_FLAGGED_SHARE = 0.02                      # of a batch: the only envs a test may leave unchecked
N = 130                                       # two waves and a ragged tail


# ---- resets ---------------------------------------------------------------------------------
@dataclass(frozen=True)
class Reset:
    pieces: int
    difficulty: int
    players: int = 4
    seed: int = 1000
    n: int = N

    @property
    def id(self):
        return f"{self.pieces}pc-{'EMH'[self.difficulty]}-{self.players}p-n{self.n}"


# seed windows in which the oracle raises no error flag (asserted by the CPU test)
RESET_GRID = tuple(
    [Reset(pc, d) for d in (MEDIUM, HARD) for pc in (2, 4, 5, 6, 7, 8, 9)] +
    [Reset(pc, d, pl) for pl in (2, 3) for pc in (6, 7) for d in (MEDIUM, HARD)] +
    [Reset(pc, EASY) for pc in (1, 2, 3)] +
    [Reset(7, HARD, n=1), Reset(7, MEDIUM, n=65)] +
    [Reset(10, HARD, seed=1155)])             # the fourth candidate batch
# what the grid reaches, by case id: (envs with total > 128, envs with total > 192,
# envs with dimx or dimy >= 47) -- minima the CPU test asserts
REACHES = {"7pc-M-4p-n130": (3, 0, 0), "7pc-H-4p-n130": (7, 0, 0), "8pc-M-4p-n130": (5, 0, 1),
           "8pc-H-4p-n130": (15, 0, 0), "9pc-M-4p-n130": (7, 0, 1), "9pc-H-4p-n130": (25, 0, 2),
           "10pc-H-4p-n130": (68, 2, 0)}

# one env of 130 overflows the observation grid (seed 1139: dimx or dimy > 49)
OVERFLOW = Reset(9, MEDIUM, seed=1070)
OVERFLOW_ENVS = (69,)

# One env of 130 (seed 141707) whose generation leaves the hex lattice.  A travel piece for which
# no placement is free stays reset at the origin while the list of placed pieces still names it
# (map.cpp:277-307 resets the piece before it looks for candidates); the recursion that follows
# takes connection points from it there, and when it is a small piece (its hexes lie half a cell off
# the lattice at the origin) the pieces connected to it lie half a cell off the map's lattice: they
# coincide with no hex, so every such placement counts as free.  The reference and the oracle
# (float coordinates) go on and finish a map; the engine keeps such hexes in a list beside its grid.
# 3 of the 32,770 seeds 140000 + i at 6 pieces HARD do this (envs 1707, 9887, 22857), about one
# generation in 30,000 at 4 to 7 pieces HARD, none of 65,536 at 3 pieces.
OFF_LATTICE = Reset(6, HARD, seed=141650)
OFF_LATTICE_ENVS = (57,)

# map generation gives up in every env (n = 8): no travel piece at all, EASY's three travel pieces
# for four places, and more places than travel pieces.  At 255 pieces every failed placement recurses
# with the pieces kept: 65 pieces placed, hexes 64 to 70 cells from the origin -- past the engine's
# kMaxCoord = 62, where it used to report the map as too wide (GRID_OVER) while the oracle, with no
# such bound, runs out of attempts (MAPGEN_FAIL).  (MEDIUM: the oracle takes 1.7 s per env, HARD 3.7 s)
FAILURES = (Reset(0, MEDIUM, n=8), Reset(4, EASY, n=8), Reset(255, MEDIUM, n=8))

# the sweep for the engine's own limits (cog_engine.h kMaxCoord = 62, kMaxPlaced = 96)
SWEEP = dict(seed=20000, n=256, pieces=(7, 8, 9, 10, 11, 12), difficulties=(MEDIUM, HARD), players=4)
K_MAX_COORD, K_MAX_PLACED = 62, 96


def gen_census(orc):
    """What the oracle's last generation reached in every env: its gen_stats plus `dim` (the larger
    of dimx, dimy), `edge` (cells between the start piece and the nearest edge of the box: 0 when it
    lies on index 0 or dim - 1) and `absc` (the largest |coordinate| ever placed)."""
    g = dict(orc.gen_stats())
    g["flags"] = orc.flags()
    g["dim"] = np.maximum(g["dimx"], g["dimy"])
    g["edge"] = np.minimum(np.minimum(g["sx0"], g["sy0"]),
                           np.minimum(g["dimx"] - 1 - g["sx1"], g["dimy"] - 1 - g["sy1"]))
    g["absc"] = np.maximum(-g["cmin"], g["cmax"])
    return g


@functools.lru_cache(maxsize=None)
def reset_reference(case: Reset):
    """The oracle after case's reset (threaded: envs are independent) and the census of it; shared,
    read-only.  A generation failure leaves the flags to tell (the threaded reset goes on)."""
    orc = po.OracleVec(case.n)
    try:
        orc.reset_threaded(case.seed, case.players, case.pieces, case.difficulty, 100000,
                           threads=min(case.n, po.host_threads()))   # (more threads than envs: one thread gets all)
        raised = False
    except RuntimeError:
        raised = True
    return orc, gen_census(orc), raised


# ---- stepping -------------------------------------------------------------------------------
@dataclass(frozen=True)
class Run:
    id: str
    kind: str | None                  # rollout_kind it must select; "host": the host loop; None: one launch per step
    n: int
    players: int
    pieces: int
    difficulty: int
    seed: int
    max_steps: int
    steps: int
    stored: bool
    chunk: int | None = None
    checkpoints: tuple = ()
    min_resets: int = 0               # auto-resets in the checked blocks, at least
    min_edge_moves: int = 1           # moves onto the box's outermost cells, at least

    @property
    def blocks(self):
        if self.n <= 2 * lc.BLOCK:
            return ((0, self.n),)
        return ((0, lc.BLOCK), (self.n - lc.BLOCK, self.n))


RUNS = {r.id: r for r in (
    # host loop, every step checked
    # (the selected-mask driver never moves a player: its cases hold the maps and masks, no moves)
    Run("host-sel-7H", "host", 130, 4, 7, HARD, 1000, 100000, 300, False, min_edge_moves=0),
    Run("host-sel-8M-3p", "host", 96, 3, 8, MEDIUM, 1000, 30, 300, False, min_resets=96, min_edge_moves=0),
    Run("host-sto-7M-2p", "host", 64, 2, 7, MEDIUM, 1000, 30, 300, True, min_resets=64),
    # rollouts, checked at checkpoints
    Run("trio-7H-c20", "trio", 200, 4, 7, HARD, 1000, 30, 180, False, 20, (60, 180), min_resets=100, min_edge_moves=0),
    Run("trio-7H-long", "trio", 200, 4, 7, HARD, 1000, 30, 180, False, 1000, (180,), min_resets=100, min_edge_moves=0),
    Run("duo-7H", "duo", 130, 4, 7, HARD, 1000, 20, 160, True, 40, (80, 160), min_resets=100),
    Run("step-7H", None, 130, 4, 7, HARD, 1000, 20, 160, True, None, (80, 160), min_resets=100),
    # 5 pieces MEDIUM: these batches generate 60,000 maps, every one of which must succeed for
    # runner.sync() not to raise.  At 7 pieces one generation in about 5,000 overflows or gives up, at
    # 6 one in 15,000; the oracle ran the whole batch of 32,770 from this seed without either (and
    # without a map that leaves the hex lattice, OFF_LATTICE above)
    Run("pipe-5M", "pipe", 16450, 4, 5, MEDIUM, 800000, 20, 160, True, 40, (80, 160), min_resets=150),
    Run("wave-5M", "wave", 32770, 4, 5, MEDIUM, 800000, 20, 160, True, 40, (80, 160), min_resets=150),
)}


class OracleRun(lc.OracleRun):
    """lategame_cases.OracleRun over a Run's blocks, reset threaded, with either driver mask."""

    def __init__(self, run: Run):
        self.blocks, self.parts, self.steps_done, self.stored = run.blocks, [], 0, run.stored
        for lo, hi in self.blocks:
            orc, osm = po.OracleVec(hi - lo), po.OracleSampler(hi - lo, run.seed + lo)
            orc.reset_threaded(run.seed + lo, run.players, run.pieces, run.difficulty, run.max_steps)
            self.parts.append((orc, osm))

    def step(self):
        for orc, osm in self.parts:
            osm.sample(po.stored_masks(orc) if self.stored else orc.selected_action_masks)
            orc.step(osm.actions)
        self.steps_done += 1


@dataclass
class RunCensus:
    resets: int                       # dones over the run
    moves: int                        # effective move actions
    edge_moves: int                   # of them, onto a cell with index <= 1 or >= dim - 2
    flags: np.ndarray                 # the hazard flags at the end, blocks concatenated
    off_lattice: int                  # generations (resets and auto-resets) that placed a hex off the lattice
    snapshots: dict                   # {steps done: lategame_cases.Snapshot}

    def row(self):
        return (f"{self.resets} auto-resets, {self.moves} moves, {self.edge_moves} of them onto the box's "
                f"outermost cells, flags {int(np.bitwise_or.reduce(self.flags)):#04x}")


def run_census(run: Run, count_moves=True) -> RunCensus:
    """The oracle side of `run`: snapshots at its checkpoints and the counts of what it reaches.  A
    move is counted as the step takes it (no play, no special, move != 0), at the mover's cell after
    the step; a step that ends the episode is not counted (the reset has moved the player)."""
    orun = OracleRun(run)
    resets = moves = edge_moves = 0
    off = sum(int((orc.gen_stats()["offlat"] > 0).sum()) for orc, _ in orun.parts)
    snaps = {}
    for _ in range(run.steps):
        before = [orc.agent_selection.copy() for orc, _ in orun.parts]
        orun.step()
        for (orc, osm), ag in zip(orun.parts, before):
            resets += int(orc.dones.sum())
            if orc.dones.any():
                off += int((orc.gen_stats(np.nonzero(orc.dones)[0])["offlat"] > 0).sum())
            if not count_moves:
                continue
            a = osm.actions
            moved = np.nonzero((a["play"] == 0) & (a["play_special"] == 0) & (a["move"] != 0) & ~orc.dones)[0]
            if moved.size:
                cells, dims = orc.player_cells()
                c = cells[moved, ag[moved]]
                moves += moved.size
                edge_moves += int(((c <= 1) | (c >= dims[moved] - 2)).any(1).sum())
        if orun.steps_done in run.checkpoints:
            snaps[orun.steps_done] = lc.snapshot(orun)
    flags = np.concatenate([orc.flags() for orc, _ in orun.parts])
    return RunCensus(resets, moves, edge_moves, flags, off, snaps)


@functools.lru_cache(maxsize=None)
def run_reference(rid: str) -> RunCensus:
    """run_census of RUNS[rid] without the move counts (the GPU tests' shared, read-only reference)."""
    return run_census(RUNS[rid], count_moves=False)


def check_run(run: Run, c: RunCensus):
    """What a run must reach on the oracle alone (conditions that keep a case, not tolerances)."""
    assert not (c.flags & ERR).any(), f"{run.id}: the oracle flags envs {np.nonzero(c.flags & ERR)[0]}"
    assert c.off_lattice == 0, f"{run.id}: {c.off_lattice} generations leave the lattice"
    assert c.resets >= run.min_resets, f"{run.id}: {c.resets} auto-resets"
    assert all(k in c.snapshots for k in run.checkpoints)


# ---- an overflow at an auto-reset inside a launch (found in a search of 4,096 seeds: 32 batches of
# 128 envs, seeds 30000 + 128 k, 8 pieces MEDIUM, 12-turn episodes, 240 steps; 7 of them hold one) ----
AUTORESET_OVERFLOW = dict(n=128, seed=30256, players=4, pieces=8, difficulty=MEDIUM, max_steps=12,
                          fail_step=132, fail_env=102, checkpoint=120, past=80, chunk=40)
