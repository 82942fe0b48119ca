"""Reset-parameter corners (tests/test_corners_cpu.py, tests/test_gpu_corners.py): batches of one
player and max_steps 0..3, walked through every driver on the harness of tests/driver_cases.py (all
six views against the oracle after every op, the hazard flags per env at the end).

One player: the next agent is the acting agent, which every step kernel special-cases (the action
mask loaded from the acting agent's record, the cells of the next agent following the acting one's,
the stores of k_env_step / k_env_step_pub, the lane drivers' record, the LDS heads of the pipe, the
duo stepper and storer, the fix-up's own step); selected and stored masks both take the duo, the
pipe or the wave by size, never the trio.  max_steps 0 ends every env at its first step after every
reset, so every env of every workgroup ends, parks and regenerates its map at every step of every
launch; at 1 it ends at the first turn end.

Every table maps a case id to (n, sequence); KINDS tells which Harness each table needs.
"""
from __future__ import annotations

import driver_cases as dc

HARD = 2
P, P0 = dc.PAIR_STEPS, 24                                  # steps per op; at max_steps 0 (T20: 20 + 4, T2: 12 launches)
SIZES = (200, 33)
SIZES_MS0 = (70, 33)                                       # 70: one full workgroup of 64 envs and one of 6
HANDOVER, HANDOVER0 = 10, 5                                # host steps between the two ops of a TINY row; at max_steps 0


def X(seed, players, max_steps, pieces=3):
    return ("X", seed, players, pieces, HARD, max_steps)


def op(d, max_steps=8):
    return (d, P0 if max_steps == 0 else P)


# ---- SOLO: one player at max_steps 8 ---------------------------------------------------------------
SOLO = {}
for _n in SIZES:
    for _d in dc.STEP_DRIVERS:
        SOLO[f"1p-ms8-{_d}-H-{_d}-n{_n}"] = (_n, [X(77, 1, 8), (_d, P), ("H", P), (_d, P)])
    for _a in dc.REDUCED_DRIVERS:
        for _b in dc.REDUCED_DRIVERS:
            SOLO[f"1p-ms8-pair-{_a}-{_b}-n{_n}"] = (_n, dc.pair_sequence(_a, _b, players=1))

# ---- SOLO_LONG: one player, one piece, no episode end: moves, purchases and specials ---------------
# (seed 177: on the oracle no env of the 200 reaches the end hex within 300 steps, 171 hold a card type >= 8
# at the end; the greedy policy of G buys none by itself, so G takes the last 100 steps after 200 of Hs)
SOLO_LONG_N, SOLO_LONG_SEED, SOLO_LONG_STEPS, SOLO_LONG_WIDE = 200, 177, 300, 50
SOLO_LONG = {f"1p-1piece-ms100000-{_d}": (SOLO_LONG_N, [X(SOLO_LONG_SEED, 1, 100000, pieces=1), (_d, SOLO_LONG_STEPS)])
             for _d in ("Hs", "S20", "S1000", "Ls")}
SOLO_LONG["1p-1piece-ms100000-G"] = (SOLO_LONG_N, [X(SOLO_LONG_SEED, 1, 100000, pieces=1), ("Hs", 200), ("G", 100)])

# ---- TINY: max_steps 0..3 with 4..1 players: X d H d ---------------------------------------------------
TINY_ALL_DRIVERS = ((4, 0), (4, 1), (1, 0), (1, 2))        # the other twelve take REDUCED_DRIVERS
TINY = {}
for _ms in (0, 1, 2, 3):
    for _p in (4, 3, 2, 1):
        for _d in (dc.STEP_DRIVERS if (_p, _ms) in TINY_ALL_DRIVERS else dc.REDUCED_DRIVERS):
            for _n in (SIZES_MS0 if _ms == 0 else SIZES):
                TINY[f"{_p}p-ms{_ms}-{_d}-n{_n}"] = (_n, [X(77, _p, _ms), op(_d, _ms), ("H", HANDOVER if _ms else HANDOVER0),
                                                     op(_d, _ms)])

# ---- STATE: the host-side state across a change of players and a max_steps of 0 ----------------------
STATE_N = 70
T20, S20, T20Z, S20Z = ("T20", P), ("S20", P), ("T20", P0), ("S20", P0)
STATE = {
    # lean_clock and cdeck_ok across 4 -> 1 -> 4 (ms 0) -> 3 (ms 1) -> the same again -> 4 (ms 40: launches
    # of 20 + 10 steps below the no-fix-up bound, then 20 + 10 past it)
    "players-and-ms0": (STATE_N, [X(77, 4, 8), T20, X(78, 1, 8), T20, S20, X(79, 4, 0), T20Z, T20Z, X(80, 3, 1), T20, "X0",
                                  T20, X(81, 4, 40), T20, T20]),
    # auto-reset off at ms 0: every env is done after one step, the rest are dead steps
    "autoreset-off-at-ms0": (STATE_N, [X(77, 4, 8), T20, X(79, 4, 0), "A0", T20Z, T20Z, "X0", "A1", T20Z, X(80, 3, 1), T20]),
    "invalidate-and-clear-at-ms0": (STATE_N, [X(79, 4, 0), T20Z, "I", T20Z, "C", T20Z]),
}
# step ops that hold no episode end on the oracle: with auto-reset off at ms 0 every env is already done in
# the second launch; at max_steps 40 no 4-player env ends within 60 steps (the two ops walk the
# no-fix-up bound, 0 + 20 and 20 + 10 below it, 30 + 20 past it)
STATE_NO_END_OPS = {"autoreset-off-at-ms0": (5,), "players-and-ms0": (13, 14)}
# two shards (device=[0, 0]); at ms 0 the steps are cut to 40 in all (12,040 oracle resets)
TWO_SHARD_N = 301
TWO_SHARD = {
    "two-shards-1p-ms8": (TWO_SHARD_N, [X(77, 1, 8), ("H", P), ("Th20", P), S20, ("L", P)]),
    "two-shards-4p-ms0": (TWO_SHARD_N, [X(77, 4, 0), ("H", 6), ("Th20", P0), ("S20", 6), ("L", 4)]),
}
LAZY = {"lazy-views-4p-ms0": (STATE_N, [X(77, 4, 0), T20Z, S20Z, "V", T20Z])}

# ---- BIG: the pipe and the wave selected by size with one player --------------------------------------
BIG_RESET = X(77, 1, 8)
BIG = {f"{kind}-1p-ms8-{name}": (n, [BIG_RESET] + list(seq[1:]))
       for kind, n in dc.BIG_SIZES.items() for name, seq in dc.BIG_CASES.items()}

# what a Harness of each table is made with (besides cg, n and the sampler seed)
KINDS = {"solo": {}, "solo_long": {}, "tiny": {}, "state": {}, "two_shard": {"device": [0, 0]}, "lazy": {"lazy_views": True},
         "big": {}}
TABLES = {"solo": SOLO, "solo_long": SOLO_LONG, "tiny": TINY, "state": STATE, "two_shard": TWO_SHARD, "lazy": LAZY, "big": BIG}
SAMPLER_SEED = dc.PAIR_SEED
MAX_ORACLE_RESETS = 13000                                  # per case (about 0.34 ms each with map generation)


def step_ops(seq):
    """Indices of the ops of seq that step the envs."""
    return [k for k, o in enumerate(seq) if not isinstance(o, str) and o[0] not in ("X", "B") and o[1] > 0]


def ms_at(seq):
    """max_steps and auto-reset in force at every op of seq: [(max_steps, autoreset)]."""
    out, ms, on = [], None, True
    for o in seq:
        if not isinstance(o, str) and o[0] == "X":
            ms = o[5]
        elif o in ("A0", "A1"):
            on = o == "A1"
        out.append((ms, on))
    return out
