"""State snapshots (tests/test_state_snapshot_cpu.py, tests/test_gpu_state_snapshot.py): the oracle
side of envs.snapshot() / envs.restore(snap, src).

The oracle cannot save or load a state, so its side of a restore is a replay: a fresh OracleVec is
reset with the same parameters and fed the actions recorded up to the snapshot point (replay()).  A
fork's twin is an OracleVec(1) reset with seed + src[j] (u32 wrap, vec_environment.h:41) and fed
source env src[j]'s recorded actions (Twins): env i of a batch is the 1-env batch seeded seed + i,
which the CPU test asserts across auto-resets.  The cases record the actions themselves: the prefix
before a snapshot runs as one-step ops of the host loop (driver H of tests/driver_cases.py), and the
Harness keeps each step's actions in `last`.

The cases (4 players unless said, 3 pieces, HARD, max_steps 8 as driver_cases.PAIR_MAX_STEPS, so
that the 30 steps between snapshot and restore cross auto-resets and the maps differ at restore
time):
  undo    X, 10 steps, snapshot, 30 steps under driver A, restore, 30 steps under driver B
  fork    a snapshot of 70 envs after 10 steps, restored through src into handles of 70, 33 envs;
          a snapshot of 1 env into 70
"""
from __future__ import annotations

import numpy as np

import driver_cases as dc
import pyoracle as po

SEED, SAMPLER_SEED, PIECES, DIFFICULTY, MAX_STEPS = 4242, 99, 3, 2, dc.PAIR_MAX_STEPS
PREFIX, BETWEEN, AFTER = 10, 30, 30
SIZES = (70, 33, 1)                   # a full 64-env workgroup and a ragged one; 33; 1
SHARD_N, SHARD_DEVICES = 130, [0, 0]
FORK_STEPS, FORK_ROLLOUT = 40, 30
TWIN_STEPS = 100                      # episodes at max_steps 8 end 22 to 45 steps after they began: two ends inside
VIEWS = dc.FIELDS + dc.PLAIN
# the wide-deck case: a prefix under the stored masks (Hs: the selected-mask loop never buys) at
# max_steps 100000, after which most envs' decks hold a card of type >= 8 (the trio's compact decks
# cannot hold it: such an env parks at step 0 of a launch, and the fix-up runs its steps)
WIDE = dict(n=70, seed=SEED + 1, players=4, max_steps=100000, prefix=60, driver="Hs")
# resets the restore has to undo: snapshot at 4 players, then a reset with these, restore, T20
OTHER_RESET = ("X", SEED + 7, 2, PIECES, DIFFICULTY, 40)


def reset_op(players=4, seed=SEED, max_steps=MAX_STEPS):
    return ("X", seed, players, PIECES, DIFFICULTY, max_steps)


def per_step(driver, steps):
    """The ops of `steps` steps under `driver`: one op a step (every step compared) for the drivers
    that launch per step, one op for the chunked rollouts (a launch is 20 steps)."""
    return [(driver, steps)] if dc._CHUNKED.match(driver) else [(driver, 1)] * steps


def record_prefix(h, reset, steps, driver="H"):
    """Reset `h` and run `steps` recorded host-loop steps; returns the actions, one (n,) array a step."""
    dc.run(h, [reset])
    acts = []
    for _ in range(steps):
        dc.run(h, [(driver, 1)])
        acts.append(h.last.copy())
    return acts


def replay(n, reset, acts):
    """A fresh OracleVec(n) at the snapshot point: the reset's parameters, then the recorded actions."""
    _, seed, players, pieces, difficulty, max_steps = reset
    orc = po.OracleVec(n)
    orc.reset(seed, players, pieces, difficulty, max_steps)
    for a in acts:
        orc.step(a)
    return orc


def views_of(orc):
    """Copies of the six views."""
    return {nm: np.array(getattr(orc, nm), copy=True) for nm in VIEWS}


def views_differ(a, b):
    """The first view (and leaf) in which two view dicts, or objects with the views as attributes,
    differ; None when all six are equal."""
    get = (lambda o, nm: o[nm]) if isinstance(a, dict) else getattr
    getb = (lambda o, nm: o[nm]) if isinstance(b, dict) else getattr
    for nm in dc.FIELDS:
        bad = po.named_equal(get(a, nm), getb(b, nm))
        if bad is not None:
            return f"{nm}.{bad}"
    for nm in dc.PLAIN:
        if not np.array_equal(np.asarray(get(a, nm)), np.asarray(getb(b, nm))):
            return nm
    return None


def after_restore(h, orc, players, max_steps):
    """The Harness's oracle side and host-state mirror after env.restore(): the replayed oracle, the
    snapshot's batch parameters, no compact decks."""
    h.orc = orc
    h.players, h.max_steps, h.cdeck = players, max_steps, False
    h.done_prev = np.array(orc.dones, dtype=bool)


class Twins:
    """One OracleVec(1) per destination env of a fork: twin j is source env src[j], replayed."""

    def __init__(self, reset, acts, src):
        _, seed, players, pieces, difficulty, max_steps = reset
        self.src = [int(s) for s in src]
        self.envs = []
        for s in self.src:
            t = po.OracleVec(1)
            t.reset((seed + s) & 0xFFFFFFFF, players, pieces, difficulty, max_steps)
            for a in acts:
                t.step(a[s:s + 1])
            self.envs.append(t)
        self.n = len(self.envs)
        self.ends = 0

    def view(self, nm):
        return np.concatenate([np.asarray(getattr(t, nm)) for t in self.envs])

    def views(self):
        return {nm: self.view(nm) for nm in VIEWS}

    def step(self, actions):
        for j, t in enumerate(self.envs):
            t.step(actions[j:j + 1])
            self.ends += int(t.dones[0])

    def flags(self):
        return np.array([t.flags(0) for t in self.envs], dtype=np.uint32)


def fork_sources(n_dst, n_src, seed=5):
    """The src vectors of the fork case: random with repeats, all one index, reversed (wrapped when
    the destination is longer than the snapshot)."""
    rng = np.random.default_rng(seed)
    return {"random": rng.integers(0, n_src, size=n_dst), "one": np.full(n_dst, min(5, n_src - 1)),
            "reversed": (n_src - 1 - np.arange(n_dst)) % n_src}
