"""Late-game cases for the full-dynamics rollout kernels (tests/test_lategame_cpu.py,
tests/test_gpu_lategame.py): the named configurations, and a census of what the oracle does in
each of them.

The short full-dynamics tests (150-400 steps, max_steps 25-40 turns, 3 map pieces) end their
episodes at max_steps and hardly play a special or remove a card.  With one map piece, max_steps
100,000 and some thousands of steps the uniform sampler reaches the rest by itself: players
reaching the end hex (has_won, non-zero rewards, several winners in one end), the six specials
(cards 15..20: Transmitter, Cartographer, Compass, Scientist, Travel log, Native), the remove
path, exhausted shop piles.  census() counts these on the CPU oracle alone, so that every test
can assert that it still reaches them.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import pyoracle as po

MAX_STEPS = 100000                    # turns: no episode ends at max_steps inside the horizon
HORIZON = 8000                        # steps
CHECKPOINTS = (2000, 4000, 6000, 8000)
SPECIALS = (15, 16, 17, 18, 19, 20)   # card ids: Transmitter .. Native
BLOCK = 128                           # D and E: the first and the last BLOCK envs are checked

# what every configuration must reach on the oracle (conditions that keep a test from losing its
# case, not tolerances)
MIN_NATURAL_ENDS, MIN_EACH_SPECIAL, MIN_REMOVES = 10, 100, 100


@dataclass(frozen=True)
class Config:
    id: str
    kind: str | None                  # rollout_kind(n, players, True) it must select; None: one launch per step
    n: int
    players: int
    pieces: int
    difficulty: int                   # 0 EASY, 1 MEDIUM, 2 HARD
    seed: int
    chunk: int | None                 # runner.set_chunk; None: never set
    flags: tuple = ()                 # the OR of the oracle's hazard flags must be one of these (empty: any)
    two_winners: bool = False         # at least one end with two winners

    @property
    def blocks(self):
        """[lo, hi) ranges of the envs the oracle runs and the GPU tests check."""
        if self.n <= 2 * BLOCK:
            return ((0, self.n),)
        return ((0, BLOCK), (self.n - BLOCK, self.n))


CONFIGS = {c.id: c for c in (
    Config("A", "duo", 130, 4, 1, 0, 5000, 250),
    Config("B", "duo", 130, 2, 1, 2, 5001, 37, flags=(0xa4, 0xa6)),
    Config("C", "duo", 130, 3, 2, 2, 5002, 250, flags=(0xa4, 0xa6)),
    Config("C'", "duo", 130, 3, 1, 1, 5002, 37, flags=(0xa4, 0xa6), two_winners=True),
    Config("D", "pipe", 16450, 4, 1, 0, 5003, 1000),
    Config("E", "wave", 32770, 4, 1, 0, 5003, 1000),
    Config("F", None, 130, 4, 1, 2, 5004, None),
)}
IDS = tuple(CONFIGS)

FIELDS = ("observations", "selected_action_masks", "infos")
PLAIN = ("rewards", "dones", "agent_selection")


class OracleRun:
    """The oracle side of a configuration: one (OracleVec, OracleSampler) pair per block of envs,
    freshly reset.  Env i of a batch is a 1-env batch seeded seed + i (envs are independent), so
    the block [lo, hi) of a larger batch is a (hi - lo)-env batch seeded seed + lo."""

    def __init__(self, blocks, seed, players, pieces, difficulty, max_steps=MAX_STEPS):
        self.blocks = tuple(blocks)
        self.parts = []
        for lo, hi in self.blocks:
            orc, osm = po.OracleVec(hi - lo), po.OracleSampler(hi - lo, seed + lo)
            orc.reset(seed + lo, players, pieces, difficulty, max_steps)
            self.parts.append((orc, osm))
        self.steps_done = 0

    @classmethod
    def of(cls, cfg: Config):
        return cls(cfg.blocks, cfg.seed, cfg.players, cfg.pieces, cfg.difficulty)

    @property
    def n(self):
        return sum(hi - lo for lo, hi in self.blocks)

    def step(self):
        for orc, osm in self.parts:
            osm.sample(po.stored_masks(orc))
            orc.step(osm.actions)
        self.steps_done += 1


@dataclass
class Snapshot:
    """Copies of the oracle's outputs after `steps` steps, one entry per block."""
    steps: int
    blocks: tuple
    state: list                       # per block: {field: array copy}

    def differences(self, env, what=""):
        """Every output of `env` (an engine handle whose host views are in sync, or any object with
        the same attributes) against this snapshot over the checked blocks: a list of messages."""
        out = []
        for (lo, hi), st in zip(self.blocks, self.state):
            where = f"{what} after {self.steps} steps, envs [{lo}, {hi})"
            for nm in FIELDS:
                bad = po.named_equal(getattr(env, nm)[lo:hi], st[nm])
                if bad is not None:
                    out.append(f"{where}: {nm}.{bad} differs from the oracle")
            for nm in PLAIN:
                a, b = np.asarray(getattr(env, nm)[lo:hi]), st[nm]
                if not np.array_equal(a, b):
                    i = int(np.nonzero((a != b).reshape(hi - lo, -1).any(1))[0][0])
                    out.append(f"{where}: {nm} differs from the oracle (first at env {lo + i})")
        return out


def snapshot(run: OracleRun) -> Snapshot:
    state = []
    for orc, _ in run.parts:
        st = {nm: getattr(orc, nm).copy() for nm in FIELDS + PLAIN}
        st["flags"] = orc.flags()
        state.append(st)
    return Snapshot(run.steps_done, run.blocks, state)


@dataclass
class Census:
    steps: int
    natural_ends: int                 # dones with a positive reward
    first_end: np.ndarray             # per env: step index of its first natural end, -1 if none
    ends_by_winners: dict             # {number of winners: natural ends}
    specials: dict                    # {card id 15..20: times played}
    removes: int
    flags: int                        # OR of the oracle's hazard flags over the envs, at the end
    per_block: list                   # the same counts for each block alone
    snapshots: dict = field(default_factory=dict)   # {steps done: Snapshot}

    @property
    def t_star(self):
        """Step index of the first natural end in any env (None if there is none)."""
        seen = self.first_end[self.first_end >= 0]
        return int(seen.min()) if seen.size else None

    def row(self):
        w = ", ".join(f"{k} winner{'s' if k > 1 else ''}: {v}" for k, v in sorted(self.ends_by_winners.items()))
        return (f"{self.natural_ends} natural ends ({w}; first at step {self.t_star}), specials "
                f"{'/'.join(str(self.specials[c]) for c in SPECIALS)}, {self.removes} removes, flags {self.flags:#04x}")


def _count(actions, dones, rewards, players):
    """Counts from the sampled actions and the step outputs alone.  actions: ACTION[steps, n],
    dones: bool[steps, n], rewards: f4[steps, n, 4].  The effective action follows the step's
    precedence: play > play_special > move > get_from_shop > remove."""
    no_play = actions["play"] == 0
    special = np.where(no_play, actions["play_special"], 0)
    specials = {c: int((special == c + 1).sum()) for c in SPECIALS}
    removes = int((no_play & (actions["play_special"] == 0) & (actions["move"] == 0) &
                   (actions["get_from_shop"] == 0) & (actions["remove"] != 0)).sum())
    winners = (rewards[:, :, :players] > 0).sum(2)
    natural = dones & (winners > 0)
    by_winners = {int(k): int((natural & (winners == k)).sum()) for k in np.unique(winners[natural])}
    any_end = natural.any(0)
    first = np.where(any_end, natural.argmax(0), -1)
    return int(natural.sum()), first, by_winners, specials, removes


def census(run: OracleRun, steps=HORIZON, checkpoints=(), players=4) -> Census:
    """`steps` x (osm.sample(stored masks); orc.step(actions)) on the oracle, counting what the run
    reaches.  Snapshots (copies) of the oracle's outputs are kept after each of `checkpoints` steps
    and after the step of the first natural end in any env (the only moment its dones and rewards
    can be seen).  A map-generation failure of the oracle propagates as RuntimeError."""
    n = run.n
    actions = np.zeros((steps, n), dtype=po.ACTION)
    dones = np.zeros((steps, n), dtype=bool)
    rewards = np.zeros((steps, n, 4), dtype=np.float32)
    offs = np.cumsum([0] + [hi - lo for lo, hi in run.blocks])
    snaps, ended = {}, False
    for t in range(steps):
        run.step()
        for k, (orc, osm) in enumerate(run.parts):
            sl = slice(offs[k], offs[k + 1])
            actions[t, sl], dones[t, sl], rewards[t, sl] = osm.actions, orc.dones, orc.rewards
        first_end_now = not ended and bool((dones[t] & (rewards[t] > 0).any(1)).any())
        ended |= first_end_now
        if first_end_now or run.steps_done in checkpoints:
            snaps[run.steps_done] = snapshot(run)
    flags = [orc.flags() for orc, _ in run.parts]
    total = _count(actions, dones, rewards, players)
    per_block = []
    for k in range(len(run.blocks)):
        sl = slice(offs[k], offs[k + 1])
        b = _count(actions[:, sl], dones[:, sl], rewards[:, sl], players)
        per_block.append(Census(steps, b[0], b[1], b[2], b[3], b[4], int(np.bitwise_or.reduce(flags[k])), []))
    return Census(steps, total[0], total[1], total[2], total[3], total[4],
                  int(np.bitwise_or.reduce(np.concatenate(flags))), per_block, snaps)


@functools.lru_cache(maxsize=None)
def reference(cid: str) -> Census:
    """The census of configuration `cid` over the whole horizon with the standard checkpoints,
    computed once and shared (read-only) by the tests that need it."""
    cfg = CONFIGS[cid]
    return census(OracleRun.of(cfg), HORIZON, CHECKPOINTS, cfg.players)


def check_conditions(cfg: Config, c: Census):
    """The conditions a configuration must meet on the oracle alone; every block of D and E meets
    them by itself."""
    for k, b in enumerate(c.per_block):
        where = f"config {cfg.id} envs [{cfg.blocks[k][0]}, {cfg.blocks[k][1]})"
        assert b.natural_ends >= MIN_NATURAL_ENDS, f"{where}: {b.natural_ends} natural ends"
        assert min(b.specials.values()) >= MIN_EACH_SPECIAL, f"{where}: specials {b.specials}"
        assert b.removes >= MIN_REMOVES, f"{where}: {b.removes} removes"
    if cfg.two_winners:
        assert c.ends_by_winners.get(2, 0) >= 1, f"config {cfg.id}: no end with two winners: {c.ends_by_winners}"
    if cfg.flags:
        assert c.flags in cfg.flags, f"config {cfg.id}: hazard flags {c.flags:#x}"


# ---- the map-generation failure at an auto-reset (tests/test_gpu_lategame.py) ----------------
MAPGEN_CASE = dict(n=128, seed=1000, players=4, pieces=1, difficulty=1, max_steps=400,
                   fail_step=7326, fail_env=105, checkpoint=7000, chunk=250)
