"""Host actions the mask forbids (tests/test_offmask_cpu.py, tests/test_gpu_offmask.py, the `offmask`
rows of tests/launch_form_cases.py): the cases of the M op of tests/driver_cases.py and the census
that says, on the oracle alone, what each case reaches.

cog_env::step never reads the mask (environment.cpp:91-181): it executes the first non-zero head in
the order play, play_special, move, get_from_shop, remove on u_char counters that wrap (SURVEY A.6
Q23).  An index inside its head is therefore defined behaviour of the reference wherever the oracle
raises no REF_UNSAFE flag, and the engine is held to it bit for bit: a card played from an empty
hand leaves hand[c] = 255, a remove with no pending removes leaves 255 of them, a purchase from an
empty shop slot leaves 255 in it, a move in a closed direction walks onto mountains, other players'
hexes and off the map.

Every case is a list of driver_cases ops; an M op is one step, so that all views are compared after
every step.  A "hand-over" is X, 30 M steps (10 through each path, runner.step() last), a step
driver for 30 steps, 30 M steps, the driver again: every rollout kernel starts from the state such
actions leave.
"""
from __future__ import annotations

import numpy as np

import driver_cases as dc
import pyoracle as po

SEED = 909
N, N_SWEEP = 200, 261                                      # 261 = 3 x 87: every (head, value) three times a step
PATHS = ("step", "step_device", "runner")
KINDS = dc.OFFMASK_KINDS
FRAC = 0.5
FRACS = {k: FRAC for k in KINDS}
FRACS.update(move=0.75)               # (at 0.5 the moves leave the map's array on 100 of 200 envs: no margin)
FRAC_ENDS = 0.2                       # where episodes are to end: an altered action is seldom a pass
STEPS = {k: 60 for k in KINDS}
STEPS.update(sweep=87, move=90, shop=90, remove=90)
# the heads whose executed actions a kind puts on zero mask bytes at least 100 times (`all` leaves the
# play head non-zero in 21 records of 22, and the step's priority chain executes it; play_special next)
TARGETS = {"single": (0, 1, 2, 3, 4), "replace": (0, 1, 2, 3, 4), "all": (0, 1), "play": (0,), "special": (1,), "remove": (2,),
           "move": (3,), "shop": (4,), "sweep": (0, 1, 2, 3, 4)}
PILE_KINDS = ("play", "special", "remove", "single", "sweep")       # half the envs end with a pile byte >= 128
SHOP_KINDS = ("shop", "single")                            # (sweep buys from each slot once per env: none runs empty)
REMOVE_KINDS = ("remove", "single", "sweep")
MOVE_KINDS = ("move",)


def X(seed, players, max_steps):
    return ("X", seed, players, 3, 2, max_steps)


def M(path, kind, frac, seed, steps):
    """`steps` M ops of one step each, seeded seed, seed + 1, ..."""
    return [("M", path, 1, seed + j, kind, 1.0 if kind == "sweep" else frac) for j in range(steps)]


def M_mixed(kind, frac, seed, steps=30):
    """`steps` M steps, a third through each path, the runner's last."""
    k = steps // 3
    return M("step", kind, frac, seed, k) + M("step_device", kind, frac, seed + k, k) + \
        M("runner", kind, frac, seed + 2 * k, steps - 2 * k)


# every kind x every path: one reset, 60 to 90 M steps, 4 players, HARD, max_steps 100000
KIND_CASES = {f"{kind}-{path}": (N_SWEEP if kind == "sweep" else N,
                                 [X(SEED, 4, 100000)] + M(path, kind, FRACS[kind], 1000 * (k + 1), STEPS[kind]) + ["C"])
              for k, kind in enumerate(KINDS) for path in PATHS}
# players and episode ends: single and all with 3, 2 and 1 players at max_steps 100000 (60 steps), and with
# 4 to 1 players at max_steps 12 (90 steps with a fifth of the envs altered: episodes end and auto-reset
# out of wrapped states)
PLAYER_CASES = {}
for _kind in ("single", "all"):
    for _k, (_p, _ms) in enumerate([(3, 100000), (2, 100000), (1, 100000), (4, 12), (3, 12), (2, 12), (1, 12)]):
        PLAYER_CASES[f"{_kind}-{_p}p-ms{_ms}"] = (N, [X(SEED + 1 + _k, _p, _ms)] + (
            M_mixed(_kind, FRAC, 20000 + 100 * _k, 60) if _ms > 12 else M_mixed(_kind, FRAC_ENDS, 20000 + 100 * _k, 90)) + ["C"])
# auto-reset off past every env's end: the reference's dead step changes nothing, whatever bytes arrive
AUTORESET_OFF_CASE = (N, [X(SEED, 4, 4), "A0"] + M_mixed("single", FRAC_ENDS, 30000, 45) + M_mixed("all", 1.0, 30050, 15) +
                      ["C", "X0", "A1"] + M_mixed("single", FRAC, 30100, 15) + ["C"])
AUTORESET_OFF_ALL_DONE_AT = 2 + 45                         # ops applied when every env has ended (15 dead steps follow)

HANDOVER_MAX_STEPS = (100000, 40)


def M_moves(seed):
    """30 M steps that leave decks narrow on half the envs (a trio launch steps those itself): moves on
    half the envs through env.step and runner.step(), `single` on a tenth through step_device between."""
    return M("step", "move", FRAC, seed, 10) + M("step_device", "single", 0.1, seed + 10, 10) + M("runner", "move", FRAC, seed + 20, 10)


def handover(driver, max_steps, steps=30):
    """X, M_moves, the driver, 30 `single` steps on half the envs, the driver again.  At the first entry
    some 50 envs have a move in progress, 27 of them with narrow decks, and 80 are wide; at the second
    every deck is wide, with pending removes (n_removes up to 255) on 70 to 90 envs and free cards."""
    return [X(SEED, 4, max_steps)] + M_moves(40000) + [(driver, steps)] + M_mixed("single", FRAC, 40100) + [(driver, steps), "C"]


HANDOVER_CASES = {f"{d}-ms{ms}": (N, handover(d, ms)) for d in dc.STEP_DRIVERS for ms in HANDOVER_MAX_STEPS}
SHARD_N = 301
SHARD_CASES = {d: (SHARD_N, dc.for_shards(handover(d, 40))) for d in ("T20", "S20")}
# the large batches: M ops of 5 steps (a compare of all views costs 0.5 GB of traffic there)
BIG_HANDOVER = [X(SEED, 4, 40)] + [("M", p, 5, 50000 + k, "single", FRAC) for k, p in enumerate(PATHS)] + [("S50", 50)] + \
    [("M", p, 5, 50010 + k, "single", FRAC) for k, p in enumerate(PATHS)] + [("T20", 20), "C"]
# the launch-form rows: one `all` hand-over under the launcher's switches
# (M_moves first: `all` names a card type >= 8 in nearly every record, which leaves every deck wide;
# 12 `single` steps before every later driver: `all` alone leaves a handful of players not lean_player)
FORM_N = 200


def _singles(seed):
    return M_mixed("single", FRAC, seed, 12)


FORM_HANDOVER = [X(SEED, 4, 40)] + M_moves(60000) + [("T20", 30)] + M_mixed("all", FRAC, 60100) + _singles(60150) + \
    [("T20", 30)] + _singles(60200) + [("S20", 30), "C"]
FORM_HOST_HANDOVER = [X(SEED, 4, 40)] + M_moves(60000) + [("H", 30)] + M_mixed("all", FRAC, 60100) + _singles(60150) + \
    [("R1", 30)] + _singles(60200) + [("Th20", 30)] + _singles(60250) + [("L", 30)] + _singles(60300) + [("Hs", 30)] + \
    _singles(60350) + [("Ls", 30), "C"]
FEATURES_CASE = (N, [X(SEED, 4, 100000)] + M_mixed("all", FRAC, 70000, 60))


# ---- the census ------------------------------------------------------------------------------------
class Census:
    """What a walk reaches, counted on the oracle alone (a driver_cases.Harness with cg=None calls
    before / after around every M step and entry before every step driver)."""

    def __init__(self):
        self.zero = np.zeros(5, dtype=np.int64)              # executed actions on a zero mask byte, per head
        self.shop255 = self.removes_wrapped = 0              # shop bytes of 255 seen; n_removes 0 -> 255
        self.outside = self.onto_player = self.onto_end = 0  # moves: off the bounding box, onto a player, onto an end hex
        self.entries = []
        self.flags = None                                    # every env's hazard flags, ored over the walk
        self._pending = []

    @staticmethod
    def _s16(v):
        return v - 0x10000 if v & 0x8000 else v

    def before(self, h, acts, hit):
        orc, n = h.orc, h.n
        m = np.ascontiguousarray(orc.selected_action_masks).view(np.uint8).reshape(n, 128)
        head = dc.executed_head(acts)
        dead = np.array(orc.dones, dtype=bool) if not h.autoreset else np.zeros(n, dtype=bool)
        for k, (name, (off, _)) in enumerate(zip(dc.HEAD_NAMES, dc.HEADS)):
            sel = np.nonzero(hit & (head == k) & ~dead)[0]
            self.zero[k] += int((m[sel, off + acts[name][sel].astype(np.int64)] == 0).sum())
        self._pending = []
        if n > 4096:                                         # (the large batches: the mask counts and the entries alone)
            return
        for i in np.nonzero(hit & ((head == 2) | (head == 3)) & ~dead)[0]:
            d = orc.debug_state(int(i))
            self._pending.append((int(i), int(head[i]), d[2], (d[6 + 5 * d[2]] >> 16) & 0xff))

    def after(self, h):
        orc = h.orc
        shop = np.ascontiguousarray(orc.observations["shared"]["shop"])
        self.shop255 += int((shop == 255).any())
        self.flags = orc.flags() if self.flags is None else self.flags | orc.flags()
        for i, head, ag, removes in self._pending:
            if orc.dones[i] and h.autoreset:                 # (the records are the next episode's: a move onto
                self.onto_end += int(head == 3 and orc.rewards[i, ag] > 0)   # an end hex shows in the reward)
                continue
            d = orc.debug_state(i)
            self.onto_end += int(head == 3 and d[6 + 5 * ag] & 0xff != 0)    # has_won: Player::move, the hex is an end
            if head == 2:
                self.removes_wrapped += int(removes == 0 and (d[6 + 5 * ag] >> 16) & 0xff == 255)
                continue
            loc = d[6 + 5 * ag + 4]
            ix = (self._s16(loc & 0xffff) - self._s16(d[26] & 0xffff)) // 2 + 1
            iy = (self._s16(loc >> 16) - self._s16(d[26] >> 16)) // 2 + 1
            self.outside += int(ix < 0 or iy < 0 or ix >= (d[27] & 0xffff) or iy >= (d[27] >> 16))
            self.onto_player += int(any(d[6 + 5 * q + 4] == loc for q in range(h.players) if q != ag))

    def entry(self, h, op):
        """At entry to a step driver: the envs whose current player is not lean_player (rollout_trio.h:
        has_won, a move in progress, pending removes, a free card or a free move) and the wide ones."""
        removes = free = mip = nonlean = 0
        for i in range(h.n):
            d = h.orc.debug_state(i)
            w0, w1 = d[6 + 5 * d[2]], d[6 + 5 * d[2] + 1]
            r, f, m_ = (w0 >> 16) & 0xff, (w0 >> 24) | (w1 & 0xff), (w0 >> 8) & 0xff
            removes, free, mip = removes + int(r != 0), free + int(f != 0), mip + int(m_ != 0)
            nonlean += int((w0 | (w1 & 0xff)) != 0)
        self.entries.append(dict(op=op, nonlean=nonlean, removes=removes, free=free, mip=mip, wide=dc.wide_envs(h.orc)))


def piles_wrapped(orc):
    """Envs with a pile byte >= 128 in some deck."""
    piles = np.ascontiguousarray(orc.observations["player_data"]["obs"]).view(np.uint8).reshape(orc.n, -1)
    return int((piles >= 128).any(1).sum())


def oracle_walk(n, seq, threads=0):
    """The sequence on the oracle alone with a census; returns the Harness (h.census)."""
    h = dc.Harness(None, n, SEED, threads=threads)
    h.census = Census()
    return dc.run(h, seq)


# ---- the reference's streams (tests/golden/ref_offmask.json, oracle/gen_golden.py --offmask) ---------
STREAM_KINDS, STREAM_PLAYERS = ("single", "replace", "all"), (4, 3, 2)
STREAM_STEPS, STREAM_FRAC, STREAM_SCREENED, STREAM_KEEP, STREAM_LEAST = 300, 0.6, 64, 3, 20


def stream_seed(kind, players):
    return 31000 + 1000 * STREAM_KINDS.index(kind) + 100 * players


class Stream:
    """Env `index` of the group (kind, players): a 1-env batch seeded stream_seed + index, its sampler
    the same, its altered actions from a generator of its own, so that the stream is the same alone and
    as env `index` of a batch."""

    def __init__(self, kind, players, index):
        self.kind, self.players, self.index = kind, players, index
        self.seed = stream_seed(kind, players) + index
        self.rng = np.random.default_rng([self.seed, 7])
        self.t = 0

    def next_actions(self, legal):
        acts, hit = dc.offmask_actions(self.rng, legal, self.kind, STREAM_FRAC, self.t)
        self.t += 1
        return acts, hit


def stream_run(e, s, stream, steps):
    """A stream on a 1-env vec `e` and sampler `s` (the oracle's or the reference's): digests after the
    reset and after every step (uint8[steps + 1, 8])."""
    e.reset(stream.seed, stream.players, 3, 2, 100000)
    acts = np.zeros(1, dtype=po.ACTION)
    dig = [po.step_digest(e.observations, e.selected_action_masks, e.rewards, e.dones, e.agent_selection, e.infos, acts)]
    for _ in range(steps):
        s.sample(e.selected_action_masks)
        acts, _ = stream.next_actions(np.array(s.actions, copy=True))
        e.step(acts)
        dig.append(po.step_digest(e.observations, e.selected_action_masks, e.rewards, e.dones, e.agent_selection, e.infos, acts))
    return np.frombuffer(b"".join(dig), dtype=np.uint8).reshape(-1, 8)


def stream_safe_steps(stream_args):
    """Steps of a stream the reference can run: up to the step before the oracle's first REF_UNSAFE flag
    (-1: not even the reset), and the off-mask actions among them."""
    st = Stream(*stream_args)
    o, s = po.OracleVec(1), po.OracleSampler(1, st.seed)
    try:
        o.reset(st.seed, st.players, 3, 2, 100000)
    except RuntimeError:
        return -1, 0
    if o.flags(0) & po.REF_UNSAFE:
        return -1, 0
    off = 0
    for t in range(STREAM_STEPS):
        s.sample(o.selected_action_masks)
        acts, _ = st.next_actions(np.array(s.actions, copy=True))
        k = int(dc.executed_head(acts)[0])
        m = np.ascontiguousarray(o.selected_action_masks).view(np.uint8).reshape(128)
        zero = k >= 0 and m[dc.HEADS[k][0] + int(acts[dc.HEAD_NAMES[k]][0])] == 0
        try:
            o.step(acts)
        except RuntimeError:
            return t, off
        if o.flags(0) & po.REF_UNSAFE:
            return t, off
        off += int(zero)
    return STREAM_STEPS, off
