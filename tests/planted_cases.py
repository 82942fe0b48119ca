"""Planted draws (tests/test_planted_draws_cpu.py, tests/test_gpu_planted_draws.py, the `planted`
rows of tests/launch_form_cases.py): generator states chosen so that a given draw lands in the top
32 values of minstd_rand0's range, where uniform_int_distribution may reject it and every kernel
leaves its fast path.

A draw r is risky when r >= K_SMALL_SAFE = RANGE - 31 and rejected when r >= k * (RANGE // k) for a
pile of k; r == RANGE is rejected for every k.  Seeds are states: env i starts at mr_seed(seed + i),
sampler i at mr_seed(seed + first + i), so the state state_before(r, k) makes the k-th draw of that
generator equal r, whichever site consumes it.  Map generation takes the generator by value
(map.cpp:697), so k <= 16 plants the k-th map-generation draw and the k-th initial-hand draw of one
reset, and k = 17..40 the map generation of a reset() with no arguments directly after it.

The batch: N = 70 envs with the planted one at index IDX = 37, lane 37 of a 64-env workgroup with
ordinary lanes on both sides and a second workgroup of 6 (lane 5 of the second workgroup at
COG_TRIO_EPW=32).  The seed a case carries is the planted state - 37; a state below 37 is skipped.

Nothing is listed by hand: every case list comes from a search over k and r on the oracle alone,
reading its census (cog_oracle.h orc_census: which site consumed a risky draw, accepted or
rejected), so an edit of the oracle cannot leave a stale list behind.  Searches run one env (the
planted one: envs are independent) and are cached for the process.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import pyoracle as po

P = 2 ** 31 - 1
RANGE = 2147483645                                         # minstd_rand0's max - min: the largest draw r
K_SMALL_SAFE = RANGE - 31                                  # the lowest risky draw
INV = pow(16807, -1, P)
N, IDX = 70, 37
R_VALUES = (RANGE, RANGE - 1, RANGE - 7, K_SMALL_SAFE)     # always rejected; for some k; the lowest risky
R_CONTROL = K_SMALL_SAFE - 1                               # the highest safe value: no census cell
R_ALL_RISKY = tuple(range(K_SMALL_SAFE, RANGE + 1))
CHUNK = 20                                                 # the launch length of T20 / Th20 / S20
TAIL = 8                                                   # steps after the planted one, at the least
PLAIN_ENV_SEED, PLAIN_SAMPLER_SEED = 77, 4242              # the generator a case does not plant (as state)
HORIZON = 70                                               # steps searched for the planted draw
SAMPLER_T = (0, 1, 2, 3, 4, 5, 15, 16, 17, 18, 19, 20, 21, 23, 24)
PER_CELL = 3
CELLS = tuple(f"{row}/{cls}" for row in ("reset/map", "reset/hands", "steps-selected/deck", "steps-stored/deck",
                                         "steps-stored/active", "steps-autoreset/map", "steps-autoreset/hands",
                                         "sampler/one", "sampler/many")
              for cls in ("accepted", "rejected"))
REJECTED_POSITIONS = (0, 1, 2, 3, range(4, 15), 16, 17, 18, 19)    # of the sampler cases, in a 20-step launch

# group: "reset" | "reset0" | "steps" | "sampler" | "double"; the seeds are what the batch of N is
# given (the planted state - IDX); mode: "sel" | "sto"; steps: driver steps after the reset (0 for
# the reset groups); cells: the census cells the case holds; step: the step that consumes the planted
# draw, pos: its position in a 20-step launch; k, r: what was planted
Case = namedtuple("Case", "group env_seed sampler_seed players max_steps mode steps cells step pos k r")


def state_before(r, k):
    """The generator state whose k-th draw (k >= 1) is r."""
    return (r + 1) * pow(INV, k, P) % P


def draws_apart(lo=1, hi=40):
    """(r1, d, r2): risky values r1, r2 with r2 drawn d draws after r1 from one generator.  Empty for
    d <= 40 (the risky states are -1..-32 mod P; 16807^d maps none of 1..32 into 1..32 there), so the
    case with two events in one run plants the env's generator and the sampler's."""
    out = []
    for r1 in R_ALL_RISKY:
        x = r1 + 1
        for d in range(1, hi + 1):
            x = x * 16807 % P
            if d >= lo and K_SMALL_SAFE <= x - 1 <= RANGE:
                out.append((r1, d, x - 1))
    return out


def _cells_of(env_census, smp_census, mode):
    """Cell names from the census of the planted env (uint32[3, 3, 2]) and sampler (uint32[2, 2]).  The
    deck cells are the draws of a step itself (turn ends, the draw specials); the hands dealt by the
    auto-reset that ends a step are cells of their own (the engine deals them in its map generators'
    kernels, not in draw_n)."""
    cells = []
    for c, cls in enumerate(("accepted", "rejected")):
        if env_census[0, 2, c]:
            cells.append(f"reset/map/{cls}")
        if env_census[0, 0, c]:
            cells.append(f"reset/hands/{cls}")
        if env_census[1, 0, c]:
            cells.append(f"steps-{'selected' if mode == 'sel' else 'stored'}/deck/{cls}")
        if env_census[1, 1, c]:
            cells.append(f"steps-{'selected' if mode == 'sel' else 'stored'}/active/{cls}")
        if env_census[2, 2, c]:
            cells.append(f"steps-autoreset/map/{cls}")
        if env_census[2, 0, c]:
            cells.append(f"steps-autoreset/hands/{cls}")
        if smp_census[0, c]:
            cells.append(f"sampler/one/{cls}")
        if smp_census[1, c]:
            cells.append(f"sampler/many/{cls}")
    return tuple(cells)


def run_one(env_state, smp_state, players, max_steps, mode, steps, reset0=False, env_planted=False):
    """The planted env alone on the oracle.  Returns (cells, step at which the first counted draw was
    consumed or None, flags, for env_planted the second later step at which the env's generator was
    drawn from again within `steps` or None), or None where map generation fails."""
    orc, osm = po.OracleVec(1), po.OracleSampler(1, smp_state)
    try:
        orc.reset(env_state, players, 3, 2, max_steps)
        if reset0:
            orc.reset_default()
    except RuntimeError:
        return None
    first, until = None, None
    if steps:
        # the whole horizon inside the oracle first: most states never meet their draw
        if not po.run(orc, osm, steps, stored=mode == "sto") or orc.flags(0) & po.F_MAPGEN_FAIL:
            return None
        cells = _cells_of(orc.census(0), osm.census(0), mode)
        if any(c.startswith(("steps", "sampler")) for c in cells):
            o2, s2 = po.OracleVec(1), po.OracleSampler(1, smp_state)
            o2.reset(env_state, players, 3, 2, max_steps)
            o2.census_clear()
            for t in range(steps):
                if mode == "sto":
                    s2.sample_stored(o2)
                else:
                    s2.sample(o2.selected_action_masks)
                o2.step(s2.actions)
                if first is None and (o2.census(0).any() or s2.census(0).any()):
                    first, state, later = t, o2.debug_state(0)[0], 0
                elif first is not None:
                    # the env's generator drawn from at two later steps: a state that a wrong fallback
                    # left one draw off shows in what those draw (stored masks: a turn outlasts TAIL)
                    later += int(o2.debug_state(0)[0] != state)
                    state = o2.debug_state(0)[0]
                    if later == 2 or not env_planted:
                        until = t
                        break
    else:
        cells = _cells_of(orc.census(0), osm.census(0), mode)
    return cells, first, int(orc.flags(0)), until


def _case(group, env_state, smp_state, players, max_steps, mode, cells, step, k, r, until=None):
    steps = 0 if step is None else max(step + 1 + TAIL, (until or 0) + 1)
    return Case(group, env_state - IDX, smp_state - IDX, players, max_steps, mode, steps, tuple(cells), step,
                None if step is None else step % CHUNK, k, r)


@functools.lru_cache(maxsize=None)
def reset_cases():
    """k = 1..16 for reset(seed, ...) and k = 17..40 for a reset() with no arguments directly after
    it, every r of R_VALUES and the control."""
    out = []
    for group, ks in (("reset", range(1, 17)), ("reset0", range(17, 41))):
        for k in ks:
            for r in R_VALUES + (R_CONTROL,):
                x = state_before(r, k)
                if x < IDX:
                    continue
                got = run_one(x, PLAIN_SAMPLER_SEED, 4, 100000, "sel", 0, reset0=group == "reset0")
                if got is None:
                    continue
                cells = tuple(c for c in got[0] if c.startswith("reset"))
                if cells or r == R_CONTROL:
                    out.append(_case(group, x, PLAIN_SAMPLER_SEED, 4, 100000, "sel", cells, None, k, r))
    return tuple(out)


def _search_steps(configs, ks, rs, sites, out):
    """Per (players, max_steps, mode): walk k x r until every cell the configuration can hold -- `sites`
    of its mask mode, the auto-reset's map generation at a small max_steps -- has PER_CELL cases; a case
    is kept while one of its cells still wants one."""
    wants = {}
    for players, max_steps, mode, smp_state in configs:
        want = wants.setdefault((players, max_steps, mode), {})
        want.update({} if want else {f"steps-{'selected' if mode == 'sel' else 'stored'}/{site}/{cls}": 0 for site in sites
                for cls in ("accepted", "rejected")})
        if max_steps < HORIZON and "deck" in sites:
            want.update({f"steps-autoreset/{site}/{cls}": want.get(f"steps-autoreset/{site}/{cls}", 0)
                         for site in ("map", "hands") for cls in ("accepted", "rejected")})
        for k in ks:
            if min(want.values()) >= PER_CELL:
                break
            for r in rs:
                x = state_before(r, k)
                if x < IDX:
                    continue
                got = run_one(x, smp_state, players, max_steps, mode, HORIZON + 40, env_planted=True)
                if got is None or got[1] is None or got[1] >= HORIZON or got[3] is None:
                    continue
                cells = tuple(c for c in got[0] if c.startswith("steps"))
                if not any(want.get(c, PER_CELL) < PER_CELL for c in cells):
                    continue
                for c in cells:
                    if c in want:
                        want[c] += 1
                out.append(_case("steps", x, smp_state, players, max_steps, mode, cells, got[1], k, r, got[3]))


# for take_from_active: a pile of one active card, the usual one, rejects RANGE alone
R_ACTIVE = (RANGE, RANGE - 1, K_SMALL_SAFE)
ACTIVE_SAMPLERS = 64                                       # ordinary sampler states tried for it


@functools.lru_cache(maxsize=None)
def step_cases():
    """The env planted at k >= 17: PER_CELL cases per census cell for every (players, max_steps, mask
    mode) searched; 4 players at k = 17..160, 3 and 2 players at k = 17..60; take_from_active (rare:
    it needs a move onto a discard or remove hex, stored masks, and an env draws some 40 times in 70
    steps) from R_ACTIVE at k = 17..48 under up to ACTIVE_SAMPLERS ordinary sampler states;
    then the control value at the (k, configuration) of the first case of every cell."""
    out = []
    S = PLAIN_SAMPLER_SEED
    _search_steps([(4, ms, m, S) for ms in (8, 100000) for m in ("sel", "sto")], range(17, 161), R_VALUES, ("deck",), out)
    _search_steps([(p, 8, m, S) for p in (3, 2) for m in ("sel", "sto")], range(17, 61), R_VALUES, ("deck",), out)
    _search_steps([(4, 100000, "sto", S + v) for v in range(ACTIVE_SAMPLERS)], range(17, 49), R_ACTIVE, ("active",), out)
    seen = set()
    for c in list(out):
        for cell in c.cells:
            if cell not in seen:
                seen.add(cell)
                x = state_before(R_CONTROL, c.k)
                if x >= IDX and not any(q.env_seed == x - IDX and q[2:7] == c[2:7] for q in out):
                    out.append(Case("steps", x - IDX, c.sampler_seed, c.players, c.max_steps, c.mode, c.steps, (), c.step,
                                    c.pos, c.k, R_CONTROL))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sampler_cases():
    """The sampler planted at draw 5t + j + 1: head j of step t while every head has a candidate and no
    earlier draw was rejected; t of SAMPLER_T, j = 0..4, every r of R_VALUES; the control at j = 0, 4."""
    out = []
    for t in SAMPLER_T:
        for j in range(5):
            for r in R_VALUES + ((R_CONTROL,) if j in (0, 4) else ()):
                x = state_before(r, 5 * t + j + 1)
                if x < IDX:
                    continue
                got = run_one(PLAIN_ENV_SEED, x, 4, 8, "sel", t + 1 + TAIL)
                if got is None:
                    continue
                cells = tuple(c for c in got[0] if c.startswith("sampler"))
                if r == R_CONTROL:
                    assert not got[0], (t, j, got)
                    out.append(Case("sampler", PLAIN_ENV_SEED - IDX, x - IDX, 4, 8, "sel", t + 1 + TAIL, (), t, t % CHUNK,
                                    5 * t + j + 1, r))
                elif cells and got[1] == t:
                    out.append(_case("sampler", PLAIN_ENV_SEED, x, 4, 8, "sel", cells, t, 5 * t + j + 1, r))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def double_cases():
    """Two planted events in one run.  No two risky values lie within 40 draws of each other in one
    generator (draws_apart() is empty), so the env and the sampler are both planted: the first step
    case with a rejected draw, with the sampler planted to reject at head 0 of the step after it."""
    for c in step_cases():
        if any(cell.endswith("rejected") for cell in c.cells) and c.mode == "sel" and c.players == 4:
            x = state_before(RANGE, 5 * (c.step + 1) + 1)
            got = run_one(c.env_seed + IDX, x, c.players, c.max_steps, c.mode, c.steps)
            if got is not None and x >= IDX and any(q.startswith("sampler") for q in got[0]) \
                    and any(q.startswith("steps") for q in got[0]):
                return (Case("double", c.env_seed, x - IDX, c.players, c.max_steps, c.mode, c.steps + 1, got[0], c.step,
                             c.pos, c.k, c.r),)
    return ()


def all_cases():
    return reset_cases() + step_cases() + sampler_cases() + double_cases()


def reduced_cases():
    """For the launch-form rows: one case per census cell, then sampler cases with a rejection until
    every launch position of REJECTED_POSITIONS is held, and the double case."""
    out, cells = [], set()
    for c in all_cases():
        if c.group in ("steps", "sampler") and any(q not in cells for q in c.cells):
            cells.update(c.cells)
            out.append(c)
    held = set()
    for c in sampler_cases():
        if any(q.endswith("rejected") for q in c.cells):
            slot = next((k for k, p in enumerate(REJECTED_POSITIONS) if c.pos == p or (isinstance(p, range) and c.pos in p)), None)
            if slot is not None and slot not in held:
                held.add(slot)
                if c not in out:
                    out.append(c)
    return tuple(out) + double_cases()


def cell_counts(cases):
    counts = {c: 0 for c in CELLS}
    for c in cases:
        for q in c.cells:
            counts[q] += 1
    return counts


def ops_of(case, driver):
    """The Harness ops of a case under a step driver (the reset groups take none)."""
    ops = [("X", case.env_seed & 0xFFFFFFFF, case.players, 3, 2, case.max_steps)]
    if case.group == "reset0":
        ops.append("X0")
    if case.steps:
        ops.append((driver, case.steps))
    return ops


DEVICE_VIEW = ("T20", "T2", "T1000", "S20", "S2")


def walk(h, case, driver, what, device_actions=True):
    """One case on a driver_cases.Harness: the sampler anew, the reset(s), the driver, the sampler's
    device actions after a device-view rollout (a single shard, through torch: device_actions), a host
    step that shows where the sampler's generator stands, the hazard flags (compared, then cleared)."""
    if case.steps:
        h.new_sampler(case.sampler_seed)
    ops = ops_of(case, driver)
    if case.steps:
        ops.append(("H", 1))
    for k, op in enumerate(ops):
        try:
            h.apply(op)
            if k == len(ops) - 2 and case.steps and device_actions and driver in DEVICE_VIEW and h.env.num_shards == 1:
                h.compare_device_actions(str(op))
        except AssertionError as e:
            raise AssertionError(f"{what}, {case}: {e}\n  after the sequence {ops[:k + 1]!r}") from None
    try:
        h.apply("C")
    except AssertionError as e:
        raise AssertionError(f"{what}, {case}: {e}") from None


def trace_digests(e, s, case):
    """Per-step digests of the planted env alone -- e, s: a 1-env vec and sampler of the oracle or of the
    reference, made for case.env_seed + IDX and case.sampler_seed + IDX -- after the reset(s), then after
    every step.  Stored masks are those of the env's own agent, as the stored-mask kernels read them:
    agent 0 after a reset (an auto-reset shows as dones), else the agent_selection view."""
    e.reset(case.env_seed + IDX, case.players, 3, 2, case.max_steps)
    if case.group == "reset0":
        e.reset_default()
    dig = [po.step_digest(e.observations, e.selected_action_masks, e.rewards, e.dones, e.agent_selection, e.infos, s.actions)]
    agent = 0
    for _ in range(case.steps):
        s.sample(e.observations["player_data"]["action_mask"][:, agent].copy() if case.mode == "sto" else e.selected_action_masks)
        e.step(s.actions)
        agent = 0 if e.dones[0] else int(e.agent_selection[0])
        dig.append(po.step_digest(e.observations, e.selected_action_masks, e.rewards, e.dones, e.agent_selection, e.infos,
                                  s.actions))
    return np.frombuffer(b"".join(dig), dtype=np.uint8).reshape(-1, 8)


def oracle_digests(case):
    """trace_digests on the oracle, and the env's flags at the end."""
    orc, osm = po.OracleVec(1), po.OracleSampler(1, case.sampler_seed + IDX)
    return trace_digests(orc, osm, case), int(orc.flags(0))


# ---- seed edges: (env seed, sampler seed, sampler first_index) at N = 70; index 37 is where each sum wraps
SEED_EDGES = {
    # env 37: (2^32 - 37 + 37) mod 2^32 = 0 -> state 1 (mr_seed's zero case); the sampler's sum is taken
    # in 64 bits: sampler 37 is mr_seed(2^32) = 2
    "env-wraps-to-0": (2 ** 32 - 37, 2 ** 32 - 37, 0),
    # env 37: seeds P and 2P, multiples of the modulus -> state 1
    "env-P": (P - 37, 99, 0),
    "env-2P": (2 * P - 37, 99, 0),
    # seed + first + i reaches 2^32 and 2^33 at i = 37
    "sampler-past-2^32": (77, 2 ** 32 - 40, 3),
    "sampler-past-2^33": (77, 2 ** 32 - 40, 2 ** 32 + 3),
    "sampler-first-2^33": (77, 5, 2 ** 33 - 42),
}


def case_key(case):
    return f"{case.group}:{case.env_seed}:{case.sampler_seed}:{case.players}:{case.max_steps}:{case.mode}:{case.steps}"
