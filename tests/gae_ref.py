"""numpy reference of the per-seat advantage estimator (include/cog.h cog_policy_gae,
city_of_gold.turn_gae), shared by tests/test_policy_gae_cpu.py and tests/test_gpu_policy_gae.py.

  scan    the recursion as include/cog.h states it: per env and seat, next value / advantage / pending
          reward, rows walked from T - 1 down to 0; float64, or float32 (dtype=) with the kernel's
          operations (not necessarily its contractions)
  brute   the definition it has to equal: every env split at its dones, every seat's own rows pulled
          out of every episode, textbook GAE on that subsequence (bootstrapped with 0 after a done,
          with last_values at the window's end)
  window  random windows: agents in runs of 2, 3 or 4 players per env, dones with a given
          probability, rewards NaN wherever not done
  cases   the windows the GPU tests run, so that the CPU test can pin their tolerance
  oracle_window  agents, dones and rewards of the C oracle under the full dynamics

gamma and lam reach the kernel as float32 (the C ABI's type), so every form here rounds them to
float32 first: what is compared is the arithmetic, not the parameters' rounding (d adv / d gamma is
of the order of |delta| / (1 - gamma lam)^2, a few hundred times the 3e-8 that 0.99 moves by)."""
from __future__ import annotations

import functools

import numpy as np

# The largest |scan float32 - scan float64| over everything the GPU tests compare against scan within
# a tolerance (all_gpu_inputs below), advantages and returns alike, as tests/test_policy_gae_cpu.py
# measures it (it fails if this figure is no longer the measured one); TOL is 4 times that: the kernel
# contracts to FMAs and may associate differently from numpy.
MEASURED_F32_DEVIATION = 2.87e-6                           # measured 2.861e-06 (T = 512, gamma = lam = 1), |adv| up to 6.6
TOL = 4 * MEASURED_F32_DEVIATION

SHAPES = ((1, 1), (2, 63), (7, 64), (9, 65), (33, 200), (128, 300), (512, 64))
PARAMS = ((0.99, 0.95), (1.0, 1.0), (0.5, 0.5), (0.997, 0.0))


def f32_params(gamma, lam):
    return float(np.float32(gamma)), float(np.float32(lam))


def scan(values, agents, rewards, dones, last_values=None, gamma=0.99, lam=0.95, dtype=np.float64):
    """(advantages, returns), (T, n) each, in `dtype`."""
    f = np.dtype(dtype).type
    T, n = values.shape
    g, l = (f(x) for x in f32_params(gamma, lam))
    gl = f(g * l)
    nv = np.zeros((n, 4), dtype=f) if last_values is None else np.array(last_values, dtype=f)
    A, R = np.zeros((n, 4), dtype=f), np.zeros((n, 4), dtype=f)
    adv, ret = np.zeros((T, n), dtype=f), np.zeros((T, n), dtype=f)
    idx = np.arange(n)
    for t in range(T - 1, -1, -1):
        d = np.asarray(dones[t]) != 0
        if d.any():
            nv[d], A[d], R[d] = 0, 0, np.asarray(rewards[t])[d].astype(f)
        a = np.asarray(agents[t]).astype(np.int64) & 3
        v = np.asarray(values[t]).astype(f)
        delta = (R[idx, a] + g * nv[idx, a]) - v
        cur = delta + gl * A[idx, a]
        assert cur.dtype == f
        adv[t], ret[t] = cur, cur + v
        A[idx, a], nv[idx, a], R[idx, a] = cur, v, 0
    return adv, ret


def brute(values, agents, rewards, dones, last_values=None, gamma=0.99, lam=0.95):
    """The same by the definition, float64: per env, per episode, per seat, textbook GAE."""
    T, n = values.shape
    g, l = f32_params(gamma, lam)
    values = np.asarray(values, dtype=np.float64)
    adv, ret = np.zeros((T, n)), np.zeros((T, n))
    for i in range(n):
        ends = [int(t) for t in np.flatnonzero(np.asarray(dones[:, i]) != 0)]
        start = 0
        for e in ends + ([T - 1] if not ends or ends[-1] != T - 1 else []):
            done = bool(dones[e, i])
            for p in range(4):
                rows = [t for t in range(start, e + 1) if (int(agents[t, i]) & 3) == p]
                if not rows:
                    continue
                v = values[rows, i]
                r = np.zeros(len(rows))
                boot = 0.0
                if done:
                    r[-1] = float(rewards[e, i, p])
                elif last_values is not None:
                    boot = float(last_values[i, p])
                nxt = np.append(v[1:], boot)
                delta = r + g * nxt - v
                a = 0.0
                for k in range(len(rows) - 1, -1, -1):
                    a = delta[k] + g * l * a
                    adv[rows[k], i], ret[rows[k], i] = a, a + v[k]
            start = e + 1
    return adv, ret


def window(rng, T, n, p_done, integers=False):
    """A random window: dict of values (T, n) f4, agents (T, n) u1, rewards (T, n, 4) f4 (NaN wherever
    not done), dones (T, n) u1, last_values (n, 4) f4, players (n,).  A seat acts for a run of 1..5
    rows, then the next of the env's 2, 3 or 4 seats; the row after a done starts with seat 0.
    integers: values, rewards and last values are integers in [-8, 8]."""
    players = rng.integers(2, 5, size=n)
    seat = rng.integers(0, 4, size=n) % players            # the window opens mid-episode
    left = rng.integers(1, 6, size=n)
    agents = np.zeros((T, n), dtype=np.uint8)
    dones = (rng.random((T, n)) < p_done).astype(np.uint8)
    for t in range(T):
        agents[t] = seat
        left = left - 1
        turn = left == 0
        seat = np.where(turn, (seat + 1) % players, seat)
        left = np.where(turn, rng.integers(1, 6, size=n), left)
        d = dones[t] != 0
        seat = np.where(d, 0, seat)
        left = np.where(d, rng.integers(1, 6, size=n), left)
    if integers:
        draw = lambda shape: rng.integers(-8, 9, size=shape).astype(np.float32)   # noqa: E731
    else:
        draw = lambda shape: rng.normal(size=shape).astype(np.float32)            # noqa: E731
    rewards = np.where((dones != 0)[:, :, None], draw((T, n, 4)), np.float32(np.nan)).astype(np.float32)
    return dict(values=draw((T, n)), agents=agents, rewards=rewards, dones=dones, last_values=draw((n, 4)), players=players)


def p_done_for(T):
    """Done probability sized to the window: about two dones per env, at most every second row."""
    return min(0.5, 2.0 / T)


@functools.lru_cache(maxsize=None)
def case(T, n, integers=False):
    """The window of shape (T, n) that the GPU tests use (read-only, shared)."""
    rng = np.random.default_rng([T, n, int(integers), 20])
    return window(rng, T, n, p_done_for(T), integers)


def features(w):
    """Which of the cases the issue names a window holds."""
    d = w["dones"] != 0
    return dict(done_at_row_0=bool(d[0].any()), done_at_last_row=bool(d[-1].any()),
                consecutive_dones=bool((d[1:] & d[:-1]).any()), env_without_done=bool((~d.any(0)).any()))


def arrays(w):
    return w["values"], w["agents"], w["rewards"], w["dones"]


# ---- recorded from the oracle (the engine matches it bit for bit) ------------------------------
REC = dict(n=200, T=96, max_steps=6, reset_seed=5, sampler_seed=7, pieces=3, difficulty=2)
# one player (seat 0 alone: per-seat GAE is the textbook form): a turn is never shorter, so that REC's
# window holds 0 to 4 episode ends per env; at max_steps 7 from seed 6 it holds 1 to 3, as check_oracle_window asks
REC_SOLO = dict(REC, max_steps=7, reset_seed=6)


def rec(players):
    return REC_SOLO if players == 1 else REC


@functools.lru_cache(maxsize=None)
def oracle_window(players):
    """agents (before each step), dones and rewards (after it) of T steps of the C oracle under the
    full dynamics (the sampler draws from the current agent's stored mask), REC's configuration."""
    import pyoracle as po
    n, T = REC["n"], REC["T"]
    orc, osm = po.OracleVec(n), po.OracleSampler(n, REC["sampler_seed"])
    orc.reset(rec(players)["reset_seed"], players, REC["pieces"], REC["difficulty"], rec(players)["max_steps"])
    agents = np.zeros((T, n), dtype=np.uint8)
    dones = np.zeros((T, n), dtype=np.uint8)
    rewards = np.zeros((T, n, 4), dtype=np.float32)
    for t in range(T):
        agents[t] = orc.agent_selection
        osm.sample(po.stored_masks(orc))
        orc.step(osm.actions)
        dones[t], rewards[t] = orc.dones, orc.rewards
    return dict(agents=agents, dones=dones, rewards=rewards)


def check_oracle_window(w, players):
    """The conditions the recorded test rests on."""
    d = w["dones"] != 0
    per_env = d.sum(0)
    assert per_env.min() >= 1 and per_env.max() <= 3, (per_env.min(), per_env.max())
    for p in range(players):
        assert ((w["agents"] & 3) == p).any(0).all(), f"seat {p} does not act in every env"
    assert not (w["agents"] >= players).any()
    assert d[-1].any(), "no env is done at the last row"
    assert not w["rewards"].any(), "a turn-limit end has no winner"


@functools.lru_cache(maxsize=None)
def recorded_case(players):
    """The oracle's window with values, last values, and rewards planted for check (b): random on
    the done rows, NaN elsewhere."""
    w = oracle_window(players)
    rng = np.random.default_rng([players, 21])
    n, T = REC["n"], REC["T"]
    planted = np.where((w["dones"] != 0)[:, :, None], rng.normal(size=(T, n, 4)), np.nan).astype(np.float32)
    return dict(values=rng.normal(size=(T, n)).astype(np.float32), agents=w["agents"], rewards=w["rewards"],
                planted=planted, dones=w["dones"], last_values=rng.normal(size=(n, 4)).astype(np.float32))


def last_done_row(dones):
    """Per env: the row of its last done, -1 without one."""
    d = np.asarray(dones) != 0
    T = d.shape[0]
    return np.where(d.any(0), T - 1 - d[::-1].argmax(0), -1)


def all_gpu_inputs(with_oracle=True):
    """Every (label, args, kwargs) of scan that a GPU test compares the kernel against within TOL."""
    for T, n in SHAPES:
        w = case(T, n)
        for gamma, lam in PARAMS:
            yield f"random T={T} n={n} gamma={gamma} lam={lam}", arrays(w), dict(last_values=w["last_values"], gamma=gamma, lam=lam)
    if with_oracle:
        for players in (4, 3, 2, 1):
            c = recorded_case(players)
            yield (f"recorded, {players} players", (c["values"], c["agents"], c["planted"], c["dones"]),
                   dict(last_values=c["last_values"]))
