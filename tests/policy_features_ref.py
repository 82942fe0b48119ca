"""numpy reference of the policy features (include/cog.h cog_env_policy_features,
city_of_gold.policy_features), and the oracle runs the tests of it share
(tests/test_policy_features_cpu.py, tests/test_gpu_policy_features.py).

features_ref works from what an OracleVec publishes -- its ObsData records, its agent_selection and
its player_cells() -- and takes the map channels from observations.shared.map, not from hex codes:
the kernel reads the engine's compact hex-code grid, and the comparison holds that path to the
published map.  Values are float32; to_bf16_bits rounds them to bfloat16 (nearest even) by bit
arithmetic, which the CPU tests hold to torch's own conversion."""
from __future__ import annotations

import numpy as np

import pyoracle as po

VEC, CHANNELS, GRID, MAX_RADIUS = 208, 10, 48, 24
PILES = ("draw", "hand", "active", "played", "discard")     # DeckObs order, 21 types each


def to_bf16_bits(x):
    """float32 -> the uint16 bit patterns of bfloat16, round to nearest even (no NaN here)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_bits_to_float(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def features_ref(obs_records, agent_selection, cells, n_players, radius, seats=None):
    """(vec float32 (n, 208), local float32 (n, 10, W, W)) of n ObsData records; cells: int (n, 4, 2),
    every player's (ix, iy); n_players: an int or (n,) ints; seats: (n,) seat numbers (their low two
    bits count), an int, or None for the acting seat, agent_selection & 3."""
    obs = np.asarray(obs_records)
    n = obs.shape[0]
    W = 2 * radius + 1
    nps = np.broadcast_to(np.asarray(n_players, dtype=np.int64), (n,))
    seats = agent_selection if seats is None else seats
    seats = np.broadcast_to(np.asarray(seats, dtype=np.int64), (n,)) & 3
    vec = np.zeros((n, VEC), dtype=np.float32)
    local = np.zeros((n, CHANNELS, W, W), dtype=np.float32)
    for i in range(n):
        s, npl = int(seats[i]), int(nps[i])
        if s >= npl:
            continue
        sh, pd = obs[i]["shared"], obs[i]["player_data"]
        ix, iy = int(cells[i, s, 0]), int(cells[i, s, 1])
        v = vec[i]
        v[0] = float(sh["phase"])
        v[1:4] = sh["current_resources"]
        v[4:22] = sh["shop"].astype(np.float32)
        v[22] = npl
        v[23], v[24] = ix, iy
        v[25:130] = np.concatenate([pd[s]["obs"][p] for p in PILES]).astype(np.float32)
        # the window: cell (ix - radius + a, iy - radius + b), the part of it inside the grid
        a0, a1 = max(0, radius - ix), min(W, GRID + radius - ix)
        b0, b1 = max(0, radius - iy), min(W, GRID + radius - iy)
        if a0 < a1 and b0 < b1:
            part = sh["map"][ix - radius + a0:ix - radius + a1, iy - radius + b0:iy - radius + b1, 1:7]
            local[i, 0:6, a0:a1, b0:b1] = np.moveaxis(part, 2, 0).astype(np.float32)
            local[i, 9, a0:a1, b0:b1] = 1.0
        for r in (1, 2, 3):
            if r >= npl:
                continue
            p = (s + r) % npl
            px, py = int(cells[i, p, 0]), int(cells[i, p, 1])
            deck = pd[p]["obs"]
            k = 130 + 26 * (r - 1)
            v[k] = 1.0
            v[k + 1], v[k + 2] = px - ix, py - iy
            v[k + 3] = int(deck["hand"].astype(np.int64).sum())
            v[k + 4] = int(deck["draw"].astype(np.int64).sum())
            v[k + 5:k + 26] = sum(deck[q].astype(np.int64) for q in PILES).astype(np.float32)
            a, b = px - ix + radius, py - iy + radius
            if 0 <= a < W and 0 <= b < W and 0 <= px < GRID and 0 <= py < GRID:
                local[i, 5 + r, a, b] = 1.0
    return vec, local


def oracle_features(orc, players, radius, seats=None):
    return features_ref(orc.observations, orc.agent_selection, orc.player_cells()[0], players, radius, seats)


# ---- the oracle runs the tests share -----------------------------------------------------------
# (n, reset seed, players, pieces, difficulty, sampler seed); max_steps is the default 100000
RUN_A = dict(n=32, seed=7, players=4, pieces=3, difficulty=0, sampler_seed=7)
RUN_B = dict(n=32, seed=7, players=4, pieces=10, difficulty=2, sampler_seed=7)
RUN_A_CHECKS = (0, 1, 5, 20, 60, 120)                       # steps of run A at which the GPU tests compare
RUN_B_STEPS = 60


def oracle_pair(run, n=None, players=None):
    n = run["n"] if n is None else n
    orc, osm = po.OracleVec(n), po.OracleSampler(n, run["sampler_seed"])
    orc.reset(run["seed"], run["players"] if players is None else players, run["pieces"], run["difficulty"], 100000)
    return orc, osm


def oracle_step(orc, osm):
    """One step under the full dynamics: the stored mask of every env's own agent."""
    osm.sample_stored(orc)
    orc.step(osm.actions)
