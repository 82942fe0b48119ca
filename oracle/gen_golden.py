"""Generate tests/golden/ fixtures from the reference core compiled in this container
(oracle/_ref/libref.so = unmodified /root/reference/src/*.cpp + include/*.h + ref_harness.cpp).

TEST INFRASTRUCTURE ONLY; needs /root/reference (dev container), never runs on the GPU box.

Every run is first screened with the C oracle: the reference built against the image's
libstdc++ 11 aborts where map generation erases past the end of valid_indices (map.cpp:727,
needs GCC>=13) or where 2/3-player B-start maps overflow player_locations (map.cpp:347-352).
Reference runs stop one step before the first such hazard.  While generating, the oracle is
compared with the reference at every step (any disagreement aborts generation).

Digest per step (8 bytes): SHA-256 prefix over the named leaf fields (padding excluded) of
observations, selected_action_masks, rewards, dones, agent_selection, infos, actions
(SURVEY App. B.3), for ONE env.  Batch runs are compared env by env (envs are independent:
env i of a batch == a 1-env batch seeded seed+i, sampler seeded sseed+i).

    python oracle/gen_golden.py              # writes tests/golden/*.npz and *.json
    python oracle/gen_golden.py --workloads  # ref_workloads.{npz,json} only
    python oracle/gen_golden.py --lategame   # ref_lategame.json + ref_lategame_digests.npz only
    python oracle/gen_golden.py --bigmaps    # ref_maps_big.json only
    python oracle/gen_golden.py --corners    # ref_corners.json + ref_corners_digests.npz only
    python oracle/gen_golden.py --planted    # ref_planted.json + ref_planted_digests.npz only
    python oracle/gen_golden.py --offmask    # ref_offmask.json + ref_offmask_digests.npz only
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pyoracle as po  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")


def digest_env(e, actions):
    return po.step_digest(e.observations, e.selected_action_masks, e.rewards, e.dones,
                          e.agent_selection, e.infos, actions)


def masks_of(e, mode):
    return e.selected_action_masks if mode == "sel" else po.stored_masks(e)


def screen(seed, np_, npc, diff, max_steps, sseed, mode, steps):
    """Number of steps the reference can run safely (-1: not even the reset)."""
    o = po.OracleVec(1)
    s = po.OracleSampler(1, sseed)
    try:
        o.reset(seed, np_, npc, diff, max_steps)
    except RuntimeError:
        return -1
    if o.flags(0) & po.REF_UNSAFE:
        return -1
    for t in range(steps):
        s.sample(masks_of(o, mode))
        try:
            o.step(s.actions)
        except RuntimeError:                                 # (a failed map generation at an auto-reset)
            return t
        if o.flags(0) & po.REF_UNSAFE:
            return t
    return steps


def ref_trace(seed, np_, npc, diff, max_steps, sseed, mode, steps):
    """Reference digests for t = 0..steps (t=0 right after reset), oracle-checked."""
    r, rs = po.RefVec1(), po.RefSampler1(sseed)
    o, os_ = po.OracleVec(1), po.OracleSampler(1, sseed)
    r.reset(seed, np_, npc, diff, max_steps)
    o.reset(seed, np_, npc, diff, max_steps)
    out = [digest_env(r, rs.actions)]
    resets = 0
    for t in range(steps):
        rs.sample(masks_of(r, mode))
        os_.sample(masks_of(o, mode))
        r.step(rs.actions)
        o.step(os_.actions)
        resets += int(r.dones[0])
        d = digest_env(r, rs.actions)
        if d != digest_env(o, os_.actions):
            raise SystemExit(f"oracle != reference: seed={seed} diff={diff} mode={mode} step={t}")
        out.append(d)
    return out, resets


def traces():
    sets = []
    # name, seed, n_players, n_pieces, difficulty, max_steps, sampler seed, mode, steps, n_envs
    specs = [
        ("C2shape_sel_medium", 12345, 4, 3, 1, 100000, 12345, "sel", 1000, 16),
        ("C3shape_sel_hard", 12345, 4, 3, 2, 100000, 12345, "sel", 1000, 16),
        ("stored_hard_ms30", 7, 4, 3, 2, 30, 7, "sto", 1500, 16),
        ("stored_medium_ms40_bstart", 70000, 4, 3, 1, 40, 70000, "sto", 1500, 16),
        ("c1like_2p_medium_sel", 0, 2, 3, 1, 100000, 0, "sel", 20000, 1),
        ("c1like_2p_medium_sto", 0, 2, 3, 1, 100000, 0, "sto", 5000, 1),
        ("p3_hard_sto_ms60", 300, 3, 3, 2, 60, 300, "sto", 1500, 8),
    ]
    for name, seed, np_, npc, diff, ms, sseed, mode, steps, n in specs:
        envs = []
        i = 0
        while len(envs) < n and i < 64 * n:
            L = screen(seed + i, np_, npc, diff, ms, sseed + i, mode, steps)
            if L > 0:
                dig, resets = ref_trace(seed + i, np_, npc, diff, ms, sseed + i, mode, L)
                envs.append(dict(index=i, steps=L, resets=resets,
                                 digests=np.frombuffer(b"".join(dig), dtype=np.uint8).reshape(-1, 8)))
            i += 1
        tot = sum(e["steps"] for e in envs)
        print(f"{name}: {len(envs)} envs, {tot} reference steps, {sum(e['resets'] for e in envs)} resets")
        sets.append(dict(name=name, seed=seed, n_players=np_, n_pieces=npc, difficulty=diff, max_steps=ms,
                         sampler_seed=sseed, mode=mode, envs=envs))
    return sets


def maps():
    """Reset-only digests for every hazard-free seed of the survey's map sets."""
    out = []
    for diff in (0, 1, 2):
        for npc in ((1, 3) if diff == 0 else (3, 5)):
            for lo in (0, 4096, 63744, 70000):
                for s in range(lo, lo + 256):
                    if screen(s, 4, npc, diff, 100000, s, "sel", 0) < 0:
                        continue
                    r = po.RefVec1()
                    r.reset(s, 4, npc, diff, 100000)
                    o = po.OracleVec(1)
                    o.reset(s, 4, npc, diff, 100000)
                    zero = np.zeros(1, dtype=po.ACTION)
                    d = digest_env(r, zero)
                    if d != digest_env(o, zero):
                        raise SystemExit(f"map mismatch seed={s} diff={diff} npc={npc}")
                    out.append((diff, npc, s, d.hex()))
    print(f"maps: {len(out)} hazard-free reference maps")
    return out


def sampler_kat():
    rng = np.random.default_rng(2024)
    n = 256
    masks = np.zeros((3, n), dtype=po.MASK)
    raw = masks.view(np.uint8).reshape(3, n, 128)
    raw[:, :, :92] = rng.random((3, n, 92)) < 0.35
    raw[:, :5, :] = 0
    acts = np.zeros((3, n), dtype=po.ACTION)
    for i in range(n):
        rs = po.RefSampler1(99 + i)
        for k in range(3):
            rs.sample(masks[k, i:i + 1])
            acts[k, i] = rs.actions[0]
    return masks, acts


# Whole workloads pinned by the reference: final-state digests of every env the reference can run
# (name, n_envs, n_players, n_pieces, difficulty, seed, steps).  c5: bench.py's timed workload
# (65,536 envs, seeds 12345 + i, sampler seeds the same; 5 warm-up + 1,200 steps, the length
# tests/test_gpu_timed_workloads.py drives); c3: BASELINE config C3 at its own size.
WORKLOADS = [("c5", 65536, 4, 3, 2, 12345, 1205), ("c3", 8192, 4, 3, 1, 12345, 1000)]


def _ref_final_digests(job):
    """Worker: the reference's own loop (ref_run_selected) for each listed env, digest at the end."""
    seed0, idx, np_, npc, diff, steps = job
    out = np.zeros((len(idx), 8), dtype=np.uint8)
    for k, i in enumerate(idx):
        r, s = po.RefVec1(), po.RefSampler1(seed0 + int(i))
        r.reset(seed0 + int(i), np_, npc, diff, 100000)
        r.run_selected(s, steps)
        out[k] = np.frombuffer(digest_env(r, s.actions), dtype=np.uint8)
    return out


def workloads():
    """Per workload: the oracle runs the whole batch (threaded) to find the envs the reference can
    run (hazard flags), the reference runs each of those from its seed, and both final states'
    digests must agree env by env (any difference aborts)."""
    from multiprocessing import Pool
    arrays, meta = {}, []
    for name, n, np_, npc, diff, seed, steps in WORKLOADS:
        o, s = po.OracleVec(n), po.OracleSampler(n, seed)
        o.reset_threaded(seed, np_, npc, diff, 100000)
        po.run_threaded(o, s, steps, po.host_threads())
        flags = o.flags()
        safe = (flags & po.REF_UNSAFE) == 0
        idx = np.nonzero(safe)[0].astype(np.uint32)
        odig = po.batch_digest(o.observations[idx], o.selected_action_masks[idx], o.rewards[idx], o.dones[idx],
                               o.agent_selection[idx], o.infos[idx], s.actions[idx])
        del o, s
        jobs = [(seed, part, np_, npc, diff, steps) for part in np.array_split(idx, 64)]
        with Pool(max(1, (os.cpu_count() or 2) - 1)) as pool:
            rdig = np.concatenate(pool.map(_ref_final_digests, jobs))
        bad = np.nonzero((rdig != odig).any(1))[0]
        if bad.size:
            raise SystemExit(f"{name}: oracle != reference at env {int(idx[bad[0]])} after {steps} steps")
        arrays[f"{name}_safe"] = np.packbits(safe)
        arrays[f"{name}_digests"] = rdig
        meta.append(dict(name=name, n_envs=n, n_players=np_, n_pieces=npc, difficulty=diff, seed=seed,
                         sampler_seed=seed, steps=steps, mode="sel", ref_envs=int(idx.size),
                         oracle_only_envs=int(n - idx.size)))
        print(f"{name}: {idx.size} of {n} envs pinned by the reference after {steps} steps "
              f"({n - idx.size} hazard envs: oracle only)")
    np.savez(os.path.join(OUT, "ref_workloads.npz"), **arrays)
    with open(os.path.join(OUT, "ref_workloads.json"), "w") as f:
        json.dump(dict(source="oracle/_ref (unmodified reference core) via oracle/gen_golden.py --workloads",
                       digest="sha256[:8] per env over named leaves of obs, sel, rewards, dones, agent_sel, "
                              "infos, actions after `steps` x (sample(selected masks); step) from reset",
                       arrays="<name>_safe: packbits of the envs the reference ran; <name>_digests: "
                              "uint8[ref_envs, 8] in env order",
                       workloads=meta), f, indent=0)


# The late game, pinned by the reference: 1-env batches, stored masks, one map piece and max_steps
# 100,000, so that episodes end when a player reaches the end hex and the uniform sampler plays
# every special (cards 15..20) and the remove path.  HARD with 4 players is the only family the
# reference built against libstdc++ 11 can run for long with auto-resets (EASY and MEDIUM erase
# past the end of valid_indices, fewer players abort on a B start).
LATEGAME = dict(name="lategame_hard_4p_1piece", n_players=4, n_pieces=1, difficulty=2, max_steps=100000,
                mode="sto", steps=6000, first_seed=6000, screened=256, keep=8, min_each_special=20)


def lategame_screen(seed, cfg):
    """Oracle-only run of one seed: None if the reference cannot run it (a REF_UNSAFE flag anywhere
    in the horizon, or a failed map generation), else its counts (natural ends, specials per card,
    removes).  The effective action follows the step's precedence:
    play > play_special > move > get_from_shop > remove."""
    o, s = po.OracleVec(1), po.OracleSampler(1, seed)
    try:
        o.reset(seed, cfg["n_players"], cfg["n_pieces"], cfg["difficulty"], cfg["max_steps"])
    except RuntimeError:
        return None
    ends, removes, specials = [], 0, {c: 0 for c in range(15, 21)}
    for t in range(cfg["steps"]):
        if o.flags(0) & po.REF_UNSAFE:
            return None
        s.sample(po.stored_masks(o))
        a = s.actions[0]
        try:
            o.step(s.actions)
        except RuntimeError:
            return None
        if not a["play"]:
            if a["play_special"]:
                specials[int(a["play_special"]) - 1] += 1
            elif not a["move"] and not a["get_from_shop"] and a["remove"]:
                removes += 1
        if o.dones[0] and (o.rewards[0] > 0).any():
            ends.append(t)
    if o.flags(0) & po.REF_UNSAFE:
        return None
    return dict(natural_ends=ends, specials=specials, removes=removes)


def lategame():
    cfg = LATEGAME
    # more than half of the envs never buy a special card under the uniform sampler: of the
    # screened seeds with a natural end, keep those that play the most kinds of specials (then the
    # most specials), in seed order
    cands = []
    for seed in range(cfg["first_seed"], cfg["first_seed"] + cfg["screened"]):
        c = lategame_screen(seed, cfg)
        if c is not None and c["natural_ends"]:
            cands.append((seed, c))
    print(f"lategame: {len(cands)} of {cfg['screened']} screened seeds are reference-safe with a natural end")
    cands.sort(key=lambda sc: (-sum(v > 0 for v in sc[1]["specials"].values()), -sum(sc[1]["specials"].values())))
    kept, arrays = [], {}
    for seed, c in sorted(cands[:cfg["keep"]], key=lambda sc: sc[0]):
        dig, resets = ref_trace(seed, cfg["n_players"], cfg["n_pieces"], cfg["difficulty"], cfg["max_steps"],
                                seed, cfg["mode"], cfg["steps"])
        assert resets == len(c["natural_ends"])
        arrays[f"{cfg['name']}__{len(kept)}"] = np.frombuffer(b"".join(dig), dtype=np.uint8).reshape(-1, 8)
        kept.append(dict(seed=seed, sampler_seed=seed, steps=cfg["steps"], natural_ends=c["natural_ends"],
                         specials={str(k): v for k, v in c["specials"].items()}, removes=c["removes"]))
        print(f"lategame: seed {seed}: ends at {c['natural_ends']}, specials {list(c['specials'].values())}, "
              f"{c['removes']} removes")
    assert len(kept) == cfg["keep"], f"only {len(kept)} seeds with a natural end among {cfg['screened']}"
    totals = {str(c): sum(e["specials"][str(c)] for e in kept) for c in range(15, 21)}
    assert min(totals.values()) >= cfg["min_each_special"], totals
    np.savez_compressed(os.path.join(OUT, "ref_lategame_digests.npz"), **arrays)
    with open(os.path.join(OUT, "ref_lategame.json"), "w") as f:
        json.dump(dict(source="oracle/_ref (unmodified reference core) via oracle/gen_golden.py --lategame",
                       digest="sha256[:8] over named leaves of obs, sel, rewards, dones, agent_sel, infos, actions",
                       digests_file="ref_lategame_digests.npz (key <name>__<k>, uint8[steps+1, 8]: after reset, "
                                    "then after every step)",
                       name=cfg["name"], n_players=cfg["n_players"], n_pieces=cfg["n_pieces"],
                       difficulty=cfg["difficulty"], max_steps=cfg["max_steps"], mode=cfg["mode"],
                       steps=cfg["steps"], total_specials=totals,
                       total_natural_ends=sum(len(e["natural_ends"]) for e in kept),
                       total_removes=sum(e["removes"] for e in kept), envs=kept), f, indent=0)
    print(f"lategame: {len(kept)} seeds, specials {totals}")


# Big maps, pinned by the reference: reset-only digests at 2, 4, 6 and 7 map pieces (ref_maps.json
# stops at 5), with 2 and 3 players too (A starts only: a B start overflows player_locations).
# Each group (difficulty, pieces, players) takes its seeds from the first 256-aligned window in
# which the oracle raises no error flag, so that a test can reset the whole window as one batch;
# from 6 pieces on most seeds erase past the end of valid_indices and cannot run here.
# off_lattice: (difficulty, pieces, seed) of maps on which a failed travel placement leaves a small
# piece reset at the origin and the recursion connects pieces to it there, half a cell off the map's
# lattice (the oracle's gen_stats count such hexes); found among seeds 700000 + i and 1100000 + i,
# i < 65536, the four of them that the reference built here can run.
BIGMAPS = dict(pieces=(2, 4, 6, 7), difficulties=(1, 2), window=256, windows_tried=16,
               keep={4: 24, 3: 8, 2: 8},
               off_lattice=((2, 4, 713086), (2, 4, 762327), (2, 4, 1124763), (2, 4, 1163566)))


def bigmaps():
    cfg, out = BIGMAPS, []
    err = po.F_MAPGEN_FAIL | po.F_GRID_OVER
    zero = np.zeros(1, dtype=po.ACTION)
    for diff in cfg["difficulties"]:
        for npc in cfg["pieces"]:
            for np_ in (4, 3, 2):
                for w in range(cfg["windows_tried"]):
                    lo = w * cfg["window"]
                    o = po.OracleVec(cfg["window"])
                    try:
                        o.reset_threaded(lo, np_, npc, diff, 100000)
                    except RuntimeError:
                        continue
                    flags = o.flags()
                    if not (flags & err).any():
                        break
                else:
                    raise SystemExit(f"no clean window: diff={diff} npc={npc} players={np_}")
                safe = [lo + int(i) for i in np.nonzero((flags & po.REF_UNSAFE) == 0)[0]][:cfg["keep"][np_]]
                for s in safe:
                    r, o1 = po.RefVec1(), po.OracleVec(1)
                    r.reset(s, np_, npc, diff, 100000)
                    o1.reset(s, np_, npc, diff, 100000)
                    d = digest_env(r, zero)
                    if d != digest_env(o1, zero):
                        raise SystemExit(f"map mismatch seed={s} diff={diff} npc={npc} players={np_}")
                    out.append((diff, npc, s, d.hex(), np_))
                print(f"bigmaps: diff {diff}, {npc} pieces, {np_} players: {len(safe)} reference maps from window {lo}")
    off = []
    for diff, npc, s in cfg["off_lattice"]:
        r, o1 = po.RefVec1(), po.OracleVec(1)
        o1.reset(s, 4, npc, diff, 100000)
        assert not o1.flags(0) & po.REF_UNSAFE and o1.gen_stats()["offlat"][0] > 0, s
        r.reset(s, 4, npc, diff, 100000)
        d = digest_env(r, zero)
        if d != digest_env(o1, zero):
            raise SystemExit(f"off-lattice map mismatch seed={s} diff={diff} npc={npc}")
        off.append((diff, npc, s, d.hex(), 4))
    with open(os.path.join(OUT, "ref_maps_big.json"), "w") as f:
        json.dump(dict(source="oracle/_ref (unmodified reference core) via oracle/gen_golden.py --bigmaps",
                       entry="[difficulty, n_pieces, seed, digest, n_players]: sha256[:8] over named leaves of obs, "
                             "sel, rewards, dones, agent_sel, infos and one all-zero action record, after reset",
                       window=cfg["window"], entries=out, off_lattice=off), f)
    print(f"bigmaps: {len(out)} reference maps, {len(off)} off-lattice ones")


# The corners of the reset parameters, pinned by the reference: one player (the turn passes back to
# the same player) and max_steps 0..3 (an episode ends at its first step, or at one of its first
# turn ends).  Every env runs to one step before its first REF_UNSAFE flag or failed map generation
# on the oracle: with fewer than 4 players every second reset is a B start, which the reference
# built here cannot run, so those groups screen 64 seeds and keep the ones that run 8 steps or more.
# (name, n_players, n_pieces, max_steps, mode, steps, first seed, seeds screened, seeds kept, least steps)
def corner_groups():
    g = [("solo_1piece_sto", 1, 1, 100000, "sto", 2000, 9100, 64, 4, 2000),
         ("solo_1piece_sel", 1, 1, 100000, "sel", 1000, 9200, 64, 4, 1000),
         ("solo_3pieces_ms30_sto", 1, 3, 30, "sto", 600, 9300, 256, 4, 600)]
    for ms in (0, 1, 2, 3):
        for mode in ("sto", "sel"):
            g.append((f"p4_1piece_ms{ms}_{mode}", 4, 1, ms, mode, 80, 9400 + 10 * ms, 64, 8, 80))
    for players in (3, 2, 1):
        for ms in (1, 2, 3):
            mode = "sel" if (players + ms) % 2 else "sto"
            g.append((f"p{players}_3pieces_ms{ms}_{mode}", players, 3, ms, mode, 24, 9500 + 100 * players + 10 * ms, 64, 64, 8))
    return g


def corners():
    sets, arrays = [], {}
    for name, np_, npc, ms, mode, steps, seed, screened, keep, least in corner_groups():
        envs, digs = [], []
        for i in range(screened):
            if len(envs) == keep:
                break
            L = screen(seed + i, np_, npc, 2, ms, seed + i, mode, steps)
            if L < least:
                continue
            dig, resets = ref_trace(seed + i, np_, npc, 2, ms, seed + i, mode, L)
            digs.append(np.frombuffer(b"".join(dig), dtype=np.uint8).reshape(-1, 8))
            envs.append(dict(index=i, steps=L, resets=resets))
        assert envs and (keep == screened or len(envs) == keep), f"{name}: {len(envs)} seeds of {screened} run {least} steps"
        print(f"corners: {name}: {len(envs)} envs, {sum(e['steps'] for e in envs)} reference steps, "
              f"{sum(e['resets'] for e in envs)} episode ends")
        arrays[name] = np.concatenate(digs)                  # (one array per set: 347 zip members cost 100 KB)
        sets.append(dict(name=name, seed=seed, n_players=np_, n_pieces=npc, difficulty=2, max_steps=ms, sampler_seed=seed,
                         mode=mode, index=[e["index"] for e in envs], steps=[e["steps"] for e in envs],
                         resets=[e["resets"] for e in envs]))
    np.savez(os.path.join(OUT, "ref_corners_digests.npz"), **arrays)
    with open(os.path.join(OUT, "ref_corners.json"), "w") as f:
        json.dump(dict(source="oracle/_ref (unmodified reference core) via oracle/gen_golden.py --corners",
                       digest="sha256[:8] over named leaves of obs, sel, rewards, dones, agent_sel, infos, actions",
                       digests_file="ref_corners_digests.npz (key <set>: the envs of the set one after another, each "
                                    "uint8[steps[k] + 1, 8]: after reset, then after every step); env k of a set: seed + "
                                    "index[k], sampler seed + index[k]; resets[k]: its episode ends",
                       sets=sets), f)


def planted_safe_steps(pc, case):
    """Steps of `case` the reference can run, from the oracle's flags after the reset(s) and after every
    step (-1: not even the resets; a failed map generation ends the run like a flag)."""
    o, s = po.OracleVec(1), po.OracleSampler(1, case.sampler_seed + pc.IDX)
    try:
        o.reset(case.env_seed + pc.IDX, case.players, 3, 2, case.max_steps)
        if case.group == "reset0":
            o.reset_default()
    except RuntimeError:
        return -1
    if o.flags(0) & po.REF_UNSAFE:
        return -1
    agent = 0
    for t in range(case.steps):
        s.sample(o.observations["player_data"]["action_mask"][:, agent].copy() if case.mode == "sto" else o.selected_action_masks)
        try:
            o.step(s.actions)
        except RuntimeError:
            return t
        if o.flags(0) & po.REF_UNSAFE:
            return t
        agent = 0 if o.dones[0] else int(o.agent_selection[0])
    return case.steps


def planted():
    """The planted draws (tests/planted_cases.py), pinned by the reference: for the planted env alone,
    the reference's digests after the reset(s) and after every step it can run of every case."""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    import planted_cases as pc
    keys, lengths, digs = [], [], []
    out_reset, cut, whole = 0, 0, 0
    for case in pc.all_cases():
        L = planted_safe_steps(pc, case)
        if L < 0:
            out_reset += 1
            continue
        cut += int(L < case.steps)
        whole += int(L == case.steps)
        run = case._replace(steps=L)
        d = pc.trace_digests(po.RefVec1(), po.RefSampler1(case.sampler_seed + pc.IDX), run)
        if not np.array_equal(d, pc.trace_digests(po.OracleVec(1), po.OracleSampler(1, case.sampler_seed + pc.IDX), run)):
            raise SystemExit(f"oracle != reference: planted case {case}")
        keys.append(pc.case_key(case))
        lengths.append(L)
        digs.append(d)
    np.savez(os.path.join(OUT, "ref_planted_digests.npz"), digests=np.concatenate(digs))
    with open(os.path.join(OUT, "ref_planted.json"), "w") as f:
        json.dump(dict(source="oracle/_ref (unmodified reference core) via oracle/gen_golden.py --planted",
                       digest="sha256[:8] over named leaves of obs, sel, rewards, dones, agent_sel, infos, actions, of the "
                              "planted env alone (a 1-env batch seeded env seed + 37, sampler seed + 37)",
                       digests_file="ref_planted_digests.npz (digests: the cases one after another, each uint8[steps[k] + 1, "
                                    "8]: after the reset(s), then after every step)",
                       key="group:env seed:sampler seed:players:max_steps:mask mode:steps of the case",
                       screened=dict(cases=len(keys) + out_reset, recorded_whole=whole, recorded_cut=cut, left_out=out_reset,
                                     why="the reference built against libstdc++ 11 cannot run past a REF_UNSAFE flag of "
                                         "the oracle (an erase past the end of valid_indices, a B start with fewer than 4 "
                                         "players, a lookup outside hex_array) or a failed map generation: a case whose "
                                         "reset raises one is left out, a case whose step t raises one is recorded up to "
                                         "step t - 1"),
                       keys=keys, steps=lengths), f, separators=(",", ":"))
    print(f"planted: {len(keys)} cases recorded ({whole} whole, {cut} cut at a hazard), {out_reset} left out")


def offmask():
    """Host actions the mask forbids (tests/offmask_cases.py), pinned by the reference: single-env streams
    of kinds single, replace and all with 4, 3 and 2 players, 300 steps with 60 % of the sampled actions
    altered, each cut at the step before the oracle's first REF_UNSAFE flag.  Per group the first
    STREAM_KEEP seeds that run STREAM_LEAST steps or more; the fixture holds the groups' parameters, each
    stream's index, length and off-mask count, and the reference's digests.  The actions come from the
    stream's seed (tests/offmask_cases.py Stream)."""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    import offmask_cases as oc
    groups, digs = [], []
    for kind in oc.STREAM_KINDS:
        for players in oc.STREAM_PLAYERS:
            index, steps, off = [], [], []
            for i in range(oc.STREAM_SCREENED):
                if len(index) == oc.STREAM_KEEP:
                    break
                L, k = oc.stream_safe_steps((kind, players, i))
                if L < oc.STREAM_LEAST:
                    continue
                d = oc.stream_run(po.RefVec1(), po.RefSampler1(oc.stream_seed(kind, players) + i), oc.Stream(kind, players, i), L)
                o = oc.stream_run(po.OracleVec(1), po.OracleSampler(1, oc.stream_seed(kind, players) + i),
                                  oc.Stream(kind, players, i), L)
                if not np.array_equal(d, o):
                    t = int(np.nonzero((d != o).any(1))[0][0])
                    raise SystemExit(f"oracle != reference: offmask stream {kind}, {players} players, index {i}, step {t}")
                index.append(i)
                steps.append(L)
                off.append(k)
                digs.append(d)
            assert len(index) == oc.STREAM_KEEP, f"{kind}, {players} players: {len(index)} streams of {oc.STREAM_SCREENED} seeds"
            print(f"offmask: {kind}, {players} players: indices {index}, steps {steps}, off-mask actions {off}")
            groups.append(dict(kind=kind, n_players=players, seed=oc.stream_seed(kind, players), index=index, steps=steps,
                               off_mask=off))
    np.savez(os.path.join(OUT, "ref_offmask_digests.npz"), digests=np.concatenate(digs))
    with open(os.path.join(OUT, "ref_offmask.json"), "w") as f:
        json.dump(dict(source="oracle/_ref (unmodified reference core) via oracle/gen_golden.py --offmask",
                       digest="sha256[:8] over named leaves of obs, sel, rewards, dones, agent_sel, infos, actions",
                       digests_file="ref_offmask_digests.npz (digests: the streams one after another in group order, each "
                                    "uint8[steps[k] + 1, 8]: after the reset, then after every step)",
                       stream="env seed + index[k] and sampler seed + index[k], n_pieces 3, HARD, max_steps 100000, the "
                              "sampler on the selected mask, then the action altered as tests/offmask_cases.py Stream does "
                              f"(fraction {oc.STREAM_FRAC}); off_mask: executed actions on a zero mask byte",
                       groups=groups), f, separators=(",", ":"))


def main():
    assert po.ref_available(), "build the reference first: make -C oracle ref"
    os.makedirs(OUT, exist_ok=True)
    if "--offmask" in sys.argv:
        offmask()
        return
    if "--bigmaps" in sys.argv:
        bigmaps()
        return
    if "--workloads" in sys.argv:
        workloads()
        return
    if "--lategame" in sys.argv:
        lategame()
        return
    if "--corners" in sys.argv:
        corners()
        return
    if "--planted" in sys.argv:
        planted()
        return
    t = traces()
    arrays = {}
    for st in t:
        for k, e in enumerate(st["envs"]):
            arrays[f"{st['name']}__{k}"] = e.pop("digests")
    np.savez(os.path.join(OUT, "ref_trace_digests.npz"), **arrays)
    with open(os.path.join(OUT, "ref_traces.json"), "w") as f:
        json.dump(dict(source="oracle/_ref (unmodified reference core) via oracle/gen_golden.py",
                       digest="sha256[:8] over named leaves of obs, sel, rewards, dones, agent_sel, infos, actions",
                       digests_file="ref_trace_digests.npz (key <set>__<k>, uint8[steps+1, 8])",
                       sets=t), f, indent=0)
    m = maps()
    with open(os.path.join(OUT, "ref_maps.json"), "w") as f:
        json.dump(dict(source="oracle/_ref via oracle/gen_golden.py", entries=m), f)
    masks, acts = sampler_kat()
    np.savez_compressed(os.path.join(OUT, "ref_sampler_kat.npz"), masks=masks.view(np.uint8),
                        actions=acts.view(np.uint8), seed=np.array([99]))
    print("wrote", sorted(os.listdir(OUT)))


if __name__ == "__main__":
    main()
