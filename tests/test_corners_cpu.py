"""CPU side of the reset-parameter corners (tests/corner_cases.py, tests/test_gpu_corners.py):

  the oracle against the unmodified reference with one player and with max_steps 0..3
  (tests/golden/ref_corners.json + ref_corners_digests.npz, oracle/gen_golden.py --corners): every
  step's digest of every env, each up to one step before the reference built here cannot go on
  what each GPU row relies on, counted on the oracle alone: an episode end in every step op of every
  solo / tiny / state row (ends == n x steps wherever max_steps is 0 and auto-reset on), none and 50
  envs with a card type >= 8 in the solo_long rows, no failed map generation anywhere, at most
  13,000 oracle resets per row, the big rows on the pipe and the wave, trio launches entered with
  and without the compact deck image in the state rows
  the launch-form rows' corners sequence (tests/launch_form_cases.py) in the same way
  oracle/asan_harness.c --corners under AddressSanitizer + UndefinedBehaviorSanitizer
"""
import json
import multiprocessing
import os
import subprocess

import numpy as np
import pytest

import corner_cases as cc
import driver_cases as dc
import launch_form_cases as lf
import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")

with open(os.path.join(GOLD, "ref_corners.json")) as _f:
    SETS = json.load(_f)["sets"]


# ---- the oracle against the reference ---------------------------------------------------------------
@pytest.mark.parametrize("st", SETS, ids=[s["name"] for s in SETS])
def test_oracle_matches_reference_corners(st):
    dig = np.load(os.path.join(GOLD, "ref_corners_digests.npz"))[st["name"]]
    assert dig.shape == (sum(st["steps"]) + len(st["steps"]), 8)
    at, ends = 0, 0
    for i, steps, resets in zip(st["index"], st["steps"], st["resets"]):
        o, s = po.OracleVec(1), po.OracleSampler(1, st["sampler_seed"] + i)
        o.reset(st["seed"] + i, st["n_players"], st["n_pieces"], st["difficulty"], st["max_steps"])
        for t in range(steps + 1):
            got = po.step_digest(o.observations, o.selected_action_masks, o.rewards, o.dones, o.agent_selection, o.infos,
                                 s.actions)
            assert got == dig[at + t].tobytes(), f"{st['name']}: seed {st['seed'] + i} differs from the reference at step {t}"
            if t == steps:
                break
            s.sample(o.selected_action_masks if st["mode"] == "sel" else po.stored_masks(o))
            o.step(s.actions)
            ends += int(o.dones[0])
        at += steps + 1
        assert not o.flags(0) & po.REF_UNSAFE
    assert ends == sum(st["resets"])
    if st["max_steps"] == 0:
        assert ends == sum(st["steps"]), "at max_steps 0 every step ends its episode"


def test_fixture_covers_the_corners():
    by = {s["name"]: s for s in SETS}
    assert len(by) == 20 and sum(sum(s["steps"]) for s in SETS) > 20000
    for name in ("solo_1piece_sto", "solo_1piece_sel", "solo_3pieces_ms30_sto"):
        assert by[name]["n_players"] == 1 and len(by[name]["index"]) == 4
    assert by["solo_1piece_sto"]["steps"] == [2000] * 4 and sum(by["solo_3pieces_ms30_sto"]["resets"]) >= 5
    for ms in (0, 1, 2, 3):
        for mode in ("sto", "sel"):
            s = by[f"p4_1piece_ms{ms}_{mode}"]
            assert (s["n_players"], s["max_steps"], s["steps"]) == (4, ms, [80] * 8) and sum(s["resets"]) >= 20
    for players in (3, 2, 1):
        for ms in (1, 2, 3):
            s = [x for x in SETS if x["name"].startswith(f"p{players}_3pieces_ms{ms}_")][0]
            assert (s["n_players"], s["max_steps"]) == (players, ms) and min(s["steps"]) >= 8 and sum(s["resets"]) >= 10
    size = sum(os.path.getsize(os.path.join(GOLD, f)) for f in ("ref_corners.json", "ref_corners_digests.npz"))
    assert size < 250 * 1024


def test_screen_stops_before_a_failed_map_generation():
    """oracle/gen_golden.py screen(): an auto-reset whose map generation fails on the oracle ends the
    screened run there (one piece, HARD, max_steps 0: a reset at every step)."""
    import gen_golden as gg
    found = 0
    for seed in range(200):
        o, s = po.OracleVec(1), po.OracleSampler(1, seed)
        o.reset(seed, 4, 1, 2, 0)
        fail_at = None
        for t in range(40):
            if o.flags(0) & po.REF_UNSAFE:
                break
            s.sample(po.stored_masks(o))
            try:
                o.step(s.actions)
            except RuntimeError:
                fail_at = t
                break
        if fail_at is not None:
            assert gg.screen(seed, 4, 1, 2, 0, seed, "sto", 40) == fail_at
            found += 1
    assert found >= 1, "no seed fails a map generation: the case lost its point"


# ---- what the GPU rows rely on ------------------------------------------------------------------------
def census(job):
    table, case = job
    n, seq = cc.TABLES[table][case]
    try:
        h = dc.run(dc.Harness(None, n, cc.SAMPLER_SEED), seq)
    except RuntimeError as e:                                # (a failed map generation)
        return table, case, repr(e), None, 0, 0, 0
    return table, case, None, h.op_ends, dc.wide_envs(h.orc), h.trio_loaded, h.trio_clear


def census_all(tables):
    jobs = [(t, c) for t in tables for c in cc.TABLES[t]]
    workers = max(1, min(8, po.host_threads()))
    if workers == 1:
        return [census(j) for j in jobs]
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        return pool.map(census, jobs, chunksize=4)


def check_row(table, case, op_ends, skip=()):
    n, seq = cc.TABLES[table][case]
    at = cc.ms_at(seq)
    assert len(op_ends) == len(seq)
    assert sum(op_ends) <= cc.MAX_ORACLE_RESETS, f"{case}: {sum(op_ends)} oracle resets"
    for k in cc.step_ops(seq):
        ms, on = at[k]
        if ms == 0 and on:
            assert op_ends[k] == n * seq[k][1], f"{case}: op {k} {seq[k]!r} holds {op_ends[k]} ends, not n x steps"
        elif k in skip:
            assert op_ends[k] == 0, f"{case}: op {k} {seq[k]!r} does hold ends: {op_ends}"
        else:
            assert op_ends[k] >= 1, f"{case}: op {k} {seq[k]!r} holds no episode end: {op_ends}"


@pytest.mark.slow
@pytest.mark.parametrize("table", ["solo", "tiny"])
def test_solo_and_tiny_rows_keep_their_cases(table):
    """Measured on the oracle (ends per step op, least over the rows, the hand-over's host steps
    included): solo 33 at n = 200 and 4 at 33; tiny at max_steps 1 / 2 / 3 398 / 170 / 37 at n = 200,
    45 / 21 / 4 at 33; n x steps at max_steps 0.  The rows run on up to 8 processes (26 s on 8 cores)."""
    rows = census_all([table])
    assert len(rows) == len(cc.TABLES[table])
    for t, case, err, op_ends, *_ in rows:
        assert err is None, f"{case}: {err}"
        check_row(t, case, op_ends)
    ids = set(cc.TABLES[table])
    if table == "tiny":
        for p in (4, 3, 2, 1):
            for ms in (0, 1, 2, 3):
                drivers = dc.STEP_DRIVERS if (p, ms) in cc.TINY_ALL_DRIVERS else dc.REDUCED_DRIVERS
                for n in (cc.SIZES_MS0 if ms == 0 else cc.SIZES):
                    assert {f"{p}p-ms{ms}-{d}-n{n}" for d in drivers} <= ids
        assert len(ids) == 2 * (4 * 18 + 12 * 6)
    else:
        assert len(ids) == 2 * (18 + 36)


def test_solo_long_rows_hold_no_end_and_wide_decks():
    for t, case, err, op_ends, wide, *_ in census_all(["solo_long"]):
        assert err is None, f"{case}: {err}"
        n, seq = cc.SOLO_LONG[case]
        assert sum(op_ends) == 0 and wide >= cc.SOLO_LONG_WIDE, (case, op_ends, wide)
        assert sum(o[1] for o in seq[1:]) == cc.SOLO_LONG_STEPS and seq[0][2:4] == (1, 1)


def test_state_rows_keep_their_cases():
    rows = {case: r for r in census_all(["state", "two_shard", "lazy"]) for case in [r[1]]}
    for case, (t, _, err, op_ends, wide, loaded, clear) in rows.items():
        assert err is None, f"{case}: {err}"
        check_row(t, case, op_ends, cc.STATE_NO_END_OPS.get(case, ()))
    for case in ("players-and-ms0", "autoreset-off-at-ms0"):  # (>= 3 players at max_steps >= 1: the trio, both ways)
        assert rows[case][5] >= 1 and rows[case][6] >= 1, (case, rows[case][5:])
    assert rows["invalidate-and-clear-at-ms0"][5:] == (0, 0), "max_steps 0 takes no trio launch"
    seq = cc.STATE["players-and-ms0"][1]
    assert [o[2:6:3] for o in seq if not isinstance(o, str) and o[0] == "X"] == [(4, 8), (1, 8), (4, 0), (3, 1), (4, 40)] and "X0" in seq
    for case, (n, seq) in cc.TWO_SHARD.items():
        assert n == cc.TWO_SHARD_N and not any(o[0] in dc.SINGLE_SHARD_ONLY for o in seq)


def test_big_rows_take_the_pipe_and_the_wave(cg):
    if os.environ.get("COG_ROLLOUT") or os.environ.get("COG_TRIO"):
        pytest.skip("rollout kind forced by the environment")
    C = cg._city_of_gold
    assert len(cc.BIG) == 8
    for case, (n, seq) in cc.BIG.items():
        kind = case.split("-")[0]
        assert n == dc.BIG_SIZES[kind] and seq[0] == cc.BIG_RESET and seq[0][2] == 1
        assert C.rollout_kind(n, 1, False) == C.rollout_kind(n, 1, True) == kind
        assert seq[1:] == dc.BIG_CASES[case.split("ms8-")[1]][1:]
    h = dc.run(dc.Harness(None, 400, cc.SAMPLER_SEED), cc.BIG["pipe-1p-ms8-S50_H_S50"][1])
    assert all(e >= 1 for e in h.op_ends[1:]), h.op_ends    # (a 400-env batch of the same walk: ends in every op)


@pytest.mark.parametrize("n", lf.SIZES)
def test_launch_form_corners_sequence_keeps_its_cases(n):
    h = dc.run(dc.Harness(None, n, dc.PAIR_SEED), lf.CORNERS_SEQ)
    at = cc.ms_at(lf.CORNERS_SEQ)
    for k in cc.step_ops(lf.CORNERS_SEQ):
        if at[k][0] == 0:
            assert h.op_ends[k] == n * lf.CORNERS_SEQ[k][1]
        else:
            assert h.op_ends[k] >= 1, (n, k, h.op_ends)
    assert h.trio_loaded >= 1 and h.trio_clear >= 1          # (the 3-player stretch at max_steps 1)
    assert [o[2:6:3] for o in lf.CORNERS_SEQ if not isinstance(o, str) and o[0] == "X"] == [(4, 0), (3, 1), (1, 8), (1, 2)]


def test_launch_form_corners_rows():
    rows = [r for r in lf.ROWS.values() if r.seq in ("corners", "corners-host")]
    assert [r.name for r in rows] == ["corners-default", "corners-no-lat", "corners-epw32", "corners-wpc1", "corners-duo",
                                      "corners-pipe", "corners-wave", "corners-host-no-zerocopy", "corners-host-no-spec"]
    for r in rows:
        assert r.kinds[(1, False)] == r.kinds[(1, True)] != "trio"
        assert r.sizes == (lf.SIZES if r.seq == "corners" else (200,))
    for what, seq in lf.CORNERS_HOST_SEQS.items():
        n = lf.CORNERS_HOST_MS0_N if what == "max_steps 0" else 200
        h = dc.run(dc.Harness(None, n, dc.PAIR_SEED), seq)
        assert [o[0] for o in seq[1:]] == [o[0] for o in lf.HOST_SEQ[1:]]
        assert all(e >= 1 for e in h.op_ends[1:]), (what, h.op_ends)
        if what == "max_steps 0":
            assert h.op_ends[1:] == [n * k for _, k in seq[1:]]


# ---- the stand-alone oracle harness ---------------------------------------------------------------------
def test_oracle_harness_corner_scenarios_clean_under_asan_ubsan(tmp_path):
    """oracle/asan_harness.c --corners: max_steps 0 and 1 (a reset with map generation at every step or
    turn end) and one player, stored and selected masks, in a stand-alone program built with both
    sanitizers: nothing reported, the plain build's hashes."""
    cc_ = os.environ.get("CC", "gcc")                        # (a missing toolchain skips; a failed build of the harness fails)
    probe = subprocess.run([cc_, "-fsanitize=address,undefined", "-x", "c", "-", "-o", str(tmp_path / "probe")],
                           input="int main(void) { return 0; }\n", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("no sanitizer toolchain: " + probe.stderr[-400:])
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "asan"], capture_output=True, text=True)
    assert r.returncode == 0, "make asan failed:\n" + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    plain = subprocess.run([os.path.join(ROOT, "oracle", "_asan", "harness"), "--corners"], capture_output=True, text=True,
                           timeout=120)
    asan = subprocess.run([os.path.join(ROOT, "oracle", "_asan", "harness_asan"), "--corners"], capture_output=True,
                          text=True, env=env, timeout=300)
    assert plain.returncode == 0 and asan.returncode == 0, asan.stderr[-2000:]
    assert "runtime error" not in asan.stderr and "AddressSanitizer" not in asan.stderr, asan.stderr[-2000:]
    assert asan.stdout == plain.stdout
    rows = {ln.split()[0]: ln.split() for ln in plain.stdout.splitlines() if ln.strip()}
    assert sorted(rows) == ["sel_hard_1p_1piece", "sel_hard_ms1_3p", "sto_hard_1p_ms8", "sto_hard_ms0_4p", "sto_hard_ms1_4p"]
    assert int(rows["sto_hard_ms0_4p"][2]) == 16 * 40       # dones summed over the steps: every env at every step
    assert int(rows["sto_hard_ms1_4p"][2]) > 16 and int(rows["sel_hard_ms1_3p"][2]) > 16 and int(rows["sto_hard_1p_ms8"][2]) > 16
