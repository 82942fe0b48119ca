"""Launch forms (tests/test_gpu_launch_forms.py, tests/test_driver_sequences_cpu.py): the rows of
environment switches under which the rollout launcher takes another kernel or another form of one
(cog_engine.hip rollout_kind, trio_epw, trio_pad_lds, fixup_grid, trio_form; cog_abi.cpp's host-path
switches), the sequences each row walks, and the child process that walks them.

The switches are read once into statics, so a row is a child process whose environment carries it.
The child (child_main) first checks cog_rollout_kind and cog_trio_form_of against what the row must
show -- a misspelt or ignored switch fails there, before any launch -- then walks a
driver_cases.Harness through the row's sequences (all six views against the oracle after every op,
then the hazard flags per env) and prints the form as JSON on its last line.

Batch sizes: 200 envs are three full trio workgroups and one of 8 envs at 64 envs per workgroup, six
full ones and one of 8 at 32; 33 envs are one workgroup at 64, two at 32 with the second holding one
env.  16,385 envs are 257 workgroups: one more than a whole MI355X has CUs.
"""
from __future__ import annotations

import json
import sys

import driver_cases as dc
import offmask_cases as oc

P = dc.PAIR_STEPS                                          # steps per op (30)
SIZES = (200, 33)
BIG_N = 16385
LDS_PER_CU = 163840                                        # gfx950
TRIO_LDS_MAX = 54613                                       # rollout_trio.h's static_assert on sizeof(TrioLds)
TRIO_LDS_MIN = LDS_PER_CU // 3 - 2048                      # below it $COG_TRIO_WPC=3 would pad (it does not)


def X(seed, players, max_steps):
    return ("X", seed, players, 3, 2, max_steps)


T20, S20 = ("T20", P), ("S20", P)
# the rollout sequence.  ops 1..6: launches of 20 + 10, 2 x 15 and 30 steps between stored-mask
# launches and host steps; 8..10 with 3 players; 12..14 walk the no-fix-up bound at max_steps 40
# (0 + 20, 20 + 10, then past it); 17, 18 with auto-reset off until every env has ended
ROLLOUT_SEQ = [X(77, 4, 8), T20, S20, T20, ("H", 5), ("T2", P), ("T1000", P),
               X(78, 3, 8), T20, S20, T20,
               X(80, 4, 40), T20, T20, T20,
               X(81, 4, 8), "A0", T20, T20, "X0", "A1", T20, "C"]
ROLLOUT_END_OPS = (1, 2, 3, 4, 5, 6, 8, 9, 10, 17, 18)    # ops that hold an episode end on the oracle
ROLLOUT_ALL_DONE_AT = 19                                   # ops applied when every env of 200 has ended
# 2 players behind a forced pipe / wave: the oracle raises ERASE_PAST / Q9_OOB / OOB_LOOKUP /
# B_START_LT4 there (the flags must match per env)
TWO_PLAYER_TAIL = [X(79, 2, 8), T20, S20, T20]
REDO_SEQ = [X(77, 4, 8), T20, T20, T20, X(77, 4, 100000), T20, T20, T20]
HOST_SEQ = [X(77, 4, 8), ("H", P), ("Hc", P), ("Hs", P), ("R1", P), ("Rr", 5), ("Th20", P), ("L", P), ("Ls", P),
            ("H", P), T20, ("H", P)]
HOST_TWO_SHARD_N = 301
# the reset-parameter corners (tests/corner_cases.py): max_steps 0 (launches of 20 + 4, 8 and 8 steps: every env
# ends at every step, 8,000 oracle resets at n = 200; 4 players take the kernels of 2 there), 3 players at
# max_steps 1 (the trio, an end at every turn end), one player at max_steps 8 and 2 (the next agent is the
# acting agent)
P0 = 24
CORNERS_SEQ = [X(77, 4, 0), ("T20", P0), ("S20", 8), ("T20", 8), X(78, 3, 1), T20, S20, T20,
               X(79, 1, 8), T20, S20, T20, ("H", 5), X(80, 1, 2), T20, S20, "C"]
# the host walk after a reset with one player (at the row's n) and at max_steps 0 (70 envs, 8 steps per op)
CORNERS_HOST_MS0_N, CORNERS_HOST_MS0_STEPS = 70, 8
CORNERS_HOST_SEQS = {"one player": [X(77, 1, 8)] + HOST_SEQ[1:],
                     "max_steps 0": [X(77, 4, 0)] + [(d, min(k, CORNERS_HOST_MS0_STEPS)) for d, k in HOST_SEQ[1:]]}


# the planted draws (tests/planted_cases.py): the reduced list -- a case per census cell, a sampler
# rejection at every launch position, the case with two events -- at 70 envs with the planted one at
# index 37, under the rollout drivers or (COG_NO_SPEC) the host drivers
PLANTED_DRIVERS, PLANTED_HOST_DRIVERS = ("T20", "S20"), ("H", "Hc", "Hs", "R1", "L", "Ls")
PLANTED_N = 70


class Row:
    """env: the switches; sizes: the batch sizes it runs at; seq: "rollout" | "rollout+2p" | "redo" |
    "big" | "host" | "corners" | "corners-host" | "planted" | "planted-host" | "offmask" | "offmask-host"; kinds: what rollout_kind must say for (players, stored) -> name."""

    def __init__(self, name, env, seq="rollout", sizes=SIZES, kinds=None):
        self.name, self.env, self.seq, self.sizes = name, dict(env), seq, tuple(sizes)
        self.kinds = kinds if kinds is not None else {(4, False): "trio", (3, False): "trio", (2, False): "duo",
                                                      (4, True): "duo", (1, False): "duo", (1, True): "duo"}


def _all(kind):
    return {(p, s): kind for p in (4, 3, 2, 1) for s in (False, True)}


ROWS = {r.name: r for r in (
    Row("default", {}),
    Row("no-lat", {"COG_TRIO_JT": "0"}),
    Row("lat-shared-cu", {"COG_TRIO_JT": "1"}, seq="big", sizes=(BIG_N,),
        kinds={(4, False): "trio", (4, True): "pipe"}),
    Row("epw32", {"COG_TRIO_EPW": "32"}),
    Row("epw32-no-lat", {"COG_TRIO_EPW": "32", "COG_TRIO_JT": "0"}),
    Row("wpc1", {"COG_TRIO_WPC": "1"}),
    Row("wpc2", {"COG_TRIO_WPC": "2"}),
    Row("wpc3", {"COG_TRIO_WPC": "3"}),
    Row("wpc4", {"COG_TRIO_WPC": "4"}),
    Row("redo-no-lat", {"COG_DEBUG_REDO_STEP": "7", "COG_TRIO_JT": "0"}, seq="redo", sizes=(200,)),
    Row("redo-epw32", {"COG_DEBUG_REDO_STEP": "7", "COG_TRIO_EPW": "32"}, seq="redo", sizes=(200,)),
    Row("round3-duo", {"COG_TRIO": "0"}, kinds={(4, False): "duo", (3, False): "duo", (2, False): "duo", (4, True): "duo"}),
    Row("pipe", {"COG_ROLLOUT": "pipe"}, seq="rollout+2p", kinds=_all("pipe")),
    Row("wave", {"COG_ROLLOUT": "wave"}, seq="rollout+2p", kinds=_all("wave")),
    # the host paths: one shard, two shards and the views first touched after device work, in one child
    Row("host-default", {}, seq="host", sizes=(200,)),
    Row("host-no-zerocopy", {"COG_NO_ZEROCOPY": "1"}, seq="host", sizes=(200,)),
    Row("host-no-hbm-masks", {"COG_NO_HBM_MASKS": "1"}, seq="host", sizes=(200,)),
    Row("host-no-spec", {"COG_NO_SPEC": "1"}, seq="host", sizes=(200,)),
    # one player and max_steps 0..2 under the forms (one player selects like two: never the trio)
    Row("corners-default", {}, seq="corners"),
    Row("corners-no-lat", {"COG_TRIO_JT": "0"}, seq="corners"),
    Row("corners-epw32", {"COG_TRIO_EPW": "32"}, seq="corners"),
    Row("corners-wpc1", {"COG_TRIO_WPC": "1"}, seq="corners"),
    Row("corners-duo", {"COG_TRIO": "0"}, seq="corners",
        kinds={(4, False): "duo", (3, False): "duo", (2, False): "duo", (4, True): "duo", (1, False): "duo", (1, True): "duo"}),
    Row("corners-pipe", {"COG_ROLLOUT": "pipe"}, seq="corners", kinds=_all("pipe")),
    Row("corners-wave", {"COG_ROLLOUT": "wave"}, seq="corners", kinds=_all("wave")),
    Row("corners-host-no-zerocopy", {"COG_NO_ZEROCOPY": "1"}, seq="corners-host", sizes=(200,)),
    Row("corners-host-no-spec", {"COG_NO_SPEC": "1"}, seq="corners-host", sizes=(200,)),
    # the draws that reject (the non-LAT trio's sample_lean takes uid_tab_accepted, not the index table)
    Row("planted-no-lat", {"COG_TRIO_JT": "0"}, seq="planted", sizes=(PLANTED_N,)),
    Row("planted-lat", {"COG_TRIO_JT": "1"}, seq="planted", sizes=(PLANTED_N,)),
    Row("planted-epw32", {"COG_TRIO_EPW": "32"}, seq="planted", sizes=(PLANTED_N,)),
    Row("planted-duo", {"COG_TRIO": "0"}, seq="planted", sizes=(PLANTED_N,),
        kinds={(4, False): "duo", (3, False): "duo", (2, False): "duo", (4, True): "duo"}),
    Row("planted-pipe", {"COG_ROLLOUT": "pipe"}, seq="planted", sizes=(PLANTED_N,), kinds=_all("pipe")),
    Row("planted-wave", {"COG_ROLLOUT": "wave"}, seq="planted", sizes=(PLANTED_N,), kinds=_all("wave")),
    Row("planted-host-no-spec", {"COG_NO_SPEC": "1"}, seq="planted-host", sizes=(PLANTED_N,)),
    # host actions the mask forbids (tests/offmask_cases.py): a hand-over into the trio and the stored-mask
    # kernel under the trio's forms, and through the host drivers under the staged publish and masks over PCIe
    # (these children load torch: the M op writes the sampler's device actions through it)
    Row("offmask-default", {}, seq="offmask", sizes=(oc.FORM_N,)),
    Row("offmask-epw32", {"COG_TRIO_EPW": "32"}, seq="offmask", sizes=(oc.FORM_N,)),
    Row("offmask-wpc1", {"COG_TRIO_WPC": "1"}, seq="offmask", sizes=(oc.FORM_N,)),
    Row("offmask-wpc2", {"COG_TRIO_WPC": "2"}, seq="offmask", sizes=(oc.FORM_N,)),
    Row("offmask-no-lat", {"COG_TRIO_JT": "0"}, seq="offmask", sizes=(oc.FORM_N,)),
    Row("offmask-host-no-zerocopy", {"COG_NO_ZEROCOPY": "1"}, seq="offmask-host", sizes=(oc.FORM_N,)),
    Row("offmask-host-no-hbm-masks", {"COG_NO_HBM_MASKS": "1"}, seq="offmask-host", sizes=(oc.FORM_N,)),
)}
CASES = [(r.name, n) for r in ROWS.values() for n in r.sizes]
SWITCHES = sorted({k for r in ROWS.values() for k in r.env} | {"COG_SPIN_US", "COG_RUNNER_CHUNK", "COG_DEBUG_PARK_NOFIX"})


def sequence_of(row):
    if row.seq == "rollout":
        return list(ROLLOUT_SEQ)
    if row.seq == "rollout+2p":
        return ROLLOUT_SEQ + TWO_PLAYER_TAIL
    if row.seq == "redo":
        return list(REDO_SEQ)
    if row.seq == "big":
        return list(dc.BIG_CASES["T20_S50_T20"])
    if row.seq == "corners":
        return list(CORNERS_SEQ)
    if row.seq == "corners-host":
        return list(CORNERS_HOST_SEQS["one player"])
    if row.seq == "offmask":
        return list(oc.FORM_HANDOVER)
    if row.seq == "offmask-host":
        return list(oc.FORM_HOST_HANDOVER)
    return list(HOST_SEQ)


def check_form(row, n, form, kinds):
    """What the row must show, from rollout_kind's answers (kinds: "players,stored" -> name) and
    trio_form(n).  Raises AssertionError naming the figure."""
    env = row.env
    for (players, stored), want in row.kinds.items():
        got = kinds[f"{players},{int(stored)}"]
        assert got == want, f"{row.name}: rollout_kind(n={n}, players={players}, stored={stored}) is {got!r}, not {want!r}"
    epw = int(env.get("COG_TRIO_EPW", 64))
    assert form["epw"] == epw, f"{row.name}: epw {form['epw']}, not {epw}"
    assert form["workgroups"] == -(-n // epw), f"{row.name}: {form['workgroups']} workgroups for {n} envs at {epw}"
    assert form["cus"] >= 1 and form["fixup_grid"] == max(1, min(form["workgroups"], form["cus"])), form
    if "COG_TRIO_JT" in env:
        assert form["lat"] == int(env["COG_TRIO_JT"]), f"{row.name}: lat {form['lat']}"
    else:
        assert form["lat"] == int(form["workgroups"] <= form["cus"]), form
    if row.name.endswith("no-lat"):                        # the form a device of fewer CUs takes here
        assert form["lat"] == 0 and form["workgroups"] <= form["cus"], form
    if row.name == "lat-shared-cu":
        assert form["lat"] == 1 and form["workgroups"] > form["cus"], form
    if "COG_TRIO_WPC" in env:
        k = int(env["COG_TRIO_WPC"])
        # pad_lds = LDS per CU / k - 2048 - sizeof(TrioLds).  k = 1, 2: the struct's size it implies is
        # a multiple of 4 within the struct's static bounds, and k padded workgroups fit a CU where
        # k + 1 do not.  k = 3, 4: a third of a CU's LDS (54,613 bytes) or less leaves no room beside
        # TrioLds and the 2,048-byte margin, so no pad (three per CU is what the struct alone gives)
        assert form["wpc"] == k, f"{row.name}: wpc {form['wpc']}, not {k}"
        if k >= 3:
            assert form["pad_lds"] == 0, f"{row.name}: pad_lds {form['pad_lds']}"
        else:
            lds = LDS_PER_CU // k - 2048 - form["pad_lds"]
            assert form["pad_lds"] > 0 and TRIO_LDS_MIN < lds <= TRIO_LDS_MAX and lds % 4 == 0, \
                f"{row.name}: pad_lds {form['pad_lds']}"
            assert k * (lds + form["pad_lds"]) <= LDS_PER_CU < (k + 1) * (lds + form["pad_lds"]), form
    else:
        wpc = 2 if form["workgroups"] > form["cus"] else 0
        assert form["wpc"] == wpc and (form["pad_lds"] > 0) == (wpc > 0), form


def child_main(argv):
    """argv: row name, n, for the planted rows the file of their cases (the parent's search, as JSON).
    Run in a child process whose environment carries the row's switches."""
    import city_of_gold as cg
    import pyoracle as po
    row, n = ROWS[argv[0]], int(argv[1])
    C = cg._city_of_gold
    shard_n = n
    form = C.trio_form(shard_n)
    kinds = {f"{p},{int(s)}": C.rollout_kind(shard_n, p, s) for p in (4, 3, 2, 1) for s in (False, True)}
    check_form(row, n, form, kinds)
    out = dict(row=row.name, n=n, form=form, kinds=kinds)
    seq = sequence_of(row)
    if row.seq in ("planted", "planted-host"):
        import planted_cases as pc
        with open(argv[2]) as f:
            cases = [pc.Case(*[tuple(x) if isinstance(x, list) else x for x in c]) for c in json.load(f)]
        assert n == pc.N and len(cases) >= 16
        h = dc.Harness(cg, n, pc.PLAIN_SAMPLER_SEED)
        for driver in (PLANTED_DRIVERS if row.seq == "planted" else PLANTED_HOST_DRIVERS):
            for case in cases:
                pc.walk(h, case, driver, f"{row.name}, {driver}", device_actions=False)
                if "COG_NO_SPEC" in row.env:
                    assert h.smp.spec_stats()[1] == 0, f"{driver}: a speculative sample taken under COG_NO_SPEC"
        out["ends"], out["cases"] = h.ends, len(cases)
    elif row.seq in ("host", "corners-host"):
        spec_off = "COG_NO_SPEC" in row.env
        walks = (("one shard", {}, n, seq), ("two shards", {"device": [0, 0]}, HOST_TWO_SHARD_N, seq),
                 ("lazy views", {"lazy_views": True}, dc.PAIR_N, dc.LAZY_VIEWS_CASE))
        if row.seq == "corners-host":
            walks = (("one player", {}, n, seq), ("max_steps 0", {}, CORNERS_HOST_MS0_N, CORNERS_HOST_SEQS["max_steps 0"]))
            out["ends"] = 0
        for what, kw, hn, s in walks:
            h = dc.Harness(cg, hn, dc.PAIR_SEED, **kw)
            assert h.env.num_shards == (2 if what == "two shards" else 1)
            for k, op in enumerate(s):
                try:
                    h.apply(op)
                except AssertionError as e:
                    raise AssertionError(f"{what}: {e}\n  after the sequence {s[:k + 1]!r}") from None
                hits = h.smp.spec_stats()[1]
                if spec_off:
                    assert hits == 0, f"{what}: {hits} speculative samples taken under COG_NO_SPEC after {op!r}"
                elif what == "one shard" and k == 1 and not row.env:     # (single-shard samplers speculate)
                    assert hits > 0, f"{what}: no speculative sample taken in {op!r}"
            h.compare_hazards(what + ", at the end")
            if s is not dc.LAZY_VIEWS_CASE:
                assert all(e >= 1 for e in h.op_ends[1:]), f"{what}: an op without an episode end: {h.op_ends}"
            if what == "max_steps 0":
                assert h.op_ends[1:] == [hn * k for _, k in s[1:]], f"{what}: not every env ends at every step: {h.op_ends}"
            if row.seq == "corners-host":
                out["ends"] += h.ends
            out[what.replace(" ", "_") + "_spec_hits"] = int(h.smp.spec_stats()[1])
    else:
        threads = po.host_threads() if n > 4096 else 0
        # (the offmask rows: the sampler seed of tests/test_offmask_cpu.py's census of the same walk)
        h = dc.run(dc.Harness(cg, n, oc.SEED if row.seq.startswith("offmask") else dc.PAIR_SEED, threads=threads), seq)
        h.compare_hazards("at the end")
        if row.seq == "rollout+2p":
            assert h.orc.flags().any(), "the 2-player tail raised no flag on the oracle: the case lost its point"
        out["ends"] = h.ends
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(child_main(sys.argv[1:]))
