"""CPU side of the off-mask tests (tests/offmask_cases.py, tests/test_gpu_offmask.py): host actions
inside their heads that the mask does not allow.

  the census, on the oracle alone, of every case the GPU file runs: what it must reach to keep its
  point.  These are conditions, not equalities; DESIGN.md section 5 has the measured counts.
    every kind       >= 100 executed actions on a zero mask byte for each head the kind targets
    play / special / remove / single / sweep     >= half the envs end with a pile byte >= 128
    shop / single              a shop byte of 255 (a purchase from an empty slot)
    remove / single / sweep    n_removes 0 -> 255 (a remove with none pending)
    move             Q24_CLAMP on >= 10 envs, OOB_LOOKUP on >= half, a position outside the map's
                     bounding box, a move onto another player's hex, a move onto an end hex
    max_steps 12     >= 50 episode ends (the auto-reset out of wrapped states)
    auto-reset off   every env has ended before the 15 dead steps
    hand-overs       at entry to every step driver >= 20 envs whose player is not lean_player and >= 20
                     wide envs; over the two entries pending removes, moves in progress (>= 20 each)
                     and free cards or moves (>= 1)
  the oracle against the reference: tests/golden/ref_offmask.json + ref_offmask_digests.npz (27
  single-env streams of kinds single, replace, all with 4, 3, 2 players from the unmodified reference,
  oracle/gen_golden.py --offmask), and live against oracle/_ref/libref.so where it exists
  (the stand-alone oracle harness over its --offmask scenarios under AddressSanitizer +
  UndefinedBehaviorSanitizer: tests/test_oracle_asan.py)
  the M op's action generator itself
"""
import json
import os

import numpy as np
import pytest

import driver_cases as dc
import offmask_cases as oc
import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


# ---- the generator -------------------------------------------------------------------------------
def test_offmask_actions_stay_inside_their_heads():
    rng = np.random.default_rng(5)
    n = 4000
    legal = np.zeros(n, dtype=po.ACTION)
    legal["play"], legal["move"] = 3, 2
    top = np.array(dc.CLAMP)
    for kind in dc.OFFMASK_KINDS:
        acts, hit = dc.offmask_actions(rng, legal, kind, 0.5, t=7)
        v = np.stack([acts[nm] for nm in dc.HEAD_NAMES], 1).astype(int)
        assert (v <= top).all() and (v >= 0).all(), kind
        assert po.named_equal(acts[~hit], legal[~hit]) is None, kind
        assert np.array_equal(np.ascontiguousarray(acts).view(np.uint8).reshape(n, 64)[:, 5:], np.zeros((n, 59), np.uint8))
        if kind == "sweep":
            assert hit.all()
            continue
        assert 0.45 < hit.mean() < 0.55, kind
        nz = (v[hit] != 0).sum(1)
        if kind == "all":
            for k in range(5):                               # every value of every head, 0 included
                assert set(np.unique(v[hit][:, k])) == set(range(top[k] + 1)), (kind, k)
        elif kind == "replace":
            assert ((v[hit] != [3, 0, 0, 2, 0]).sum(1) <= 1).all() and (v[hit][:, 0] != 0).all()
        else:
            assert (nz == 1).all(), kind
            heads = set(np.nonzero((v[hit] != 0).any(0))[0])
            assert heads == ({dc._ONE_HEAD[kind]} if kind in dc._ONE_HEAD else {0, 1, 2, 3, 4}), kind
            for k in heads:                                  # every value 1..top of the head
                assert set(np.unique(v[hit][:, k])) - {0} == set(range(1, top[k] + 1)), (kind, k)


def test_sweep_meets_every_pair():
    """261 envs: every (head, value >= 1) pair three times at every step; every env meets every pair in
    87 steps; the executed head is the slot's head (the other heads are 0)."""
    assert len(dc.SWEEP_SLOTS) == 87 == sum(dc.CLAMP) and oc.N_SWEEP == 3 * 87
    legal = np.zeros(oc.N_SWEEP, dtype=po.ACTION)
    seen = np.zeros((oc.N_SWEEP, 87), dtype=int)
    for t in range(87):
        acts, _ = dc.offmask_actions(np.random.default_rng(0), legal, "sweep", 1.0, t)
        head = dc.executed_head(acts)
        slot = np.array([dc.SWEEP_SLOTS.index((int(k), int(acts[dc.HEAD_NAMES[k]][i]))) for i, k in enumerate(head)])
        assert (np.bincount(slot, minlength=87) == 3).all(), t
        seen[np.arange(oc.N_SWEEP), slot] += 1
    assert (seen == 1).all()


def test_executed_head_is_the_reference_chain():
    a = np.zeros(6, dtype=po.ACTION)
    for i, heads in enumerate([(), (2,), (2, 4), (2, 4, 3), (2, 4, 3, 1), (0, 1, 2, 3, 4)]):
        for k in heads:
            a[dc.HEAD_NAMES[k]][i] = 1
    assert dc.executed_head(a).tolist() == [-1, 2, 4, 3, 1, 0]


# ---- the census ------------------------------------------------------------------------------------
def flag_envs(c, f):
    return int(((c.flags & f) != 0).sum())


@pytest.mark.parametrize("kind", oc.KINDS)
def test_kind_cases_reach_what_they_are_for(kind):
    n, seq = oc.KIND_CASES[f"{kind}-step"]
    for path in oc.PATHS[1:]:                                # (the oracle's side of the three paths is one walk)
        n2, other = oc.KIND_CASES[f"{kind}-{path}"]
        assert n2 == n and [op if isinstance(op, str) else op[:1] + op[2:] for op in other] == \
            [op if isinstance(op, str) else op[:1] + op[2:] for op in seq]
    assert 60 <= sum(1 for op in seq if op[0] == "M") <= 90 and n == (oc.N_SWEEP if kind == "sweep" else oc.N)
    h = oc.oracle_walk(n, seq)
    c = h.census
    for k in oc.TARGETS[kind]:
        assert c.zero[k] >= 100, f"{kind}: {c.zero.tolist()} executed actions on a zero mask byte"
    if kind in oc.PILE_KINDS:
        assert 2 * oc.piles_wrapped(h.orc) >= n, f"{kind}: {oc.piles_wrapped(h.orc)} envs with a pile byte >= 128"
    if kind in oc.SHOP_KINDS:
        assert c.shop255 >= 1, f"{kind}: no shop byte wrapped to 255"
    if kind in oc.REMOVE_KINDS:
        assert c.removes_wrapped >= 1, f"{kind}: no n_removes wrapped"
    if kind in oc.MOVE_KINDS:
        assert flag_envs(c, po.F_Q24_CLAMP) >= 10 and 2 * flag_envs(c, po.F_OOB_LOOKUP) >= n, \
            (flag_envs(c, po.F_Q24_CLAMP), flag_envs(c, po.F_OOB_LOOKUP))
        assert c.outside >= 1 and c.onto_player >= 1 and c.onto_end >= 1, (c.outside, c.onto_player, c.onto_end)
    assert not flag_envs(c, po.F_SCAN_OVER)                  # (unreachable: DESIGN.md section 5)


@pytest.mark.parametrize("name", list(oc.PLAYER_CASES))
def test_player_cases_reach_what_they_are_for(name):
    n, seq = oc.PLAYER_CASES[name]
    kind = name.split("-")[0]
    h = oc.oracle_walk(n, seq)
    for k in oc.TARGETS[kind]:
        assert h.census.zero[k] >= 100, f"{name}: {h.census.zero.tolist()}"
    if seq[0][5] == 12:
        assert h.ends >= 50, f"{name}: {h.ends} episode ends"
    else:
        assert 2 * oc.piles_wrapped(h.orc) >= n


def test_autoreset_off_case_ends_every_env_before_the_dead_steps():
    n, seq = oc.AUTORESET_OFF_CASE
    h = dc.Harness(None, n, oc.SEED)
    h.census = oc.Census()
    views = None
    for k, op in enumerate(seq):
        h.apply(op)
        if k + 1 == oc.AUTORESET_OFF_ALL_DONE_AT:
            assert np.asarray(h.orc.dones).all(), "an env has not ended before the dead steps"
            views = {nm: np.array(getattr(h.orc, nm), copy=True) for nm in dc.FIELDS + dc.PLAIN}
            zero = h.census.zero.copy()
        elif views is not None and op[0] == "M" and k < oc.AUTORESET_OFF_ALL_DONE_AT + 15:
            assert op[4] == "all" and op[5] == 1.0
            for nm in dc.FIELDS:                             # the reference's dead step changes nothing
                assert po.named_equal(getattr(h.orc, nm), views[nm]) is None, (k, nm)
            for nm in dc.PLAIN:
                assert np.array_equal(getattr(h.orc, nm), views[nm]), (k, nm)
    assert seq[oc.AUTORESET_OFF_ALL_DONE_AT + 15] == "C" and zero.sum() >= 100
    assert h.op_ends[-2] >= 0 and not np.asarray(h.orc.dones).all(), "the envs step again after X0, A1"


def check_entries(name, entries, n_entries):
    assert len(entries) == n_entries, (name, entries)
    for e in entries:
        assert e["nonlean"] >= 20 and e["wide"] >= 20, f"{name}: entry {e}"
    assert sum(e["removes"] for e in entries) >= 20 and sum(e["mip"] for e in entries) >= 20 and \
        sum(e["free"] for e in entries) >= 1, f"{name}: {entries}"


@pytest.mark.parametrize("name", list(oc.HANDOVER_CASES))
def test_handover_cases_enter_the_drivers_from_wrapped_states(name):
    n, seq = oc.HANDOVER_CASES[name]
    h = oc.oracle_walk(n, seq)
    check_entries(name, h.census.entries, 2)
    assert oc.piles_wrapped(h.orc) >= 20 and (h.census.zero >= 100).all(), (oc.piles_wrapped(h.orc), h.census.zero)
    if name.startswith("T"):                                 # (runner.step() before a trio launch: no compact image)
        assert h.trio_clear == 2 and [op[1] for op in seq if op[0] == "M"][29] == "runner"


def test_shard_big_and_form_handovers_on_the_oracle():
    for d, (n, seq) in oc.SHARD_CASES.items():
        assert not any(op[0] in dc.SINGLE_SHARD_ONLY for op in seq if not isinstance(op, str))
        check_entries(f"two shards, {d}", oc.oracle_walk(n, seq).census.entries, 2)
    # the launch-form rows (their child seeds its sampler with oc.SEED too: this is the walk it takes)
    h = oc.oracle_walk(oc.FORM_N, oc.FORM_HANDOVER)
    e = h.census.entries
    check_entries("form rows", e, 3)
    assert h.ends >= 1 and 20 <= e[0]["wide"] <= oc.FORM_N - 20, "the first trio launch needs narrow decks too"
    assert h.trio_clear == 2 and (h.census.zero >= 100).all()    # (both T20 ops follow runner.step(): no compact image)
    h = oc.oracle_walk(oc.FORM_N, oc.FORM_HOST_HANDOVER)
    check_entries("host form rows", h.census.entries, 6)
    assert h.ends >= 1 and (h.census.zero >= 100).all()


@pytest.mark.parametrize("kind", list(dc.BIG_SIZES))
def test_big_handover_on_the_oracle(kind):
    h = oc.oracle_walk(dc.BIG_SIZES[kind], oc.BIG_HANDOVER, threads=po.host_threads())
    for e in h.census.entries:
        assert e["nonlean"] >= 20 and e["wide"] >= 20, e
    assert (h.census.zero >= 100).all()


# ---- the oracle against the reference --------------------------------------------------------------
with open(os.path.join(GOLD, "ref_offmask.json")) as _f:
    GROUPS = json.load(_f)["groups"]
DIGESTS = np.load(os.path.join(GOLD, "ref_offmask_digests.npz"))["digests"]


def streams():
    at = 0
    for g in GROUPS:
        for i, steps, off in zip(g["index"], g["steps"], g["off_mask"]):
            yield g, i, steps, off, DIGESTS[at:at + steps + 1]
            at += steps + 1
    assert at == DIGESTS.shape[0]


def test_reference_streams_hold_their_conditions():
    all_ = list(streams())
    assert len(all_) >= 24 and {(g["kind"], g["n_players"]) for g in GROUPS} == \
        {(k, p) for k in oc.STREAM_KINDS for p in oc.STREAM_PLAYERS}
    assert min(s[2] for s in all_) >= oc.STREAM_LEAST
    assert sum(1 for s in all_ if s[2] == oc.STREAM_STEPS and s[3] >= 60) >= 16
    for name in ("ref_offmask_digests.npz", "ref_offmask.json"):
        assert os.path.getsize(os.path.join(GOLD, name)) <= min(
            os.path.getsize(os.path.join(GOLD, f)) for f in os.listdir(GOLD) if f.endswith("_digests.npz") and "offmask" not in f)
    for g in GROUPS:
        assert g["seed"] == oc.stream_seed(g["kind"], g["n_players"])
        kept = iter(g["index"])                              # the first seeds that run 20 steps or more, in order
        nxt = next(kept)
        for i in range(max(g["index"]) + 1):
            L, off = oc.stream_safe_steps((g["kind"], g["n_players"], i))
            if i == nxt:
                k = g["index"].index(i)
                assert (L, off) == (g["steps"][k], g["off_mask"][k]), (g["kind"], g["n_players"], i)
                nxt = next(kept, None)
            else:
                assert L < oc.STREAM_LEAST, (g["kind"], g["n_players"], i, L)


def test_oracle_matches_the_reference_on_offmask_streams():
    for g, i, steps, _, want in streams():
        seed = g["seed"] + i
        got = oc.stream_run(po.OracleVec(1), po.OracleSampler(1, seed), oc.Stream(g["kind"], g["n_players"], i), steps)
        bad = np.nonzero((got != want).any(1))[0]
        assert not bad.size, f"{g['kind']}, {g['n_players']} players, index {i}: the oracle leaves the reference at step {bad[0]}"
        if po.ref_available():                               # live, step by step
            live = oc.stream_run(po.RefVec1(), po.RefSampler1(seed), oc.Stream(g["kind"], g["n_players"], i), steps)
            assert np.array_equal(live, want), f"{g['kind']}, {g['n_players']} players, index {i}: the fixture is stale"
