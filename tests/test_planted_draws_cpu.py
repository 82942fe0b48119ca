"""CPU: what the planted-draw cases (tests/planted_cases.py) must hold to keep their point, on the
oracle alone, and the oracle held to the reference's own recording of them.

These are conditions, asserted on every run: the case lists are searched on the oracle, so an edit of
the oracle or of the search that loses a census cell fails here, not silently on the GPU.
"""
import json
import os

import numpy as np

import driver_cases as dc
import planted_cases as pc
import pyoracle as po

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_state_before_plants_the_kth_draw():
    for r in pc.R_VALUES + (pc.R_CONTROL, 0, 12345):
        for k in (1, 2, 16, 17, 121, 400):
            x = pc.state_before(r, k)
            assert 1 <= x < pc.P
            for _ in range(k):
                x = x * 16807 % pc.P
            assert x - 1 == r
    assert pc.K_SMALL_SAFE == pc.RANGE - 31 and len(pc.R_ALL_RISKY) == 32


def test_every_census_cell_is_held_by_three_cases():
    counts = pc.cell_counts(pc.all_cases())
    print(counts)
    assert set(counts) == set(pc.CELLS)
    short = {c: k for c, k in counts.items() if k < 3}
    assert not short, f"census cells held by fewer than 3 cases: {short}"


def test_the_reduced_list_holds_every_step_and_sampler_cell_and_launch_position():
    red = pc.reduced_cases()
    counts = pc.cell_counts(red)
    assert all(counts[c] >= 1 for c in pc.CELLS if not c.startswith("reset")), counts
    held = {c.pos for c in red if c.group == "sampler" and any(q.endswith("rejected") for q in c.cells)}
    for p in pc.REJECTED_POSITIONS:
        assert (held & set(p)) if isinstance(p, range) else p in held, f"no rejection at launch position {p}: {sorted(held)}"
    assert len(red) <= 40                                  # (a launch-form row walks all of them)


def test_sampler_rejections_at_every_launch_position():
    cases = pc.sampler_cases()
    held = {c.pos for c in cases if any(q.endswith("rejected") for q in c.cells)}
    for p in pc.REJECTED_POSITIONS:
        assert (held & set(p)) if isinstance(p, range) else p in held, f"no rejection at launch position {p}: {sorted(held)}"
    # every (t, j) of the grid holds its always-rejected draw at step t
    got = {(c.step, c.k - 5 * c.step - 1) for c in cases if c.r == pc.RANGE and c.cells}
    assert got == {(t, j) for t in pc.SAMPLER_T for j in range(5)}
    assert all(c.step == (c.k - 1) // 5 and c.steps == c.step + 1 + pc.TAIL for c in cases)


def test_a_map_generation_at_an_autoreset_holds_a_rejected_draw():
    hit = [c for c in pc.step_cases() if "steps-autoreset/map/rejected" in c.cells]
    # selected masks with >= 3 players: inside a trio launch, the env that parks for the fix-up
    assert any(c.mode == "sel" and c.players >= 3 and c.steps <= 4 * pc.CHUNK for c in hit), hit
    assert any(c.mode == "sel" and c.players >= 3 and c.pos not in (None, 0) for c in hit), hit
    assert any(c.mode == "sto" for c in hit), hit
    assert any(c.players == 2 for c in pc.step_cases()) and any(c.players == 3 for c in pc.step_cases())
    assert {c.max_steps for c in pc.step_cases()} == {8, 100000}


def test_one_case_has_two_planted_events():
    assert pc.draws_apart() == []                          # (else: plant both in one generator as well)
    (c,) = pc.double_cases()
    assert any(q.startswith("steps") for q in c.cells) and any(q.startswith("sampler") for q in c.cells)
    orc, osm = po.OracleVec(1), po.OracleSampler(1, c.sampler_seed + pc.IDX)
    orc.reset(c.env_seed + pc.IDX, c.players, 3, 2, c.max_steps)
    po.run(orc, osm, c.steps, stored=c.mode == "sto")
    assert int(orc.census(0).sum()) >= 1 and int(osm.census(0).sum()) >= 1


def test_the_control_value_appears_in_no_census_cell():
    controls = [c for c in pc.all_cases() if c.r == pc.R_CONTROL]
    assert {c.group for c in controls} == {"reset", "reset0", "steps", "sampler"} and len(controls) >= 40
    for c in controls:
        assert c.cells == ()
        orc, osm = po.OracleVec(1), po.OracleSampler(1, c.sampler_seed + pc.IDX)
        orc.reset(c.env_seed + pc.IDX, c.players, 3, 2, c.max_steps)
        if c.group == "reset0":
            orc.reset_default()
        po.run(orc, osm, c.steps, stored=c.mode == "sto")
        assert not orc.census(0).any() and not osm.census(0).any(), c


def test_in_the_batch_of_70_the_planted_env_alone_holds_the_events():
    """The searches run the planted env alone; in the batch the tests run it is env 37, and no other env
    or sampler counts a risky draw."""
    for c in pc.reduced_cases()[:12] + tuple(c for c in pc.reset_cases() if c.cells)[:8]:
        h = dc.Harness(None, pc.N, c.sampler_seed)
        dc.run(h, pc.ops_of(c, "S20" if c.mode == "sto" else "T20"))
        env = np.array([h.orc.census(i).sum() for i in range(pc.N)])
        smp = np.array([h.osm.census(i).sum() for i in range(pc.N)])
        got = pc._cells_of(h.orc.census(pc.IDX), h.osm.census(pc.IDX), c.mode)
        assert set(c.cells) <= set(got), (c, got)
        assert env[pc.IDX] + smp[pc.IDX] >= 1 and env.sum() + smp.sum() == env[pc.IDX] + smp[pc.IDX], c


def test_census_is_per_env_under_the_threaded_drivers():
    """orc_run_threaded over 4 threads counts what the serial loop counts, env by env."""
    c = next(c for c in pc.step_cases() if c.cells and c.mode == "sel" and c.players == 4)
    counts = []
    for threads in (0, 4):
        orc, osm = po.OracleVec(pc.N), po.OracleSampler(pc.N, c.sampler_seed)
        orc.reset(c.env_seed, c.players, 3, 2, c.max_steps)
        if threads:
            po.run_threaded(orc, osm, c.steps, threads)
        else:
            po.run(orc, osm, c.steps)
        counts.append(np.stack([orc.census(i) for i in range(pc.N)]))
        osm.census_clear()
        orc.census_clear()
        assert not orc.census(pc.IDX).any() and not osm.census(pc.IDX).any()
    assert np.array_equal(counts[0], counts[1]) and counts[0][pc.IDX].any()


def test_sampler_state_accessor():
    osm = po.OracleSampler(3, 10, first=5)
    assert [osm.state(i) for i in range(3)] == [15, 16, 17]
    assert po.OracleSampler(1, 2 ** 32 - 1, first=1).state(0) == 2          # mr_seed(2^32)


def test_seed_edges_start_where_they_should():
    for name, (seed, sseed, first) in pc.SEED_EDGES.items():
        orc, osm = po.OracleVec(pc.N), po.OracleSampler(pc.N, sseed, first)
        orc.reset(seed, 4, 3, 2, 8)
        if name.startswith("env"):
            assert (seed + pc.IDX) % 2 ** 32 % pc.P == 0
            one = po.OracleVec(1)
            one.reset(1, 4, 3, 2, 8)                           # state 1
            assert orc.debug_state(pc.IDX) == one.debug_state(0), name
        if name == "env-wraps-to-0":
            assert osm.state(pc.IDX) == 2
        if name.startswith("sampler"):
            total = sseed + first + pc.IDX
            assert osm.state(pc.IDX) == total % pc.P and total in (2 ** 32, 2 ** 33), name


def test_the_oracle_equals_the_reference_recording():
    """tests/golden/ref_planted*: the unmodified reference's per-step digests of the planted env of every
    case it can run.  Every case without a REF_UNSAFE flag must be among them, whole."""
    meta = json.load(open(os.path.join(GOLDEN, "ref_planted.json")))
    digs = np.load(os.path.join(GOLDEN, "ref_planted_digests.npz"))["digests"]
    size = os.path.getsize(os.path.join(GOLDEN, "ref_planted.json")) + os.path.getsize(os.path.join(GOLDEN, "ref_planted_digests.npz"))
    assert size < 200 * 1000
    at, rec = 0, {}
    for key, steps in zip(meta["keys"], meta["steps"]):
        rec[key] = digs[at:at + steps + 1]
        at += steps + 1
    assert at == digs.shape[0]
    sc = meta["screened"]
    assert sc["recorded_whole"] + sc["recorded_cut"] == len(rec) and sc["left_out"] + len(rec) == sc["cases"]
    whole = 0
    for c in pc.all_cases():
        got, flags = pc.oracle_digests(c)
        key = pc.case_key(c)
        if not flags & po.REF_UNSAFE:
            assert key in rec and rec[key].shape[0] == c.steps + 1, f"{c}: raises no REF_UNSAFE flag and is not recorded whole"
            whole += 1
        if key in rec:
            want = rec[key]
            bad = np.nonzero((got[:want.shape[0]] != want).any(1))[0]
            assert bad.size == 0, f"{c}: the oracle leaves the reference at step {int(bad[0]) - 1}"
    assert whole >= 400 and whole == sc["recorded_whole"]
    held = pc.cell_counts([c for c in pc.all_cases() if pc.case_key(c) in rec and rec[pc.case_key(c)].shape[0] == c.steps + 1])
    assert all(k >= 1 for k in held.values()), f"a census cell without a case the reference ran whole: {held}"
