"""GPU: every launch form a switch or the CU count selects (tests/launch_form_cases.py has the rows,
their sequences and the child; tests/test_driver_sequences_cpu.py counts on the oracle alone what
the sequences rely on).  The launcher picks a rollout kernel and its form from the batch size, the
device's CU count and environment switches read once into statics; the rest of the suite runs only
what one whole MI355X (256 CUs) gives at the sizes it uses.  Here every row is a child process whose
environment carries the switches.  The child asserts rollout_kind and trio_form first, walks a
driver_cases.Harness through the row's sequence (all six views against the oracle after every op,
then the hazard flags per env), and prints the form as JSON on its last line, which the parent
checks again.

  default          no switch: the form this machine picks (printed), n = 200 and 33
  no-lat           COG_TRIO_JT=0: k_env_rollout_trio<.., LAT = false> with workgroups <= cus, what a
                   partitioned device takes at these sizes
  lat-shared-cu    COG_TRIO_JT=1 at 16,385 envs: the LAT form with 257 workgroups (T20 S50 T20, the
                   oracle on host threads)
  epw32 (-no-lat)  COG_TRIO_EPW=32: lanes 32.. idle, 200 = 6 x 32 + 8, 33 = 32 + 1
  wpc1..4          COG_TRIO_WPC: the dynamic LDS pad; 108,768 bytes at 1 (161,792 with TrioLds),
                   26,848 at 2, none at 3 and 4 (a third of a CU's LDS leaves no room for one)
  redo-*           COG_DEBUG_REDO_STEP=7: every env parked at step 7 of each launch, the fix-up's
                   redo path, with LAT off and with 32 envs per workgroup
  round3-duo       COG_TRIO=0: k_env_rollout_duo<MASK_SELECTED> with 4 and 3 players
  pipe, wave       COG_ROLLOUT: k_env_rollout_pipe / k_env_rollout for selected and stored masks with
                   4, 3 and 2 players on ragged small batches; the 2-player tail raises ERASE_PAST,
                   Q9_OOB, OOB_LOOKUP and B_START_LT4 on the oracle, compared per env
  host-*           X H Hc Hs R1 Rr(5) Th20 L Ls H T20 H on one shard (200) and on two (301), and the
                   views first touched after device work, under COG_NO_ZEROCOPY (the staged publish),
                   COG_NO_HBM_MASKS (masks sampled over PCIe) and COG_NO_SPEC (spec_stats()[1] == 0;
                   > 0 after the first H without a switch)
  corners-*        the reset-parameter corners (tests/corner_cases.py) under the forms: 4 players at max_steps 0
                   (every env ends at every step; such a batch keeps off the trio), 3 players at
                   max_steps 1 (the trio: an end at every turn end), one player at max_steps 8 and 2,
                   each as T20 S20 T20, with no switch, COG_TRIO_JT=0, COG_TRIO_EPW=32, COG_TRIO_WPC=1,
                   COG_TRIO=0 and COG_ROLLOUT=pipe / wave (one player selects like two: rollout_kind is
                   asserted for 1 player too); the host walk after a reset with one player and (70
                   envs, 8 steps per op) at max_steps 0 under COG_NO_ZEROCOPY and COG_NO_SPEC
  planted-*        the draws that reject (tests/planted_cases.py: a case per census cell, a sampler rejection
                   at every launch position, the case with two events; 70 envs, the planted one at index
                   37) under T20 and S20 with COG_TRIO_JT=0 (sample_lean's uid_tab_accepted branch) and 1,
                   COG_TRIO_EPW=32 (lane 5 of the second workgroup), COG_TRIO=0, COG_ROLLOUT=pipe / wave,
                   and under H Hc Hs R1 L Ls with COG_NO_SPEC; the parent searches the cases once and
                   hands them to the child as a file
  offmask-*        host actions the mask forbids (tests/offmask_cases.py: moves in closed directions, then `all`:
                   every head uniform in 0..top, on half the envs through env.step, step_device and
                   runner.step()) handed over to T20 T20 S20 with no switch, COG_TRIO_EPW=32, COG_TRIO_WPC=1
                   and 2 and COG_TRIO_JT=0, and to H R1 Th20 L Hs Ls under COG_NO_ZEROCOPY and
                   COG_NO_HBM_MASKS; 200 envs (these children load torch)
  encode           env.time_encode(1, variant) for the production kernel (0), k_encode_lds<false> (1)
                   and k_encode_direct (2): observations equal their copy and the oracle; then the
                   map bytes of the device records are overwritten with 0xEE and the kernel must put
                   back every one of the 144 blocks of every env (no batch of the oracle's fills them
                   all with non-zero cells -- maps are anchored at the grid's origin, a 10-piece HARD
                   batch reaches 115 of 144 -- so the overwrite is what makes an unwritten block
                   show); 1-piece EASY at n = 200 and 1, 3 pieces HARD, 10 pieces HARD on maps up to
                   46 cells; again after 60 steps of 20-step launches with auto-resets (maps
                   regenerated inside a launch); on two shards only shard 0 is rewritten

After a child has ended by a signal, by exit status 134 or 139, at its timeout, or has reported a
HIP memory fault, every remaining case of the module skips with that reason.

Durations on the MI355X (pytest --durations=0, the child's start, import and oracle walk included;
no child but the offmask-* rows' loads torch): a rollout row 0.86-1.21 s at n = 200 and 0.43-0.61 s at 33 (pipe and wave, with
their 2-player tail, the longest); redo 0.61-0.72 s; a host row (three harnesses in one child)
1.70-1.85 s; lat-shared-cu at 16,385 envs 1.73-1.79 s, within the 1.2-3.2 s of the big cases of
test_gpu_driver_sequences.py; an encode case 0.01-0.25 s (the first one brings torch's GPU side up).
45 cases, 29 s together.
The 7 offmask-* rows: 2.1-2.4 s each (torch's import included), 18 s together.
The 16 corners-* rows: 3.4-3.6 s at n = 200 (8,000 oracle resets at max_steps 0), 0.9-1.3 s at 33, the two host
rows 2.3-2.5 s; 37 s together.

That the cases bite, tried on three scratch builds of the engine (never committed), the whole GPU suite
run against each; every edit keeps its addresses in range and gives wrong bytes:
  build 1, 15 of this module's cases fail, the other 813 tests of the suite pass:
    `l < epw &&` dropped from trio_drawer's `live` (what stays is `wbase + l < n`, so the lanes
    32.. of a 32-env workgroup work on envs of the batch that the next workgroup owns): epw32 at
    200 and 33 and redo-epw32 fail at their first T20 (observations.shared.map, player_data.obs.draw);
    invisible at 64 envs per workgroup
    `if (k != 143)` before k_encode_direct's encode_block (a block skipped, nothing stored): all six
    variant-2 cases fail, "leaves env 0 block 143 (map byte 16016) 0xee"; without the overwrite the
    block's old bytes would have been the right ones
    getenv("COG_TRIO_JT") misspelt: no-lat (200, 33), epw32-no-lat (200, 33), redo-no-lat and
    lat-shared-cu fail in the child's form check, before any launch ("no-lat: lat 1")
  build 2, 4 cases fail, the other 824 pass:
    the lane driver's next player `na` taken two seats on for the selected masks with >= 3 players,
    outside the fix-up (an index below n_players: another player's records, no address out of range):
    pipe and wave at 200 and 33 fail at their first T20; the suite's other selected-mask runs of these
    kernels have 2 players
  build 3, 2 cases fail, the other 826 pass:
    duo_stepper's `na1` (the player after the new agent) taken two seats on for the selected masks
    with >= 3 players (again an index below n_players): round3-duo at 200 and 33 fail at their first T20
Not shown by an edit: one that only the LAT = false form at small n sees (an edit in a `LAT` branch
is seen by the suite's launches of 24,576 envs and more); those rows were shown through the switch.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import bigmap_cases as bc
import driver_cases as dc
import launch_form_cases as lf
import pyoracle as po

pytestmark = pytest.mark.gpu

CHILD = r"""
import sys
sys.path[:0] = sys.argv[1:4]
import launch_form_cases as lf
sys.exit(lf.child_main(sys.argv[4:]))
"""
FAULT_TEXT = re.compile(r"illegal memory access|Memory access fault|HSA_STATUS_ERROR|hipErrorIllegalAddress|"
                        r"Segmentation fault|core dumped", re.I)
CRASHED = []                                               # the reason, once a child has crashed


@pytest.fixture(autouse=True)
def stop_after_a_crash():
    if CRASHED:
        pytest.skip("an earlier case of this module crashed: " + CRASHED[0])


def run_child(cg, tmp_path, row, n, timeout, extra=()):
    tests = os.path.dirname(os.path.abspath(__file__))
    pkg = os.path.dirname(os.path.dirname(cg.__file__))
    oracle_dir = os.path.dirname(os.path.abspath(po.__file__))
    script = tmp_path / "launch_form.py"
    script.write_text(CHILD)
    env = {k: v for k, v in os.environ.items() if k not in lf.SWITCHES and k not in ("COG_ROLLOUT", "COG_TRIO")}
    env.update(row.env)
    if not row.seq.startswith("offmask"):                  # (no other sequence has a G, D or M op)
        env["COG_NO_TORCH"] = "1"
    what = f"{row.name} at n = {n}"
    try:
        r = subprocess.run([sys.executable, str(script), tests, pkg, oracle_dir, row.name, str(n), *extra], capture_output=True,
                           text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        CRASHED.append(f"{what} ran into its timeout of {timeout} s")
        raise AssertionError(CRASHED[0]) from None
    if r.returncode < 0 or r.returncode in (134, 139) or FAULT_TEXT.search(r.stderr) or FAULT_TEXT.search(r.stdout):
        CRASHED.append(f"{what} ended with status {r.returncode}")
        raise AssertionError(CRASHED[0] + "\n" + r.stderr[-3000:])
    assert r.returncode == 0, f"{what}:\n{r.stderr[-3000:]}"
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["row"] == row.name and out["n"] == n
    lf.check_form(row, n, out["form"], out["kinds"])
    print(f"{what}: {out}")
    return out


@pytest.mark.parametrize("name,n", lf.CASES, ids=[f"{r}-n{n}" for r, n in lf.CASES])
def test_launch_form(cg, tmp_path, name, n):
    row = lf.ROWS[name]
    extra = ()
    if row.seq.startswith("planted"):
        import planted_cases as pc
        (tmp_path / "planted.json").write_text(json.dumps(pc.reduced_cases()))
        extra = (str(tmp_path / "planted.json"),)
    out = run_child(cg, tmp_path, row, n, 240 if n > 4096 else 150, extra)
    if row.seq.startswith("planted"):
        assert out["cases"] == len(pc.reduced_cases())
    assert out["form"]["cus"] == cg._city_of_gold.trio_form(n)["cus"]
    if row.seq == "host":
        if "COG_NO_SPEC" in row.env:
            assert out["one_shard_spec_hits"] == out["two_shards_spec_hits"] == out["lazy_views_spec_hits"] == 0
        elif not row.env:                                   # (the self-publishing step alone speculates: not the
            assert out["one_shard_spec_hits"] > 0            # staged publish of COG_NO_ZEROCOPY)
    elif n <= 4096:                                        # (the threaded oracle of the large batch counts no ends)
        assert out["ends"] >= 1


# ---- the encode variants (in-process: no switch) --------------------------------------------------
MAP_BYTES = 48 * 48 * 7                                    # shared.map: the first 16,128 bytes of ObsData
SCRIBBLE = 0xEE
BIG = bc.Reset(10, bc.HARD, seed=1155)
ENCODE_CASES = {"1pc-easy-n200": (200, 77, 1, 0), "1pc-easy-n1": (1, 77, 1, 0), "3pc-hard-n200": (200, 77, 3, 2),
                "10pc-hard-n130": (BIG.n, BIG.seed, BIG.pieces, BIG.difficulty)}
_ORACLES = {}


def reset_oracle(case):
    if case not in _ORACLES:                               # (shared, read-only)
        n, seed, pieces, difficulty = ENCODE_CASES[case]
        if case == "10pc-hard-n130":
            _ORACLES[case] = bc.reset_reference(BIG)[0]
        else:
            _ORACLES[case] = po.OracleVec(n)
            _ORACLES[case].reset(seed, 4, pieces, difficulty, 100000)
    return _ORACLES[case]


def check_encode(cg, env, want, variant, what, shards=1):
    """env's observations equal `want` (the oracle's) now; they still do after time_encode, and after
    time_encode over device records whose map bytes were overwritten (shard 0: put back whole;
    another shard: left as overwritten, its other fields alone)."""
    import torch
    n = want.shape[0]
    env.sync_host()
    before = env.observations.copy()
    assert po.named_equal(before, want) is None, f"{what}: observations.{po.named_equal(before, want)} before the encode"
    env.time_encode(1, variant)
    env.sync_host()
    for ref, nm in ((before, "their copy"), (want, "the oracle")):
        bad = po.named_equal(env.observations, ref)
        assert bad is None, f"{what}: observations.{bad} differs from {nm} after time_encode(1, {variant})"
    want_map = np.ascontiguousarray(want["shared"]["map"]).view(np.uint8).reshape(n, MAP_BYTES)
    tens = [cg.device_tensors(env, shard=k)["observations"] for k in range(shards)]
    for t in tens:
        t[:, :MAP_BYTES] = SCRIBBLE
    torch.cuda.synchronize()
    env.sync_host()
    seen = np.ascontiguousarray(env.observations["shared"]["map"]).view(np.uint8)
    assert (seen == SCRIBBLE).all(), f"{what}: the host views do not show the overwritten device records"
    env.time_encode(1, variant)
    env.sync_host()
    n0 = env.shard_info(0)[1]
    got = tens[0][:, :MAP_BYTES].cpu().numpy()
    if not np.array_equal(got, want_map[:n0]):
        i, b = (int(x[0]) for x in np.nonzero(got != want_map[:n0]))
        raise AssertionError(f"{what}: variant {variant} leaves env {i} block {b // 112} (map byte {b}) "
                             f"{int(got[i, b]):#x}, the oracle has {int(want_map[i, b]):#x}")
    bad = po.named_equal(env.observations[:n0], want[:n0])
    assert bad is None, f"{what}: observations.{bad} differs from the oracle after time_encode over overwritten records"
    if shards > 1:
        rest = env.observations[n0:].copy()
        m = np.ascontiguousarray(rest["shared"]["map"]).view(np.uint8)
        assert (m == SCRIBBLE).all(), f"{what}: time_encode wrote records of shard 1"
        rest["shared"]["map"] = want["shared"]["map"][n0:]
        bad = po.named_equal(rest, want[n0:])
        assert bad is None, f"{what}: shard 1's observations.{bad} changed"


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("case", list(ENCODE_CASES))
def test_encode_variant_after_reset(cg, case, variant):
    n, seed, pieces, difficulty = ENCODE_CASES[case]
    orc = reset_oracle(case)
    env = cg.vec.get_vec_env(n)()
    env.reset(seed, 4, pieces, cg.Difficulty(difficulty), 100000, False)
    check_encode(cg, env, orc.observations, variant, case)


def test_encode_variants_after_autoresets_inside_launches(cg):
    """60 steps in 20-step trio launches at max_steps 8: envs regenerated by the wave's own encode
    inside a launch are encoded again by the streaming kernels, every variant."""
    h = dc.run(dc.Harness(cg, 200, dc.PAIR_SEED), [dc.X4, ("T20", 60)])
    assert h.op_ends[1] >= 200, h.op_ends
    for variant in (0, 1, 2):
        check_encode(cg, h.env, h.orc.observations, variant, f"after 60 steps, variant {variant}")


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_encode_variant_on_two_shards_writes_shard_0_alone(cg, variant):
    h = dc.run(dc.Harness(cg, 301, dc.PAIR_SEED, device=[0, 0]), [dc.X4, ("T20", 60)])
    assert h.env.num_shards == 2 and 0 < h.env.shard_info(0)[1] < 301
    check_encode(cg, h.env, h.orc.observations, variant, f"two shards, variant {variant}", shards=2)
