"""The C oracle under AddressSanitizer + UndefinedBehaviorSanitizer (CPU only).

The reference's Debug build compiles its core with -fsanitize=address,undefined
(reference CMakeLists.txt:97-105).  Our host-side restatement of that core (oracle/cog_oracle.c)
deliberately reproduces u8 wrap-around and flat-DeckObs scans; this test runs it
over the golden trace scenarios (oracle/gen_golden.py traces(): stored-mask driver with
auto-resets, B-start seeds, 2/3/4 players, selected-mask loop) built with both sanitizers and
-fno-sanitize-recover, and checks that nothing is reported and that every output record hashes
the same as in the plain build (oracle/asan_harness.c, `make -C oracle asan`).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
ASAN_ENV = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
                UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def harness():
    r = subprocess.run(["make", "-s", "-C", ORACLE, "_asan/harness"], capture_output=True, text=True)
    assert r.returncode == 0, "the plain harness does not build:\n" + r.stderr[-2000:]
    r = subprocess.run(["make", "-s", "-C", ORACLE, "asan"], capture_output=True, text=True)
    if r.returncode != 0:                                  # (the same sources just built: the sanitizers are what is missing)
        pytest.skip("no sanitizer toolchain: " + r.stderr[-400:])
    return os.path.join(ORACLE, "_asan", "harness"), os.path.join(ORACLE, "_asan", "harness_asan")


def test_sanitizer_is_live(harness):
    _, asan = harness
    r = subprocess.run([asan, "--selftest"], capture_output=True, text=True, env=ASAN_ENV, timeout=60)
    assert r.returncode != 0
    assert "runtime error" in r.stderr or "AddressSanitizer" in r.stderr


def test_oracle_clean_under_asan_ubsan(harness):
    plain, asan = harness
    p = subprocess.run([plain], capture_output=True, text=True, timeout=300)
    a = subprocess.run([asan], capture_output=True, text=True, env=ASAN_ENV, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert a.returncode == 0, a.stderr[-2000:]
    assert "runtime error" not in a.stderr and "AddressSanitizer" not in a.stderr, a.stderr[-2000:]
    lines = a.stdout.split("\n")
    assert len([ln for ln in lines if ln.strip()]) == 7
    assert a.stdout == p.stdout                            # same outputs, every step, every record
    resets = {ln.split()[0]: int(ln.split()[2]) for ln in lines if ln.strip()}
    assert resets["stored_hard_ms30"] > 0 and resets["stored_medium_ms40_bstart"] > 0   # auto-resets ran


KINDS = ("single", "replace", "all", "play", "special", "remove", "move", "shop", "sweep")   # tests/driver_cases.py OFFMASK_KINDS


def test_offmask_scenarios_clean_under_asan_ubsan(harness):
    """--offmask: host actions inside their heads that no mask allows (tests/offmask_cases.py): every kind,
    16 envs, 1 to 4 players, max_steps 12 and 100000, 300 steps, the altered bytes from the harness's own
    generator: nothing reported, the plain build's hashes."""
    plain, asan = harness
    p = subprocess.run([plain, "--offmask"], capture_output=True, text=True, timeout=120)
    a = subprocess.run([asan, "--offmask"], capture_output=True, text=True, env=ASAN_ENV, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert a.returncode == 0, a.stderr[-2000:]
    assert "runtime error" not in a.stderr and "AddressSanitizer" not in a.stderr, a.stderr[-2000:]
    assert a.stdout == p.stdout
    rows = {ln.split()[0]: ln.split() for ln in p.stdout.splitlines() if ln.strip()}
    assert len(rows) == 18
    for kind in KINDS:
        mine = [nm for nm in rows if nm.startswith(f"offmask_{kind}_")]
        assert len(mine) == 2 and {nm.rsplit("_", 1)[1] for nm in mine} == {"ms12", "ms100000"}, kind
    assert {(nm.split("_")[2], nm.split("_")[3]) for nm in rows} >= {(f"{q}p", ms) for q in (1, 2, 3, 4) for ms in ("ms12", "ms100000")}
    assert sum(int(r[2]) for nm, r in rows.items() if nm.endswith("ms12")) > 100     # episode ends with their resets
