"""GPU: the draws that reject, planted under every driver (tests/planted_cases.py has the cases and
how they are found; tests/test_planted_draws_cpu.py asserts on the oracle alone that every census
cell, launch position and the control value are among them).

Every kernel that draws has a fast path that assumes the draw is accepted and a fallback for a draw
in the top 32 values of the generator's range, taken about once in 2^26 draws: by chance essentially
never outside the largest rollouts.  Here the generator states are chosen so that a given draw lands
there.  Each case walks a driver_cases.Harness of 70 envs with the planted env at index 37, engine
against oracle: all six views after every op, the sampler's actions (the host view, or the device
buffer after a device-view rollout), then a host step that shows where the sampler's generator
stands, then the hazard flags per env.  One test id per driver and group:

  reset     X, and X0 directly after it: map generation and the initial hands, k = 1..40
  steps     the env planted at k >= 17: turn-end deck draws (draw_n's seq term), take_from_active,
            map generation at an auto-reset inside a launch and in the fix-up; 4, 3 and 2 players,
            max_steps 8 and 100,000; selected-mask cases under the selected-mask drivers, stored-mask
            cases under the stored-mask ones
  sampler   the sampler planted at head j of step t: sample_heads' riskv branch and pick, the
            speculative sample of k_env_step (H: the spare buffer swapped in), the trio's presample /
            sample_lean and the realignment three steps after a rejection (T20, Th20, T2, T1000), the
            duo / pipe / wave samplers (S20, S2, L, Ls)
  two shards, seed edges: see the tests

Durations on the MI355X (pytest --durations): see DESIGN.md section 5, "Planted draws".
"""
import pytest

import driver_cases as dc
import planted_cases as pc

pytestmark = pytest.mark.gpu

SELECTED_DRIVERS = ("H", "Hc", "D", "R1", "L", "T20", "Th20", "T2", "T1000")
STORED_DRIVERS = ("Hs", "Ls", "S20", "S2")
DRIVERS = ("H", "Hc", "Hs", "D", "R1", "L", "Ls", "T20", "Th20", "T2", "T1000", "S20", "S2")
walk = pc.walk


def test_reset_group(cg):
    h = dc.Harness(cg, pc.N, pc.PLAIN_SAMPLER_SEED)
    for case in pc.reset_cases():
        walk(h, case, None, "reset")


@pytest.mark.parametrize("driver", DRIVERS)
def test_steps_group(cg, driver):
    mode = "sto" if driver in STORED_DRIVERS else "sel"
    cases = [c for c in pc.step_cases() + pc.double_cases() if c.mode == mode]
    assert len(cases) >= 20
    h = dc.Harness(cg, pc.N, pc.PLAIN_SAMPLER_SEED)
    for case in cases:
        walk(h, case, driver, driver)


# the sampler group by census cell (330 cases in one id took 6 s): a head with one candidate, accepted
# and rejected; a head with two or more; the control value
SAMPLER_PARTS = {"one-accepted": ("sampler/one/accepted",), "one-rejected": ("sampler/one/rejected",),
                 "many": ("sampler/many/accepted", "sampler/many/rejected"), "control": ()}


@pytest.mark.parametrize("part", list(SAMPLER_PARTS))
@pytest.mark.parametrize("driver", DRIVERS)
def test_sampler_group(cg, driver, part):
    cells = SAMPLER_PARTS[part]
    cases = [c for c in pc.sampler_cases() if (set(c.cells) & set(cells) if cells else not c.cells)]
    assert len(cases) >= 25
    h = dc.Harness(cg, pc.N, pc.PLAIN_SAMPLER_SEED)
    hits = 0
    for case in cases:
        walk(h, case, driver, driver)
        hits += h.smp.spec_stats()[1]
    if driver == "H":                                      # (the speculative sample met the planted draws)
        assert hits >= len(cases), f"{hits} speculative samples taken under H"


def test_sampler_parts_hold_every_case():
    held = [c for cells in SAMPLER_PARTS.values() for c in pc.sampler_cases()
            if (set(c.cells) & set(cells) if cells else not c.cells)]
    assert sorted(held) == sorted(pc.sampler_cases())


def test_two_shards(cg):
    """device=[0, 0]: 35 + 35 envs, index 37 in the second shard; the reduced list under H, T20, S20."""
    h = dc.Harness(cg, pc.N, pc.PLAIN_SAMPLER_SEED, device=[0, 0])
    assert h.env.num_shards == 2 and h.env.shard_info(1)[0] <= pc.IDX
    for driver in ("H", "T20", "S20"):
        for case in pc.reduced_cases():
            walk(h, case, driver, f"two shards, {driver}")
    for case in pc.reset_cases()[::7]:
        walk(h, case, None, "two shards, reset")


# ---- seed edges (planted_cases.SEED_EDGES; test_planted_draws_cpu.py checks the states on the oracle) ----
@pytest.mark.parametrize("shards", [1, 2])
@pytest.mark.parametrize("edge", list(pc.SEED_EDGES))
def test_seed_edge(cg, edge, shards):
    """Seeds and sampler first_index values whose sum with the index wraps 2^32, 2^33 or a multiple of
    the generator's modulus at index 37, through H, T20 and S20."""
    seed, sseed, first = pc.SEED_EDGES[edge]
    kw = {"device": [0, 0]} if shards == 2 else {}
    for driver in ("H", "T20", "S20"):
        h = dc.Harness(cg, pc.N, sseed, first=first, **kw)
        dc.run(h, [("X", seed, 4, 3, 2, 8), (driver, 30), ("H", 1), "C"])
