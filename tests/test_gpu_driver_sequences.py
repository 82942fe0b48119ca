"""GPU: every hand-over between drivers on one handle (tests/driver_cases.py has the ops, their
oracle mirror and the named cases; tests/test_driver_sequences_cpu.py counts on the oracle alone
what each case relies on).  A handle carries host-side state from call to call -- whether a trio
launch goes without k_env_fixup (EnvShard::lean_clock), whether it loads the compact deck image
the last trio left (cdeck_ok), whether a host step publishes itself (host_synced, pub_done,
mir_valid), the speculative sample, the auto-reset switch, the last reset's players and max_steps
-- and every entry point sets or clears some of it by hand.  Here both sides walk the same list of
ops and all six views (and the sampler's actions view, wherever the op refreshes it) are compared
bit-exact over named fields after every op; a mismatch names the sequence up to the failing op.

  pairs         X a(30) b(30) a(30) for every ordered pair of the 18 step drivers, 200 envs (three
                trio workgroups, the last ragged), 4 players, HARD, max_steps 8: segments 2 and 3
                each hold episode ends with their auto-resets (asserted from the oracle's dones);
                the same over H, G, T20, S20, L, Rr with 3 and with 2 players (selected-mask
                rollouts are the duo there)
  big           the hand-overs T20 S50 T20, S50 H(5) S50, S50 X0 S50, S50 G(5) T20 at 16,385 envs
                (stored masks: k_env_rollout_pipe) and 32,769 (the one-wave k_env_rollout), the
                oracle on host threads
  state         reset_default, resets that change the players (4, 2, 3, 4) and max_steps (the
                no-fix-up bound), invalidate_device with nothing edited, chunk changes on one
                runner, hazard clears, a host-view runner between device-view launches, a 0-step
                op of every driver between two trio rollouts, views first touched after device work
  autoreset     set_autoreset(False) on a batch under H, L, T20, S20, R1 until every env has ended
                and stays done, reset, the switch on again; and a mixed run
  random        eight seeded sequences of 40 ops from all of the above, on one shard and on two
  bad actions   host action indices past their heads through env.step, env.step_device and
                runner.step(): clamped to (21, 21, 21, 6, 18), COG_HAZ_BAD_ACTION on exactly the
                envs that held one

Durations on the MI355X (pytest --durations=0, the oracle side included): a pair 0.10-0.33 s (396
cases, 58 s together); big pipe 1.2-1.6 s, wave 2.4-3.2 s (the oracle's resets and rollouts on host
threads; 17 s together); state 0.10-0.20 s (25 cases, 3.0 s); views first touched 0.14 s; autoreset
0.10 s each (6); random 0.3-0.6 s on one shard, 0.5-0.9 s on two (9.5 s together); bad actions
0.05 s.  89 s together.

That the cases bite, tried on scratch builds of cog_abi.cpp (never committed; a stale compact image
gives wrong counts, not an index out of range: rollout_trio.h masks the card type to 0..7 and the
draw clamps its table index and scan result):
  `cdeck_ok = false` removed from env_reset_impl: 6 fail -- state[reset_default] (`T20 X0 T20`:
  observations.shared.map differs after the second T20), state[players], random 2 and 7 on both
  shard layouts
  `cdeck_ok = false` removed from cog_env_step: 25 fail -- the 18 pairs a -> b with a in T2, T20,
  T1000, Th2, Th20, Th1000 and b in H, Hc, Hs (4 players), pair 3p-T20-H,
  state[first_reset_then_default], random 0 (both layouts) and 4, 6, 7 on two shards
(lean_clock was left alone: a wrong edit there ends in the F_PARK_NOFIX error path by design.)
"""
import numpy as np
import pytest

import driver_cases as dc
import pyoracle as po

pytestmark = pytest.mark.gpu

PAIRS = [(4, a, b) for a in dc.STEP_DRIVERS for b in dc.STEP_DRIVERS] + \
        [(p, a, b) for p in (3, 2) for a in dc.REDUCED_DRIVERS for b in dc.REDUCED_DRIVERS]


@pytest.mark.parametrize("players,a,b", PAIRS, ids=[f"{p}p-{a}-{b}" for p, a, b in PAIRS])
def test_pair(cg, players, a, b):
    h = dc.run(dc.Harness(cg, dc.PAIR_N, dc.PAIR_SEED), dc.pair_sequence(a, b, players))
    assert h.op_ends[2] >= 1 and h.op_ends[3] >= 1, f"no episode end in a later segment: {h.op_ends}"
    h.compare_hazards("at the end")
    if a == b == "H":                                        # (the speculative sample is on this path)
        assert h.smp.spec_stats()[1] > 0


@pytest.mark.parametrize("case", list(dc.BIG_CASES))
@pytest.mark.parametrize("kind", list(dc.BIG_SIZES))
def test_big_batch_handovers(cg, kind, case):
    n = dc.BIG_SIZES[kind]
    assert cg._city_of_gold.rollout_kind(n, 4, True) == kind
    assert cg._city_of_gold.rollout_kind(n, 4, False) == "trio"
    dc.run(dc.Harness(cg, n, dc.PAIR_SEED, threads=po.host_threads()), dc.BIG_CASES[case])


@pytest.mark.parametrize("case", list(dc.STATE_CASES))
def test_state_op_between_launches(cg, case):
    h = dc.run(dc.Harness(cg, dc.PAIR_N, dc.PAIR_SEED), dc.STATE_CASES[case])
    assert h.ends >= 1
    h.compare_hazards("at the end")


def test_views_first_touched_after_device_work(cg):
    h = dc.Harness(cg, dc.PAIR_N, dc.PAIR_SEED, lazy_views=True)
    dc.run(h, dc.LAZY_VIEWS_CASE)
    assert h.views and h.op_ends[1] and h.op_ends[2]
    h.compare_hazards("at the end")


@pytest.mark.parametrize("case", list(dc.AUTORESET_CASES))
def test_autoreset_off_on_a_batch(cg, case):
    seq = dc.AUTORESET_CASES[case]
    h = dc.Harness(cg, dc.PAIR_N, dc.PAIR_SEED)
    for k, op in enumerate(seq):
        try:
            h.apply(op)
        except AssertionError as e:
            raise AssertionError(f"{e}\n  after the sequence {seq[:k + 1]!r}") from None
        if k == dc.AUTORESET_QUARTER_AT:
            assert int(np.asarray(h.orc.dones).sum()) * 4 >= dc.PAIR_N, "fewer than a quarter of the envs have ended"
    h.compare_hazards("at the end")


@pytest.mark.parametrize("shards", [1, 2], ids=["one-shard", "two-shards"])
@pytest.mark.parametrize("seed", dc.RANDOM_SEEDS)
def test_random_sequence(cg, seed, shards):
    seq = dc.random_sequence(seed)
    if shards == 1:
        h = dc.Harness(cg, 200, 1234 + seed)
    else:
        seq = dc.for_shards(seq)
        h = dc.Harness(cg, 301, 1234 + seed, device=[0, 0])
        assert h.env.num_shards == 2
    dc.run(h, seq)
    h.compare_hazards("at the end")


def test_host_actions_past_their_heads(cg):
    h = dc.Harness(cg, dc.PAIR_N, dc.PAIR_SEED)
    flagged = []
    for k, op in enumerate(dc.BAD_ACTION_CASE):
        if op == "C":
            flagged.append(int(((h.env.hazards()[1] & dc.BAD_ACTION) != 0).sum()))
        try:
            h.apply(op)                                      # ("C" compares the flags per env, then clears)
        except AssertionError as e:
            raise AssertionError(f"{e}\n  after the sequence {dc.BAD_ACTION_CASE[:k + 1]!r}") from None
        if op == "C":
            assert not h.env.hazards()[0] & dc.BAD_ACTION, "clear_hazards() left COG_HAZ_BAD_ACTION set"
    # per path: flagged after its three steps, none after the legal steps that follow the clear
    assert len(flagged) == 6 and all(flagged[0::2]) and not any(flagged[1::2]), flagged
