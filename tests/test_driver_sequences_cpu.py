"""CPU side of the driver-sequence tests (tests/driver_cases.py, tests/test_gpu_driver_sequences.py):

  the oracle's auto-reset switch (OracleVec.set_autoreset) against its definition: cog_env::step
  (environment.cpp:91-95) without the vec wrapper's reset (vec_environment.h:56-59), and the
  stand-alone oracle harness over its switched-off and clamped-action scenarios under
  AddressSanitizer + UndefinedBehaviorSanitizer
  the conditions each GPU case relies on, counted on the oracle alone: episode ends in segments
  2 and 3 of every pair, a quarter of the envs ended before the switched-off drivers are compared,
  decks with card types >= 8 after greedy steps, and for every random sequence ends, wide decks
  and trio launches entered with and without the compact deck image
  G's numpy argmax against tests/policy_ref.py's float64 reference on the same masks
  the sequences of the launch-form rows (tests/launch_form_cases.py, tests/test_gpu_launch_forms.py):
  episode ends in every op that is meant to hold one, wide decks, trio launches entered both ways,
  the flags the 2-player tail raises, and the rows' own form checks against cog_trio_form_of
"""
import os
import subprocess

import numpy as np
import pytest

import driver_cases as dc
import launch_form_cases as lf
import policy_ref as pr
import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, SEED = 16, 77
ALL = dc.FIELDS + dc.PLAIN


def views(orc, i=None):
    sl = slice(None) if i is None else slice(i, i + 1)
    return {nm: np.array(getattr(orc, nm)[sl], copy=True) for nm in ALL}


def same(a, b):
    for nm in dc.FIELDS:
        if po.named_equal(a[nm], b[nm]) is not None:
            return False
    return all(np.array_equal(a[nm], b[nm]) for nm in dc.PLAIN)


def sample_for(osm, orc, stored):
    osm.sample(po.stored_masks(orc) if stored else orc.selected_action_masks)


# ---- the switch against its definition ----------------------------------------------------------
@pytest.mark.parametrize("stored", [False, True], ids=["selected", "stored"])
def test_autoreset_off_is_the_single_env_step(stored):
    steps = 90
    orc, osm = po.OracleVec(N), po.OracleSampler(N, SEED)
    orc.reset(SEED, 4, 3, 2, 8)
    orc.set_autoreset(False)
    masks, actions, hist = [], [], []
    end_at = np.full(N, -1)
    for t in range(steps):
        m = (po.stored_masks(orc) if stored else orc.selected_action_masks).copy()
        osm.sample(m)
        masks.append(m)
        actions.append(osm.actions.copy())
        orc.step(osm.actions)
        hist.append(views(orc))
        end_at = np.where((end_at < 0) & orc.dones, t, end_at)
    assert (end_at >= 0).all() and end_at.max() < steps - 10, "every env ends well inside the run"
    for i in range(N):
        e = int(end_at[i])
        for t in range(e, steps):                           # dones stay 1, no byte of the env changes
            assert hist[t]["dones"][i]
            for nm in ALL:
                a, b = hist[t][nm][i:i + 1], hist[e][nm][i:i + 1]
                assert (po.named_equal(a, b) is None) if nm in dc.FIELDS else np.array_equal(a, b), (i, t, nm)
        # the env alone, stopped at its ending step: the same switch (every view) and the wrapper
        # with its reset (what the reset leaves alone: rewards, dones, infos; all views before the end)
        for switched in (False, True):
            one, smp1 = po.OracleVec(1), po.OracleSampler(1, SEED, first=i)
            one.reset(SEED + i, 4, 3, 2, 8)
            one.set_autoreset(switched)
            for t in range(e + 1):
                sample_for(smp1, one, stored)
                assert po.named_equal(smp1.actions, actions[t][i:i + 1]) is None
                one.step(smp1.actions)
                if t < e:
                    assert same(views(one), {nm: hist[t][nm][i:i + 1] for nm in ALL}), (i, t, switched)
            got, want = views(one), {nm: hist[steps - 1][nm][i:i + 1] for nm in ALL}
            if not switched:
                assert same(got, want), f"env {i}: not the 1-env run stopped at step {e}"
            else:
                assert np.array_equal(got["rewards"], want["rewards"]) and got["dones"][0]
                assert po.named_equal(got["infos"], want["infos"]) is None
    # the sampler still draws for a finished env: a fresh sampler fed the same masks gives the
    # recorded actions at every step, and they keep changing after the end
    again = po.OracleSampler(N, SEED)
    for t in range(steps):
        again.sample(masks[t])
        assert po.named_equal(again.actions, actions[t]) is None, t
    tail = np.stack([np.stack([a[nm] for nm in dc.HEAD_NAMES], 1) for a in actions[-10:]])
    assert ((tail != tail[0]).any(axis=(0, 2))).sum() >= N // 2, "the draws after the end do not move"


def test_autoreset_off_then_reset_restarts():
    for default in (True, False):
        orc, osm = po.OracleVec(N), po.OracleSampler(N, SEED)
        orc.reset(SEED, 4, 3, 2, 8)
        orc.set_autoreset(False)
        for _ in range(80):
            sample_for(osm, orc, False)
            orc.step(osm.actions)
        assert orc.dones.all()
        before = views(orc)
        if default:
            orc.reset_default()
        else:
            orc.reset(SEED + 100, 4, 3, 2, 8)
        assert orc.dones.all(), "a reset leaves the dones view alone (vec_environment.h:32-44)"
        assert (orc.observations["shared"]["phase"] == 0).all()
        sample_for(osm, orc, False)
        orc.step(osm.actions)
        assert not orc.dones.any(), "the envs step again"
        assert po.named_equal(orc.observations, before["observations"]) is not None
        for _ in range(80):
            sample_for(osm, orc, False)
            orc.step(osm.actions)
        assert orc.dones.all(), "and end again, staying done"
        orc.set_autoreset(True)                              # the switch back on: the next step resets them
        sample_for(osm, orc, False)
        orc.step(osm.actions)
        assert orc.dones.all()
        sample_for(osm, orc, False)
        orc.step(osm.actions)
        assert not orc.dones.any()


def test_stored_sampling_takes_the_envs_own_agent():
    """OracleSampler.sample_stored equals sample(po.stored_masks) while the agent_selection view is
    current, and after a reset takes agent 0's record whatever the stale view shows."""
    a, b = po.OracleVec(N), po.OracleVec(N)
    sa, sb = po.OracleSampler(N, 5), po.OracleSampler(N, 5)
    for o in (a, b):
        o.reset(SEED, 3, 3, 2, 8)
    for t in range(40):
        sa.sample(po.stored_masks(a))
        sb.sample_stored(b)
        assert po.named_equal(sa.actions, sb.actions) is None, t
        a.step(sa.actions)
        b.step(sb.actions)
    assert (b.agent_selection != 0).any()
    b.reset_default()
    assert (b.agent_selection != 0).any(), "the view is stale after a reset"
    sb.sample_stored(b)
    sa.sample(np.ascontiguousarray(b.observations["player_data"]["action_mask"][:, 0]))
    assert po.named_equal(sa.actions, sb.actions) is None
    # the threaded loop with stored masks is the same loop
    c, sc = po.OracleVec(N), po.OracleSampler(N, 5)
    c.reset(SEED, 3, 3, 2, 8)
    po.run_threaded(c, sc, 40, 3, stored=True)
    a2, sa2 = po.OracleVec(N), po.OracleSampler(N, 5)
    a2.reset(SEED, 3, 3, 2, 8)
    for _ in range(40):
        sa2.sample_stored(a2)
        a2.step(sa2.actions)
    assert same(views(c), views(a2)) and po.named_equal(sc.actions, sa2.actions) is None


def test_threaded_reset_default_is_reset_default():
    n = 300
    a, b = po.OracleVec(n), po.OracleVec(n)
    sa, sb = po.OracleSampler(n, 1), po.OracleSampler(n, 1)
    for o, s in ((a, sa), (b, sb)):
        o.reset(SEED, 4, 3, 2, 8)
        po.run_threaded(o, s, 40, 2, stored=True)
    a.reset_default()
    b.reset_default(threads=3)
    assert same(views(a), views(b))
    for o, s in ((a, sa), (b, sb)):
        po.run_threaded(o, s, 40, 2)
    assert same(views(a), views(b)) and np.array_equal(a.flags(), b.flags())


def test_oracle_harness_driver_scenarios_clean_under_asan_ubsan():
    """oracle/asan_harness.c --drivers: the switch off past every env's end and back on, and host
    actions clamped to (21, 21, 21, 6, 18) whether legal or not, in a stand-alone program built with
    both sanitizers: nothing reported, the plain build's hashes."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "asan"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no sanitizer toolchain: " + r.stderr[-400:])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    plain = subprocess.run([os.path.join(ROOT, "oracle", "_asan", "harness"), "--drivers"], capture_output=True, text=True,
                           timeout=120)
    asan = subprocess.run([os.path.join(ROOT, "oracle", "_asan", "harness_asan"), "--drivers"], capture_output=True,
                          text=True, env=env, timeout=300)
    assert plain.returncode == 0 and asan.returncode == 0, asan.stderr[-2000:]
    assert "runtime error" not in asan.stderr and "AddressSanitizer" not in asan.stderr, asan.stderr[-2000:]
    assert asan.stdout == plain.stdout
    rows = {ln.split()[0]: ln.split() for ln in plain.stdout.splitlines() if ln.strip()}
    assert len(rows) == 4
    # dones summed over the steps: with the switch off an ended env counts at every later step
    assert int(rows["stored_hard_ms8_noreset"][2]) > 16 * 60 and int(rows["sel_hard_ms8_noreset_3p"][2]) > 16 * 60
    assert int(rows["clamped_host_actions_sel"][2]) > 0 and int(rows["clamped_host_actions_sto"][2]) > 0


# ---- what the GPU cases rely on ------------------------------------------------------------------
def oracle_run(seq, n=dc.PAIR_N, seed=dc.PAIR_SEED):
    return dc.run(dc.Harness(None, n, seed), seq)


@pytest.mark.slow
@pytest.mark.parametrize("players,drivers", [(4, dc.STEP_DRIVERS), (3, dc.REDUCED_DRIVERS), (2, dc.REDUCED_DRIVERS)],
                         ids=["4p", "3p", "2p"])
def test_pairs_hold_episode_ends_in_segments_2_and_3(players, drivers):
    """Every ordered pair: segments 2 and 3 of X a b a each hold an episode end with its auto-reset
    (measured: at least 40 in segment 2 and 74 in segment 3 of every pair, 2 to 4 players)."""
    worst = [10 ** 9, 10 ** 9]
    for a in drivers:
        for b in drivers:
            e = oracle_run(dc.pair_sequence(a, b, players)).op_ends
            assert e[2] >= 1 and e[3] >= 1, f"pair {a} -> {b}, {players} players: ends per op {e}"
            worst = [min(worst[0], e[2]), min(worst[1], e[3])]
    assert worst[0] >= 20 and worst[1] >= 20, worst


def test_state_cases_on_the_oracle():
    for name, seq in dc.STATE_CASES.items():
        h = oracle_run(seq)
        assert h.ends >= 20, (name, h.op_ends)
        assert h.trio_loaded >= 1 and h.trio_clear >= 1, name
    h = oracle_run(dc.STATE_CASES["players"])
    assert h.op_ends[1] and h.op_ends[3] and h.op_ends[5], h.op_ends    # ends with 4, 2 and 3 players
    h = oracle_run(dc.LAZY_VIEWS_CASE)
    assert h.op_ends[1] and h.op_ends[2] and h.op_ends[4], h.op_ends


@pytest.mark.parametrize("name", list(dc.AUTORESET_CASES))
def test_autoreset_cases_end_a_quarter_of_the_envs(name):
    seq = dc.AUTORESET_CASES[name]
    h = dc.Harness(None, dc.PAIR_N, dc.PAIR_SEED)
    for k, op in enumerate(seq):
        h.apply(op)
        if k == dc.AUTORESET_QUARTER_AT:
            assert int(np.asarray(h.orc.dones).sum()) * 4 >= dc.PAIR_N, f"{name}: fewer than a quarter have ended"
    assert h.op_ends[-1] >= 1, f"{name}: no end after the switch is on again: {h.op_ends}"


def test_greedy_steps_leave_wide_decks():
    """10 greedy and 10 uniform stored-mask steps alternating for 120 steps (200 envs, HARD, 3 pieces,
    seed 77): episode ends and envs holding a card type >= 8, which a trio launch must park."""
    want = {(4, 8): (281, 82), (3, 8): (280, 78), (2, 12): (151, 116)}
    for (players, max_steps), (ends, wide) in want.items():
        h = oracle_run([("X", 77, players, 3, 2, max_steps)] + [("G", 10), ("Hs", 10)] * 6)
        assert (h.ends, dc.wide_envs(h.orc)) == (ends, wide), (players, max_steps, h.ends, dc.wide_envs(h.orc))
    for name in ("pipe", "wave"):                           # S50 -> G(5) -> T20: the trio meets wide decks
        h = oracle_run(dc.BIG_CASES["S50_G_T20"][:3])
        assert dc.wide_envs(h.orc) >= 1, name


@pytest.mark.parametrize("seed", dc.RANDOM_SEEDS)
def test_random_sequences_keep_their_cases(seed):
    seq = dc.random_sequence(seed)
    assert len(seq) == dc.RANDOM_OPS and seq == dc.random_sequence(seed)
    for n, s in ((200, seq), (301, dc.for_shards(seq))):
        h = dc.run(dc.Harness(None, n, 1234 + seed), s)
        census = dict(ends=h.ends, wide=h.wide_max, trio_loaded=h.trio_loaded, trio_clear=h.trio_clear)
        assert all(v > 0 for v in census.values()), f"seed {seed}, n {n}: {census}"
    assert not any(op[0] in dc.SINGLE_SHARD_ONLY for op in dc.for_shards(seq) if not isinstance(op, str))


def test_random_sequences_draw_from_every_op():
    ops = [op if isinstance(op, str) else op[0] for s in dc.RANDOM_SEEDS for op in dc.random_sequence(s)]
    for name in dc.STEP_DRIVERS + ("X", "X0", "I", "C", "A0", "A1"):
        assert name in ops, name
    resets = [op for s in dc.RANDOM_SEEDS for op in dc.random_sequence(s) if not isinstance(op, str) and op[0] == "X"]
    assert {op[2] for op in resets} == {2, 3, 4} and {op[4] for op in resets} == {0, 1, 2}
    assert min(op[5] for op in resets) >= 8 and max(op[5] for op in resets) <= 40


def test_bad_action_case_on_the_oracle():
    h = dc.Harness(None, dc.PAIR_N, dc.PAIR_SEED)
    hits = []
    for op in dc.BAD_ACTION_CASE:
        if op == "C" and h.bad_ever.any():
            hits.append(int(h.bad_ever.sum()))
        h.apply(op)
    assert len(hits) == 3 and all(dc.PAIR_N // 2 <= k < dc.PAIR_N for k in hits), f"some envs, not all: {hits}"
    rng = np.random.default_rng(0)
    legal = np.zeros(1000, dtype=po.ACTION)
    raw, clamped, rows = dc.bad_actions(rng, legal)
    over = raw[:, :5] > np.array(dc.CLAMP)
    assert np.array_equal(over.any(1), rows) and 0.05 < over.mean() < 0.15
    for k, nm in enumerate(dc.HEAD_NAMES):
        assert np.array_equal(clamped[nm], np.where(over[:, k], dc.CLAMP[k], 0))


# ---- the launch-form rows ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", lf.SIZES)
def test_launch_form_rollout_sequence_keeps_its_cases(n):
    """Measured on the oracle at n = 200 (33): ends in ops 1..6 30, 170, 166, 24, 159, 156 (3, 30, 28, 5,
    24, 28), in 8..10 17, 177, 150 (1, 32, 22), in the two T20 ops after A0 22, 178 (3, 30), every env
    done before X0; up to 64 (12) envs with a card type >= 8 at once; trio launches entered with
    cdeck_ok 1 / 0: 28 / 8; no hazard flag.  Conditions, not equalities."""
    h = dc.Harness(None, n, dc.PAIR_SEED)
    for k, op in enumerate(lf.ROLLOUT_SEQ):
        h.apply(op)
        if k + 1 == lf.ROLLOUT_ALL_DONE_AT:
            assert np.asarray(h.orc.dones).all(), "an env has not ended before X0"
    assert lf.ROLLOUT_SEQ[lf.ROLLOUT_ALL_DONE_AT] == "X0"
    for k in lf.ROLLOUT_END_OPS:
        assert h.op_ends[k] >= 1, f"n {n}: op {k} {lf.ROLLOUT_SEQ[k]!r} holds no episode end: {h.op_ends}"
    assert h.wide_max > 0 and h.trio_loaded > 0 and h.trio_clear > 0, (h.wide_max, h.trio_loaded, h.trio_clear)
    assert not h.orc.flags().any(), "the rollout sequence raises a hazard flag on the oracle"
    # the 2-player tail behind a forced pipe / wave: flags to compare per env, and ends
    for op in lf.TWO_PLAYER_TAIL:
        h.apply(op)
    flags = h.orc.flags()
    for f in (po.F_ERASE_PAST, po.F_Q9_OOB, po.F_OOB_LOOKUP, po.F_B_START_LT4):
        assert (flags & f).any(), f"n {n}: flag {f:#x} is not raised"
    assert h.op_ends[-1] >= 1 and h.op_ends[-2] >= 1, h.op_ends


def test_launch_form_host_and_redo_sequences_keep_their_cases():
    for n in (200, lf.HOST_TWO_SHARD_N):                     # (measured at 200: 28 to 180 ends per op)
        h = oracle_run(lf.HOST_SEQ, n)
        assert all(e >= 1 for e in h.op_ends[1:]), (n, h.op_ends)
    h = oracle_run(lf.REDO_SEQ)                              # (30, 180, 194 ends at max_steps 8, then none)
    assert all(e >= 1 for e in h.op_ends[1:4]) and h.trio_loaded > 0 and h.trio_clear > 0, h.op_ends


def test_launch_form_rows_cover_the_forms():
    """Every row's switches are among those the engine's sources read, the rows span both values of
    every form figure, and check_form accepts what a device of 256 CUs gives and refuses a switch
    that was ignored (cog_trio_form_of needs no device; this process has read no switch)."""
    src = "".join(open(os.path.join(ROOT, "gym-eldorado_amd", "csrc", f)).read() for f in ("cog_engine.hip", "cog_abi.cpp"))
    for r in lf.ROWS.values():
        for k in r.env:
            assert f'getenv("{k}")' in src, f"{r.name}: no source reads ${k}"
        assert r.sizes and lf.sequence_of(r)[0][0] == "X"
    assert {(r, n) for r, n in lf.CASES} >= {(r, n) for r in ("default", "no-lat", "epw32", "epw32-no-lat", "wpc1", "wpc2",
                                                              "wpc3", "wpc4", "round3-duo", "pipe", "wave") for n in (200, 33)}
    if any(os.environ.get(k) for k in lf.SWITCHES + ["COG_ROLLOUT", "COG_TRIO"]):
        return                                               # (forms forced from outside: the rest does not apply)
    from city_of_gold import _city_of_gold as C
    for n in (200, 33, lf.BIG_N):
        form = C.trio_form(n)
        kinds = {f"{p},{int(s)}": C.rollout_kind(n, p, s) for p in (4, 3, 2, 1) for s in (False, True)}
        assert form["cus"] == 256 or C.device_count() > 0
        if n != lf.BIG_N:
            lf.check_form(lf.ROWS["default"], n, form, kinds)
            for other in ("no-lat", "epw32", "wpc1", "wpc3", "round3-duo", "pipe"):
                with pytest.raises(AssertionError):
                    lf.check_form(lf.ROWS[other], n, form, kinds)
        else:
            assert form["workgroups"] == 257 and (form["cus"] != 256 or (form["lat"], form["wpc"], form["fixup_grid"]) == (0, 2, 256))


# ---- G's mirror ------------------------------------------------------------------------------------
def test_greedy_mirror_against_the_float64_reference():
    rng = np.random.default_rng(11)
    n = 600
    logits = dc.logits_table(n)
    masks = [pr.random_masks(rng, n)]
    orc, osm = po.OracleVec(n), po.OracleSampler(n, 3)
    orc.reset(3, 4, 3, 2, 8)
    for t in range(60):                                      # masks of a real run, stored and selected
        osm.sample(po.stored_masks(orc))
        orc.step(osm.actions)
        if t % 10 == 9:
            masks += [po.stored_masks(orc).view(np.uint8).reshape(n, 128), orc.selected_action_masks.view(np.uint8).reshape(n, 128)]
    tied = logits.copy()
    tied[:, ::2] = 0.5                                       # equal maxima: the lowest index wins
    empty = 0
    for m in masks:
        m = np.ascontiguousarray(m)
        rec = m.view(po.MASK).reshape(n)
        for lg in (logits, tied):
            want = pr.sample(lg, m, greedy=True)["actions"]
            got = dc.greedy_actions(lg, rec)
            assert np.array_equal(np.stack([got[nm] for nm in dc.HEAD_NAMES], 1), want)
        empty += int((~(m[:, 22:44] != 0).any(1)).sum())
    assert empty > 0, "no head without a valid entry: the rule for it went untested"
