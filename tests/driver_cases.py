"""Driver sequences (tests/test_driver_sequences_cpu.py, tests/test_gpu_driver_sequences.py): every
way of advancing one handle as an op with an engine side and an oracle side, so that a test is a
list of op ids and run() walks both sides through it, comparing all views after every op.

A handle carries host-side state from call to call (cog_abi.cpp: EnvShard::lean_clock and cdeck_ok,
host_synced / pub_done / mir_valid, SamplerSpec::ok, park_seq, autoreset, the last reset's players
and max_steps); what a kernel may assume depends on which call came before it.  The ops:

  step drivers, ("id", steps)                          engine                      oracle
    H       smp.sample(env.selected_action_masks); env.step(smp.get_actions())     sample selected; step
    Hc      the same with a copy of the actions (staged, no speculation)          same
    Hs      the host loop on po.stored_masks(env)                                 sample stored (views); step
    D       smp.sample(...); env.step_device(the sampler's device actions)        sample selected; step
    G       smp.sample_policy(logits, env, "stored", greedy=True); step_device    numpy argmax over the stored
            with the fixed table logits_table(n)                                  mask (views); sampler untouched
    R1      runner.sample(); runner.step_sync() on a host-view runner            sample selected; step
    Rr      runner.step() with no pending sample; runner.sync()                   step with the last actions again
    T<k>    selected-mask runner, device views, set_chunk(k), rollout(steps),     sample selected; step
            sync(), env.sync_host()
    Th<k>   the same on a host-view runner (sync() publishes)                     same
    S<k>    stored-mask runner, device views, chunked                             sample stored (own agent); step
    L, Ls   host-view runners with chunk 1 (one launch per step), selected /      as T / S
            stored masks
  state ops
    ("X", seed, players, pieces, difficulty, max_steps)    reset with parameters
    "X0"    env.reset() / reset_default          "I"   invalidate_device(), nothing edited
    "C"     hazards() compared, then cleared     "A0" / "A1"   set_autoreset(False / True)
    "V"     the host views touched for the first time (a Harness made with lazy_views=True compares
            nothing before it)
  ("B", path, steps, seed)   host actions with a tenth of the (env, head) slots past their head and
            garbage in bytes 5..63, through path "step" | "step_device" | "runner"; the oracle gets
            them clamped to CLAMP, what the engine documents (COG_HAZ_BAD_ACTION)

  ("M", path, steps, seed, kind, frac)   host actions inside their heads that the mask need not allow
            (tests/offmask_cases.py), through the same three paths; both sides get the same bytes: the
            reference executes such an action as it stands (environment.cpp:91-181 never reads the mask)

"stored (views)" is po.stored_masks: the record of the agent the agent_selection view shows, which
a reset leaves alone (vec_environment.h:32-44), as a host loop or sample_policy reads it; the
stored-mask kernels sample for the env's own agent (0 after a reset), OracleSampler.sample_stored.

The Harness also counts, on the oracle alone, what a case must hold to keep its point (episode ends
per op, envs with a card type >= 8 in a deck) and mirrors the table of cog_abi.cpp that decides
with which cdeck_ok a trio launch is entered, so that the CPU suite can assert that every sequence
enters trio launches both ways.
"""
from __future__ import annotations

import re

import numpy as np

import pyoracle as po

FIELDS = ("observations", "selected_action_masks", "infos")
PLAIN = ("rewards", "dones", "agent_selection")
HEADS = ((0, 22), (22, 22), (44, 22), (66, 7), (73, 19))      # (offset, size) in ActionMask byte order
HEAD_NAMES = ("play", "play_special", "remove", "move", "get_from_shop")
CLAMP = (21, 21, 21, 6, 18)           # step_action<MASK_EXTERNAL>: an index past its head becomes this
BAD_ACTION = 0x100                    # COG_HAZ_BAD_ACTION

STEP_DRIVERS = ("H", "Hc", "Hs", "D", "G", "R1", "Rr", "T2", "T20", "T1000", "Th2", "Th20", "Th1000",
                "S2", "S20", "S1000", "L", "Ls")
REDUCED_DRIVERS = ("H", "G", "T20", "S20", "L", "Rr")
SINGLE_SHARD_ONLY = ("D", "G")        # step_device and sample_policy take one device pointer
STATE_OPS = ("X0", "I", "C", "A0", "A1", "V")
_CHUNKED = re.compile(r"^(Th|T|S)(\d+)$")

# the pair table: X -> a(s) -> b(s) -> a(s); on the oracle every 24-step window after the first
# holds episode ends at max_steps 8 (tests/test_driver_sequences_cpu.py asserts it per pair)
PAIR_N, PAIR_SEED, PAIR_MAX_STEPS, PAIR_STEPS = 200, 77, 8, 30


def logits_table(n):
    """G's fixed (n, 92) float32 logits."""
    return np.random.default_rng(3).standard_normal((n, 92)).astype(np.float32)


def greedy_actions(logits, masks):
    """cog.h COG_POLICY_GREEDY in numpy: per head the valid entry with the largest logit, ties to the
    lowest index, 0 for a head with no valid entry.  masks: (n,) ActionMask records."""
    n = logits.shape[0]
    valid = np.ascontiguousarray(masks).view(np.uint8).reshape(n, 128)[:, :92] != 0
    out = np.zeros(n, dtype=po.ACTION)
    for name, (off, k) in zip(HEAD_NAMES, HEADS):
        v = valid[:, off:off + k]
        l = np.where(v, logits[:, off:off + k], -np.inf)
        out[name] = np.where(v.any(1), l.argmax(1), 0)       # (argmax: the first of equal maxima)
    return out


def bad_actions(rng, legal):
    """From (n,) legal ActionData records: (raw (n, 64) uint8 with a random tenth of the (env, head)
    slots past their head -- 22..255 / 7..255 / 19..255 -- and garbage in bytes 5..63, the records
    clamped to CLAMP, bool[n]: the env holds such a slot)."""
    n = legal.shape[0]
    raw = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    clamped = legal.copy()
    hit = rng.random((n, 5)) < 0.1
    for k, name in enumerate(HEAD_NAMES):
        over = rng.integers(CLAMP[k] + 1, 256, size=n, dtype=np.uint8)
        raw[:, k] = np.where(hit[:, k], over, legal[name])
        clamped[name] = np.where(hit[:, k], CLAMP[k], legal[name])
    return raw, clamped, hit.any(1)


# ---- host actions off the mask (the M op; tests/offmask_cases.py has the cases and their census) ----
OFFMASK_KINDS = ("single", "replace", "all", "play", "special", "remove", "move", "shop", "sweep")
_ONE_HEAD = {"play": 0, "special": 1, "remove": 2, "move": 3, "shop": 4}
SWEEP_SLOTS = tuple((k, v) for k in range(5) for v in range(1, CLAMP[k] + 1))     # 87 (head, value >= 1) pairs
PRIORITY = (0, 1, 3, 4, 2)            # cog_env::step takes the first non-zero head of play, play_special,
                                      # move, get_from_shop, remove (environment.cpp:98-171)


def executed_head(actions):
    """The head cog_env::step executes for each (n,) ActionData record, -1 for a pass."""
    out = np.full(actions.shape[0], -1)
    for k in reversed(PRIORITY):
        out = np.where(actions[HEAD_NAMES[k]] != 0, k, out)
    return out


def offmask_actions(rng, legal, kind, frac, t=0, first=0):
    """From (n,) legal ActionData records: (the records with a random `frac` of the envs altered after
    `kind`, bool[n]: the env was altered).  Every value stays inside its head (1..CLAMP[k], or 0), so
    no index is clamped and COG_HAZ_BAD_ACTION stays clear.
      single   one random head uniform in 1..top, the other heads 0
      replace  one random head uniform in 1..top, the other heads as sampled
      all      every head uniform in 0..top
      play, special, remove, move, shop    `single` with that head
      sweep    env e takes SWEEP_SLOTS[(first + e + t) % 87] at step t, every env (frac is 1)"""
    n = legal.shape[0]
    out = np.zeros(n, dtype=po.ACTION)                       # (bytes 5..63 zero: a copy leaves the padding undefined)
    top = np.array(CLAMP)
    u_hit, u_head, u_val = rng.random(n), rng.integers(0, 5, size=n), rng.random((n, 5))
    if kind == "sweep":
        hit = np.ones(n, dtype=bool)
        slot = (first + np.arange(n) + t) % len(SWEEP_SLOTS)
        head = np.array([s[0] for s in SWEEP_SLOTS])[slot]
        val = np.array([s[1] for s in SWEEP_SLOTS])[slot][:, None].repeat(5, 1)
    else:
        hit = u_hit < frac
        head = np.full(n, _ONE_HEAD[kind]) if kind in _ONE_HEAD else u_head
        val = 1 + np.minimum((u_val * top).astype(np.int64), top - 1)          # uniform in 1..top
    for k, name in enumerate(HEAD_NAMES):
        if kind == "all":
            v = np.minimum((u_val[:, k] * (top[k] + 1)).astype(np.int64), top[k])   # uniform in 0..top
        elif kind == "replace":
            v = np.where(head == k, val[:, k], legal[name])
        else:
            v = np.where(head == k, val[:, k], 0)
        out[name] = np.where(hit, v, legal[name]).astype(np.uint8)
    return out, hit


def wide_envs(orc):
    """Envs with a card of type >= 8 in some pile of some player (the trio's compact decks cannot
    hold them: such an env parks at step 0 of every trio launch)."""
    n = orc.n
    piles = np.ascontiguousarray(orc.observations["player_data"]["obs"]).view(np.uint8).reshape(n, 4, 5, 21)
    return int((piles[:, :, :, 8:] != 0).any(axis=(1, 2, 3)).sum())


class Harness:
    """One engine handle (env, sampler, its runners) and the oracle pair that mirrors it.  cg=None:
    the oracle side alone (the CPU census).  threads > 0: the oracle's rollouts and resets run on
    that many host threads (the large batches).  first: the sampler's first_index (sampler i is seeded
    sampler_seed + first + i)."""

    def __init__(self, cg, n, sampler_seed, device=None, threads=0, lazy_views=False, first=0):
        self.cg, self.n, self.threads, self.first = cg, n, threads, first
        self.orc, self.osm = po.OracleVec(n), po.OracleSampler(n, sampler_seed, first)
        self.last = np.zeros(n, dtype=po.ACTION)             # what the sampler's device actions hold
        self.logits = logits_table(n)
        self.autoreset, self.players, self.max_steps = True, 4, 100000
        self.views, self.acts_fresh = not lazy_views, False
        self.bad_ever = np.zeros(n, dtype=bool)
        self.done_prev = np.zeros(n, dtype=bool)
        # census (oracle and the host-state mirror alone)
        self.ends, self.op_ends, self.wide_max = 0, [], 0
        self.cdeck, self.trio_loaded, self.trio_clear = False, 0, 0
        self.m_t, self.census = 0, None                      # M's step clock (sweep); offmask_cases.Census
        if cg is not None:
            kw = self.kw = {} if device is None else {"device": device}
            self.env = cg.vec.get_vec_env(n)(**kw)
            self.smp = cg.vec.get_vec_sampler(n)(sampler_seed, first_index=first, **kw)
            self.runners, self.t_logits = {}, None

    def new_sampler(self, sampler_seed):
        """The sampler made anew for `sampler_seed` on both sides (tests/planted_cases.py: a seed is a
        generator state); the runners, which hold the old sampler, go with it."""
        self.osm = po.OracleSampler(self.n, sampler_seed, self.first)
        self.last = np.zeros(self.n, dtype=po.ACTION)
        self.acts_fresh = False
        if self.cg is not None:
            self.runners = {}
            self.smp = self.cg.vec.get_vec_sampler(self.n)(sampler_seed, first_index=self.first, **self.kw)

    # ---- engine parts --------------------------------------------------------------------------
    def runner(self, stored, device_views):
        key = (stored, device_views)
        if key not in self.runners:
            self.runners[key] = self.cg.vec.get_runner(self.n)(self.env, self.smp, None, device_views=device_views,
                                                               stored_masks=stored)
        return self.runners[key]

    def torch_device(self):
        import torch
        return torch.device("cuda", self.smp.device)

    def compare(self, what):
        env, orc = self.env, self.orc
        for nm in FIELDS:
            a, b = getattr(env, nm), getattr(orc, nm)
            if self.n > 4096 and np.array_equal(a.view(np.uint8), b.view(np.uint8)):
                continue                                     # (whole records alike: no leaf can differ)
            bad = po.named_equal(a, b)
            assert bad is None, f"{what}: {nm}.{bad} differs from the oracle"
        for nm in PLAIN:
            a, b = np.asarray(getattr(env, nm)), np.asarray(getattr(orc, nm))
            if not np.array_equal(a, b):
                i = int(np.nonzero((a != b).reshape(self.n, -1).any(1))[0][0])
                raise AssertionError(f"{what}: {nm} differs from the oracle (first at env {i})")
        if self.acts_fresh:
            bad = po.named_equal(self.smp.get_actions(), self.last)
            assert bad is None, f"{what}: the sampler's actions view differs in {bad}"

    def compare_device_actions(self, what):
        """The sampler's device actions against the oracle sampler's (a single shard, through torch)."""
        import torch
        acts = torch.from_dlpack(self.smp.dlpack()).cpu().numpy().view(po.ACTION).reshape(self.n)
        bad = po.named_equal(acts, self.last)
        if bad is not None:
            i = int(np.nonzero(acts[bad] != self.last[bad])[0][0])
            raise AssertionError(f"{what}: the sampler's device actions differ in {bad} (first at env {i})")

    def compare_hazards(self, what):
        per = self.env.hazards()[1]
        assert np.array_equal((per & BAD_ACTION) != 0, self.bad_ever), f"{what}: COG_HAZ_BAD_ACTION is on the wrong envs"
        rest, want = per & ~np.uint32(BAD_ACTION), self.orc.flags()
        if not np.array_equal(rest, want):
            i = int(np.nonzero(rest != want)[0][0])
            raise AssertionError(f"{what}: hazard flags differ (first at env {i}: {int(rest[i]):#x}, oracle {int(want[i]):#x})")

    # ---- oracle parts --------------------------------------------------------------------------
    def _count(self):
        d = np.array(self.orc.dones, dtype=bool)
        self.ends += int(d.sum()) if self.autoreset else int((d & ~self.done_prev).sum())
        self.done_prev = d

    def _oracle_steps(self, steps, source):
        """source: "selected" | "stored_view" | "stored_own" | "greedy" | "repeat"."""
        orc, osm = self.orc, self.osm
        if self.threads and steps and source in ("selected", "stored_own"):
            po.run_threaded(orc, osm, steps, self.threads, stored=source == "stored_own")
            self.last = osm.actions.copy()
            return
        for _ in range(steps):
            if source == "selected":
                osm.sample(orc.selected_action_masks)
            elif source == "stored_view":
                osm.sample(po.stored_masks(orc))
            elif source == "stored_own":
                osm.sample_stored(orc)
            if source == "greedy":
                self.last = greedy_actions(self.logits, po.stored_masks(orc))
            elif source != "repeat":
                self.last = osm.actions.copy()
            orc.step(self.last)
            self._count()

    def _trio_model(self, steps, chunk):
        """EnvShard::cdeck_ok as runner_launch_fused leaves it, and how the trio launches of this
        rollout were entered (selected masks, >= 3 players, max_steps >= 1, a chunk > 1: the trio at
        every size)."""
        if not steps:
            return
        if chunk > 1 and self.players >= 3 and self.max_steps:
            launches = -(-steps // chunk)
            self.trio_loaded += launches - (0 if self.cdeck else 1)
            self.trio_clear += 0 if self.cdeck else 1
            self.cdeck = True
        else:
            self.cdeck = False

    # ---- the ops -------------------------------------------------------------------------------
    def apply(self, op):
        name, args = (op, ()) if isinstance(op, str) else (op[0], tuple(op[1:]))
        ends0 = self.ends
        eng = self.cg is not None
        if name == "X":
            seed, players, pieces, difficulty, max_steps = args
            if eng:
                self.env.reset(seed, players, pieces, self.cg.Difficulty(difficulty), max_steps, False)
            if self.threads:
                self.orc.reset_threaded(seed, players, pieces, difficulty, max_steps, self.threads)
            else:
                self.orc.reset(seed, players, pieces, difficulty, max_steps)
            self.players, self.max_steps, self.cdeck = players, max_steps, False
        elif name == "X0":
            if eng:
                self.env.reset()
            self.orc.reset_default(self.threads)
            self.cdeck = False
        elif name == "I":
            if eng:
                self.env.invalidate_device()
            self.cdeck = False
        elif name == "C":
            if eng:
                self.compare_hazards(name)
                self.env.clear_hazards()
            self.orc.clear_flags()
            self.bad_ever[:] = False
        elif name in ("A0", "A1"):
            on = name == "A1"
            if eng:
                self.env.set_autoreset(on)
            self.orc.set_autoreset(on)
            self.autoreset, self.cdeck = on, False
            self.done_prev = np.zeros(self.n, dtype=bool)
        elif name == "V":
            if eng:
                self.env.observations                        # (allocates and fills the host views)
            self.views = True
        elif name == "B":
            self._bad(*args)
        elif name == "M":
            self._offmask(*args)
        else:
            self._step_driver(name, *args)
        self.op_ends.append(self.ends - ends0)
        self.wide_max = max(self.wide_max, wide_envs(self.orc)) if self.n <= 4096 else self.wide_max
        if eng and self.views:
            self.compare(str(name))

    def _step_driver(self, name, steps):
        eng = self.cg is not None
        if self.census is not None:
            self.census.entry(self, name)
        m = _CHUNKED.match(name)
        if m or name in ("L", "Ls"):
            kind, chunk = (m.group(1), int(m.group(2))) if m else ("Th" if name == "L" else "Sh", 1)
            stored, device_views = kind in ("S", "Sh"), kind in ("T", "S")
            if eng:
                r = self.runner(stored, device_views)
                r.set_chunk(chunk)
                r.rollout(steps)
                r.sync()
                if device_views and self.views:
                    self.env.sync_host()
                self.acts_fresh = not device_views           # (a host-view sync publishes the actions too)
            self._oracle_steps(steps, "stored_own" if stored else "selected")
            self._trio_model(steps, 1 if stored else chunk)
            return
        if steps:
            self.cdeck = False                               # (every other driver takes full steps)
        if name in ("H", "Hc", "Hs", "D"):
            if eng:
                env, smp = self.env, self.smp
                acts = smp.get_actions()
                for _ in range(steps):
                    smp.sample(po.stored_masks(env) if name == "Hs" else env.selected_action_masks)
                    if name == "D":
                        env.step_device(smp.device_actions())    # (asked for after the sample: a taken
                    else:                                        # speculation swaps the buffers)
                        env.step(acts.copy() if name == "Hc" else acts)
                self.acts_fresh = self.acts_fresh or steps > 0
            self._oracle_steps(steps, "stored_view" if name == "Hs" else "selected")
        elif name == "G":
            if eng:
                import torch
                if self.t_logits is None:
                    self.t_logits = torch.from_numpy(self.logits).to(self.torch_device())
                for _ in range(steps):
                    acts, _, _ = self.smp.sample_policy(self.t_logits, self.env, "stored", greedy=True)
                    self.env.step_device(acts.data_ptr())
                if steps:
                    self.acts_fresh = False                  # (sample_policy leaves the host view alone)
                    got = acts[:, :5].cpu().numpy()          # (the last step's, from the device)
            self._oracle_steps(steps, "greedy")
            if eng and steps:
                want = np.stack([self.last[nm] for nm in HEAD_NAMES], axis=1)
                assert np.array_equal(got, want), "G: the greedy actions differ from the numpy mirror"
        elif name == "R1":
            if eng:
                r = self.runner(False, False)
                for _ in range(steps):
                    r.sample()
                    r.step_sync()
                self.acts_fresh = self.acts_fresh or steps > 0
            self._oracle_steps(steps, "selected")
        elif name == "Rr":
            if eng:
                r = self.runner(False, False)
                for _ in range(steps):
                    r.step()
                r.sync()
                self.acts_fresh = True                       # (the sync publishes the device actions)
            self._oracle_steps(steps, "repeat")
        else:
            raise ValueError(f"unknown op {name!r}")

    def _bad(self, path, steps, seed):
        eng = self.cg is not None
        rng = np.random.default_rng(seed)
        if steps:
            self.cdeck = False
        for _ in range(steps):
            self.osm.sample(self.orc.selected_action_masks)  # the legal records the bad slots go into
            raw, clamped, hit = bad_actions(rng, self.osm.actions.copy())
            self.bad_ever |= hit
            if eng:
                import torch
                self.smp.sample(self.env.selected_action_masks)   # (the two samplers stay in step)
                if path == "step":
                    self.env.step(raw.view(po.ACTION).reshape(self.n))
                elif path == "step_device":
                    t = torch.from_numpy(raw).to(self.torch_device())
                    self.env.step_device(t.data_ptr())
                else:
                    d = torch.from_dlpack(self.smp.dlpack())
                    d.copy_(torch.from_numpy(raw))
                    torch.cuda.synchronize(d.device)         # (the engine's stream reads them next)
                    r = self.runner(False, False)
                    r.step()
                    r.sync()
                self.acts_fresh = False
            self.last = clamped
            self.orc.step(clamped)
            self._count()

    def _offmask(self, path, steps, seed, kind, frac):
        eng = self.cg is not None
        rng = np.random.default_rng(seed)
        if steps:
            self.cdeck = False
        for _ in range(steps):
            self.osm.sample(self.orc.selected_action_masks)  # the legal records the altered ones replace
            acts, hit = offmask_actions(rng, self.osm.actions.copy(), kind, frac, self.m_t, self.first)
            self.m_t += 1
            if self.census is not None:
                self.census.before(self, acts, hit)
            if eng:
                import torch
                self.smp.sample(self.env.selected_action_masks)   # (the two samplers stay in step)
                raw = np.ascontiguousarray(acts).view(np.uint8).reshape(self.n, 64)
                if path == "step":
                    self.env.step(acts)
                elif path == "step_device":
                    t = torch.from_numpy(raw).to(self.torch_device())
                    self.env.step_device(t.data_ptr())
                else:
                    d = torch.from_dlpack(self.smp.dlpack())
                    d.copy_(torch.from_numpy(raw))
                    torch.cuda.synchronize(d.device)         # (the engine's stream reads them next)
                    r = self.runner(False, False)
                    r.step()
                    r.sync()
                self.acts_fresh = False
            self.last = acts
            self.orc.step(acts)
            self._count()
            if self.census is not None:
                self.census.after(self)


def run(h: Harness, seq):
    """Apply the ops of `seq` to both sides of `h`, comparing after every op; a mismatch names the
    sequence up to and including the op that failed, a plain list that replays by hand."""
    seq = list(seq)
    for k, op in enumerate(seq):
        try:
            h.apply(op)
        except AssertionError as e:
            raise AssertionError(f"{e}\n  after the sequence {seq[:k + 1]!r}") from None
    return h


def pair_sequence(a, b, players=4):
    x = ("X", PAIR_SEED, players, 3, 2, PAIR_MAX_STEPS)
    return [x, (a, PAIR_STEPS), (b, PAIR_STEPS), (a, PAIR_STEPS)]


# ---- the named cases of tests/test_gpu_driver_sequences.py --------------------------------------
X4 = ("X", PAIR_SEED, 4, 3, 2, PAIR_MAX_STEPS)
T20, TH20, S20 = ("T20", PAIR_STEPS), ("Th20", PAIR_STEPS), ("S20", PAIR_STEPS)

# state ops between launches (n = PAIR_N).  The last reset of "players" has max_steps 40: its first
# two T20 ops (launches of 20 + 10 steps each) stay below the no-fix-up bound lean_clock + K <
# max_steps (0 + 20, 20 + 10; 30 + 20 is past it: a fix-up follows from there on)
STATE_CASES = {
    "reset_default": [X4, T20, "X0", T20],
    "players": [X4, T20, ("X", 78, 2, 3, 2, 8), T20, ("X", 79, 3, 3, 2, 8), T20, ("X", 80, 4, 3, 2, 40), T20, T20, T20],
    "invalidate": [X4, T20, "I", T20],
    "chunks": [X4, ("T2", PAIR_STEPS), ("T1000", PAIR_STEPS), T20],
    "clear_hazards": [X4, T20, "C", T20],
    "host_view_runner": [X4, T20, TH20, T20],
    "first_reset_then_default": [X4, "X0", T20, ("H", PAIR_STEPS), T20],
}
STATE_CASES.update({f"zero_steps_{d}": [X4, T20, (d, 0), T20] for d in STEP_DRIVERS})
LAZY_VIEWS_CASE = [X4, T20, S20, "V", T20]                 # (a Harness with lazy_views=True)

# auto-reset off on a batch: the driver twice (past the end of at least a quarter of the envs, on
# the oracle), everything restarted, the switch on again, the driver once more
AUTORESET_DRIVERS = ("H", "L", "T20", "S20", "R1")
AUTORESET_CASES = {d: [X4, "A0", (d, PAIR_STEPS), (d, PAIR_STEPS), "X0", "A1", (d, PAIR_STEPS)] for d in AUTORESET_DRIVERS}
AUTORESET_CASES["mixed"] = [X4, "A0", T20, ("H", 10), S20, "A1", T20]
AUTORESET_QUARTER_AT = 3                                   # ops applied when the quarter is counted

# the rollout kernels small batches never select: stored masks pick the pipe at 16,385..32,768 envs
# and the one-wave kernel above; the smallest ragged sizes past each bound
BIG_SIZES = {"pipe": 16385, "wave": 32769}
BIG_CASES = {
    "T20_S50_T20": [X4, T20, ("S50", 50), T20],
    "S50_H_S50": [X4, ("S50", 50), ("H", 5), ("S50", 50)],
    "S50_X0_S50": [X4, ("S50", 50), "X0", ("S50", 50)],
    "S50_G_T20": [X4, ("S50", 50), ("G", 5), T20],
}

# host actions past their heads through the three paths that take them, one step per op (every step
# compared), the flags checked and cleared after each path (three steps leave about a fifth of the
# envs without such an index), legal host steps between
BAD_ACTION_CASE = [X4]
for _k, _path in enumerate(("step", "step_device", "runner")):
    BAD_ACTION_CASE += [("B", _path, 1, 10 * _k + j) for j in range(3)] + ["C", ("H", 10), "C"]


# ---- the seeded random sequences ---------------------------------------------------------------
RANDOM_SEEDS = tuple(range(8))
RANDOM_OPS = 40


def random_sequence(seed, length=RANDOM_OPS):
    """`length` ops from all of the above after a first reset: step drivers of 1..40 steps (a few of
    0), resets with 2-4 players, max_steps 8-40 and every difficulty, reset_default, invalidations,
    hazard clears, and stretches with auto-reset off."""
    rng = np.random.default_rng(9000 + seed)

    trio_family = tuple(d for d in STEP_DRIVERS if d[0] == "T")
    drivers = STEP_DRIVERS + trio_family                     # (the carried trio state: twice the weight)

    def reset():
        players = (2, 3, 3, 4, 4)[int(rng.integers(0, 5))]
        return ("X", 500 + 37 * seed + int(rng.integers(0, 1000)), players, 3, int(rng.integers(0, 3)),
                int(rng.integers(8, 41)))
    seq = [reset()]
    off = False
    while len(seq) < length:
        u = rng.random()
        if u < 0.70:
            d = drivers[int(rng.integers(0, len(drivers)))]
            steps = 0 if rng.random() < 0.05 else int(rng.integers(1, 41))
            seq.append((d, steps))
        elif u < 0.80:
            seq.append(reset())
        elif u < 0.85:
            seq.append("X0")
        elif u < 0.90:
            seq.append("I")
        elif u < 0.94:
            seq.append("C")
        else:
            off = not off
            seq.append("A0" if off else "A1")
    return seq


def for_shards(seq):
    """The sequence for a handle of several shards: D and G (single-shard by contract) become H, and an
    M op takes env.step (step_device and the sampler's device actions are one device pointer each)."""
    seq = [("M", "step") + tuple(op[2:]) if not isinstance(op, str) and op[0] == "M" else op for op in seq]
    return [("H", op[1]) if not isinstance(op, str) and op[0] in SINGLE_SHARD_ONLY else op for op in seq]
