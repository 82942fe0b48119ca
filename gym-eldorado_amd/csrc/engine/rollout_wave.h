// engine/rollout_wave.h -- the persistent rollout, one wave per 64 envs: LaneLds, the park codes and list,
// OutRing, DeckImage, rollout_pass, k_env_rollout, k_env_rollout_pipe.
// A part of cog_engine.hip, included there inside namespace cog where this text used to stand; not
// meant to be compiled or included alone.
// Needs, defined before it in cog_engine.hip: the PH / STAMP macros, Heads / MBits and the sampler, RegEnv
// and step_regs, and the lane drivers (Snap, the store phase, step_action, end_of_step_a / _b).
// k_env_fixup, after the parts in cog_engine.hip, runs its rollout_pass.
// ------------------------------------------------------------------------------------------
// Persistent rollout: K x (sample; step) per launch (the runner's device loop, runner.h:46-55).
// Every step stores its outputs exactly as a single-step launch does (the HBM state after each
// step is the reference's); what changes is where the next step reads its inputs from: the
// env-level records stay in VGPRs and every player's records (deck, counters, neighbourhood
// cache, stored mask) in this wave's LDS, so a step issues no global loads unless it resets.
template <int NL>                     // NL: envs (lanes) per workgroup
struct LaneLds {
  uint4 deck[4][7][NL];               // [player][granule][lane]: lane-contiguous, conflict-free
  uint4 pl[4][NL];
  uint2 cells[4][NL];
  uint4 heads[4][NL];                 // stored masks (MBits + pad)
  UidEntry tab[kUidTab];              // the uniform's division table
};
template <class LaneLds>
DEV void lds_fill_players(LaneLds &L, const DevState &s, size_t i, int l) {
  const uint4 *pv4 = reinterpret_cast<const uint4 *>(s.priv + i);
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const uint4 *dk = reinterpret_cast<const uint4 *>(deck_ptr(s, i, p));
#pragma unroll
    for (int k = 0; k < 7; k++) L.deck[p][k][l] = dk[k];
    L.pl[p][l] = pv4[4 + p];
    L.cells[p][l] = reinterpret_cast<const uint2 *>(pv4 + 8)[p];
    L.heads[p][l] = s.heads[5 * i + 1 + p];
  }
}
// The wave's player records are stored cooperatively at the end of a launch: consecutive
// work-items take consecutive 16-B granules of one env's records (its counters and neighbourhood
// caches are EnvPriv granules 4..9, its stored-mask bit vectors 4 consecutive heads), so one
// store instruction covers a few contiguous runs instead of 64 envs' scattered granules.
// Measured (profiles/r02_b_fixedcost.txt): the per-work-item store cost 6.2 us per launch at
// 65,536 envs, this one about 1 us.  The same transposition for the launch's loads was slower (19.7 against
// 9.5 us): those stay one env per work-item (lds_fill_players).  ne = the wave's envs; a
// work-item past the end of a ragged last wave stores env ne - 1's records again.
template <class LaneLds, int NL>
DEV void lds_store_wave(const LaneLds &L, const DevState &s, size_t base, int ne) {
  const int l = threadIdx.x;                               // (past the end: env ne - 1's records again)
#pragma unroll
  for (int j = 0; j < 4 * NL / 64; j++) {
    const int f = j * 64 + l, e = min(f >> 2, ne - 1), q = f & 3;
    reinterpret_cast<uint4 *>(s.priv + base + e)[4 + q] = L.pl[q][e];
  }
#pragma unroll
  for (int j = 0; j < 2 * NL / 64; j++) {
    const int f = j * 64 + l, e = min(f >> 1, ne - 1), q = f & 1;
    const uint2 a = L.cells[2 * q][e], b = L.cells[2 * q + 1][e];
    reinterpret_cast<uint4 *>(s.priv + base + e)[8 + q] = make_uint4(a.x, a.y, b.x, b.y);
  }
#pragma unroll
  for (int j = 0; j < 4 * NL / 64; j++) {
    const int f = j * 64 + l, e = min(f >> 2, ne - 1), p = f & 3;
    s.heads[5 * (base + e) + 1 + p] = L.heads[p][e];
  }
}
// the env-level private records of env i (EnvPriv granules 0, 1, 3, the selected mask's bits)
DEV void store_env_private(const DevState &s, size_t i, const Snap &S) {
  uint4 *pw = reinterpret_cast<uint4 *>(s.priv + i);
  pw[0] = S.g0;
  pw[1] = S.g1;
  reinterpret_cast<uint32_t *>(pw + 3)[0] = S.info_steps;
  s.heads[5 * i] = mbits_u4(S.sel);
}
// every private record of env i (EnvPriv granules 0, 1, 3, all players, all mask bit vectors)
// from the rollout's on-chip copies
template <class LaneLds>
DEV void store_private_all(const DevState &s, size_t i, const Snap &S, const LaneLds &L, int l) {
  uint4 *pw = reinterpret_cast<uint4 *>(s.priv + i);
  pw[0] = S.g0;
  pw[1] = S.g1;
  reinterpret_cast<uint32_t *>(pw + 3)[0] = S.info_steps;
  s.heads[5 * i] = mbits_u4(S.sel);
#pragma unroll
  for (int p = 0; p < 4; p++) {
    pw[4 + p] = L.pl[p][l];
    reinterpret_cast<uint2 *>(pw + 8)[p] = L.cells[p][l];
    s.heads[5 * i + 1 + p] = L.heads[p][l];
  }
}
template <class LaneLds>
DEV void lds_players(const LaneLds &L, int l, int ag, int na, Snap &S) {
  S.pla = L.pl[ag][l];
  S.pln = L.pl[na][l];
  S.ca = L.cells[ag][l];
  S.cn = L.cells[na][l];
  S.sta = mbits_of(L.heads[ag][l]);
  S.stn = mbits_of(L.heads[na][l]);
#pragma unroll
  for (int k = 0; k < 7; k++) S.dk[k] = L.deck[ag][k][l];
}

// The rollout is one kernel in two passes.  The lean pass (FIX = false) carries no episode-end
// code: a lane whose env finishes (or starts done) at step t stores its state, keeps t (its
// "park" code) and leaves the loop; the other lanes go on.  After the loop, a wave with a parked
// lane runs the fix-up pass (FIX = true, a wave-uniform branch) for exactly those lanes: it
// completes step t's episode end (finish_episode, dones, auto-reset, encode) and runs the env's
// remaining steps with the full step (resets included).  Nothing reads the env in between and
// envs are independent (no barrier between the reference's workers either, runner.h:39-62), so
// the outputs are those of one full-step loop; the lean loop keeps the reset path's registers
// out of its allocation.  A wave with nothing parked ends after the lean pass (round 1 launched
// the fix-up as a second kernel: 4.8 us per launch even when it had nothing to do).
// park codes: bits 0..29 the step t; kParkFinish: step t finished the episode (else the env
// started step t done); kParkRedo: step t was not run (the trio's stepping wave met an action
// outside its lean step, lean_player in trio_stepper) -- the fix-up runs it with the full step
constexpr uint32_t kParkNone = ~0u, kParkFinish = 1u << 31, kParkRedo = 1u << 30;
constexpr uint32_t kParkStep = kParkRedo - 1u;
// The records of a wave's envs seen from the wave's first env: a per-wave (scalar) base and a
// per-lane index below 64, so that record addresses are a scalar base plus a 32-bit lane offset
// (the saddr form of global loads and stores) instead of 64-bit products of a global index,
// which the compiler rematerialises at every store under the kernel's register pressure.
DEV DevState wave_view(const DevState &s, size_t base) {
  DevState v = s;
  v.obs += base * COG_OBS_BYTES;
  v.sel += base * COG_MASK_BYTES;
  v.info += base * COG_INFO_BYTES;
  v.rew += base * 4;
  v.done += base;
  v.agent += base;
  v.priv += base;
  v.grid += base * (size_t)kGridBytes;
  v.cgrid += base * COG_CELLS;
  v.heads += 5 * base;
  v.cdeck += 10 * base;
  v.cwide += base;
  v.gen += base;
  v.park += base;
  v.first += base;
  v.n = s.n > base ? s.n - base : 0;
  return v;
}
// a duo / trio workgroup with a parked env appends its index to the launch's parked list (one
// atomic per such wave), so that k_env_fixup visits only those (DevState::parkq)
DEV void park_list_push(const DevState &s_glob, bool parked) {
  if (__builtin_amdgcn_ballot_w64(parked) && (threadIdx.x & 63) == 0) {
    if (s_glob.no_fixup) {                                 // the host showed no park could happen
      atomicOr(&s_glob.status[0], F_PARK_NOFIX);
      atomicAdd(&s_glob.status[1], 1u);
      *s_glob.err = 1u;
    }
    const uint32_t j = atomicAdd(&s_glob.parkq[s_glob.park_par], 1u);
    s_glob.parkq[2 + j] = blockIdx.x;
  }
}
// the other counter back to 0 for the next launch (the previous launch's fix-up, which read it,
// has completed: same stream)
DEV void park_list_clear_other(const DevState &s_glob) {
  if (blockIdx.x == 0 && threadIdx.x == 0) s_glob.parkq[s_glob.park_par ^ 1u] = 0u;
}
// Two-wave rollout for small shards (k_env_rollout_pipe): the stepping wave hands each step's
// outputs to a second wave of its workgroup through a double-buffered LDS ring, and the second
// wave finds what changed and issues the store phase (mask expansions and the granule stores)
// while the first runs the next step.  One record per lane and step, [buffer][granule][lane]:
//   0-2   ObsData 16128.. (phase, resources, shop) after the step, 3-5 before it
//   6-12  the acting player's DeckObs after the step
//   13    selected-mask bits after, .w = flags: 28 valid, 29 moved, 30 next player != acting
//         player (the storing wave keeps every player's deck as last stored, DeckImage)
//   14    acting player's stored-mask bits after, .w = ag | na << 8 | Info steps byte << 16
//   15    next player's stored-mask bits after
//   16-18 the three mask bit vectors before the step (9 dwords), then the action (8 bytes)
//   19    EnvPriv granule 2 (locations) when moved
constexpr int kOutG = 20;
struct OutRing {
  uint4 g[2][kOutG][64];
};
DEV void out_record_write(OutRing &O, int b, int l, int ag, int na, const Snap &S, const RegEnv &R,
                          const uint8_t act[5]) {
  const uint32_t gm = 1u << 28 | (R.moved ? 1u << 29 : 0u) | (na != ag ? 1u << 30 : 0u);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    O.g[b][k][l] = make_uint4(R.sh[4 * k], R.sh[4 * k + 1], R.sh[4 * k + 2], R.sh[4 * k + 3]);
    O.g[b][3 + k][l] = S.sh[k];
  }
#pragma unroll
  for (int k = 0; k < 7; k++) O.g[b][6 + k][l] = make_uint4(R.d[4 * k], R.d[4 * k + 1], R.d[4 * k + 2], R.d[4 * k + 3]);
  const MBits bs = bits_of(R.sel), ba = bits_of(R.sta), bn = bits_of(R.stn);
  O.g[b][13][l] = make_uint4(bs.w0, bs.w1, bs.w2, gm);
  O.g[b][14][l] = make_uint4(ba.w0, ba.w1, ba.w2,
                             (uint32_t)ag | (uint32_t)na << 8 | ((R.info_steps >> (8 * ag)) & 0xffu) << 16);
  O.g[b][15][l] = make_uint4(bn.w0, bn.w1, bn.w2, 0u);
  O.g[b][16][l] = make_uint4(S.sel.w0, S.sel.w1, S.sel.w2, S.sta.w0);
  O.g[b][17][l] = make_uint4(S.sta.w1, S.sta.w2, S.stn.w0, S.stn.w1);
  O.g[b][18][l] = make_uint4(S.stn.w2,
                             (uint32_t)act[0] | (uint32_t)act[1] << 8 | (uint32_t)act[2] << 16 | (uint32_t)act[3] << 24,
                             (uint32_t)act[4], 0u);
  O.g[b][19][l] = R.g2;
}
DEV uint4 sel4(bool c, const uint4 &a, const uint4 &b) {
  return make_uint4(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w);
}
// the storing wave's copy of every player's DeckObs as it stands in HBM (loaded at the start of
// the launch, then updated by its own stores): the previous value of the acting player's deck
struct DeckImage {
  uint4 d[4][7];
};
DEV void deck_image_load(DeckImage &I, const DevState &s, size_t i) {
#pragma unroll
  for (int p = 0; p < 4; p++) {
    const uint4 *dk = reinterpret_cast<const uint4 *>(deck_ptr(s, i, p));
#pragma unroll
    for (int k = 0; k < 7; k++) I.d[p][k] = dk[k];
  }
}
// the storing wave: exactly the stores store_outputs + store_action issue, in the same order
DEV void out_record_store(const OutRing &O, int b, int l, const DevState &s, size_t i, uint8_t *actions_out,
                          DeckImage &I) {
  const uint4 m = O.g[b][13][l];
  const uint32_t gm = m.w;
  if (!((gm >> 28) & 1u)) return;
  const uint4 x = O.g[b][14][l], o0 = O.g[b][16][l], o1 = O.g[b][17][l], o2 = O.g[b][18][l];
  const int ag = (int)(x.w & 0xffu), na = (int)((x.w >> 8) & 0xffu);
  uint8_t *ob = s.obs + i * COG_OBS_BYTES;
  s.info[i * COG_INFO_BYTES + COG_AGENT_INFO0 + COG_AGENT_INFO_STRIDE * ag] = (uint8_t)(x.w >> 16);
  if ((gm >> 29) & 1u) reinterpret_cast<uint4 *>(s.priv + i)[2] = O.g[b][19][l];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const uint4 v = O.g[b][k][l];
    if (ne4(v, O.g[b][3 + k][l])) reinterpret_cast<uint4 *>(ob + COG_OBS_PHASE)[k] = v;
  }
  uint8_t *deck = deck_ptr(s, i, ag);
#pragma unroll
  for (int k = 0; k < 7; k++) {
    const uint4 v = O.g[b][6 + k][l];
    uint4 old = I.d[3][k];                                 // (selects: a register array indexed
#pragma unroll                                             // by a lane value would go to scratch)
    for (int p = 2; p >= 0; p--) old = sel4(ag == p, I.d[p][k], old);
    if (ne4(v, old)) reinterpret_cast<uint4 *>(deck)[k] = v;
#pragma unroll
    for (int p = 0; p < 4; p++) I.d[p][k] = sel4(ag == p, v, I.d[p][k]);
  }
  const MBits bs{m.x, m.y, m.z}, ba{x.x, x.y, x.z};
  store_mask_record(reinterpret_cast<uint4 *>(s.sel + i * COG_MASK_BYTES), bs,
                    mask_diff_granules(bs, MBits{o0.x, o0.y, o0.z}));
  store_mask_record(reinterpret_cast<uint4 *>(deck + COG_PD_MASK), ba, mask_diff_granules(ba, MBits{o0.w, o1.x, o1.y}));
  if ((gm >> 30) & 1u) {
    const uint4 y = O.g[b][15][l];
    const MBits bn{y.x, y.y, y.z};
    store_mask_record(reinterpret_cast<uint4 *>(deck_ptr(s, i, na) + COG_PD_MASK), bn,
                      mask_diff_granules(bn, MBits{o1.z, o1.w, o2.x}));
  }
  reinterpret_cast<uint2 *>(actions_out + i * COG_ACTION_BYTES)[0] = make_uint2(o2.y, o2.z);
}

// wbase_in: the wave's first env (k_env_fixup: a parked workgroup's); default blockIdx.x * NL
template <int SRC, bool FIX, int NL, bool PIPE = false>
DEV uint32_t rollout_pass(LaneLds<NL> &L, const DevState &s_glob, int steps, uint32_t *__restrict__ rngs_glob,
                          uint8_t *__restrict__ actions_glob, uint32_t park, OutRing *O = nullptr,
                          size_t wbase_in = ~(size_t)0) {
  const int l = threadIdx.x;                               // (the stepping wave: threads 0..NL-1)
  const size_t wbase = wbase_in != ~(size_t)0 ? wbase_in : (size_t)blockIdx.x * NL;
  const size_t i0 = wbase + l;
  // (s, i): the wave's view and the lane's index in it, for every record access; the wave's
  // generation, its encode and the regenerated-map list take the shard's (s_glob, i_glob)
  const DevState s = wave_view(s_glob, wbase);
  const size_t i = (size_t)l;
  const size_t i_glob = i0 < s_glob.n ? i0 : 0;
  uint32_t *__restrict__ rngs = rngs_glob + wbase;
  uint8_t *__restrict__ actions_out = actions_glob + wbase * COG_ACTION_BYTES;
  int t_first = 0;                                         // fix-up: this lane's first full step
  bool live = i0 < s_glob.n && (!FIX || park != kParkNone);
  Snap S;
  uint32_t srng = 0, out = ~0u;                           // out: end_of_step's output cache
  auto next_of = [&](int a) { return a + 1 >= (int)(S.g1.x & 0xffu) ? 0 : a + 1; };   // n_players
  if (live) {
    load_env(s, i, S);
    lds_fill_players(L, s, i, l);
    srng = rngs[i];
  }

  if (FIX) {                                               // step `park`'s episode end
    bool enc = false, rs = false;
    uint32_t agent = 0;
    if (live && (park & kParkRedo)) {                      // step `park` itself was not run
      t_first = (int)(park & kParkStep);
    } else if (live) {
      t_first = (int)(park & kParkStep) + 1;
      agent = S.g1.y & 0xffu;
      const bool finish = (park & kParkFinish) != 0u;
      rs = end_of_step_a(s, i, !finish, finish, agent, out);
    }
    const bool ok = wave_generate(s_glob, i_glob, rs);               // converged: the whole wave generates
    if (live) {
      if (rs) enc = end_of_step_b(s_glob, i_glob, ok, agent, out);
      load_env(s, i, S);                                   // reset: reload from the stored state
      lds_fill_players(L, s, i, l);
    }
    wave_encode(s_glob, i_glob, enc);                                // converged: the whole wave encodes
  }
  if (live) {
    const int ag = (int)(S.g1.y & 0xffu);
    lds_players(L, l, ag, next_of(ag), S);
  }
  // Every load above completes before the loop: the loop issues no load whose wait could be
  // merged with them, so the wait-count pass places no per-iteration vmcnt wait for registers
  // they wrote (such a wait, executed every step, would also wait for the step's stores).
  __builtin_amdgcn_s_waitcnt(0);
  if (PIPE && !FIX) __syncthreads();                       // the decks in LDS: the storing wave's image
  PH_DECL;
  for (int t = 0; t < steps; t++) {
    if (PIPE) {                                            // every lane, every step: the records
      if (t) __syncthreads();                              // of step t - 1 to the storing wave
      if (!live) O->g[t & 1][13][l] = make_uint4(0u, 0u, 0u, 0u);   // (no record)
    }
    if (!FIX && !PIPE && !live) break;                     // lean: a parked lane leaves the loop
    bool enc = false, ended = false, rs = false;
    uint32_t agent = 0;
    if (live && t >= t_first) {
      RegEnv R;
      regs_env(R, S);
      R.tab = L.tab;
      const int ag = (int)R.agent();                       // S holds ag's and na's records: read
      const int na = ag + 1 >= (int)R.n_players() ? 0 : ag + 1;   // at the end of the last step
      uint8_t act[5];
      PH(0);
      if (SRC == MASK_SELECTED) step_action<SRC>(R, make_uint2(0u, 0u), srng, act);
      regs_players(R, S);
      if (SRC == MASK_STORED) step_action<SRC>(R, make_uint2(0u, 0u), srng, act);
      PH(1);
      const bool was_done = R.done() != 0u;
      const bool finish = !was_done && step_regs(R, act, s, i, na PH_PASS);
      if (finish) R.set_done(1u);
      PH(2);
      // the player records to this wave's LDS, and the next step's players back, before the
      // store phase: the LDS round trip overlaps the stores instead of stalling the loop's tail
      L.pl[ag][l] = pack_player(R.P);
      L.cells[ag][l] = R.cells_a;
      L.heads[ag][l] = mbits_u4(bits_of(R.sta));
      if (na != ag) L.heads[na][l] = mbits_u4(bits_of(R.stn));
#pragma unroll
      for (int k = 0; k < 7; k++) L.deck[ag][k][l] = make_uint4(R.d[4 * k], R.d[4 * k + 1], R.d[4 * k + 2], R.d[4 * k + 3]);
      agent = R.agent();
      Snap N;                                              // the next step's player records
      lds_players(L, l, (int)agent, next_of((int)agent), N);
      PH(3);
      if (PIPE) {
        out_record_write(*O, t & 1, l, ag, na, S, R, act);
      } else {
        store_outputs(s, i, ag, na, S, R);
        store_action(actions_out + i * COG_ACTION_BYTES, act);
      }
      PH(4);
      // the next step's image: registers (env level) and the player records just read
      S.g0 = make_uint4(R.rng, R.seed, R.max_steps, R.turn_counter);
      S.g1 = make_uint4(R.g1x, R.g1y, R.in_market, R.flags);
      S.g2 = R.g2;
      S.avail = R.avail;
      S.info_steps = R.info_steps;
#pragma unroll
      for (int k = 0; k < 3; k++) S.sh[k] = make_uint4(R.sh[4 * k], R.sh[4 * k + 1], R.sh[4 * k + 2], R.sh[4 * k + 3]);
      S.sel = bits_of(R.sel);
      S.pla = N.pla; S.pln = N.pln; S.ca = N.ca; S.cn = N.cn; S.sta = N.sta; S.stn = N.stn;
#pragma unroll
      for (int k = 0; k < 7; k++) S.dk[k] = N.dk[k];
      if (was_done || finish) {                            // episode end: state to HBM first
        store_private_all(s, i, S, L, l);
        if (!FIX) {                                        // hand the env to the fix-up pass
          rngs[i] = srng;
          park = (uint32_t)t | (finish ? kParkFinish : 0u);
          live = false;
          continue;
        }
        ended = true;
        rs = end_of_step_a(s, i, was_done, finish, agent, out);
      } else {
        end_of_step_a(s, i, false, false, agent, out);
      }
      PH(5);
    }
    if (FIX) {                                             // converged: the whole wave generates
      const bool ok = wave_generate(s_glob, i_glob, rs);
      if (ended) {
        if (rs) enc = end_of_step_b(s_glob, i_glob, ok, agent, out);
        load_env(s, i, S);                                 // reload from the stored state
        lds_fill_players(L, s, i, l);
        agent = S.g1.y & 0xffu;
        lds_players(L, l, (int)agent, next_of((int)agent), S);
      }
      wave_encode(s_glob, i_glob, enc);                              // converged: the whole wave encodes
    }
    PH(6);
  }
  if (PIPE && steps > 0) __syncthreads();                 // the last step's records
  if (live) {                                              // env-level private state back to HBM
    store_env_private(s, i, S);                            // (the player records: lds_store_wave)
    rngs[i] = srng;
  }
  if (!FIX) PH_FLUSH(s);
  return FIX ? kParkNone : park;
}

template <int SRC, int NL>
__global__ void __launch_bounds__(NL) k_env_rollout(DevState s, int steps, uint32_t *__restrict__ rngs,
                                                    uint8_t *__restrict__ actions_out) {
  __shared__ LaneLds<NL> L;
  const size_t base = (size_t)blockIdx.x * NL;
  const int ne = (int)min((size_t)NL, s.n - base);
  uid_tab_fill(L.tab);
  const uint32_t park = rollout_pass<SRC, false, NL>(L, s, steps, rngs, actions_out, kParkNone);
  if (__builtin_amdgcn_ballot_w64(park != kParkNone))    // (wave-uniform)
    rollout_pass<SRC, true, NL>(L, s, steps, rngs, actions_out, park);
  __syncthreads();
  lds_store_wave<LaneLds<NL>, NL>(L, s, base, ne);
}

// Shards of <= 32,768 envs leave SIMDs idle (one 64-env wave per SIMD at most): each workgroup
// gets a second wave for its store phase (OutRing above).  Barriers: one at the start, one per
// step (the stepping wave hands over step t - 1 at the top of step t, the last step after its
// loop), one when the storing wave's stores have completed, one before the epilogue.  The fix-up
// pass (episode ends, resets) then runs on the stepping wave alone with the plain store phase,
// after an L1 invalidate, since it reloads records the storing wave wrote.
template <int SRC>
__global__ void __launch_bounds__(128) k_env_rollout_pipe(DevState s, int steps, uint32_t *__restrict__ rngs,
                                                          uint8_t *__restrict__ actions_out) {
  __shared__ LaneLds<64> L;
  __shared__ OutRing O;
  const size_t base = (size_t)blockIdx.x * 64;
  const int ne = (int)min((size_t)64, s.n - base);
  // (roles rotated per workgroup, so that a CU's two workgroups could not put both stepping waves
  // on one SIMD, measured the same: profiles/r04y_trio_role_rotation.txt)
  const int role = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform
  uid_tab_fill(L.tab);
  uint32_t park = kParkNone;
  if (role == 0) {
    park = rollout_pass<SRC, false, 64, true>(L, s, steps, rngs, actions_out, kParkNone, &O);
    __syncthreads();                                       // the storing wave's stores are done
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");     // (drop L1 lines they replaced)
    if (__builtin_amdgcn_ballot_w64(park != kParkNone))    // (wave-uniform)
      rollout_pass<SRC, true, 64>(L, s, steps, rngs, actions_out, park);
  } else {
    const int l = (int)threadIdx.x - 64;
    const DevState v = wave_view(s, base);
    uint8_t *av = actions_out + base * COG_ACTION_BYTES;
    DeckImage I;
    __syncthreads();                                       // the stepping wave's fill is in LDS: the
    if (l < ne) {                                          // image from there, not a second read of
#pragma unroll                                             // every deck from memory
      for (int p = 0; p < 4; p++)
#pragma unroll
        for (int k = 0; k < 7; k++) I.d[p][k] = L.deck[p][k][l];
    }
    for (int t = 0; t < steps; t++) {
      __syncthreads();
      if (l < ne) out_record_store(O, t & 1, l, v, (size_t)l, av, I);
    }
    __builtin_amdgcn_s_waitcnt(0);                         // every store of this wave completed
    __syncthreads();
  }
  __syncthreads();
  if (role == 0) lds_store_wave<LaneLds<64>, 64>(L, s, base, ne);
}
