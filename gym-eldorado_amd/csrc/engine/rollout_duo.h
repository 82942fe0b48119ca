// engine/rollout_duo.h -- the duo rollout: DuoLds, the meta bits, duo_stepper, duo_turn_end, duo_storer,
// k_env_rollout_duo.
// A part of cog_engine.hip, included there inside namespace cog where this text used to stand; not
// meant to be compiled or included alone.
// Needs what engine/rollout_wave.h needs, and from it the park codes and list (park_list_push,
// park_list_clear_other), DeckImage and deck_image_load, lds_store_wave, wave_view and sel4.
// ------------------------------------------------------------------------------------------
// Duo rollout (round 3): two waves per 64-env workgroup -- a stepping wave and a storing wave --
// sized so that FOUR workgroups share a CU (32,000 B of LDS each, <= 256 VGPRs + AGPRs per
// work-item), i.e. two waves per SIMD at 65,536 envs.  A lone wave issues at most one
// instruction per quad-cycle; the SIMD's VALU takes one per two cycles, so the storing wave of
// one workgroup runs beside the stepping wave of another on the same SIMD, and the stepping wave
// runs only the game logic.
//
// Ownership.  The stepping wave keeps the env in registers (RegEnv, across steps: no per-step
// image repacking) and every player's counters, neighbourhood cache and stored-mask bits in LDS
// (`pl`, `cells`, `heads`).  The storing wave keeps every player's DeckObs as last stored
// (DeckImage, registers) and the "before" images the store phase compares with: the shared
// block (phase, resources, shop), the selected-mask bits and each player's stored-mask bits.
// Per step the stepping wave hands over only after-values through a single-buffered LDS ring
// (`ring`, 14 granules per env), and the storing wave hands back the deck of the player who
// acts after a turn change (`slot`: the next player's deck as of the step's start -- only the
// acting player's deck changes within a step).
//
// Before the loop, barrier B: the storing wave has loaded every player's deck (its image) and
// hands the acting player's to the stepping wave through the ring's deck buffer 1, so the stepping
// wave's prologue is one round of loads (no dependent read of the deck the agent selects).
// Per step t, two barriers (both waves execute them):
//   stepping wave: step t on registers; pl/cells/heads of the acting player to LDS;
//                  X_t; record t to the ring; on a turn change the next player's records from
//                  LDS and its deck from the slot; Y_t
//   storing wave:  (X_0 after its prologue) Y_t; record t from the ring into registers; update
//                  its images; the slot for step t + 1; X_{t+1}; the stores of record t
// The storing wave reaches X long before the stepping wave ends its step, and the stepping wave
// reaches Y long after the storing wave's stores were issued, so neither barrier stalls the
// stepping wave beyond its own issue.
//
// Episode ends (and envs that start a launch done) park as in k_env_rollout's lean pass: the
// lane stores its private state, records its park code in DevState::park and leaves the loop;
// k_env_fixup, launched right after on the same stream, completes them.  The fix-up's register
// appetite (map generation, the full step) therefore does not cap this kernel's occupancy.
constexpr int kRingG = 7, kSlotG = 7;
struct DuoLds {
  uint4 pl[4][64];                    // [player][lane]: PlayerPriv (packed)
  uint2 cells[4][64];                 // neighbourhood caches
  uint4 heads[4][64];                 // stored-mask bits (MBits + pad)
  uint4 ring[kRingG][64];             // step record, stepping wave -> storing wave
  uint4 deckr[2][7][64];              // the record's DeckObs, double-buffered (written before X)
  uint4 slot[kSlotG][64];             // next player's DeckObs, storing wave -> stepping wave
  UidEntry tab[kUidTab];
};
static_assert(sizeof(DuoLds) <= 40960, "four duo workgroups per CU");
// step record t: deckr[t & 1] = the acting player's DeckObs after the step, and ring granules
//   0-2   ObsData 16128..16175 (phase, resources, shop) after the step
//   3     selected-mask bits; .w = meta (below)
//   4     the acting player's stored-mask bits; .w = action bytes 0..3
//   5     the next player's stored-mask bits; .w = action byte 4
//   6     EnvPriv granule 2 (map bounds + locations), read when the acting player moved
// meta: bit 0 valid, 1 moved, 2-3 ag, 4-5 na, 6-7 na1 (the player after the next step's
// acting player), 8-15 Info steps byte of ag, 16 the episode ended (parked: dones / agent are
// left to the fix-up), 24-31 agent after the step
constexpr uint32_t kMetaValid = 1u, kMetaMoved = 2u, kMetaEnded = 1u << 16;
constexpr uint32_t kMetaStepped = 1u << 17;               // (trio) the step ran: the env was not done

DEV uint32_t next_player(uint32_t a, uint32_t np) { return a + 1u >= np ? 0u : a + 1u; }

// The env-level private records of env i from the stepping wave's registers (EnvPriv granules
// 0, 1, 3, the selected mask's bits).  The player records (counters, neighbourhood caches,
// stored-mask bits) are stored from the wave's LDS by the epilogue (lds_store_wave), parked envs'
// included, after the last update of them.  DEFER (the trio): the env rng is the drawing wave's
// (it stores it at its end), so granule 0's first dword is left alone.
template <bool DEFER>
DEV void duo_store_env_private(const DevState &s, size_t i, const RegEnv &R) {
  uint4 *pw = reinterpret_cast<uint4 *>(s.priv + i);
  if (DEFER) reinterpret_cast<uint3 *>(reinterpret_cast<uint32_t *>(pw) + 1)[0] = make_uint3(R.seed, R.max_steps, R.turn_counter);
  else pw[0] = make_uint4(R.rng, R.seed, R.max_steps, R.turn_counter);
  pw[1] = make_uint4(R.g1x, R.g1y, R.in_market, R.flags);
  reinterpret_cast<uint32_t *>(pw + 3)[0] = R.info_steps;
  s.heads[5 * i] = mbits_u4(bits_of(R.sel));
}

// The deferred turn end (the trio rollout: selected masks, >= 3 players).  The stepping wave ends
// a turn without touching the deck -- no discard, no draws -- and the drawing wave completes it
// from the step record (the acting player's deck after the step, its counters in `pl`, the saved
// mask) with the env rng, which it owns: Player::end_turn's discard + draw (player.cpp:170-180),
// then the saved mask gains the drawn cards (draw's mask updates, cards.cpp:183-211, precede
// save_actionmask).  Nothing the stepping wave reads before that player acts again depends on it:
// with >= 3 players the next two agents are other players, whose turn ends lie at least two steps
// back.  Any action outside the lean step (lean_player: never in the canonical loop) parks
// the env with kParkRedo, and k_env_fixup runs that step and the rest with the full step.

template <int SRC>
DEV void duo_stepper(DuoLds &D, const DevState &s_glob, int steps, uint32_t *__restrict__ rngs_glob) {
  const int l = threadIdx.x;
  const size_t wbase = (size_t)blockIdx.x * 64;
  const DevState s = wave_view(s_glob, wbase);
  const size_t i = (size_t)l;
  const int ne = (int)min((size_t)64, s_glob.n - wbase);
  uint32_t *__restrict__ rngs = rngs_glob + wbase;
  bool live = l < ne;
  uint32_t park = kParkNone, srng = 0;
  RegEnv R;
  int ag = 0, na = 0;
  if (live) {
    Snap S;
    load_env(s, i, S);
    regs_env(R, S);
    const uint4 *pv4 = reinterpret_cast<const uint4 *>(s.priv + i);
#pragma unroll
    for (int p = 0; p < 4; p++) {
      D.pl[p][l] = pv4[4 + p];
      D.cells[p][l] = reinterpret_cast<const uint2 *>(pv4 + 8)[p];
      D.heads[p][l] = s.heads[5 * i + 1 + p];
    }
    srng = rngs[i];
    ag = (int)R.agent();
    na = (int)next_player((uint32_t)ag, R.n_players());
    R.P = unpack_player(D.pl[ag][l]);
    R.na_active = (D.pl[na][l].y >> 16) & 0xffu;
    R.cells_a = D.cells[ag][l];
    R.cells_n = D.cells[na][l];
    R.sta = heads_of(mbits_of(D.heads[ag][l]));
    R.stn = heads_of(mbits_of(D.heads[na][l]));
  }
  R.tab = D.tab;
  // every load above completes before the loop (no per-iteration vmcnt wait covers them)
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();                                         // B: the storing wave loaded every deck;
  if (live) {                                              // the acting player's from its hand-over
#pragma unroll                                             // (no second, dependent read of memory)
    for (int k = 0; k < 7; k++) {
      const uint4 v = D.deckr[1][k][l];
      R.d[4 * k] = v.x; R.d[4 * k + 1] = v.y; R.d[4 * k + 2] = v.z; R.d[4 * k + 3] = v.w;
    }
  }
  PH_DECL;
  for (int t = 0; t < steps; t++) {
    bool ended = false, finish = false;
    uint8_t act[5];
    if (live) {
      step_action<SRC>(R, make_uint2(0u, 0u), srng, act);
      const bool was_done = R.done() != 0u;
      finish = !was_done && step_regs(R, act, s, i, na PH_PASS);
      if (finish) R.set_done(1u);
      ended = was_done || finish;
      PH(0);
      D.pl[ag][l] = pack_player(R.P);
      D.cells[ag][l] = R.cells_a;
      D.heads[ag][l] = mbits_u4(bits_of(R.sta));
      if (na != ag) D.heads[na][l] = mbits_u4(bits_of(R.stn));
#pragma unroll
      for (int k = 0; k < 7; k++)                          // (buffer t & 1: record t - 2's, taken)
        D.deckr[t & 1][k][l] = make_uint4(R.d[4 * k], R.d[4 * k + 1], R.d[4 * k + 2], R.d[4 * k + 3]);
      PH(1);
    }
    __syncthreads();                                       // X_t: record t - 1 taken, slot written
    PH(2);
    if (live) {
      const int ag1 = (int)R.agent();
      const int na1 = (int)next_player((uint32_t)ag1, R.n_players());
      const MBits bs = bits_of(R.sel), ba = bits_of(R.sta), bn = bits_of(R.stn);
      const uint32_t info = (R.info_steps >> (8 * ag)) & 0xffu;
      const uint32_t meta = kMetaValid | (R.moved ? kMetaMoved : 0u) | (uint32_t)ag << 2 | (uint32_t)na << 4 |
                            (uint32_t)na1 << 6 | info << 8 | (ended ? kMetaEnded : 0u) | (uint32_t)ag1 << 24;
#pragma unroll
      for (int k = 0; k < 3; k++) D.ring[k][l] = make_uint4(R.sh[4 * k], R.sh[4 * k + 1], R.sh[4 * k + 2], R.sh[4 * k + 3]);
      D.ring[3][l] = make_uint4(bs.w0, bs.w1, bs.w2, meta);
      D.ring[4][l] = make_uint4(ba.w0, ba.w1, ba.w2,
                                (uint32_t)act[0] | (uint32_t)act[1] << 8 | (uint32_t)act[2] << 16 | (uint32_t)act[3] << 24);
      D.ring[5][l] = make_uint4(bn.w0, bn.w1, bn.w2, (uint32_t)act[4]);
      D.ring[6][l] = R.g2;
      R.moved = false;
      if (ag1 != ag) {                                     // turn change: ag1 == na acts next
#pragma unroll
        for (int k = 0; k < 7; k++) {
          const uint4 v = D.slot[k][l];
          R.d[4 * k] = v.x; R.d[4 * k + 1] = v.y; R.d[4 * k + 2] = v.z; R.d[4 * k + 3] = v.w;
        }
        R.P = unpack_player(D.pl[ag1][l]);
        R.cells_a = R.cells_n;
        R.sta = R.stn;
        R.stn = heads_of(mbits_of(D.heads[na1][l]));
        R.cells_n = D.cells[na1][l];
        R.na_active = (D.pl[na1][l].y >> 16) & 0xffu;
      }
      if (ended) {                                         // hand the env to k_env_fixup
        duo_store_env_private<false>(s, i, R);
        rngs[i] = srng;
        park = (uint32_t)t | (finish ? kParkFinish : 0u);
        live = false;
      }
      ag = ag1;
      na = na1;
    } else {
      D.ring[3][l] = make_uint4(0u, 0u, 0u, 0u);           // no record
    }
    PH(3);
    __syncthreads();                                       // Y_t: record t in the ring
    PH(4);
  }
  __syncthreads();                                         // X_steps
  PH_FLUSH(s_glob);
  if (live) {                                              // env-level private state back to HBM
    duo_store_env_private<false>(s, i, R);
    rngs[i] = srng;
  }
  if (l < ne) s.park[i] = park;
  park_list_push(s_glob, park != kParkNone);
  lds_store_wave<DuoLds, 64>(D, s, 0, ne);                 // every player's records (cooperative)
}

DEV uint4 sel4_of(const DeckImage &I, int p, int k) {      // I.d[p][k] for a lane-varying p
  uint4 v = I.d[3][k];
#pragma unroll
  for (int q = 2; q >= 0; q--) v = sel4(p == q, I.d[q][k], v);
  return v;
}
DEV MBits selm(const MBits b[4], int p) {
  MBits v = b[3];
#pragma unroll
  for (int q = 2; q >= 0; q--) {
    v.w0 = p == q ? b[q].w0 : v.w0;
    v.w1 = p == q ? b[q].w1 : v.w1;
    v.w2 = p == q ? b[q].w2 : v.w2;
  }
  return v;
}
DEV void setm(MBits b[4], int p, const MBits &v) {
#pragma unroll
  for (int q = 0; q < 4; q++) {
    b[q].w0 = p == q ? v.w0 : b[q].w0;
    b[q].w1 = p == q ? v.w1 : b[q].w1;
    b[q].w2 = p == q ? v.w2 : b[q].w2;
  }
}

// DEFER: the turn end of record t's acting player ag (meta: ag1 != ag), on the drawing wave --
// Player::end_turn's discard + draw on the deck as the step left it, with the env rng; the saved
// mask gains the drawn cards; the player's counters and stored-mask bits go back to the LDS
// records the stepping wave reads when ag acts again.
template <class Lds>
DEV void duo_turn_end(Lds &D, int l, int ag, uint4 dk[7], MBits &ba, uint32_t &rng, uint32_t &flags) {
  RegEnv E;
#pragma unroll
  for (int k = 0; k < 7; k++) {
    E.d[4 * k] = dk[k].x; E.d[4 * k + 1] = dk[k].y; E.d[4 * k + 2] = dk[k].z; E.d[4 * k + 3] = dk[k].w;
  }
  E.P = unpack_player(D.pl[ag][l]);
  E.rng = rng;
  E.sel = heads_of(ba);
  E.flags = 0u;
  E.tab = D.tab;
  E.end_turn_deck();
#pragma unroll
  for (int k = 0; k < 7; k++) dk[k] = make_uint4(E.d[4 * k], E.d[4 * k + 1], E.d[4 * k + 2], E.d[4 * k + 3]);
  ba = bits_of(E.sel);
  rng = E.rng;
  D.pl[ag][l] = pack_player(E.P);
  D.heads[ag][l] = mbits_u4(ba);
  flags |= E.flags;
}

DEV void duo_storer(DuoLds &D, const DevState &s_glob, int steps, uint8_t *__restrict__ actions_glob) {
  const int l = (int)threadIdx.x - 64;
  const size_t wbase = (size_t)blockIdx.x * 64;
  const DevState s = wave_view(s_glob, wbase);
  const size_t i = (size_t)l;
  const bool live = wbase + (size_t)l < s_glob.n;
  uint8_t *__restrict__ av = actions_glob + wbase * COG_ACTION_BYTES;
  DeckImage I;
  uint4 shb[3];
  MBits selb = {0u, 0u, 0u}, stb[4];
  uint32_t out = ~0u;                                      // dones[i] | agent_selection[i] << 8 as stored
  if (live) {
    deck_image_load(I, s, i);
    const uint4 *sh4 = reinterpret_cast<const uint4 *>(s.obs + i * COG_OBS_BYTES + COG_OBS_PHASE);
#pragma unroll
    for (int k = 0; k < 3; k++) shb[k] = sh4[k];
    selb = mbits_of(s.heads[5 * i]);
#pragma unroll
    for (int p = 0; p < 4; p++) stb[p] = mbits_of(s.heads[5 * i + 1 + p]);
    const uint4 g1 = reinterpret_cast<const uint4 *>(s.priv + i)[1];
    const int ag0 = (int)(g1.y & 0xffu), na0 = (int)next_player(g1.y & 0xffu, g1.x & 0xffu);
#pragma unroll
    for (int k = 0; k < 7; k++) {
      D.slot[k][l] = sel4_of(I, na0, k);
      D.deckr[1][k][l] = sel4_of(I, ag0, k);               // (buffer 1 is first written at step 1)
    }
  }
  __syncthreads();                                         // B: the acting player's deck handed over
  __syncthreads();                                         // X_0
  PH_DECL;
  for (int t = 0; t < steps; t++) {
    __syncthreads();                                       // Y_t
    PH(5);
    uint4 g[kRingG], dk[7];
#pragma unroll
    for (int k = 0; k < kRingG; k++) g[k] = D.ring[k][l];
#pragma unroll
    for (int k = 0; k < 7; k++) dk[k] = D.deckr[t & 1][k][l];
    const uint32_t meta = g[3].w;
    const bool rec = live && (meta & kMetaValid);
    const int ag = (int)((meta >> 2) & 3u), na = (int)((meta >> 4) & 3u), na1 = (int)((meta >> 6) & 3u);
    if (rec) {
      uint32_t dm = 0;                                     // deck granules that changed
#pragma unroll
      for (int k = 0; k < 7; k++) {
        if (ne4(dk[k], sel4_of(I, ag, k))) dm |= 1u << k;
#pragma unroll
        for (int p = 0; p < 4; p++) I.d[p][k] = sel4(ag == p, dk[k], I.d[p][k]);
      }
#pragma unroll
      for (int k = 0; k < 7; k++) D.slot[k][l] = sel4_of(I, na1, k);
      PH(6);
      uint8_t *ob = s.obs + i * COG_OBS_BYTES;
      s.info[i * COG_INFO_BYTES + COG_AGENT_INFO0 + COG_AGENT_INFO_STRIDE * ag] = (uint8_t)(meta >> 8);
      if (meta & kMetaMoved) reinterpret_cast<uint4 *>(s.priv + i)[2] = g[6];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        if (ne4(g[k], shb[k])) reinterpret_cast<uint4 *>(ob + COG_OBS_PHASE)[k] = g[k];
        shb[k] = g[k];
      }
      uint8_t *deck = deck_ptr(s, i, ag);
#pragma unroll
      for (int k = 0; k < 7; k++)
        if ((dm >> k) & 1u) reinterpret_cast<uint4 *>(deck)[k] = dk[k];
      const MBits bs{g[3].x, g[3].y, g[3].z}, ba{g[4].x, g[4].y, g[4].z};
      store_mask_record(reinterpret_cast<uint4 *>(s.sel + i * COG_MASK_BYTES), bs, mask_diff_granules(bs, selb));
      selb = bs;
      store_mask_record(reinterpret_cast<uint4 *>(deck + COG_PD_MASK), ba, mask_diff_granules(ba, selm(stb, ag)));
      setm(stb, ag, ba);
      if (na != ag) {
        const MBits bn{g[5].x, g[5].y, g[5].z};
        store_mask_record(reinterpret_cast<uint4 *>(deck_ptr(s, i, na) + COG_PD_MASK), bn,
                          mask_diff_granules(bn, selm(stb, na)));
        setm(stb, na, bn);
      }
      reinterpret_cast<uint2 *>(av + i * COG_ACTION_BYTES)[0] = make_uint2(g[4].w, g[5].w);
      if (!(meta & kMetaEnded)) {                          // dones[i] = 0, agent_selection[i]
        const uint32_t agent = meta >> 24;                 // (an ended episode: k_env_fixup)
        if (out & 0xffu) s.done[i] = 0;
        if (((out >> 8) & 0xffu) != agent) s.agent[i] = (uint8_t)agent;
        out = agent << 8;
      }
    }
    PH(13);
    __syncthreads();                                       // X_{t+1}
    PH(7);
  }
  PH_FLUSH(s_glob);
}

template <int SRC>
__global__ void __launch_bounds__(128) k_env_rollout_duo(DevState s, int steps, uint32_t *__restrict__ rngs,
                                                         uint8_t *__restrict__ actions_out) {
  __shared__ DuoLds D;
  // (roles rotated per workgroup, so that a CU's two workgroups could not put both stepping waves
  // on one SIMD, measured the same: profiles/r04y_trio_role_rotation.txt)
  const int role = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform
  park_list_clear_other(s);
  uid_tab_fill(D.tab);
  if (role == 0) {
    __builtin_amdgcn_s_setprio(3);                         // the stepping wave wins VALU issue on
                                                           // a SIMD it shares with a storing wave
    duo_stepper<SRC>(D, s, steps, rngs);
  } else {
    duo_storer(D, s, steps, actions_out);
  }
}
