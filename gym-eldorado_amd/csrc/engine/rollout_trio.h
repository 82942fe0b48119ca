// engine/rollout_trio.h -- the trio rollout: TrioLds and its progress counters, the stepping wave's lean
// image and the compact deck, trio_stepper, trio_drawer, trio_storer, k_env_rollout_trio.
// A part of cog_engine.hip, included there inside namespace cog where this text used to stand; not
// meant to be compiled or included alone.  Needs, defined before it in cog_engine.hip: the PH / STAMP
// macros, Heads / MBits and the sampler, RegEnv and the card tables of the register-resident step,
// Snap / deck_ptr / store_mask_record of the lane drivers; from engine/rollout_wave.h the park codes and
// list and DeckImage; from engine/rollout_duo.h the duo's meta bits and store helpers.  k_env_fixup and
// the host launchers after it use its compact deck.
// ------------------------------------------------------------------------------------------
// Trio rollout (round 4): the selected-mask loop with >= 3 players at every shard size (cog_rollout_kind),
// one step's work spread over four waves per 64 envs.  The stepping wave runs the lean step
// (the lean step: sample, play or pass, turn change, done check) and nothing else; the drawing wave
// owns the decks (replays each play on its copy, runs the turn ends' discard + draws with the env
// rng); two storing waves issue the store phase, one of them also producing the sampler's
// presampled draws (presample).  History (8,192 envs, device us per step in 1,000-step launches,
// profiles/r04*_trio*.txt): the duo 2.45; its storing wave doing the draws 3.17 (it set the pace,
// profiles/r04d_duo_defer.txt); the draws on a third wave 1.96; lean step, hand-only stepping
// wave, presampled draws and two storing waves, in barrier lockstep 1.80 (the drawing wave's turn
// ends set the pace); turn ends batched over two records, still in lockstep, 1.86 (a two-record
// round is as long as the two it replaces); decoupled through progress counters (below).
//
// The waves run as a pipeline over LDS buffers, synchronised by progress counters in LDS (cnt[],
// stored after the records they publish -- in-order LDS, cnt_store; a waiting wave sleeps between
// polls) instead of barriers, so each runs at its own average rate:
//   stepping wave  step t: ring slot t % 8 free (record t - 8 stored by both storing waves), step
//                  t's presampled draws written (cnt[PRE] > t - 4); step; record t -> ring,
//                  cnt[REC] = t + 1; at a turn change, the drawing wave past the last turn ends of
//                  the new agent (its hand, counters) and of the player after it (its stored mask,
//                  hand nibbles) -- the later of the two is 1 (3 players) or 2 (4 players) turn
//                  ends back (te1, te2); with >= 3 players and turns of >= 2 steps those lie >= 2
//                  steps back.
//   drawing wave   records r, r + 1 (r even) once written: the plays replayed on the acting players'
//                  decks (img: two byte updates each), then ONE turn-end pass -- a lean turn lasts at least two steps (pass
//                  in MOVEMENT, pass in BUYING), so a player ends at most one turn in two records --
//                  and the deck granules each record changed (ring granule 2, bits 16..22);
//                  cnt[DRAW] = r + 2
//   storing wave B record r once written: step r + 4's presampled draws (cnt[PRE] = r + 1), the
//                  selected mask, Info, action, dones / agent_selection; on a second cursor
//                  kTrioBLag records behind, once drawn, the changed deck granules straight from img -- a granule a later record changed again may
//                  already hold that later value (or be read mid-update), but that record stores
//                  it again, in order, so the last store of every granule is its final value;
//                  cnt[STB] = r + 1
//   storing wave A record r once drawn: ObsData, the stored masks; cnt[STA] = r + 1
// The waits form no cycle: every wait of the stepping wave needs only records it has published.
// A wait that outlasts kTrioSpinLimit polls (a bug, never a slow wave) sets F_SYNC_TIMEOUT, the
// host error word and a sticky abort counter that ends every wait of the workgroup, so that no
// fault can hang the GPU.
//
// record t: 0 ObsData 16128.. (the phase dword from the stepping wave; the resources from the
// drawing wave; the lean step never changes the shop), 1 selected-mask bits + meta, 2 the acting
// player's stored-mask bits (saved mask at a turn end: the drawing wave adds the drawn cards) +
// action byte 0 + n_active of the acting player << 8 (the drawing wave's in the LAT form) + the deck
// granules the record changed << 16 (drawing wave).  The next player's stored mask changes only at a
// turn end, by fixed heads (the lean step), so storing wave A derives it from its own image.  The
// neighbourhood caches never change in the lean step (no moves): the stepping wave and storing wave
// A keep their own copies, and the epilogue does not store them.  The acting player's counters: the
// stepping wave's, written to LDS at a turn end (for the drawing wave) and at a park or the end (for
// the epilogue); in the LAT form the drawing wave's alone.
constexpr int kTrioRingG = 3;
constexpr int kTrioDepth = 8;                              // ring slots (records in flight)
                                                           // (16 measured the same: profiles/r05i_trio_depth16.txt, r05_trio_ab.txt r05z7)
constexpr int kTrioLead = 4;                               // presampled draws: steps ahead of the record
constexpr int kTrioBLag = 2;                               // storing wave B: deck cursor behind its front
// CNT_ABORT: set (sticky) by the first progress wait that times out; every later wait of every
// wave returns at once, so a broken invariant ends the launch promptly with the error set
// (instead of one ~0.2 s timeout per remaining wait)
enum TrioCnt : int { CNT_REC = 0, CNT_DRAW, CNT_STA, CNT_STB, CNT_PRE, CNT_FIN, CNT_ABORT, kTrioCnts };
constexpr uint32_t kTrioSpinLimit = 1u << 21;             // polls (~0.2 s)
struct TrioLds {
  uint2 img[4][5][64];                // every player's compact DeckObs (the drawing wave's): piles of types 0-7
  uint4 ring[kTrioDepth][kTrioRingG][64];   // record t (above), slot t % kTrioDepth
  uint32_t srng[kTrioDepth][64];      // the sampler state after step t, slot t % kTrioDepth
  uint3 pre[kTrioLead][64];           // step t's presampled draws, t % 4: state, head 0's draw | risk << 31, state after
  uint4 pl[4][64];
  uint4 heads[4][64];
  uint4 stbA[4][64];                  // storing wave A: every player's stored mask as last stored (bits)
  uint32_t wide[64];                  // the env's deck holds a type >= 8 (the drawing wave's prologue)
  uint32_t flg[64];                   // the other waves' hazard flags (the stepping wave's epilogue)
  uint32_t cnt[kTrioCnts];            // progress counters
  UidEntry tab[kUidTab];
};
static_assert(sizeof(TrioLds) <= 54613, "three trio workgroups per CU (trio_pad_lds keeps two)");
static_assert((kTrioDepth & (kTrioDepth - 1)) == 0 && kTrioDepth >= 4, "ring slots: a power of two");

// A wave keeps the counters it last read (wave-uniform, in SGPRs) and reads them again -- all six
// in one round trip -- only when the one it needs is short: the counters only grow, and what an
// acquire read once made visible stays so.  A waiting wave sleeps between reads.
struct TrioCnt6 {
  uint32_t rec = 0, draw = 0, sta = 0, stb = 0, pre = 0, fin = 0, abort = 0;
};
DEV void cnt_read(const TrioLds &D, TrioCnt6 &c) {
  uint32_t v[kTrioCnts];
#pragma unroll
  for (int k = 0; k < kTrioCnts; k++) v[k] = __hip_atomic_load(&D.cnt[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  c.rec = __builtin_amdgcn_readfirstlane(v[CNT_REC]);
  c.draw = __builtin_amdgcn_readfirstlane(v[CNT_DRAW]);
  c.sta = __builtin_amdgcn_readfirstlane(v[CNT_STA]);
  c.stb = __builtin_amdgcn_readfirstlane(v[CNT_STB]);
  c.pre = __builtin_amdgcn_readfirstlane(v[CNT_PRE]);
  c.fin = __builtin_amdgcn_readfirstlane(v[CNT_FIN]);
  c.abort = __builtin_amdgcn_readfirstlane(v[CNT_ABORT]);
}
// Publishes this wave's earlier LDS writes, all lanes' included, through lane 0's store of the
// counter.  The LDS executes one wave's DS instructions in issue order (their lgkmcnt returns are
// in order), so a wave that reads the counter's new value and then the records reads what was
// written before it: the ordering that matters is the compiler's, which a wavefront-scope fence
// keeps (no instruction).  A workgroup-scope release would add an s_waitcnt lgkmcnt(0) on the
// stepping wave's path every step, waiting also for its own reads in flight ($COG_TRIO_FENCE
// builds, -DCOG_TRIO_FENCE, keep that form for A/B).
DEV void cnt_store(TrioLds &D, int k, uint32_t v) {
#ifdef COG_TRIO_FENCE
  if ((threadIdx.x & 63) == 0) __hip_atomic_store(&D.cnt[k], v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  if ((threadIdx.x & 63) == 0) __hip_atomic_store(&D.cnt[k], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#endif
}
// wait (wave-uniform) until counter `field` of c (a member of c) >= v
#ifdef COG_ISSUE_COUNT
// (diagnostic ISA builds, tools/issue_frac.py: the no-wait path alone -- what a step issues when
// the counter it needs is already there; the waits are the stamps' own phases)
DEV void cnt_wait(TrioLds &, TrioCnt6 &, const uint32_t &field, uint32_t v, const DevState &) {
  if (field < v) asm volatile("s_nop 0");
}
#else
DEV void cnt_wait(TrioLds &D, TrioCnt6 &c, const uint32_t &field, uint32_t v, const DevState &s) {
  // (the common case first, alone: one scalar compare and branch -- the sticky abort matters only
  // to a wave that would wait)
  if (__builtin_expect(field >= v, 1)) return;
  if (c.abort) return;
  for (uint32_t spins = 0;; spins++) {
    cnt_read(D, c);
    if (field >= v || c.abort) return;
    if (spins >= kTrioSpinLimit) {
      if ((threadIdx.x & 63) == 0) {
        atomicOr(&s.status[0], F_SYNC_TIMEOUT);
        atomicAdd(&s.status[1], 1u);
        *s.err = 1u;
        __hip_atomic_store(&D.cnt[CNT_ABORT], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      c.abort = 1u;
      return;
    }
    __builtin_amdgcn_s_sleep(2);                           // (1 or 0: the same, r05y2)
  }
}
#endif
// the stepping wave's presampled record: {the state the step starts from, head 0's index for every
// play-head size k = 2..9 (4 bits each: uid_tab_accepted of the first draw, the narrow hand's play
// head holds at most the pass bit and types 0-7), the state after the five draws | any draw could be
// rejected << 31} -- the divisions off the stepping wave's chain (storing wave B has the slack)
DEV uint3 pre_pack(const uint4 p, bool jtab) {
  if (!jtab) return make_uint3(p.x, p.y, p.z | p.w << 31);   // head 0's draw itself
  uint32_t jt = 0u;
#pragma unroll
  for (int k = 2; k <= 9; k++) {
    const UidEntry e = uid_entry((uint32_t)k);
    jt |= uid_tab_accepted(p.y, e.s, e.m) << (4 * (k - 2));
  }
  return make_uint3(p.x, jt, p.z | p.w << 31);
}

// the epilogue's player records (lds_store_wave without the neighbourhood caches)
DEV void trio_store_players(const TrioLds &D, const DevState &s, int ne) {
  const int l = (int)(threadIdx.x & 63);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int f = j * 64 + l, e = min(f >> 2, ne - 1), q = f & 3;
    reinterpret_cast<uint4 *>(s.priv + e)[4 + q] = D.pl[q][e];
    s.heads[5 * e + 1 + q] = D.heads[q][e];
  }
}

// ---- the stepping wave's lean image and the compact deck (round 5) ----------------------------
// Decks in LDS hold types 0-7 only ("narrow": the canonical loop's decks never hold another type --
// no purchases, no specials -- DeckObs piles draw / hand / active / played / discard, 8 counts
// each, a uint2 per pile): 160 B per env instead of 448, so that four workgroups fit a CU's LDS and
// the metric's 65,536 envs step in one round.  An env whose deck holds a type >= 8 (compact_of
// says wide) is parked at step 0 and run by k_env_fixup's full step.  The acting player's hand is
// the stepping wave's copy of its compact hand pile (two dwords of u8 counts).
// DeckObs byte offset of pile p (api.h:67-82): 21 p
DEV void deck_expand(const uint2 pile[5], uint4 dk[7]) {   // compact -> the record's 7 granules
  uint32_t d[28];
#pragma unroll
  for (int k = 0; k < 28; k++) d[k] = 0u;
#pragma unroll
  for (int p = 0; p < 5; p++) {
    const int b = 21 * p, q = b >> 2, sh = b & 3;          // compile-time
    const uint32_t lo = pile[p].x, hi = pile[p].y;
    if (sh == 0) {
      d[q] |= lo;
      d[q + 1] |= hi;
    } else {
      d[q] |= lo << (8 * sh);
      d[q + 1] |= __builtin_amdgcn_alignbyte(hi, lo, 4 - sh);
      d[q + 2] |= hi >> (8 * (4 - sh));
    }
  }
#pragma unroll
  for (int k = 0; k < 7; k++) dk[k] = make_uint4(d[4 * k], d[4 * k + 1], d[4 * k + 2], d[4 * k + 3]);
}
// the record's granules -> compact piles; false: a count of a type >= 8 is non-zero (wide)
DEV bool compact_of(const uint4 dk[7], uint2 pile[5]) {
  uint32_t d[28];
#pragma unroll
  for (int k = 0; k < 7; k++) { d[4 * k] = dk[k].x; d[4 * k + 1] = dk[k].y; d[4 * k + 2] = dk[k].z; d[4 * k + 3] = dk[k].w; }
  uint32_t rest = 0u;                                      // every byte of types 8..20: one
#pragma unroll                                             // compile-time byte mask per dword
  for (int k = 0; k < 28; k++) {
    uint32_t m = 0u;
#pragma unroll
    for (int y = 4 * k; y < 4 * k + 4; y++)
      if (y < 105 && y % 21 >= 8) m |= 0xffu << (8 * (y & 3));
    if (m) rest |= d[k] & m;
  }
#pragma unroll
  for (int p = 0; p < 5; p++) {
    const int b = 21 * p, q = b >> 2, sh = b & 3;
    pile[p].x = sh ? __builtin_amdgcn_alignbyte(d[q + 1], d[q], sh) : d[q];
    pile[p].y = sh ? __builtin_amdgcn_alignbyte(d[q + 2], d[q + 1], sh) : d[q + 1];
  }
  return rest == 0u;
}
// card c (< 8) leaves the compact hand (Deck::activate's hand part, player.cpp:45-60,
// cards.cpp:242-253: hand[c] - 1, u8): the count before
DEV uint32_t hand_take(uint2 &h, int c) {
  const uint32_t sh = 8u * (uint32_t)(c & 3);
  const uint32_t w = c < 4 ? h.x : h.y;
  const uint32_t prev = (w >> sh) & 0xffu;
  const uint32_t nw = (w & ~(0xffu << sh)) | (((prev - 1u) & 0xffu) << sh);
  h.x = c < 4 ? nw : h.x;
  h.y = c < 4 ? h.y : nw;
  return prev;
}
// the selected mask's heads 1-4 are {0} (special, remove, move, shop: MBits bits 22.., w1, w2)
DEV bool heads14_zero(const MBits &b) { return (b.w0 >> 22) == 1u && b.w1 == (1u << 12) && b.w2 == 0x204u; }
constexpr uint32_t kMoveShopBits = (0x7fu << 2) | (0x7ffffu << 9);   // MBits w2: move and shop heads
// the j-th set bit of m (j < popc(m)): clear the lowest set bit j times, as many rounds as the
// wave's largest j (the play head holds the pass bit and the hand's types: j <= 3 in the canonical
// loop, where the binary search of nth_set_bit costs five full rounds)
DEV uint32_t nth_set_bit_iter(uint32_t m, uint32_t j) {
  while (__builtin_amdgcn_ballot_w64(j != 0u)) {
    m = j ? (m & (m - 1u)) : m;
    j = j ? j - 1u : 0u;
  }
  return (uint32_t)(__ffs(m) - 1);
}
// head 0's draw from the presampled record when the state is the one it starts from and heads
// 1-4 are {0} (then the five draws are the presampled ones: act 1-4 = 0); false: sample the
// sequential way
DEV bool sample_lean(const MBits &sel, const uint3 &pr, uint32_t &rng, uint32_t &a0, bool jtab, const UidEntry *tab) {
  const uint32_t m0 = sel.w0 & 0x3fffffu, k0 = __popc(m0);
  if (!(pr.x == rng && (pr.z >> 31) == 0u && heads14_zero(sel) && k0 >= 1u && k0 <= 9u)) return false;
  uint32_t j;
  if (jtab) {
    j = k0 >= 2u ? (pr.y >> (4u * (k0 - 2u))) & 15u : 0u;
  } else {
    const UidEntry e0 = tab[k0];
    j = k0 >= 2u ? uid_tab_accepted(pr.y, e0.s, e0.m) : 0u;
  }
  a0 = nth_set_bit_iter(m0, j);
  rng = pr.z;
  return true;
}
DEV uint4 pack_lean_player(uint4 pp, uint32_t n_in_hand, uint32_t n_active, uint32_t steps_taken) {
  pp.y = (pp.y & 0xff0000ffu) | (n_in_hand & 0xffu) << 8 | (n_active & 0xffu) << 16;
  pp.z = (pp.z & 0xffff00ffu) | (steps_taken & 0xffu) << 8;
  return pp;
}
// the lean step may run for this player: no move, free card, free move or pending removes in
// progress, has not won (PlayerPriv x: has_won, mip, n_removes, next_card_free; y byte 0:
// next_move_free)
DEV bool lean_player(const uint4 &pp) { return (pp.x | (pp.y & 0xffu)) == 0u; }
// the env-level private records from the stepping wave (duo_store_env_private<true> with the
// selected mask as bits)
DEV void trio_store_private(const DevState &s, size_t i, const RegEnv &R, const MBits &selb) {
  uint4 *pw = reinterpret_cast<uint4 *>(s.priv + i);
  reinterpret_cast<uint3 *>(reinterpret_cast<uint32_t *>(pw) + 1)[0] = make_uint3(R.seed, R.max_steps, R.turn_counter);
  pw[1] = make_uint4(R.g1x, R.g1y, R.in_market, R.flags);
  s.heads[5 * i] = mbits_u4(selb);                         // (Info steps: the drawing wave's)
}

template <int SRC, bool LAT>
DEV void trio_stepper(TrioLds &D, const DevState &s_glob, int steps, int epw, uint32_t *__restrict__ rngs_glob) {
  const int l = (int)(threadIdx.x & 63);
  const size_t wbase = (size_t)blockIdx.x * epw;
  const DevState s = wave_view(s_glob, wbase);
  const size_t i = (size_t)l;
  const int ne = (int)min((size_t)epw, s_glob.n - wbase);
  uint32_t *__restrict__ rngs = rngs_glob + wbase;
  bool live = l < ne;
  uint32_t park = kParkNone, srng = 0;
  PH_DECL;                                                 // (diagnostic builds: phase stamps)
  TL(10);                                                  // (and the launch timeline: slots 10..14)
  RegEnv R;                                                // env level (the lean image below)
  uint2 cells[4];                                          // every player's neighbourhood cache
  // the steps of the last two turn ends before the current step (-1: none in this launch); the
  // lean loop passes the turn strictly in order, so the last turn end of the player after the next
  // agent -- the later of the two records the turn change reads -- lies 1 (3 players) or 2 (4
  // players) turn ends back
  int te1 = -1, te2 = -1;
  int ag = 0, na = 0;
  MBits selb = {0u, 0u, 0u}, stab = selb, stnb = selb;     // selected, stored(ag), stored(na)
  // The acting player's counters (steps_taken, n_in_hand, n_active, idx_last) are kept by this
  // wave and handed to the drawing wave at turn changes when two workgroups share a CU (their
  // total work per CU counts), and by the drawing wave alone when a workgroup has its CU to
  // itself (LAT: the stepping wave's chain counts): profiles/r05_trio_ab.txt r05z3 / r05z5
  constexpr bool lat = LAT;
  uint4 pp = make_uint4(0u, 0u, 0u, 0u);                   // PlayerPriv of ag (packed)
  uint32_t n_in_hand = 0u, n_active = 0u, steps_taken = 0u;
  uint32_t own = 0u;                                       // each player's own hex code (a byte each)
  if (live) {
    Snap S;
    load_env(s, i, S);
    regs_env(R, S);
    const uint4 *pv4 = reinterpret_cast<const uint4 *>(s.priv + i);
#pragma unroll
    for (int p = 0; p < 4; p++) {
      D.pl[p][l] = pv4[4 + p];
      cells[p] = reinterpret_cast<const uint2 *>(pv4 + 8)[p];
      D.heads[p][l] = s.heads[5 * i + 1 + p];
    }
    srng = rngs[i];
    ag = (int)R.agent();
    na = (int)next_player((uint32_t)ag, R.n_players());
    pp = D.pl[ag][l];
    n_in_hand = (pp.y >> 8) & 0xffu;
    n_active = (pp.y >> 16) & 0xffu;
    steps_taken = (pp.z >> 8) & 0xffu;
#pragma unroll
    for (int p = 0; p < 4; p++) own |= (cells[p].x & 0xffu) << (8 * p);   // (neighbourhood cell 0)
    selb = S.sel;
    stab = mbits_of(D.heads[ag][l]);
    stnb = mbits_of(D.heads[na][l]);
  }
  R.tab = D.tab;
  __builtin_amdgcn_s_waitcnt(0);                           // (no per-iteration vmcnt wait covers them)
  TL(15);                                                  // (timeline: this wave's prologue done)
  __syncthreads();                                         // B: every wave's prologue is done
  uint2 H = make_uint2(0u, 0u);                            // ag's hand (compact: types 0-7)
  bool lean_p = false, narrow = false;
  if (live) {                                              // from the drawing wave's image
    H = D.img[ag][1][l];
    narrow = D.wide[l] == 0u;
    lean_p = narrow && lean_player(pp);
  }
  PH(6);                                                   // the prologue (to the barrier)
  TL(11);
  TrioCnt6 cc;
  // step t + 1's presampled record, read at the end of step t when storing wave B is known to be
  // past it (so that the read's latency overlaps the record's stores); else at step t + 1's start
  uint3 pr_next = D.pre[0][l];
  bool have_next = true;
  // the next turn change's records read ahead (pf_ok: valid)
  uint2 pf_hd = make_uint2(0u, 0u);
  uint4 pf_pla = make_uint4(0u, 0u, 0u, 0u), pf_hdn = pf_pla;
  bool pf_ok = false;
  for (int t = 0; t < steps; t++) {
    const int sl = t & (kTrioDepth - 1);
    if (t >= kTrioDepth) {                                 // slot t % kTrioDepth free
      cnt_wait(D, cc, cc.sta, (uint32_t)(t - kTrioDepth + 1), s_glob);
      cnt_wait(D, cc, cc.stb, (uint32_t)(t - kTrioDepth + 1), s_glob);
    }
    PH(9);
    if (!have_next) cnt_wait(D, cc, cc.pre, (uint32_t)(t - kTrioLead + 1), s_glob);   // (t >= kTrioLead)
    PH(2);
    bool ended = false, finish = false, turn_end = false, stepped = false;
    uint32_t a_play = 0u;
    // (round 6: the common path computed by every lane with selects -- no exec-mask branches, which
    // a 64-env wave would take on nearly every step anyway; the rare parts keep their branches)
    {
      const uint32_t srng0 = srng;
      uint3 pr = pr_next;                                  // (have_next is wave-uniform: a scalar
      if (!have_next) pr = D.pre[t & (kTrioLead - 1)][l];  // branch, not a select of addresses)
      // head 0's draw from the presampled record when the state is the one it starts from and heads
      // 1-4 are {0} (then the five draws are the presampled ones: act 1-4 = 0; sample_lean)
      const uint32_t m0 = selb.w0 & 0x3fffffu, k0 = __popc(m0);
      const bool fast = live && pr.x == srng && (pr.z >> 31) == 0u && heads14_zero(selb) && k0 - 1u < 9u;
      uint32_t j;
      if (LAT) {
        j = (pr.y >> (4u * ((k0 - 2u) & 7u))) & 15u;      // (head 0's index table, k0 = 2..9)
      } else {
        const UidEntry e0 = R.tab[k0 & (kUidTab - 1)];
        j = uid_tab_accepted(pr.y, e0.s, e0.m);
      }
      j = fast && k0 >= 2u ? j : 0u;
      const uint32_t a0 = nth_set_bit_iter(m0, j);
      a_play = fast ? a0 : 0u;
      srng = fast ? pr.z : srng;
      bool other = false;                                  // an action head other than play set
      if (__builtin_amdgcn_ballot_w64(live && !fast) && live && !fast) {   // (wave-uniform skip)
#ifdef COG_ISSUE_COUNT                                     // (diagnostic ISA builds, tools/issue_frac.py:
        other = true;                                      // the rare fallback's code out of the count)
#else
        uint8_t act[5];
        R.sel = heads_of(selb);
        step_action<SRC>(R, make_uint2(0u, 0u), srng, act);
        a_play = act[0];
        other = ((uint32_t)act[1] | act[2] | act[3] | act[4]) != 0u;
#endif
      }
      other = other || a_play > 8u;                        // (a type >= 8: not in a narrow deck's hand)
      const bool was_done = R.done() != 0u;
      // not the lean step's case (never in the canonical loop), or the test hooks: hand the env to
      // k_env_fixup before its step t
      bool hook = false;                                   // (test hooks: t uniform, so a scalar
      if (t == s.redo_at) hook = s.redo_env < 0 || (int)(wbase + i) == s.redo_env;   // branch in the loop)
      const bool parks = live && !was_done && (!lean_p || other || hook);
      stepped = live && !was_done && !parks;               // cog_env::step, the lean case (Info steps
      if (__builtin_amdgcn_ballot_w64(parks) && parks) {   // and the resources: the drawing wave's)
        srng = srng0;
#ifndef COG_ISSUE_COUNT                                    // (a rare lane's stores: out of the count)
        trio_store_private(s, i, R, selb);
        rngs[i] = srng;
#endif
        if (!lat) D.pl[ag][l] = pack_lean_player(pp, n_in_hand, n_active, steps_taken);   // (the epilogue's)
        park = (uint32_t)t | kParkRedo;
        live = false;
      }
      uint32_t phase = R.sh[0] & 0xffu;
      if (phase == COG_PHASE_INACTIVE) phase = COG_PHASE_MOVEMENT;
      if (!lat) steps_taken = stepped ? (steps_taken + 1u) & 0xffu : steps_taken;
      // Player::play_card (player.cpp:45-60): Deck::activate's hand part (the active pile and the
      // counters: the drawing wave); the play bit (its special bit stays clear: types 0-7 are not
      // special, is_special; a type >= 8 has parked above)
      const bool play = stepped && a_play != 0u;
      const int c = (int)((a_play - 1u) & 7u);
      uint2 Hp = H;
      const uint32_t prev = hand_take(Hp, c);
      H = play ? Hp : H;
      const uint32_t bp = 1u << (c + 1);
      selb.w0 = play ? (prev > 1u ? (selb.w0 | bp) : (selb.w0 & ~bp)) : selb.w0;
      if (!lat) {
        n_in_hand = play ? (n_in_hand - 1u) & 0xffu : n_in_hand;
        n_active = play ? (n_active + 1u) & 0xffu : n_active;
        pp.z = play ? (pp.z & ~0xffu) | (uint32_t)c : pp.z;   // idx_last
      }
      const uint32_t nph = phase == COG_PHASE_BUYING ? COG_PHASE_INACTIVE : phase + 1u;   // pass: next phase
      phase = stepped && !play ? nph : phase;
      turn_end = stepped && phase == COG_PHASE_INACTIVE;   // maybe_end_turn -> next_agent
      // (Player::end_turn: the drawing wave) save_actionmask, load_actionmask (na != ag: >= 3
      // players), update_observation's INACTIVE phase for the next player's stored mask
      n_active = turn_end ? 0u : n_active;
      const MBits sel0 = selb;
      selb.w0 = turn_end ? stnb.w0 : selb.w0;
      selb.w1 = turn_end ? stnb.w1 : selb.w1;
      selb.w2 = turn_end ? stnb.w2 : selb.w2;
      stab.w0 = turn_end ? sel0.w0 : stab.w0;
      stab.w1 = turn_end ? sel0.w1 : stab.w1;
      stab.w2 = turn_end ? sel0.w2 : stab.w2;
      stnb.w2 = turn_end ? (stnb.w2 & ~kMoveShopBits) | 0x204u : stnb.w2;
      R.g1y = turn_end ? (R.g1y & ~0xffu) | ((uint32_t)na & 0xffu) : R.g1y;   // R.set_agent(na)
      R.turn_counter += turn_end ? 1u : 0u;
      R.sh[0] = stepped ? (R.sh[0] & ~0xffu) | phase : R.sh[0];
      // done (environment.cpp:183-207): the (next) agent's cell or the turn counter.  Both change
      // only with the turn here (no move: the agent's cell is the one checked after its last step,
      // never an end; a player's own cell is never an out-of-bounds lookup; max_steps >= 1, which
      // the host guarantees -- at 0 the first step after a reset ends the episode, cog_abi.cpp trio_ok)
      finish = turn_end && (COG_HEX_END((own >> (8 * na)) & 0xffu) || R.turn_counter >= R.max_steps);
      R.g1x = finish ? (R.g1x & 0x00ffffffu) | (1u << 24) : R.g1x;   // R.set_done(1)
      PH(0);
      ended = live && (was_done || finish);
    }
    uint4(*ring)[64] = D.ring[sl];
    int ag1 = ag, na1 = na;
    if (live) {
      ag1 = (int)R.agent();
      na1 = (int)next_player((uint32_t)ag1, R.n_players());
    }
    const bool tc = live && ag1 != ag;                     // turn change: ag1 == na acts next
    // the new agent's records (hand, counters) and the next player's (stored mask), once the
    // drawing wave is past their last turn ends; read ahead of the record's stores, so that their
    // latency overlaps them
    // (read ahead at an earlier step of the turn when the drawing wave was past them: pf_ok)
    // (the records land in pf_* themselves: the turn change below takes them from there, and
    // re-reads ahead after it -- no copies of ten dwords through every step)
    const bool slow = tc && !pf_ok;
    if (__builtin_amdgcn_ballot_w64(slow)) {
      const int need = R.n_players() == 3u ? te1 : te2;   // the later of ag1's and na1's last turn ends
      // the drawing wave past record max(need) over the wave: its distance from t by ballots (no
      // cross-lane shuffles, which go through LDS); >= 2 in play (>= 3 players, turns of >= 2
      // steps), and from 5 on it asks for a little more than it needs.  (needw folds the lane's
      // condition into the value, so that each ballot is one compare)
      const int needw = slow && need >= 0 ? need : INT32_MIN;
      if (__builtin_amdgcn_ballot_w64(needw >= 0)) {
        int dmin = 5;
#pragma unroll
        for (int d = 4; d >= 1; d--) dmin = __builtin_amdgcn_ballot_w64(needw >= t - d) ? d : dmin;
        PH(4);
        cnt_wait(D, cc, cc.draw, (uint32_t)(t - dmin + 1), s_glob);
        PH(5);
      }
      if (slow) {
        pf_hd = D.img[ag1][1][l];
        pf_pla = D.pl[ag1][l];
        pf_hdn = D.heads[na1][l];
      }
    }
    if (live) {
      if (!lat && (tc || ended)) D.pl[ag][l] = pack_lean_player(pp, n_in_hand, n_active, steps_taken);
      const uint32_t meta = kMetaValid | (uint32_t)ag << 2 | (uint32_t)na << 4 | (uint32_t)na1 << 6 |
                            (ended ? kMetaEnded : 0u) | (stepped ? kMetaStepped : 0u) | (uint32_t)ag1 << 24;
      ring[0][l].x = R.sh[0];                              // (the resources: the drawing wave's)
      ring[1][l] = make_uint4(selb.w0, selb.w1, selb.w2, meta);
      ring[2][l] = make_uint4(stab.w0, stab.w1, stab.w2, a_play | (lat ? 0u : (n_active & 0xffu) << 8));
      D.srng[sl][l] = srng;
    } else {
      ring[1][l] = make_uint4(0u, 0u, 0u, 0u);             // no record
    }
    cnt_store(D, CNT_REC, (uint32_t)(t + 1));
    // (B rewrites slot (t + 1) % 4 only after record t + 1: this read is issued before that)
    have_next = t + 1 < kTrioLead || cc.pre >= (uint32_t)(t + 2 - kTrioLead);
    if (have_next) pr_next = D.pre[(t + 1) & (kTrioLead - 1)][l];
    PH(1);
    if (tc) {
      te2 = te1;
      te1 = t;
      H = pf_hd;                                           // its hand from the drawing wave
      pp = pf_pla;
      n_in_hand = (pf_pla.y >> 8) & 0xffu;
      n_active = (pf_pla.y >> 16) & 0xffu;
      steps_taken = (pf_pla.z >> 8) & 0xffu;
      lean_p = narrow && lean_player(pf_pla);
      stab = stnb;
      stnb = mbits_of(pf_hdn);
      pf_ok = false;
    }
    // the next turn change's records (the agent after ag1 and the player after it), read ahead
    // once the drawing wave is past their last turn ends (the counter as last read: no wait)
    if (live && !pf_ok && !ended) {
      const int need = R.n_players() == 3u ? te1 : te2;   // (as the turn change itself will ask)
      if (need < 0 || cc.draw >= (uint32_t)(need + 1)) {
        const int nn = (int)next_player((uint32_t)na1, R.n_players());
        pf_hd = D.img[na1][1][l];
        pf_pla = D.pl[na1][l];
        pf_hdn = D.heads[nn][l];
        pf_ok = true;
      }
    }
    if (live && ended) {                                   // hand the env to k_env_fixup
#ifndef COG_ISSUE_COUNT
      trio_store_private(s, i, R, selb);
      rngs[i] = srng;
#endif
      park = (uint32_t)t | (finish ? kParkFinish : 0u);
      live = false;
    }
    ag = ag1;
    na = na1;
    PH(3);
  }
  TL(12);
  if (live && !lat) D.pl[ag][l] = pack_lean_player(pp, n_in_hand, n_active, steps_taken);   // (the epilogue's)
  cnt_store(D, CNT_REC, (uint32_t)steps + 1u);             // the loop is over (storing wave A's epilogue)
  // the env-level private state back to HBM (lat: while the other waves drain; the flags word after
  // them: it takes their hazard flags); no other wave reads these words in the launch
  uint4 *pw = reinterpret_cast<uint4 *>(s.priv + i);
  if (lat) {
    if (live) {
      reinterpret_cast<uint3 *>(reinterpret_cast<uint32_t *>(pw) + 1)[0] = make_uint3(R.seed, R.max_steps, R.turn_counter);
      s.heads[5 * i] = mbits_u4(selb);
      rngs[i] = srng;
    }
    if (l < ne) s.park[i] = park;
    park_list_push(s_glob, park != kParkNone);
  }
  cnt_wait(D, cc, cc.fin, 3u, s_glob);                     // the other waves are done
  PH(7);                                                   // the drain (the other waves' last records)
  TL(13);
  const uint32_t fl = D.flg[l];                            // their hazard flags
  if (lat) {
    if (live) pw[1] = make_uint4(R.g1x, R.g1y, R.in_market, R.flags | fl);
    else if (l < ne && fl) reinterpret_cast<uint32_t *>(pw)[7] = R.flags | fl;   // a parked env: its last records'
  } else {
    if (live) {
      R.flags |= fl;
      trio_store_private(s, i, R, selb);
      rngs[i] = srng;
    } else if (l < ne && fl) {
      reinterpret_cast<uint32_t *>(pw)[7] = R.flags | fl;
    }
    if (l < ne) s.park[i] = park;
    park_list_push(s_glob, park != kParkNone);
  }
  trio_store_players(D, s, ne);                            // every player's records (cooperative)
  PH(8);                                                   // the epilogue's stores (issued)
  TL(14);
  PH_FLUSH(s_glob);
}

// One record's play on the drawing wave (trio_drawer; round 6): the acting player's counters
// (LAT), the ObsData phase / resources granule, the Info steps byte and Deck::activate's hand /
// active piles, on the values the caller read (p4: D.pl[ag], h / a: D.img[ag][1 / 2]), which it
// updates and stores back; selects instead of exec-mask branches for the common path.
template <bool LAT>
DEV void trio_draw_play(TrioLds &D, const DevState &s, int l, bool live, int slot, uint32_t mt, uint32_t w2,
                        uint32_t gx, uint4 &p4, uint2 &h, uint2 &a, uint4 &shb0, uint32_t &infob, bool &te,
                        bool &rec_out, uint32_t &dm, uint32_t &nact) {
  const size_t i = (size_t)l;
  const int ag = (int)((mt >> 2) & 3u);
  const bool valid = live && (mt & kMetaValid);
  const bool rec = valid && (mt & kMetaStepped);
  rec_out = rec;
  te = rec && (int)(mt >> 24) != ag;
  const uint32_t a_play = w2 & 0xffu;
  const bool play = rec && a_play != 0u;
  const int c = (int)((a_play - 1u) & 7u);               // (c < 8: the stepping wave parks any other type)
  if (LAT) {                                             // the acting player's counters (PlayerPriv:
    uint4 q = p4;                                        // steps_taken, n_in_hand, n_active, idx_last;
    uint32_t na = (q.y >> 16) & 0xffu;                   // Player::play_card, player.cpp:45-60; u8)
    q.z = (q.z & 0xffff00ffu) | (((q.z >> 8) + 1u) & 0xffu) << 8;
    q.y = play ? (q.y & 0xffff00ffu) | ((((q.y >> 8) & 0xffu) - 1u) & 0xffu) << 8 : q.y;
    na = play ? (na + 1u) & 0xffu : na;
    q.z = play ? (q.z & ~0xffu) | (a_play - 1u) : q.z;
    na = te ? 0u : na;                                   // Player::end_turn
    q.y = (q.y & 0xff00ffffu) | na << 16;
    p4.x = rec ? q.x : p4.x;                             // (component selects: a select of two
    p4.y = rec ? q.y : p4.y;                             // vectors compiles to one of two addresses
    p4.z = rec ? q.z : p4.z;                             // in scratch)
    if (rec) D.pl[ag][l] = p4;
    nact = rec ? na : 0u;
  }
  // the ObsData phase / resources granule and the Info byte (the stepping wave leaves the resources
  // and the counts to this wave)
  infob = rec ? (infob & ~(0xffu << (8 * ag))) | ((((infob >> (8 * ag)) + 1u) & 0xffu) << (8 * ag)) : infob;
  uint32_t phase = shb0.x & 0xffu;
  phase = phase == COG_PHASE_INACTIVE ? (uint32_t)COG_PHASE_MOVEMENT : phase;
  const bool mv = play && phase == COG_PHASE_MOVEMENT, buy = play && phase == COG_PHASE_BUYING;
  const uint32_t coin = cardf(kRes2, c);                 // Player::play_card (player.cpp:45-60)
  uint4 g0 = shb0;
  g0.y = mv ? __float_as_uint((float)cardf(kRes0, c)) : g0.y;
  g0.z = mv ? __float_as_uint((float)cardf(kRes1, c)) : g0.z;
  const float bw = __uint_as_float(g0.w) + (coin > 0 ? (float)coin : 0.5f);
  g0.w = mv ? __float_as_uint((float)coin) : buy ? __float_as_uint(bw) : g0.w;
  g0.y = te ? 0u : g0.y;                                 // Player::end_turn (+0.f)
  g0.z = te ? 0u : g0.z;
  g0.w = te ? 0u : g0.w;
  g0.x = rec ? gx : g0.x;
  if (valid) {
    reinterpret_cast<uint3 *>(&D.ring[slot][0][l].y)[0] = make_uint3(g0.y, g0.z, g0.w);   // (storing wave A)
    s.info[i * COG_INFO_BYTES + COG_AGENT_INFO0 + COG_AGENT_INFO_STRIDE * ag] = (uint8_t)(infob >> (8 * ag));
    if (ne4(g0, shb0)) reinterpret_cast<uint4 *>(s.obs + i * COG_OBS_BYTES + COG_OBS_PHASE)[0] = g0;
  }
  shb0.x = valid ? g0.x : shb0.x;
  shb0.y = valid ? g0.y : shb0.y;
  shb0.z = valid ? g0.z : shb0.z;
  shb0.w = valid ? g0.w : shb0.w;
  // Deck::activate (cards.cpp:242-253): hand[c]--, active[c]++ (u8)
  const uint32_t sh = 8u * (uint32_t)(c & 3);
  uint32_t hw = c < 4 ? h.x : h.y, aw = c < 4 ? a.x : a.y;
  hw = (hw & ~(0xffu << sh)) | ((((hw >> sh) - 1u) & 0xffu) << sh);
  aw = (aw & ~(0xffu << sh)) | ((((aw >> sh) + 1u) & 0xffu) << sh);
  const bool lo = c < 4;
  h.x = play && lo ? hw : h.x;
  h.y = play && !lo ? hw : h.y;
  a.x = play && lo ? aw : a.x;
  a.y = play && !lo ? aw : a.y;
  if (play) {
    D.img[ag][1][l] = h;
    D.img[ag][2][l] = a;
  }
  const int bh = COG_DECK_HAND + c, ba = COG_DECK_ACTIVE + c;   // the record's granules
  dm = play ? 1u << (bh >> 4) | 1u << (ba >> 4) : 0u;
}

// The drawing wave keeps every player's deck (img).  It takes records in pairs r, r + 1 (r even):
// each record's play replayed on the acting player's deck (the hand and active piles, as
// Deck::activate does); then one pass over the turn ends of either record (discard + draws,
// duo_turn_end: the env rng is this wave's).  Which granules each record changed goes to storing
// wave B (ring granule 2, bits 16..22).  It also stores each record's ObsData phase/resources
// granule and Info steps byte (the resources for storing wave A in ring granule 0), and with LAT
// keeps the acting player's counters (PlayerPriv: steps_taken, n_in_hand, n_active, idx_last).
template <bool LAT>
DEV uint32_t trio_drawer(TrioLds &D, const DevState &s_glob, int steps, int epw) {
  PH_DECL;
  TL(14);                                                  // (timeline: this wave's start)
  const int l = (int)(threadIdx.x & 63);
  const size_t wbase = (size_t)blockIdx.x * epw;
  const DevState s = wave_view(s_glob, wbase);
  const size_t i = (size_t)l;
  const bool live = l < epw && wbase + (size_t)l < s_glob.n;
  uint32_t rng = 0u;                                       // the env rng
  bool narrow = true;
  constexpr bool lat = LAT;                                // (the acting player's counters: trio_stepper)
  uint4 shb0 = make_uint4(0u, 0u, 0u, 0u);                 // ObsData 16128.. as stored: the phase
  uint32_t infob = 0u;                                     // dword and the resources; Info steps
  if (live && !s_glob.cdeck_ok) {                          // the DeckObs records (else storing wave A
#pragma unroll                                             // loads the compact image the last launch left)
    for (int p = 0; p < 4; p++) {
      const uint4 *src = reinterpret_cast<const uint4 *>(deck_ptr(s, i, p));
      uint4 dk[7];
      uint2 pile[5];
#pragma unroll
      for (int k = 0; k < 7; k++) dk[k] = src[k];
      narrow = compact_of(dk, pile) && narrow;
#pragma unroll
      for (int q = 0; q < 5; q++) D.img[p][q][l] = pile[q];
    }
  }
  if (live) {
    rng = reinterpret_cast<const uint32_t *>(s.priv + i)[0];
    infob = reinterpret_cast<const uint32_t *>(s.priv + i)[12];   // EnvPriv granule 3, dword 0
    shb0 = reinterpret_cast<const uint4 *>(s.obs + i * COG_OBS_BYTES + COG_OBS_PHASE)[0];
  }
  if (!s_glob.cdeck_ok) D.wide[l] = narrow ? 0u : 1u;      // (a wide env: the stepper parks it at step 0)
  uint32_t flags = 0u;                                     // hazard flags of the draws
  __builtin_amdgcn_s_waitcnt(0);
  TL(15);                                                  // (timeline: this wave's prologue done)
  __syncthreads();                                         // B: the decks are in LDS
  PH_RESET;
  TrioCnt6 cc;
  for (int r = 0; r < steps; r += 2) {
    const int nrec = r + 1 < steps ? 2 : 1;
    cnt_wait(D, cc, cc.rec, (uint32_t)(r + nrec), s_glob);   // the records are written
    PH(8);
    if (r + nrec >= steps) TL(11);                         // (timeline: the last records written)
    const int slot[2] = {r & (kTrioDepth - 1), (r + 1) & (kTrioDepth - 1)};
    uint32_t dm[2] = {0u, 0u}, nact[2] = {0u, 0u};
    int agj[2] = {0, 0};
    bool te[2] = {false, false}, recj[2] = {false, false};
    // (round 6: both records' words, and both acting players' counters, hand and active piles, read
    // at once -- a second record of the same player continues from the first one's values in
    // registers -- and the common path computed with selects, not exec-mask branches)
    const uint32_t mt0 = D.ring[slot[0]][1][l].w, w20 = D.ring[slot[0]][2][l].w, gx0 = D.ring[slot[0]][0][l].x;
    uint32_t mt1 = D.ring[slot[1]][1][l].w;                // (a slot past nrec: read, not used)
    const uint32_t w21 = D.ring[slot[1]][2][l].w, gx1 = D.ring[slot[1]][0][l].x;
    if (nrec < 2) mt1 = 0u;                                // (uniform: no second record)
    const int ag0 = (int)((mt0 >> 2) & 3u), ag1 = (int)((mt1 >> 2) & 3u);
    uint4 p0 = make_uint4(0u, 0u, 0u, 0u), p1 = p0;
    if (lat) {
      p0 = D.pl[ag0][l];
      p1 = D.pl[ag1][l];
    }
    uint2 h0 = D.img[ag0][1][l], a0 = D.img[ag0][2][l], h1 = D.img[ag1][1][l], a1 = D.img[ag1][2][l];
    trio_draw_play<lat>(D, s, l, live, slot[0], mt0, w20, gx0, p0, h0, a0, shb0, infob, te[0], recj[0], dm[0], nact[0]);
    agj[0] = ag0;
    if (nrec > 1) {                                        // (uniform)
      if (ag1 == ag0) {                                    // the same player: record 0's values
        p1.x = p0.x; p1.y = p0.y; p1.z = p0.z; p1.w = p0.w;
        h1.x = h0.x; h1.y = h0.y;
        a1.x = a0.x; a1.y = a0.y;
      }
      trio_draw_play<lat>(D, s, l, live, slot[1], mt1, w21, gx1, p1, h1, a1, shb0, infob, te[1], recj[1], dm[1], nact[1]);
      agj[1] = ag1;
    }
    PH(7);                                                 // (stamps: the plays)
    const bool any = te[0] || te[1];                       // (at most one of them)
    if (__builtin_amdgcn_ballot_w64(any) && any) {         // the turn end's discard + draws
      const int j = te[1] ? 1 : 0, sl = te[1] ? slot[1] : slot[0], ag = te[1] ? agj[1] : agj[0];
      uint2 pile[5];
#pragma unroll
      for (int q = 0; q < 5; q++) pile[q] = D.img[ag][q][l];
      uint4 dk[7], old[7];
      deck_expand(pile, dk);
#pragma unroll
      for (int k = 0; k < 7; k++) old[k] = dk[k];
      const uint4 x = D.ring[sl][2][l];
      MBits ba{x.x, x.y, x.z};
      duo_turn_end(D, l, ag, dk, ba, rng, flags);          // (a narrow deck stays narrow)
      D.ring[sl][2][l] = make_uint4(ba.w0, ba.w1, ba.w2, x.w);
      uint32_t dd = 0;
#pragma unroll
      for (int k = 0; k < 7; k++) dd |= ne4(dk[k], old[k]) ? 1u << k : 0u;
      (void)compact_of(dk, pile);
#pragma unroll
      for (int q = 0; q < 5; q++) D.img[ag][q][l] = pile[q];
      dm[0] |= j == 0 ? dd : 0u;
      dm[1] |= j == 1 ? dd : 0u;
    }
#pragma unroll
    for (int j = 0; j < 2; j++)                            // granule 2's last dword: the action (the
      if (j < nrec) {                                      // stepping wave's), n_active, the changed deck
        uint32_t *w = &D.ring[slot[j]][2][l].w;            // granules (storing waves A and B)
        if (lat && recj[j]) *w = (*w & 0xffu) | nact[j] << 8 | dm[j] << 16;
        else reinterpret_cast<uint16_t *>(w)[1] = (uint16_t)dm[j];
      }
    cnt_store(D, CNT_DRAW, (uint32_t)(r + nrec));
    PH(9);
  }
  TL(12);
  if (live) {
    reinterpret_cast<uint32_t *>(s.priv + i)[0] = rng;     // the env rng after its last draws
    reinterpret_cast<uint32_t *>(s.priv + i)[12] = infob;  // Info steps (a parked env's: as of the park)
  }
  PH_FLUSH(s_glob);
  return flags;
}

// The store phase of the trio on two waves: wave A (PART 0) the stored masks --
// update_observation's heads of the acting player's when the turn goes on (the lean step leaves
// them) -- and wave B (PART 1) the presampled draws (presample; with LAT head 0's index table), the
// selected-mask record, the action, dones / agent_selection and the decks.  Each keeps its own
// images of what it stored last.
template <int PART, bool LAT>
DEV uint32_t trio_storer(TrioLds &D, const DevState &s_glob, int steps, int epw, const uint32_t *__restrict__ rngs_glob,
                         uint8_t *__restrict__ actions_glob) {
  PH_DECL;
  TL(14);                                                  // (timeline: this wave's start)
  const int l = (int)(threadIdx.x & 63);
  const size_t wbase = (size_t)blockIdx.x * epw;
  const DevState s = wave_view(s_glob, wbase);
  const size_t i = (size_t)l;
  const bool live = l < epw && wbase + (size_t)l < s_glob.n;
  uint8_t *__restrict__ av = actions_glob + wbase * COG_ACTION_BYTES;
  MBits selb = {0u, 0u, 0u};                               // B: the selected mask as stored
  uint2 cells[4];                                          // A: every player's neighbourhood cache
  uint32_t out = ~0u;                                      // B: dones[i] | agent_selection[i] << 8 as stored
  RegEnv E;                                                // A: update_observation's inputs and flags
  E.flags = 0u;
  E.avail = 0u;
  uint32_t x = 1u;                                         // B: the sampler state at step 0
  if (live) {
    if (PART == 0) {
      const uint4 *sh4 = reinterpret_cast<const uint4 *>(s.obs + i * COG_OBS_BYTES + COG_OBS_PHASE);
      const uint4 sh1 = sh4[1], sh2 = sh4[2];
      const uint4 *pv4 = reinterpret_cast<const uint4 *>(s.priv + i);
#pragma unroll
      for (int p = 0; p < 4; p++) {
        D.stbA[p][l] = s.heads[5 * i + 1 + p];
        cells[p] = reinterpret_cast<const uint2 *>(pv4 + 8)[p];
      }
      const uint4 g1 = pv4[1];
      const uint32_t w[5] = {sh1.x, sh1.y, sh1.z, sh1.w, sh2.x};
      E.avail = shop_avail_of(w, (g1.y >> 8) & 0xffu, g1.z);   // (no purchase in the lean step: fixed)
      if (s_glob.cdeck_ok) {                               // the drawing wave's compact decks as the
        const uint4 *src = s.cdeck + 10 * i;               // last launch left them (DevState::cdeck)
        uint4 c[10];
#pragma unroll
        for (int g = 0; g < 10; g++) c[g] = src[g];
#pragma unroll
        for (int g = 0; g < 10; g++) {                     // entries 2g, 2g + 1 of [player][pile]
          D.img[(2 * g) / 5][(2 * g) % 5][l] = make_uint2(c[g].x, c[g].y);
          D.img[(2 * g + 1) / 5][(2 * g + 1) % 5][l] = make_uint2(c[g].z, c[g].w);
        }
      }
    } else {
      selb = mbits_of(s.heads[5 * i]);
      x = rngs_glob[wbase + (size_t)l];
    }
  }
  if (PART == 0 && s_glob.cdeck_ok) D.wide[l] = live ? s.cwide[i] : 0u;   // (else the drawing wave's)
  if (PART == 1) {                                         // steps 0..3 from the state at step 0
#pragma unroll
    for (int k = 0; k < kTrioLead; k++) {
      const uint4 p = presample(x);
      D.pre[k][l] = pre_pack(p, LAT);
      x = p.z;
    }
  }
  __builtin_amdgcn_s_waitcnt(0);
  TL(15);                                                  // (timeline: this wave's prologue done)
  __syncthreads();                                         // B
  PH_RESET;
  // B runs two cursors: record r's part that needs no draws (the presampled draws first: the
  // stepping wave waits for them), and record r - kTrioBLag's deck granules once drawn, so that
  // the presampled draws never wait for the drawing wave.  A: record r once drawn.
  constexpr int LAG = PART == 1 ? kTrioBLag : 0;
  auto deck_rec = [&](int q) {                             // B: the deck granules record q changed
    const int sl = q & (kTrioDepth - 1);
    const uint32_t meta = D.ring[sl][1][l].w;
    const int ag = (int)((meta >> 2) & 3u);
    if (live && (meta & kMetaValid)) {                     // (from img)
      const uint32_t dm = D.ring[sl][2][l].w >> 16;
      uint2 pile[5];
#pragma unroll
      for (int k = 0; k < 5; k++) pile[k] = D.img[ag][k][l];
      uint4 dk[7];
      deck_expand(pile, dk);
      uint4 *deck = reinterpret_cast<uint4 *>(deck_ptr(s, i, ag));
#pragma unroll
      for (int k = 0; k < 7; k++)
        if ((dm >> k) & 1u) deck[k] = dk[k];
    }
    cnt_store(D, CNT_STB, (uint32_t)(q + 1));
  };
  TrioCnt6 cc;
  for (int r = 0; r < steps + LAG; r++) {
    if (PART == 1 && r < steps) {                          // record r written
      const int sl = r & (kTrioDepth - 1);
      cnt_wait(D, cc, cc.rec, (uint32_t)(r + 1), s_glob);
      PH(5);
      const uint4 m = D.ring[sl][1][l];
      const uint32_t meta = m.w;
      const bool rec = live && (meta & kMetaValid);
      if (rec && r + kTrioLead < steps)                    // step r + 4's draws: the state after step r,
        D.pre[(r + kTrioLead) & (kTrioLead - 1)][l] = pre_pack(presample(mr_jump(D.srng[sl][l], kPow15)), LAT);
      cnt_store(D, CNT_PRE, (uint32_t)(r + 1));            // + 15 draws (steps r + 1 .. r + 3)
      const uint32_t a_play = D.ring[sl][2][l].w & 0xffu;
      if (rec) {
        const MBits bs{m.x, m.y, m.z};
        store_mask_record(reinterpret_cast<uint4 *>(s.sel + i * COG_MASK_BYTES), bs, mask_diff_granules(bs, selb));
        selb = bs;
        reinterpret_cast<uint2 *>(av + i * COG_ACTION_BYTES)[0] = make_uint2(a_play, 0u);   // (lean: heads 1-4 are 0)
        if (!(meta & kMetaEnded)) {                        // dones[i] = 0, agent_selection[i]
          const uint32_t agent = meta >> 24;               // (an ended episode: k_env_fixup)
          if (out & 0xffu) s.done[i] = 0;
          if (((out >> 8) & 0xffu) != agent) s.agent[i] = (uint8_t)agent;
          out = agent << 8;
        }
      }
    }
    PH(7);
    const int q = r - LAG;                                 // record q drawn
    if (q < 0) continue;                                   // (uniform)
    const int sl = q & (kTrioDepth - 1);
    cnt_wait(D, cc, cc.draw, (uint32_t)(q + 1), s_glob);
    PH(6);
    if (q == steps - 1) TL(11);                            // (timeline: the last record drawn)
    const uint32_t meta = D.ring[sl][1][l].w;
    const bool rec = live && (meta & kMetaValid);
    const int ag = (int)((meta >> 2) & 3u), na = (int)((meta >> 4) & 3u);
    if (rec && PART == 0) {
      const uint4 g0 = D.ring[sl][0][l], xa = D.ring[sl][2][l], oa = D.stbA[ag][l];
      MBits ba{xa.x, xa.y, xa.z};
      if ((int)(meta >> 24) == ag && (meta & kMetaStepped)) {   // the turn goes on: update_observation's
        const uint32_t phase = g0.x & 0xffu;               // heads of ag's stored mask
        const float r0 = __uint_as_float(g0.y), r1 = __uint_as_float(g0.z), r2 = __uint_as_float(g0.w);
        const uint32_t n_active = (xa.w >> 8) & 0xffu;     // (environment.cpp:252-279)
        uint2 ca = cells[3];                               // (selects: no indexed registers)
#pragma unroll
        for (int p = 2; p >= 0; p--) ca = ag == p ? cells[p] : ca;
        const uint32_t mv = phase == COG_PHASE_MOVEMENT ? E.move_bits(ca, r0, r1, r2, n_active) : 1u;
        const uint32_t sp = phase == COG_PHASE_BUYING ? E.shop_bits(r2) : 1u;
        ba.w2 = (ba.w2 & ~kMoveShopBits) | mv << 2 | sp << 9;
      }
      uint8_t *deck = deck_ptr(s, i, ag);
      store_mask_record(reinterpret_cast<uint4 *>(deck + COG_PD_MASK), ba, mask_diff_granules(ba, mbits_of(oa)));
      D.stbA[ag][l] = mbits_u4(ba);
      if ((int)(meta >> 24) != ag && (meta & kMetaStepped)) {   // a turn end: the new agent's stored mask
        const uint4 on = D.stbA[na][l];                    // gets update_observation's INACTIVE-phase
        const MBits bn{on.x, on.y, (on.z & ~kMoveShopBits) | 0x204u};   // heads (the lean step)
        store_mask_record(reinterpret_cast<uint4 *>(deck_ptr(s, i, na) + COG_PD_MASK), bn,
                          mask_diff_granules(bn, mbits_of(on)));
        D.stbA[na][l] = mbits_u4(bn);
      }
    }
    if (PART == 1) {
      deck_rec(q);
    } else {
      cnt_store(D, CNT_STA, (uint32_t)(q + 1));
    }
    PH(13);
  }
  TL(12);
  // A: the stored-mask bit vectors as stored (the epilogue's; the drawing wave's turn ends
  // included), once the stepping wave no longer reads them
  if (PART == 0) {
    cnt_wait(D, cc, cc.rec, (uint32_t)steps + 1u, s_glob);
    if (live) {
#pragma unroll
      for (int p = 0; p < 4; p++) D.heads[p][l] = D.stbA[p][l];
      uint4 *dst = s.cdeck + 10 * i;                       // the drawing wave's final decks (it is past
#pragma unroll                                             // the last record) for the next launch; a
      for (int g = 0; g < 10; g++) {                       // parked env's: k_env_fixup rewrites them
        const uint2 a = D.img[(2 * g) / 5][(2 * g) % 5][l], b = D.img[(2 * g + 1) / 5][(2 * g + 1) % 5][l];
        dst[g] = make_uint4(a.x, a.y, b.x, b.y);
      }
      s.cwide[i] = D.wide[l];
    }
  }
  PH_FLUSH(s_glob);
  return E.flags;                                          // (A: update_observation's lookups)
}

// four waves per workgroup: stepping, drawing and two storing waves, for epw (32 or 64) envs: lanes
// epw.. idle (trio_epw: half-empty waves fill all 256 CUs at 8,192 envs).  The drawing and storing
// waves leave their hazard flags in flg[] and count themselves done in cnt[FIN]; the stepping wave
// waits for all three before its epilogue.
// LAT (a launch of at most one workgroup per CU, DevState::trio_jt): head 0's index table in the
// presampled records and the acting player's counters on the drawing wave -- the stepping wave's
// chain is the launch's time; otherwise (two workgroups share a CU) the total work per CU counts
template <int SRC, bool LAT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) k_env_rollout_trio(DevState s, int steps, int epw, uint32_t *__restrict__ rngs,
                                                          uint8_t *__restrict__ actions_out) {
  __shared__ TrioLds D;
  // (roles rotated per workgroup, so that a CU's two workgroups could not put both stepping waves
  // on one SIMD, measured the same: profiles/r04y_trio_role_rotation.txt, r05_trio_ab.txt r05s)
  const int role = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform
  if (threadIdx.x < 64) D.flg[threadIdx.x] = 0u;
  if (threadIdx.x < kTrioCnts) D.cnt[threadIdx.x] = 0u;
  park_list_clear_other(s);
  uid_tab_fill(D.tab);                                     // (ends on a barrier)
  if (role == 0) {
    __builtin_amdgcn_s_setprio(3);
    trio_stepper<SRC, LAT>(D, s, steps, epw, rngs);
    return;
  }
  uint32_t flags;
  if (role == 1) flags = trio_drawer<LAT>(D, s, steps, epw);
  else if (role == 2) flags = trio_storer<0, LAT>(D, s, steps, epw, rngs, actions_out);
  else flags = trio_storer<1, LAT>(D, s, steps, epw, rngs, actions_out);
  const int l = (int)(threadIdx.x & 63);
  if (flags) __hip_atomic_fetch_or(&D.flg[l], flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (l == 0) __hip_atomic_fetch_add(&D.cnt[CNT_FIN], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
