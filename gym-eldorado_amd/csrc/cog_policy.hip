// cog_policy.hip -- the policy sampler (include/cog.h cog_sampler_sample_policy): one kernel from a
// batch of logits and the envs' ActionMask records to ActionData records, the joint log-probability
// and the entropy of the five masked categorical heads.
//
// Shape: one workgroup of four waves per tile of 64 envs.  The kernel is bandwidth-shaped (368 B of
// float32 logits and 96 of the 128 mask bytes read per env, 16 B written), but the work per env is
// a serial scan of 92 entries, so the tile goes through LDS once: the workgroup loads the tile's
// rows with coalesced 16-B loads (consecutive lanes read consecutive granules of a row; with
// ld == 92 the whole tile is one contiguous block), widens bfloat16 to float32 and stores the
// values at an odd dword row stride (93: lane r reading column c of its own row hits bank
// (93 r + c) mod 32, conflict-free).  The mask bytes are loaded the same way, 6 granules per env,
// and kept as 92 bits per env.  Then lane r of every wave scans row r, each wave its share of the
// heads, with the head's entries in registers (every loop is unrolled over the head's compile-time
// size).  23.25 KiB of rows + 768 B of mask bits + 2.25 KiB of the waves' terms = 26.25 KiB of LDS
// per workgroup: six workgroups (24 waves) share a CU.  The same kernel with one wave per tile doing
// all five heads took twice the time (profiles/policy_sample_time.txt).
//
// Semantics (exact up to float32 rounding; tests/test_gpu_policy_sampler.py holds the numpy form):
// per head, over the valid entries (mask byte != 0; a NaN logit counts as -inf): m = max l,
// w_j = exp(l_j - m), Z = sum w, C_j the inclusive prefix sum; the action is the smallest j with
// C_j > u Z (the last valid j when rounding leaves none), u = ((x_h - 1) >> 7) 2^-24 from the
// sampler's minstd_rand0 state advanced once per head; logp += (l_j - m) - log Z,
// entropy += log Z - sum w_j (l_j - m) / Z.  An empty head gives 0 and contributes nothing.  A head
// whose valid entries hold +inf, or nothing but -inf / NaN, takes the greedy choice (largest logit,
// lowest index) and makes the env's logp and entropy NaN.  Greedy mode takes that choice for every
// head and leaves the sampler's state alone.
//
// The policy evaluator (cog_policy_evaluate and its backward, further down) shares the staging code
// and the shape.  The advantage estimator (cog_policy_gae, after it) is a kernel of its own shape:
// one lane per (env, seat) walking the rows of a rollout window.  The policy features
// (cog_env_policy_features, at the end) read the engine's state, not logits: a tile of envs staged
// and built in LDS, then streamed out as 16-B chunks.
#include <hip/hip_runtime.h>

#include <math.h>

#include <type_traits>

#include "../../include/cog_types.h"
#include "cog_engine.h"
#include "cog_policy.h"
#include "cog_rng.h"

namespace cog {
namespace {

#define DEV __device__ __forceinline__

#include "cog_feat.h"   // feat(code, f): feature f of a hex code

constexpr int kTile = 64;                                  // envs per workgroup
constexpr int kWaves = 4;                                  // waves per workgroup
constexpr int kCols = COG_MASK_USED;                       // 92
constexpr int kQuads = kCols / 4;                          // 23 groups of four logits per row
constexpr int kRowStride = kCols + 1;                      // dwords per staged row (odd)
static_assert(kCols % 4 == 0, "rows are whole groups of four logits");
static_assert(COG_MASK_PLAY == 0 && COG_MASK_SPECIAL == 22 && COG_MASK_REMOVE == 44 && COG_MASK_MOVE == 66 &&
                  COG_MASK_SHOP == 73 && COG_MASK_USED == 92,
              "head offsets");

DEV float bf16_widen(uint32_t h) { return __uint_as_float(h << 16); }

// one bit per non-zero byte of w, bit k for byte k
DEV uint32_t nonzero_bytes(uint32_t w) {
  const uint32_t t = (((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u;
  return (((t >> 7) * 0x00204081u) >> 21) & 0xfu;
}

DEV void put4(float *tile, int row, int col, float a, float b, float c, float d) {
  float *p = tile + row * kRowStride + col;
  p[0] = a;
  p[1] = b;
  p[2] = c;
  p[3] = d;
}
DEV void put4_bf16(float *tile, int quad, uint32_t lo, uint32_t hi) {   // quad: row * 23 + group
  put4(tile, quad / kQuads, 4 * (quad % kQuads), bf16_widen(lo & 0xffffu), bf16_widen(lo >> 16), bf16_widen(hi & 0xffffu),
       bf16_widen(hi >> 16));
}

// rows [base, base + rows) of the logits into the tile, by the T threads of the workgroup.  VEC:
// 16-B loads (the launcher has checked the alignment: float32 ld % 4 == 0; bfloat16 ld == 92 or
// ld % 8 == 0; base pointer 16-B aligned)
template <bool BF16, bool VEC, int T>
DEV void stage_logits(float *tile, const void *logits, size_t ld, size_t base, int rows, int tid) {
  if (!VEC) {
#pragma unroll 4
    for (int k = 0; k < (kTile * kCols + T - 1) / T; k++) {
      const int q = k * T + tid, row = q / kCols, col = q % kCols;
      if (row < rows) {
        const size_t e = (base + row) * ld + col;
        tile[row * kRowStride + col] =
            BF16 ? bf16_widen(static_cast<const uint16_t *>(logits)[e]) : static_cast<const float *>(logits)[e];
      }
    }
  } else if (!BF16) {
    const float *L = static_cast<const float *>(logits);
#pragma unroll
    for (int k = 0; k < (kTile * kQuads + T - 1) / T; k++) {
      const int q = k * T + tid, row = q / kQuads, col = 4 * (q % kQuads);
      if (row < rows) {
        const float4 v = *reinterpret_cast<const float4 *>(L + (base + row) * ld + col);
        put4(tile, row, col, v.x, v.y, v.z, v.w);
      }
    }
  } else if (ld == (size_t)kCols) {
    // the tile is one contiguous block of rows x 23 quads of 8 B; a 16-B granule holds two quads
    // (of two rows at a row's end), and the block's last granule may be half of one
    const uint16_t *L = static_cast<const uint16_t *>(logits) + base * kCols;
    const int total = rows * kQuads;
#pragma unroll
    for (int k = 0; k < (kTile * kQuads / 2 + T - 1) / T; k++) {
      const int p = k * T + tid, g = 2 * p;
      if (g + 1 < total) {
        const uint4 v = *reinterpret_cast<const uint4 *>(L + 8 * (size_t)p);
        put4_bf16(tile, g, v.x, v.y);
        put4_bf16(tile, g + 1, v.z, v.w);
      } else if (g < total) {
        const uint2 v = *reinterpret_cast<const uint2 *>(L + 8 * (size_t)p);
        put4_bf16(tile, g, v.x, v.y);
      }
    }
  } else {
    // 16-B aligned rows: 11 granules and one half granule per row (columns 92.. are never read)
    const uint16_t *L = static_cast<const uint16_t *>(logits);
#pragma unroll
    for (int k = 0; k < (kTile * 12 + T - 1) / T; k++) {
      const int p = k * T + tid, row = p / 12, pc = p % 12;
      if (row < rows) {
        const uint16_t *src = L + (base + row) * ld + 8 * pc;
        if (pc < 11) {
          const uint4 v = *reinterpret_cast<const uint4 *>(src);
          put4_bf16(tile, row * kQuads + 2 * pc, v.x, v.y);
          put4_bf16(tile, row * kQuads + 2 * pc + 1, v.z, v.w);
        } else {
          const uint2 v = *reinterpret_cast<const uint2 *>(src);
          put4_bf16(tile, row * kQuads + 22, v.x, v.y);
        }
      }
    }
  }
}

// the mask records of rows [base, base + rows) as 96 valid bits per row (mbits: 3 dwords a row; rows
// past `rows` get zeros): granule cc (of 6) of row `row`, 16 bits each
template <int T>
DEV void stage_masks(uint32_t *mbits, const uint8_t *mask_base, size_t mask_stride, const uint8_t *agent, size_t base,
                     int rows, int tid) {
#pragma unroll
  for (int k = 0; k < (kTile * 6 + T - 1) / T; k++) {
    const int q = k * T + tid, row = q / 6, cc = q % 6;
    if (q < kTile * 6) {
      uint32_t bits = 0;
      if (row < rows) {
        const size_t e = base + row;
        const uint8_t *rec = mask_base + e * mask_stride;
        if (agent) rec += (size_t)(agent[e] & 3u) * COG_OBS_PLAYER_STRIDE;
        const uint4 v = reinterpret_cast<const uint4 *>(rec)[cc];
        bits = nonzero_bytes(v.x) | nonzero_bytes(v.y) << 4 | nonzero_bytes(v.z) << 8 | nonzero_bytes(v.w) << 12;
      }
      reinterpret_cast<uint16_t *>(mbits)[q] = (uint16_t)bits;
    }
  }
}

// the valid bits of row `lane`'s five heads
struct HeadBits {
  uint32_t play, special, remove, move, shop;
};
DEV HeadBits head_bits(const uint32_t *mbits, int lane) {
  const uint64_t lo = (uint64_t)mbits[3 * lane] | (uint64_t)mbits[3 * lane + 1] << 32;       // bits 0..63
  const uint64_t hi = (uint64_t)mbits[3 * lane + 1] | (uint64_t)mbits[3 * lane + 2] << 32;   // bits 32..95
  return {(uint32_t)(lo >> COG_MASK_PLAY) & 0x3fffffu, (uint32_t)(lo >> COG_MASK_SPECIAL) & 0x3fffffu,
          (uint32_t)(hi >> (COG_MASK_REMOVE - 32)) & 0x3fffffu, (uint32_t)(hi >> (COG_MASK_MOVE - 32)) & 0x7fu,
          (uint32_t)(hi >> (COG_MASK_SHOP - 32)) & 0x7ffffu};
}

// One head of K entries at column OFF of the lane's staged row; vb: its valid bits.  Returns the
// action; adds the head's terms to logp / ent, or sets bad for a degenerate head.
template <int OFF, int K, bool GREEDY>
DEV uint32_t sample_head(const float *row, uint32_t vb, float u, float &logp, float &ent, bool &bad) {
  if (vb == 0u) return 0u;
  float lv[K];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < K; j++) {
    const float x = row[OFF + j];
    lv[j] = ((vb >> j) & 1u) && x == x ? x : -INFINITY;
    m = fmaxf(m, lv[j]);
  }
  const bool degen = !(fabsf(m) < INFINITY);               // +inf, or nothing above -inf
  uint32_t a = 0;
  if (GREEDY || degen) {
    uint32_t eq = 0;
#pragma unroll
    for (int j = 0; j < K; j++) eq |= (lv[j] == m ? 1u : 0u) << j;
    a = (uint32_t)__ffs((int)(eq & vb)) - 1u;              // (invalid entries are -inf too: masked)
  }
  if (degen) {
    bad = true;
    return a;
  }
  float Z = 0.0f, S = 0.0f;
#pragma unroll
  for (int j = 0; j < K; j++) {
    const float d = fmaxf(lv[j] - m, -3.0e38f);            // (finite: 0 * d is 0 for a masked entry)
    const float w = __expf(d);
    lv[j] = w;
    Z += w;
    S += w * d;
  }
  float da = 0.0f;                                         // l_a - m (greedy: the maximum itself)
  if (!GREEDY) {
    const float t = u * Z;
    float C = 0.0f;
    uint32_t below = 0;                                    // C is non-decreasing: the first j with C_j > t
#pragma unroll                                             // is the number of j with C_j <= t, and its
    for (int j = 0; j < K; j++) {                          // w_j > 0, so it is a valid entry
      C += lv[j];
      below += C <= t ? 1u : 0u;
    }
    a = below < (uint32_t)K ? below : 31u - (uint32_t)__clz((int)vb);
    const float x = row[OFF + a];
    da = x == x ? x - m : -INFINITY;
  }
  const float logZ = logf(Z);
  logp += da - logZ;
  ent += logZ - S / Z;
  return a;
}

struct PolicyArgs {
  size_t n;
  const void *logits;
  size_t ld;
  const uint8_t *mask_base;
  size_t mask_stride;
  const uint8_t *agent;
  uint32_t *rng;
  uint8_t *actions;
  float *logp, *entropy;
};

// Four waves stage the tile together and split the heads (play | play_special | remove | move +
// get_from_shop: 22, 22, 22, 26 entries), lane r of each wave on env r; waves 1..3 leave their terms
// in LDS and wave 0 adds them up and stores.
template <bool BF16, bool VEC, bool GREEDY>
__global__ void __launch_bounds__(kTile *kWaves) k_policy_sample(PolicyArgs a) {
  constexpr int WAVES = kWaves;
  __shared__ float tile[kTile * kRowStride];
  __shared__ uint32_t mbits[kTile * 3];                    // 96 valid bits per env
  __shared__ float part[(WAVES - 1) * 3 * kTile];          // waves 1..3: logp, entropy, actions | bad << 31
  constexpr int T = kTile * WAVES;
  const int tid = (int)threadIdx.x, lane = tid & (kTile - 1), wave = tid / kTile;
  const size_t base = (size_t)blockIdx.x * kTile;
  const int rows = a.n - base < (size_t)kTile ? (int)(a.n - base) : kTile;
  const size_t i = base + lane;
  const bool live = lane < rows;

  float u[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  uint32_t x_new = 0;
  if (!GREEDY && live) {                                   // one draw per head, as independent products
    const uint32_t x = a.rng[i];                           // (read by every wave before the barrier; wave 0
    constexpr uint32_t c[5] = {mr_pow(1), mr_pow(2), mr_pow(3), mr_pow(4), mr_pow(5)};   // writes after it)
#pragma unroll
    for (int h = 0; h < 5; h++) {
      x_new = mr_jump(x, c[h]);
      u[h] = (float)((x_new - 1u) >> 7) * (1.0f / 16777216.0f);
    }
  }
  stage_masks<T>(mbits, a.mask_base, a.mask_stride, a.agent, base, rows, tid);
  stage_logits<BF16, VEC, T>(tile, a.logits, a.ld, base, rows, tid);
  __syncthreads();

  float logp = 0.0f, ent = 0.0f;
  bool bad = false;
  uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0;
  if (live) {
    const float *row = tile + lane * kRowStride;
    const HeadBits vb = head_bits(mbits, lane);
    if (wave == 0) a0 = sample_head<COG_MASK_PLAY, 22, GREEDY>(row, vb.play, u[0], logp, ent, bad);
    if (wave == 1) a1 = sample_head<COG_MASK_SPECIAL, 22, GREEDY>(row, vb.special, u[1], logp, ent, bad);
    if (wave == 2) a2 = sample_head<COG_MASK_REMOVE, 22, GREEDY>(row, vb.remove, u[2], logp, ent, bad);
    if (wave == 3) {
      a3 = sample_head<COG_MASK_MOVE, 7, GREEDY>(row, vb.move, u[3], logp, ent, bad);
      a4 = sample_head<COG_MASK_SHOP, 19, GREEDY>(row, vb.shop, u[4], logp, ent, bad);
    }
  }
  if (wave > 0) {
    float *p = part + (wave - 1) * 3 * kTile + lane;
    p[0] = logp;
    p[kTile] = ent;
    p[2 * kTile] = __uint_as_float(a1 | a2 | a3 | a4 << 8 | (bad ? 0x80000000u : 0u));
  }
  __syncthreads();
  if (wave > 0 || !live) return;
#pragma unroll
  for (int w = 1; w < WAVES; w++) {
    const float *p = part + (w - 1) * 3 * kTile + lane;
    logp += p[0];
    ent += p[kTile];
    const uint32_t b = __float_as_uint(p[2 * kTile]);
    bad = bad || (b >> 31) != 0u;
    if (w == 1) a1 = b & 0xffu;
    if (w == 2) a2 = b & 0xffu;
    if (w == 3) {
      a3 = b & 0xffu;
      a4 = (b >> 8) & 0xffu;
    }
  }
  if (!GREEDY) a.rng[i] = x_new;
  // the 8 bytes the uniform sampler writes at the head of the record (play .. get_from_shop, zeros)
  *reinterpret_cast<uint2 *>(a.actions + i * COG_ACTION_BYTES) = make_uint2(a0 | a1 << 8 | a2 << 16 | a3 << 24, a4);
  if (a.logp) a.logp[i] = bad ? __uint_as_float(0x7fc00000u) : logp;
  if (a.entropy) a.entropy[i] = bad ? __uint_as_float(0x7fc00000u) : ent;
}

template <bool BF16, bool VEC>
void launch_form(const PolicyArgs &a, bool greedy, dim3 grid, hipStream_t st) {
  if (greedy)
    hipLaunchKernelGGL((k_policy_sample<BF16, VEC, true>), grid, dim3(kTile * kWaves), 0, st, a);
  else
    hipLaunchKernelGGL((k_policy_sample<BF16, VEC, false>), grid, dim3(kTile * kWaves), 0, st, a);
}

// ---- the policy evaluator (include/cog.h cog_policy_evaluate / cog_policy_evaluate_backward) ----
// The same distribution seen from the learner's side: for recorded (mask, action) pairs and new
// logits, the joint log-probability of the recorded actions and the entropy (forward), and the
// gradient of both with respect to the logits (backward).  Both kernels keep the sampler's shape:
// four waves per tile of 64 rows, the tile and the mask bits staged by the sampler's own code, the
// heads split over the waves, lane r on row r.  The backward recomputes the head terms (the forward
// saves nothing) and writes each head's gradient entries over the staged logits in place; after a
// barrier the workgroup stores the tile, one contiguous block of the (n, 92) output, with 16-B
// stores.  A row with a degenerate head or an illegal recorded action is flagged in LDS and stored
// as zeros.  No atomics: the results are the same from run to run.

struct EvalArgs {
  size_t n;
  const void *logits;
  size_t ld;
  const uint8_t *actions;
  size_t action_stride;
  const uint8_t *masks;
  float *logp, *entropy;                                   // forward
  const float *g_logp, *g_entropy;                         // backward
  void *grad;
};

// The terms of one non-empty head of K entries at column OFF of the lane's staged row (vb: its valid
// bits, a: the recorded action), in R = float or double: d_j = l_j - m (clamped finite, so that
// 0 * d_j is 0), w_j = exp(d_j), Z = sum w, S = sum w_j d_j.  False for a degenerate head or an action
// that is no valid entry.
DEV float exp_r(float x) { return __expf(x); }
DEV double exp_r(double x) { return exp(x); }

template <int OFF, int K, typename R>
DEV bool head_terms(const float *row, uint32_t vb, uint32_t a, R (&d)[K], R (&w)[K], float &m, R &Z, R &S) {
  m = -INFINITY;
#pragma unroll
  for (int j = 0; j < K; j++) {
    const float x = row[OFF + j];
    const float l = ((vb >> j) & 1u) && x == x ? x : -INFINITY;
    d[j] = l;
    m = fmaxf(m, l);
  }
  if (!(fabsf(m) < INFINITY)) return false;                // +inf, or nothing above -inf
  if (a >= (uint32_t)K || !((vb >> a) & 1u)) return false;
  Z = 0;
  S = 0;
#pragma unroll
  for (int j = 0; j < K; j++) {
    d[j] = d[j] - (R)m;
    d[j] = d[j] > (R)-3.0e38f ? d[j] : (R)-3.0e38f;
    w[j] = exp_r(d[j]);
    Z += w[j];
    S += w[j] * d[j];
  }
  return true;
}

template <int OFF, int K>
DEV void eval_head(const float *row, uint32_t vb, uint32_t a, float &logp, float &ent, bool &bad) {
  if (vb == 0u) return;
  float d[K], w[K], m, Z, S;
  if (!head_terms<OFF, K, float>(row, vb, a, d, w, m, Z, S)) {
    bad = true;
    return;
  }
  const float x = row[OFF + a];                            // (a < K: checked)
  const float logZ = logf(Z);
  logp += (x == x ? x - m : -INFINITY) - logZ;
  ent += logZ - S / Z;
}

// grad_j = g_lp (1[j = a] - p_j) - g_en p_j (log p_j + H), and log p_j + H = d_j - S / Z; zeros for
// invalid entries and for an empty head.  R: the type the terms are computed in.  A float32 gradient
// is computed in float.  A bfloat16 one is computed in double and narrowed to float here, so that the
// value the store rounds to bfloat16 is the exact one's float32 neighbour: a float-computed value is
// some 1e-7 off, and where the exact one lies that close to the midpoint of two bfloat16 values it
// rounds to the wrong one of the two, a whole bfloat16 step away (a few entries in 10^5).
template <int OFF, int K, typename R>
DEV void grad_head(float *row, uint32_t vb, uint32_t a, float g_lp, float g_en, bool &bad) {
  if (vb == 0u) {
#pragma unroll
    for (int j = 0; j < K; j++) row[OFF + j] = 0.0f;
    return;
  }
  R d[K], w[K], Z, S;
  float m;
  if (!head_terms<OFF, K, R>(row, vb, a, d, w, m, Z, S)) {
    bad = true;                                            // (the whole row is stored as zeros)
    return;
  }
  const R rz = (R)1 / Z, c = S * rz;
#pragma unroll
  for (int j = 0; j < K; j++) {
    const R p = w[j] * rz;
    const R g = (R)g_lp * (((uint32_t)j == a ? (R)1 : (R)0) - p) - (R)g_en * (p * (d[j] - c));
    row[OFF + j] = (vb >> j) & 1u ? (float)g : 0.0f;
  }
}

DEV uint32_t bf16_round(float f) {                         // round to nearest even; NaN stays NaN
  const uint32_t u = __float_as_uint(f);
  return f != f ? 0x7fc0u : (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

template <bool BF16, bool VEC>
__global__ void __launch_bounds__(kTile *kWaves) k_policy_eval(EvalArgs a) {
  __shared__ float tile[kTile * kRowStride];
  __shared__ uint32_t mbits[kTile * 3];
  __shared__ float part[(kWaves - 1) * 3 * kTile];         // waves 1..3: logp, entropy, bad
  constexpr int T = kTile * kWaves;
  const int tid = (int)threadIdx.x, lane = tid & (kTile - 1), wave = tid / kTile;
  const size_t base = (size_t)blockIdx.x * kTile;
  const int rows = a.n - base < (size_t)kTile ? (int)(a.n - base) : kTile;
  const size_t i = base + lane;
  const bool live = lane < rows;
  uint32_t act = 0, act4 = 0;                              // the wave's action byte (wave 3: bytes 3 and 4)
  if (live) {
    const uint8_t *rec = a.actions + i * a.action_stride;
    act = rec[wave];
    if (wave == 3) act4 = rec[4];
  }
  stage_masks<T>(mbits, a.masks, COG_MASK_BYTES, nullptr, base, rows, tid);
  stage_logits<BF16, VEC, T>(tile, a.logits, a.ld, base, rows, tid);
  __syncthreads();

  float logp = 0.0f, ent = 0.0f;
  bool bad = false;
  if (live) {
    const float *row = tile + lane * kRowStride;
    const HeadBits vb = head_bits(mbits, lane);
    if (wave == 0) eval_head<COG_MASK_PLAY, 22>(row, vb.play, act, logp, ent, bad);
    if (wave == 1) eval_head<COG_MASK_SPECIAL, 22>(row, vb.special, act, logp, ent, bad);
    if (wave == 2) eval_head<COG_MASK_REMOVE, 22>(row, vb.remove, act, logp, ent, bad);
    if (wave == 3) {
      eval_head<COG_MASK_MOVE, 7>(row, vb.move, act, logp, ent, bad);
      eval_head<COG_MASK_SHOP, 19>(row, vb.shop, act4, logp, ent, bad);
    }
  }
  if (wave > 0) {
    float *p = part + (wave - 1) * 3 * kTile + lane;
    p[0] = logp;
    p[kTile] = ent;
    p[2 * kTile] = bad ? 1.0f : 0.0f;
  }
  __syncthreads();
  if (wave > 0 || !live) return;
#pragma unroll
  for (int w = 1; w < kWaves; w++) {
    const float *p = part + (w - 1) * 3 * kTile + lane;
    logp += p[0];
    ent += p[kTile];
    bad = bad || p[2 * kTile] != 0.0f;
  }
  if (a.logp) a.logp[i] = bad ? __uint_as_float(0x7fc00000u) : logp;
  if (a.entropy) a.entropy[i] = bad ? __uint_as_float(0x7fc00000u) : ent;
}

template <bool BF16, bool VEC>
__global__ void __launch_bounds__(kTile *kWaves) k_policy_eval_backward(EvalArgs a) {
  __shared__ float tile[kTile * kRowStride];
  __shared__ uint32_t mbits[kTile * 3];
  __shared__ uint32_t badrow[kWaves * kTile];              // per wave and row: its head is degenerate / the action illegal
  constexpr int T = kTile * kWaves;
  const int tid = (int)threadIdx.x, lane = tid & (kTile - 1), wave = tid / kTile;
  const size_t base = (size_t)blockIdx.x * kTile;
  const int rows = a.n - base < (size_t)kTile ? (int)(a.n - base) : kTile;
  const size_t i = base + lane;
  const bool live = lane < rows;
  uint32_t act = 0, act4 = 0;
  float g_lp = 0.0f, g_en = 0.0f;
  if (live) {
    const uint8_t *rec = a.actions + i * a.action_stride;
    act = rec[wave];
    if (wave == 3) act4 = rec[4];
    if (a.g_logp) g_lp = a.g_logp[i];
    if (a.g_entropy) g_en = a.g_entropy[i];
  }
  stage_masks<T>(mbits, a.masks, COG_MASK_BYTES, nullptr, base, rows, tid);
  stage_logits<BF16, VEC, T>(tile, a.logits, a.ld, base, rows, tid);
  __syncthreads();

  using R = typename std::conditional<BF16, double, float>::type;   // (see grad_head)
  bool bad = false;
  if (live) {
    float *row = tile + lane * kRowStride;
    const HeadBits vb = head_bits(mbits, lane);
    if (wave == 0) grad_head<COG_MASK_PLAY, 22, R>(row, vb.play, act, g_lp, g_en, bad);
    if (wave == 1) grad_head<COG_MASK_SPECIAL, 22, R>(row, vb.special, act, g_lp, g_en, bad);
    if (wave == 2) grad_head<COG_MASK_REMOVE, 22, R>(row, vb.remove, act, g_lp, g_en, bad);
    if (wave == 3) {
      grad_head<COG_MASK_MOVE, 7, R>(row, vb.move, act, g_lp, g_en, bad);
      grad_head<COG_MASK_SHOP, 19, R>(row, vb.shop, act4, g_lp, g_en, bad);
    }
  }
  badrow[tid] = bad ? 1u : 0u;
  __syncthreads();

  // the tile is rows x 23 quads of the contiguous output; quad q is columns 4 (q % 23).. of row q / 23
  const int total = rows * kQuads;
  auto quad = [&](int q, float (&v)[4]) {
    const int row = q / kQuads;
    const bool zero = (badrow[row] | badrow[kTile + row] | badrow[2 * kTile + row] | badrow[3 * kTile + row]) != 0u;
    const float *p = tile + row * kRowStride + 4 * (q % kQuads);
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = zero ? 0.0f : p[k];
  };
  if (!BF16) {
    float *out = static_cast<float *>(a.grad) + base * kCols;
#pragma unroll
    for (int k = 0; k < (kTile * kQuads + T - 1) / T; k++) {
      const int q = k * T + tid;
      if (q < total) {
        float v[4];
        quad(q, v);
        *reinterpret_cast<float4 *>(out + 4 * (size_t)q) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  } else {
    // a 16-B granule holds two quads of 8 B; the block's last granule may be half of one
    uint16_t *out = static_cast<uint16_t *>(a.grad) + base * kCols;
#pragma unroll
    for (int k = 0; k < (kTile * kQuads / 2 + T - 1) / T; k++) {
      const int p = k * T + tid, g = 2 * p;
      if (g < total) {
        float v[4];
        quad(g, v);
        const uint2 lo = make_uint2(bf16_round(v[0]) | bf16_round(v[1]) << 16, bf16_round(v[2]) | bf16_round(v[3]) << 16);
        if (g + 1 < total) {
          quad(g + 1, v);
          *reinterpret_cast<uint4 *>(out + 8 * (size_t)p) =
              make_uint4(lo.x, lo.y, bf16_round(v[0]) | bf16_round(v[1]) << 16, bf16_round(v[2]) | bf16_round(v[3]) << 16);
        } else {
          *reinterpret_cast<uint2 *>(out + 8 * (size_t)p) = lo;
        }
      }
    }
  }
}

// ---- per-seat advantage estimation (include/cog.h cog_policy_gae) -------------------------------
// One lane per (env, seat): lane 4 i + p walks env i's rows from T - 1 down to 0 with seat p's three
// scalars (next value, advantage at its next own row, pending reward) in registers, so no state is
// selected by a runtime seat index.  The lanes of a wave read rewards[t] as one contiguous run of
// floats; the four lanes of an env read the same values / agents / dones element, and the lane whose
// seat acts at row t stores the two outputs.  A row's addresses do not depend on the recursion, so
// the loads of kGaeRows rows are issued ahead of the chain, which is a few multiplies and adds per
// row (not contracted: the library is built with -ffp-contract=off); the rows left over at the bottom
// of the window go through the same batch with the row index clamped into the window and the
// arithmetic skipped, not through a loop of dependent single-row loads.  No atomics, no LDS: the
// same inputs give the same bits.  8 rows ahead in workgroups of 256 measured fastest of 4 / 8 / 16 /
// 24 / 32 rows x 64 / 128 / 256 threads at every shape: from 16 rows on the row
// bases no longer fit the scalar registers (40 of them spill at 16 rows, 223 at 32).

constexpr int kGaeRows = 8;                                // rows loaded ahead of the chain
constexpr int kGaeBlock = 256;                             // threads per workgroup: 64 envs

struct GaeArgs {
  size_t T, n;
  const float *values;
  size_t values_ld;
  const uint8_t *agents;
  size_t agents_ld;
  const float *rewards;
  size_t rewards_ld;                                       // floats
  const uint8_t *dones;
  size_t dones_ld;
  const float *last_values;                                // [n][4], or null: zeros
  float gamma, lam;
  float *advantages, *returns;                             // row stride n
};

struct GaeSeat {
  float nv, adv, rew;                                      // next value, next own advantage, pending reward
};

// rows top, top - 1, .. (cnt of them; FULL: kGaeRows) of env i for the lane of seat p (g = 4 i + p)
template <bool FULL>
DEV void gae_rows(const GaeArgs &a, size_t top, int cnt, size_t i, size_t g, uint32_t p, float gl, GaeSeat &s) {
  float v[kGaeRows], r[kGaeRows];
  uint32_t ag[kGaeRows], dn[kGaeRows];
#pragma unroll
  for (int k = 0; k < kGaeRows; k++) {
    const size_t t = FULL || k < cnt ? top - (size_t)k : 0;   // (a row of the window in any case)
    v[k] = a.values[t * a.values_ld + i];
    ag[k] = a.agents[t * a.agents_ld + i];
    dn[k] = a.dones[t * a.dones_ld + i];
    r[k] = a.rewards[t * a.rewards_ld + g];
  }
#pragma unroll
  for (int k = 0; k < kGaeRows; k++) {
    if (FULL || k < cnt) {
      if (dn[k] != 0u) {                                   // (the only use of a reward: elsewhere it may be NaN)
        s.nv = 0.0f;
        s.adv = 0.0f;
        s.rew = r[k];
      }
      if ((ag[k] & 3u) == p) {
        const float delta = s.rew + a.gamma * s.nv - v[k];
        s.adv = delta + gl * s.adv;
        const size_t o = (top - (size_t)k) * a.n + i;
        a.advantages[o] = s.adv;
        a.returns[o] = s.adv + v[k];
        s.nv = v[k];
        s.rew = 0.0f;
      }
    }
  }
}

__global__ void __launch_bounds__(kGaeBlock) k_turn_gae(GaeArgs a) {
  const size_t g = (size_t)blockIdx.x * kGaeBlock + threadIdx.x, i = g >> 2;
  if (i >= a.n) return;
  const uint32_t p = (uint32_t)g & 3u;
  GaeSeat s{a.last_values ? a.last_values[g] : 0.0f, 0.0f, 0.0f};
  const float gl = a.gamma * a.lam;
  size_t left = a.T;                                       // rows 0 .. left - 1 are still to do
  for (; left >= (size_t)kGaeRows; left -= kGaeRows) gae_rows<true>(a, left - 1, kGaeRows, i, g, p, gl, s);
  if (left) gae_rows<false>(a, left - 1, (int)left, i, g, p, gl, s);
}

// ---- policy features (include/cog.h cog_env_policy_features) ------------------------------------
// Two tensors per env, seen from one seat: vec, 208 flat values, and local, 10 channels over a
// W x W window of the map centred on the seat's own cell (W = 2 radius + 1); the layout is in cog.h
// and DESIGN.md section 5.  The kernel reads little (the 64 B of shared scalars, four 112-B DeckObs
// heads and 32 B of EnvPriv per env, W^2 hex codes of cgrid) and writes much (416 + 1,620 B per env
// at radius 4 in bfloat16), so it is shaped by its stores, as the encode is: a workgroup takes a
// tile of envs, stages what it reads in LDS with 16-B loads, builds each env's vec row (floats) and
// window (one word per cell: three bits per channel -- the six map features of its hex code, one
// channel per relative seat standing there, the in-grid channel; built once per cell, not per element)
// in LDS, and then streams the tile's part of each output tensor as 16-B chunks in address
// order, consecutive lanes on consecutive chunks.  An env's local row is 20 W^2 bytes in bfloat16,
// never a multiple of 16, and an out= slice is aligned to its element only, so the chunks are those
// of the tensor's own address range (chunk -> env by a reciprocal multiply), and the elements before the tile's
// first and after its last whole chunk are stored one by one.  Every value is an integer below 2^24
// or a float32 copied from the record, so float32 is exact and bfloat16 is its round to nearest
// even.  No atomics; every cgrid index is bounded by the window's own in-grid test before the read.
// Measured (profiles/policy_features_time.txt): 120 us per call at 65,536 envs,
// radius 4, bfloat16 -- a fifth of the copy peak: the chain of a workgroup's phases bounds it, not the stores.

constexpr int kFeatBlock = 256;                            // threads per workgroup
constexpr int kFeatTile = 16;                              // envs per workgroup, at most
constexpr int kFeatLds = 48 * 1024;                        // LDS a workgroup may take (fewer envs at a large radius)
// an env's staged bytes: ObsData 16128..16191 (phase, resources, shop), each player's first 112 B
// (the 105 of DeckObs), EnvPriv bytes 16..47 (n_players, map bounds, player locations)
constexpr int kFsDeck = 64, kFsDeckStride = 112, kFsPriv = kFsDeck + 4 * kFsDeckStride, kFsBytes = kFsPriv + 32;
constexpr int kFsChunks = kFsBytes / 16;                   // 34
constexpr int kFsPrivFrom = 16;                            // first staged byte of EnvPriv
static_assert(offsetof(EnvPriv, n_players) == 16 && offsetof(EnvPriv, minx) == 32 && offsetof(EnvPriv, miny) == 33 &&
                  offsetof(EnvPriv, locx) == 40 && offsetof(EnvPriv, locy) == 44,
              "the staged part of EnvPriv");
static_assert(COG_OBS_PLAYER0 - COG_OBS_PHASE == kFsDeck && COG_OBS_PHASE % 16 == 0 && COG_OBS_BYTES % 16 == 0, "staged ObsData");
constexpr int kFsSums = 16;                                // per env: hand and draw sizes of the four players, uint16 each
constexpr int feat_lds_per_env(int w2) { return kFsBytes + kFsSums + kFeatVec * 4 + 4 * (w2 + w2 / 8 + 1) + 1; }

// n / d for n < 2^19 and d < 2^15 (element and cell indices of a tile) as one 64-bit multiply:
// m = ceil(2^40 / d), and n (m d - 2^40) < 2^40 makes the quotient exact
constexpr uint64_t feat_magic(uint32_t d) { return ((1ull << 40) + d - 1) / d; }
DEV int feat_div(int n, uint64_t m) { return (int)(((uint64_t)(uint32_t)n * m) >> 40); }

struct FeatArgs {
  size_t n;
  const uint8_t *obs;
  const EnvPriv *priv;
  const uint8_t *agent, *cgrid, *seats;
  int seat, radius, tile;
  uint64_t m_w, m_w2, m_row;                               // feat_magic of W, W^2, 10 W^2
  void *vec, *local;
};

// what the staged bytes S of an env say
DEV int fs_players(const uint8_t *S) { return min((int)S[kFsPriv + offsetof(EnvPriv, n_players) - kFsPrivFrom], 4); }
DEV int fs_ix(const uint8_t *S, int p) {
  const int8_t *P = reinterpret_cast<const int8_t *>(S + kFsPriv - kFsPrivFrom);
  return (int)P[offsetof(EnvPriv, locx) + p] - (int)P[offsetof(EnvPriv, minx)] + 1;
}
DEV int fs_iy(const uint8_t *S, int p) {
  const int8_t *P = reinterpret_cast<const int8_t *>(S + kFsPriv - kFsPrivFrom);
  return (int)P[offsetof(EnvPriv, locy) + p] - (int)P[offsetof(EnvPriv, miny)] + 1;
}
DEV const uint8_t *fs_deck(const uint8_t *S, int p) { return S + kFsDeck + kFsDeckStride * p; }
DEV int fs_relative(int s, int r, int np) { return s + r >= np ? s + r - np : s + r; }   // (s + r) mod np; s, r < np

// value idx of the vec row of seat s (< np); sums: the env's [player][hand, draw] sizes
DEV float feat_vec_value(const uint8_t *S, const uint16_t *sums, int s, int np, int idx) {
  if (idx == 0) return (float)S[0];
  if (idx < 4) return reinterpret_cast<const float *>(S + (COG_OBS_RES - COG_OBS_PHASE))[idx - 1];
  if (idx < 22) return (float)S[COG_OBS_SHOP - COG_OBS_PHASE + idx - 4];
  if (idx == 22) return (float)np;
  if (idx == 23) return (float)fs_ix(S, s);
  if (idx == 24) return (float)fs_iy(S, s);
  if (idx < 130) return (float)fs_deck(S, s)[idx - 25];
  const int r = (idx - 130) / 26 + 1, k = (idx - 130) % 26;
  if (r >= np) return 0.0f;
  const int p = fs_relative(s, r, np);
  const uint8_t *D = fs_deck(S, p);
  int v = 0;
  if (k == 0) v = 1;
  else if (k == 1) v = fs_ix(S, p) - fs_ix(S, s);
  else if (k == 2) v = fs_iy(S, p) - fs_iy(S, s);
  else if (k < 5) v = sums[2 * p + (k - 3)];               // cards in hand (3), in draw (4)
  else {                                                   // a card type's total over the five piles
    const int t = k - 5;
    v = D[COG_DECK_DRAW + t] + D[COG_DECK_HAND + t] + D[COG_DECK_ACTIVE + t] + D[COG_DECK_PLAYED + t] + D[COG_DECK_DISCARD + t];
  }
  return (float)v;
}

// A window cell's word: three bits per channel, channel c at bits 3 c .. 3 c + 2 -- the encode's
// feat(code, 1..6) of its hex code (c = 0..5), relative seat r stands there (c = 5 + r), inside the
// grid (c = 9); 0 for a cell outside the grid.  Words sit in LDS at index i + (i >> 3): the lanes of
// a wave read cells 8 apart, and the skew spreads them over the banks.
DEV uint32_t feat_cell_word(uint32_t code) {
  uint32_t w = 1u << 27;
#pragma unroll
  for (int c = 0; c < 6; c++) w |= feat(code, c + 1) << (3 * c);
  return w;
}
DEV int feat_skew(int i) { return i + (i >> 3); }

struct FeatVecFill {                                       // element j of the tile's vec rows
  static constexpr bool kSmall = false;
  const float *vecL;
  template <int M>
  DEV void operator()(int j, float (&v)[M]) const {
#pragma unroll
    for (int k = 0; k < M; k++) v[k] = vecL[j + k];
  }
};
struct FeatLocalFill {                                     // element j of the tile's local rows
  static constexpr bool kSmall = true;                     // integers 0..7: exact in bfloat16 as they are
  const uint32_t *cellL;
  int w2;
  uint64_t m_w2, m_row;
  template <int M>
  DEV void operator()(int j, float (&v)[M]) const {
    const int row = kFeatChannels * w2, env = feat_div(j, m_row), rem = j - env * row, c = feat_div(rem, m_w2);
    int cell = rem - c * w2, i = env * w2 + cell, sh = 3 * c;   // i: the cell's index in the tile
#pragma unroll
    for (int k = 0; k < M; k++) {
      v[k] = (float)((cellL[feat_skew(i)] >> sh) & 7u);
      ++i;
      if (++cell == w2) {                                  // the next channel of this env, or the next env
        cell = 0;
        sh += 3;
        i -= w2;
        if (sh == 3 * kFeatChannels) {
          sh = 0;
          i += w2;
        }
      }
    }
  }
};

// SMALL: v is an integer of at most 8 bits, whose float32 form has nothing below bfloat16's last bit
template <bool SMALL>
DEV uint32_t feat_bf16(float v) { return SMALL ? __float_as_uint(v) >> 16 : bf16_round(v); }

template <bool BF16, bool SMALL>
DEV void feat_store(void *p, float v) {
  if (BF16) *static_cast<uint16_t *>(p) = (uint16_t)feat_bf16<SMALL>(v);
  else *static_cast<float *>(p) = v;
}

// elements [first, first + count) of the tensor at `base`, the tile's share: whole 16-B chunks of
// the address range by 16-B stores, the elements before the first and after the last one by one
template <bool BF16, typename Fill>
DEV void feat_stream(void *base, size_t first, int count, int tid, const Fill &fill) {
  constexpr int ES = BF16 ? 2 : 4, PER = 16 / ES;
  constexpr bool SM = Fill::kSmall;
  uint8_t *out = static_cast<uint8_t *>(base) + first * ES;
  const int head = min(count, (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15u)) & 15u) / ES));
  const int chunks = (count - head) / PER, tail = head + chunks * PER;
  if (tid < head) {
    float v[1];
    fill(tid, v);
    feat_store<BF16, SM>(out + (size_t)tid * ES, v[0]);
  }
  const int t = tail + tid - 64;                           // (the second wave's lanes: the head is the first's)
  if (tid >= 64 && t < count) {
    float v[1];
    fill(t, v);
    feat_store<BF16, SM>(out + (size_t)t * ES, v[0]);
  }
  uint4 *out16 = reinterpret_cast<uint4 *>(out + (size_t)head * ES);
  for (int q = tid; q < chunks; q += kFeatBlock) {
    float v[PER];
    fill(head + q * PER, v);
    if constexpr (BF16)
      out16[q] = make_uint4(feat_bf16<SM>(v[0]) | feat_bf16<SM>(v[1]) << 16, feat_bf16<SM>(v[2]) | feat_bf16<SM>(v[3]) << 16,
                            feat_bf16<SM>(v[4]) | feat_bf16<SM>(v[5]) << 16, feat_bf16<SM>(v[6]) | feat_bf16<SM>(v[7]) << 16);
    else
      out16[q] = make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
  }
}

template <bool BF16>
__global__ void __launch_bounds__(kFeatBlock) k_policy_features(FeatArgs a) {
  extern __shared__ uint4 feat_lds[];
  const int tid = (int)threadIdx.x, radius = a.radius, W = 2 * radius + 1, w2 = W * W;
  const size_t base = (size_t)blockIdx.x * (size_t)a.tile;
  const int rows = a.n - base < (size_t)a.tile ? (int)(a.n - base) : a.tile;
  uint8_t *stage = reinterpret_cast<uint8_t *>(feat_lds);
  uint16_t *sumL = reinterpret_cast<uint16_t *>(stage + a.tile * kFsBytes);
  float *vecL = reinterpret_cast<float *>(stage + a.tile * (kFsBytes + kFsSums));
  uint32_t *cellL = reinterpret_cast<uint32_t *>(vecL + a.tile * kFeatVec);
  uint8_t *seatL = reinterpret_cast<uint8_t *>(cellL + a.tile * (w2 + w2 / 8 + 1));

  for (int q = tid; q < rows * kFsChunks; q += kFeatBlock) {
    const int e = q / kFsChunks, c = q % kFsChunks;
    const size_t i = base + e;
    const uint8_t *src;
    if (c < 4) src = a.obs + i * COG_OBS_BYTES + COG_OBS_PHASE + 16 * c;
    else if (c < 32) src = a.obs + i * COG_OBS_BYTES + COG_OBS_PLAYER0 + COG_OBS_PLAYER_STRIDE * ((c - 4) / 7) + 16 * ((c - 4) % 7);
    else src = reinterpret_cast<const uint8_t *>(a.priv + i) + kFsPrivFrom + 16 * (c - 32);
    reinterpret_cast<uint4 *>(stage + e * kFsBytes)[c] = *reinterpret_cast<const uint4 *>(src);
    if (c == 0) seatL[e] = (uint8_t)((a.seats ? a.seats[i] : a.seat >= 0 ? (uint32_t)a.seat : a.agent[i]) & 3u);
  }
  __syncthreads();

  for (int q = tid; q < rows * 8; q += kFeatBlock) {       // every player's cards in hand and in draw
    const uint8_t *pile = fs_deck(stage + (q >> 3) * kFsBytes, (q >> 1) & 3) + (q & 1 ? COG_DECK_DRAW : COG_DECK_HAND);
    uint32_t v = 0;
#pragma unroll
    for (int t = 0; t < COG_N_CARDTYPES_; t++) v += pile[t];
    sumL[q] = (uint16_t)v;
  }
  for (int q = tid; q < rows * w2; q += kFeatBlock) {
    const int e = feat_div(q, a.m_w2), cell = q - e * w2, ca = feat_div(cell, a.m_w), cb = cell - ca * W;
    const uint8_t *S = stage + e * kFsBytes;
    const int s = seatL[e], np = fs_players(S);
    uint32_t w = 0;
    if (s < np) {
      const int cx = fs_ix(S, s) - radius + ca, cy = fs_iy(S, s) - radius + cb;
      if ((uint32_t)cx < (uint32_t)COG_GRIDSIZE_ && (uint32_t)cy < (uint32_t)COG_GRIDSIZE_) {   // the only cgrid read
        w = feat_cell_word(a.cgrid[(base + e) * COG_CELLS + cx * COG_GRIDSIZE_ + cy]);
        for (int r = 1; r < np; r++) {
          const int p = fs_relative(s, r, np);
          if (fs_ix(S, p) == cx && fs_iy(S, p) == cy) w |= 1u << (3 * (5 + r));
        }
      }
    }
    cellL[feat_skew(q)] = w;
  }
  __syncthreads();
  for (int q = tid; q < rows * kFeatVec; q += kFeatBlock) {
    const int e = q / kFeatVec, idx = q % kFeatVec;
    const uint8_t *S = stage + e * kFsBytes;
    const int s = seatL[e], np = fs_players(S);
    vecL[q] = s < np ? feat_vec_value(S, sumL + 8 * e, s, np, idx) : 0.0f;
  }
  __syncthreads();

  feat_stream<BF16>(a.vec, base * kFeatVec, rows * kFeatVec, tid, FeatVecFill{vecL});
  feat_stream<BF16>(a.local, base * (size_t)(kFeatChannels * w2), rows * kFeatChannels * w2, tid, FeatLocalFill{cellL, w2, a.m_w2, a.m_row});
}

}  // namespace

int launch_policy_features(const PolicyFeatures &p, void *stream) {
  if (!p.n) return 0;
  const int W = 2 * p.radius + 1, w2 = W * W;
  const int fit = kFeatLds / feat_lds_per_env(w2), tile = fit < kFeatTile ? fit : kFeatTile;   // >= 4 (radius 24)
  const FeatArgs a{p.n, p.obs, p.priv, p.agent, p.cgrid, p.seats, p.seat,
                   p.radius, tile, feat_magic(W), feat_magic(w2), feat_magic(kFeatChannels * w2), p.vec, p.local};
  const dim3 grid((unsigned)((p.n + tile - 1) / tile));
  const size_t lds = (size_t)tile * feat_lds_per_env(w2) + 16;
  if (p.bf16)
    hipLaunchKernelGGL(k_policy_features<true>, grid, dim3(kFeatBlock), lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(k_policy_features<false>, grid, dim3(kFeatBlock), lds, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_turn_gae(const TurnGae &p, void *stream) {
  if (!p.T || !p.n) return 0;
  const GaeArgs a{p.T,     p.n,        p.values,      p.values_ld, p.agents, p.agents_ld,  p.rewards, p.rewards_ld,
                  p.dones, p.dones_ld, p.last_values, p.gamma,     p.lam,    p.advantages, p.returns};
  const dim3 grid((unsigned)((4 * p.n + kGaeBlock - 1) / kGaeBlock));
  hipLaunchKernelGGL(k_turn_gae, grid, dim3(kGaeBlock), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_policy_eval(const PolicyEval &p, bool backward, void *stream) {
  if (!p.n) return 0;
  const EvalArgs a{p.n, p.logits, p.ld, p.actions, p.action_stride, p.masks, p.logp, p.entropy, p.g_logp, p.g_entropy, p.grad};
  const dim3 grid((unsigned)((p.n + kTile - 1) / kTile)), block(kTile * kWaves);
  hipStream_t st = (hipStream_t)stream;
  const bool aligned = (reinterpret_cast<uintptr_t>(p.logits) & 15u) == 0;
  const bool vec = aligned && (p.bf16 ? p.ld == (size_t)kCols || p.ld % 8 == 0 : p.ld % 4 == 0);   // (as the sampler)
#define COG_EVAL_LAUNCH(B, V)                                                                   \
  do {                                                                                          \
    if (backward)                                                                               \
      hipLaunchKernelGGL((k_policy_eval_backward<B, V>), grid, block, 0, st, a);                \
    else                                                                                        \
      hipLaunchKernelGGL((k_policy_eval<B, V>), grid, block, 0, st, a);                         \
  } while (0)
  if (p.bf16) {
    if (vec) COG_EVAL_LAUNCH(true, true); else COG_EVAL_LAUNCH(true, false);
  } else {
    if (vec) COG_EVAL_LAUNCH(false, true); else COG_EVAL_LAUNCH(false, false);
  }
#undef COG_EVAL_LAUNCH
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_policy_sample(const PolicyLaunch &p, void *stream) {
  if (!p.n) return 0;
  const PolicyArgs a{p.n, p.logits, p.ld, p.mask_base, p.mask_stride, p.agent, p.rng, p.actions, p.logp, p.entropy};
  const dim3 grid((unsigned)((p.n + kTile - 1) / kTile));
  hipStream_t st = (hipStream_t)stream;
  const bool aligned = (reinterpret_cast<uintptr_t>(p.logits) & 15u) == 0;
  if (p.bf16) {
    if (aligned && (p.ld == (size_t)kCols || p.ld % 8 == 0))
      launch_form<true, true>(a, p.greedy != 0, grid, st);
    else
      launch_form<true, false>(a, p.greedy != 0, grid, st);
  } else {
    if (aligned && p.ld % 4 == 0)
      launch_form<false, true>(a, p.greedy != 0, grid, st);
    else
      launch_form<false, false>(a, p.greedy != 0, grid, st);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace cog
