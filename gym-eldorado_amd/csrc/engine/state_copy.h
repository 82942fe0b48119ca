// engine/state_copy.h -- state snapshots: part of cog_engine.hip's translation unit, included at
// its very end inside namespace cog, so that every kernel before it keeps its place in the code
// object.  Needs DEV, DevState and the kSnap* layout (cog_engine.h), encode_block and kEncBlocks
// (the map-observation encode), u32x4_t, blocks_for and launched.
//
// A snapshot holds one record of kSnapBytes (4,032 B, 252 granules of 16 B) per env, laid out as
// cog_engine.h describes: granules 0..107 the small arrays (`head`), 108..251 the compact code
// grid.  The save is a coalesced copy into it.  The restore is the gather: wave w of a workgroup
// takes destination env 4 blockIdx + w, reads record src[env] once (a one-source fork reads it from
// L2), scatters the head granules into the handle's arrays, copies the code grid and encodes the
// 16,128-B map observation from it through LDS, so that every store instruction of the map writes
// 1 KiB contiguous (encode_block's 112 B per lane, transposed as k_encode_lds does), with
// non-temporal stores: the map is written once and read by nobody in this launch.
//
// What is not in a record, and why that is enough: `grid` and `gen` are read by map generation
// alone, which starts by clearing the box EnvPriv::minx..maxy from `grid` (coop_map_reset) and
// writes every GenScratch field before it reads it.  The box is the one thing that crosses a
// reset, and it arrives with the source's EnvPriv while `grid` still holds the destination's old
// map.  So the restore clears the destination's old box itself, before EnvPriv is overwritten:
// `grid` is then empty, which every box covers.

constexpr int kSnapGranules = (int)(kSnapBytes / 16), kSnapHeadGranules = (int)(kSnapCgrid / 16);   // 252, 108
constexpr int kSnapUsedHead = (int)(kSnapMisc / 16);                                                 // 104: done | agent
static_assert(kSnapGranules - kSnapHeadGranules == kEncBlocks, "one code-grid granule per encode block");

// the granule of env i's state that head granule g < kSnapUsedHead of its record holds
DEV uint4 *state_granule(const DevState &s, size_t i, int g) {
  constexpr int gSel = (int)(kSnapSel / 16), gInfo = (int)(kSnapInfo / 16), gRew = (int)(kSnapRew / 16);
  constexpr int gPriv = (int)(kSnapPriv / 16), gHeads = (int)(kSnapHeads / 16);
  uint8_t *p;
  if (g < gSel) p = s.obs + i * COG_OBS_BYTES + COG_OBS_MAP_BYTES + 16 * g;
  else if (g < gInfo) p = s.sel + i * COG_MASK_BYTES + 16 * (g - gSel);
  else if (g < gRew) p = s.info + i * COG_INFO_BYTES + 16 * (g - gInfo);
  else if (g < gPriv) p = reinterpret_cast<uint8_t *>(s.rew + 4 * i);
  else if (g < gHeads) p = reinterpret_cast<uint8_t *>(s.priv + i) + 16 * (g - gPriv);
  else p = reinterpret_cast<uint8_t *>(s.heads + 5 * i + (g - gHeads));
  return reinterpret_cast<uint4 *>(p);
}

__global__ void __launch_bounds__(256) k_state_save(DevState s, uint4 *__restrict__ snap, size_t n_granules) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_granules) return;
  const size_t i = t / kSnapGranules;
  const int g = (int)(t - i * kSnapGranules);
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (g >= kSnapHeadGranules) v = reinterpret_cast<const uint4 *>(s.cgrid + i * COG_CELLS)[g - kSnapHeadGranules];
  else if (g < kSnapUsedHead) v = *state_granule(s, i, g);
  else if (g == kSnapUsedHead) v.x = (uint32_t)s.done[i] | (uint32_t)s.agent[i] << 8;
  snap[t] = v;
}

template <class IDX>
__global__ void __launch_bounds__(256) k_src_check(const IDX *__restrict__ src, size_t n, size_t n_snap,
                                                   uint32_t *__restrict__ bad) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const IDX v = src[j];
  if (v < (IDX)0 || (unsigned long long)v >= (unsigned long long)n_snap) *bad = 1u;
}

constexpr int kRestoreWaves = 4;                          // destination envs per workgroup
template <class IDX>
__global__ void __launch_bounds__(64 * kRestoreWaves) k_state_restore(DevState s, const uint4 *__restrict__ snap,
                                                                      const IDX *__restrict__ src) {
  __shared__ uint4 stage[kRestoreWaves][64 * 7];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const size_t j = (size_t)blockIdx.x * kRestoreWaves + wave;
  const bool live = j < s.n;                               // (wave-uniform; every wave meets the barriers)
  const uint4 *rec = snap + (live ? (src ? (size_t)src[j] : j) : 0) * kSnapGranules;
  if (live) {
    // the old map's box out of `grid`, in whole granules of its rows (what lies beside the box in
    // them is 0 already); the box is read before EnvPriv is written below, and clamped to the grid
    const uint32_t box = reinterpret_cast<const uint32_t *>(s.priv + j)[offsetof(EnvPriv, minx) / 4];
    const int lo = -kGridOff, hi = kGridDim - kGridOff - 1;
    const int minx = max((int)(int8_t)(box & 0xffu), lo), miny = max((int)(int8_t)((box >> 8) & 0xffu), lo);
    const int maxx = min((int)(int8_t)((box >> 16) & 0xffu), hi), maxy = min((int)(int8_t)(box >> 24), hi);
    const int g = ((miny + kGridOff) >> 4) + (lane & 7), g1 = (maxy + kGridOff) >> 4;
    uint8_t *grid = s.grid + j * (size_t)kGridBytes;
    for (int x = minx + (lane >> 3); x <= maxx; x += 8)
      if (g <= g1) *reinterpret_cast<uint4 *>(grid + (x + kGridOff) * kGridDim + 16 * g) = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int h = lane + 64 * q;
      if (h < kSnapUsedHead) {
        *state_granule(s, j, h) = rec[h];
      } else if (h == kSnapUsedHead) {
        const uint32_t m = rec[h].x;
        s.done[j] = (uint8_t)(m & 0xffu);
        s.agent[j] = (uint8_t)((m >> 8) & 0xffu);
      }
    }
  }
  const uint8_t *cg = reinterpret_cast<const uint8_t *>(rec + kSnapHeadGranules);
  uint8_t *map = s.obs + j * COG_OBS_BYTES;
  uint8_t *st = reinterpret_cast<uint8_t *>(stage[wave]);
#pragma unroll
  for (int p = 0; p < (kEncBlocks + 63) / 64; p++) {
    const int nb = kEncBlocks - 64 * p < 64 ? kEncBlocks - 64 * p : 64;   // blocks of this pass: 64, 64, 16
    if (live && lane < nb) {
      reinterpret_cast<uint4 *>(s.cgrid + j * COG_CELLS)[64 * p + lane] = rec[kSnapHeadGranules + 64 * p + lane];
      encode_block(cg + 1024 * p, st, lane);               // block 64 p + lane -> stage bytes [112 lane, +112)
    }
    __syncthreads();
    if (live) {
      u32x4_t *out = reinterpret_cast<u32x4_t *>(map + 7168 * p);
#pragma unroll
      for (int q = 0; q < 7; q++) {
        const int c = 64 * q + lane;
        if (c < 7 * nb) {
          const uint4 v = stage[wave][c];
          const u32x4_t x = {v.x, v.y, v.z, v.w};
          __builtin_nontemporal_store(x, out + c);
        }
      }
    }
    __syncthreads();
  }
}

int launch_state_save(const DevState &s, uint8_t *snap, void *stream) {
  if (!s.n) return 0;
  const size_t ng = s.n * (size_t)kSnapGranules;
  hipLaunchKernelGGL(k_state_save, dim3(blocks_for(ng, 256)), dim3(256), 0, (hipStream_t)stream, s,
                     reinterpret_cast<uint4 *>(snap), ng);
  return launched();
}

int launch_src_check(const void *src, int src_kind, size_t n, size_t n_snap, uint32_t *bad, void *stream) {
  if (!n) return 0;
  const dim3 g(blocks_for(n, 256)), b(256);
  if (src_kind == SRC_I64)
    hipLaunchKernelGGL(k_src_check<long long>, g, b, 0, (hipStream_t)stream, static_cast<const long long *>(src), n, n_snap, bad);
  else if (src_kind == SRC_U32)
    hipLaunchKernelGGL(k_src_check<uint32_t>, g, b, 0, (hipStream_t)stream, static_cast<const uint32_t *>(src), n, n_snap, bad);
  else
    hipLaunchKernelGGL(k_src_check<int32_t>, g, b, 0, (hipStream_t)stream, static_cast<const int32_t *>(src), n, n_snap, bad);
  return launched();
}

int launch_state_restore(const DevState &s, const uint8_t *snap, const void *src, int src_kind, void *stream) {
  if (!s.n) return 0;
  const dim3 g(blocks_for(s.n, kRestoreWaves)), b(64 * kRestoreWaves);
  const uint4 *rec = reinterpret_cast<const uint4 *>(snap);
  if (src && src_kind == SRC_I64)
    hipLaunchKernelGGL(k_state_restore<long long>, g, b, 0, (hipStream_t)stream, s, rec, static_cast<const long long *>(src));
  else if (src && src_kind == SRC_U32)
    hipLaunchKernelGGL(k_state_restore<uint32_t>, g, b, 0, (hipStream_t)stream, s, rec, static_cast<const uint32_t *>(src));
  else
    hipLaunchKernelGGL(k_state_restore<int32_t>, g, b, 0, (hipStream_t)stream, s, rec, static_cast<const int32_t *>(src));
  return launched();
}
