// The staged-tile moment scheme of gmm_e_kernel (gmm.hip), probe_acc_kernel (probe.hip) and strata_mom_kernel (strata.hip): four waves walk
// tiles of 64 rows in a grid-stride loop, stage x - pivot of a tile once in LDS, share out the 16 x 16 blocks of a product on
// v_mfma_f32_16x16x4_f32 with the accumulators in registers for the whole loop and write one float32 slab in fragment order; a second
// kernel adds the slabs in double.  Each helper states the order it guarantees: the bits of the results rest on it.
#pragma once
#include "frl_common.hpp"
#define MOMENT_ROWS 64                                                           // rows of a tile: 16 per wave

// Row stride in floats of a staged tile [64][cols], cols a multiple of 16: the smallest ys >= cols with ys mod 64 in {20, 44} (not always
// the next multiple of 4: 48 and 64 columns give 84).  The moment sweep reads 4 rows x 16 columns per step (lane = 16 row + column): the
// rows start at banks 0, 20, 40, 60 (or 0, 44, 24, 4) of 64, so only the fourth wraps onto 12 banks of the first, and never within a
// half-wave: nearly conflict-free.  gmm_e_kernel's log-probability product reads 16 rows x 4 columns (lane = row + 16 column): 16 strides
// of 20 or 44 are 16 distinct multiples of 4 mod 64, which the four columns fill up: conflict-free.
static inline int frl_tile_stride(int cols) {
  while (cols % 64 != 20 && cols % 64 != 44) cols += 4;
  return cols;
}
// Observations (b, t, p), p the fastest: tile i is the pixels p0 .. p0 + 63 of one (b, t), PT = ceil(P / 64) tiles per (b, t), in
// (b, t, p0) order.  frl_obs_fit: B T P fits the int32 the kernels count in (the callers say "B * T * P < 2^31 observations").
static inline bool frl_obs_fit(int B, int T, int64_t P) { return P <= 0x7fffffffll && (int64_t)B * T <= 0x7fffffffll && (int64_t)B * T * P <= 0x7fffffffll; }
static inline int frl_moment_tiles(int B, int T, int64_t P, int& PT) { return (int)((int64_t)B * T * (PT = (int)((P + MOMENT_ROWS - 1) / MOMENT_ROWS))); }
// tile -> (b, t, p0); T = 1 where the tiles of a call run over (b, p0) alone
__device__ __forceinline__ void moment_tile(int tile, int PT, int T, int& b, int& t, int& p0) {
  const int bt = tile / PT;
  p0 = (tile - bt * PT) * MOMENT_ROWS, b = bt / T, t = bt - b * T;
}
// rows of the tile at p0 that exist: 64 but for the last tile of a (b, t)
__device__ __forceinline__ int moment_tile_rows(int P, int p0) { return P - p0 < MOMENT_ROWS ? P - p0 : MOMENT_ROWS; }

// Fragment order.  v_mfma_f32_16x16x4_f32 leaves element (row 4 (l >> 4) + r, column l & 15) of a 16 x 16 block in register r of lane l;
// a slab keeps the four registers of lane l of block blk at floats (blk * 64 + l) * 4 + r, so a lane stores its part as one float4.
__device__ __forceinline__ void moment_frag_decode(int e, int& blk, int& row, int& col) {
  const int l = (e >> 2) & 63;
  blk = e >> 8, row = 4 * (l >> 4) + (e & 3), col = l & 15;
}
__device__ __forceinline__ size_t moment_frag_index(int blk, int row, int col) { return ((size_t)blk * 64 + (row >> 2) * 16 + col) * 4 + (row & 3); }

// The slab of a workgroup: wave w owns the blocks w, w + 4, .. below nblk, accumulator i is block w + 4 i.  Stores only, no sum.
template <int NBM>
__device__ __forceinline__ void moment_store_slab(float* slab, const f32x4 (&acc)[NBM], int wave, int lane, int nblk) {
#pragma unroll
  for (int i = 0; i < NBM; ++i) {
    const int blk = wave + 4 * i;
    if (blk < nblk) *reinterpret_cast<f32x4*>(slab + ((size_t)blk * 64 + lane) * 4) = acc[i];
  }
}
// Element e = 64 blockIdx.x + (threadIdx.x & 63) of nslab slabs of slabF floats, added in double by a workgroup of 256 threads: part
// p = threadIdx.x >> 6 adds the slabs p, p + 4, p + 8, .. to +0.0 in slab order, then ((p0 + p1) + p2) + p3.  The threads of part 0 get
// the sum, the others 0.0.  live = false: no such element, nothing is read.  Holds a barrier: every thread calls it, once.  (Not the
// order of slab_reduce_t, frl_reduce.hpp, which is 8 groups x 8 in flight: routing these sums through it would change their bits.)
__device__ __forceinline__ double moment_slab_sum(const float* __restrict__ slabs, int nslab, int slabF, int e, bool live) {
  __shared__ double part[4][64];
  const int l = threadIdx.x & 63, p = threadIdx.x >> 6;
  double s = 0.0;
  if (live) {
#pragma unroll 4
    for (int g = p; g < nslab; g += 4) s += (double)slabs[(size_t)g * slabF + e];
  }
  part[p][l] = s;
  __syncthreads();
  return p == 0 ? ((part[0][l] + part[1][l]) + part[2][l]) + part[3][l] : 0.0;
}
