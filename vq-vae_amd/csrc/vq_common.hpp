// What the three generations of the nearest-code assignment share (vq_assign_chunked.hpp, vq_assign_resident.hpp,
// vq_assign_stream.hpp): constants, the workspace header and control block, the exact float64 distances, the LDS-only barrier and the
// phase stamps of the diagnostic build.
#pragma once
#include "frl_common.hpp"
#include "frl_reduce.hpp"
#include <math.h>

#define VQ_IDX_BITS 7
#define VQ_IDX_MASK 127u        // keys carry a 7-bit index inside groups of 128 codes (8 MFMA row blocks)
#define VQ_MAX_CHUNK 512
#define VQ_FAST_ROWS 128     // parked rows per batch the all-wave path handles (typical: < 1 % of the batch's rows)

#define VQ_SQ_BINS 9           // 32-bit steps of the float32 exponent range, one more for the upper halves
struct VqHeader {           // lives at the start of the workspace (zeroed by hipMemsetAsync every call)
  unsigned enmax_bits;      // (unused; kept for the layout)
  int namb;                 // number of rows flagged for exact re-evaluation (append counter of amb_list / total of the fused path)
  double sq_fix;            // multi-chunk path: squared errors of the re-evaluated rows that are inf / NaN (the finite ones: sq_bins)
  int done;                 // fused path: workgroups that have published their partial results (arrival ticket)
  int pad;
  unsigned long long sq_bins[VQ_SQ_BINS];   // multi-chunk path: exact sum of the squared errors of the re-evaluated rows (vq_sq_bins_add)
};
static_assert(sizeof(VqHeader) <= 256, "the workspace keeps 256 bytes for the header");
struct VqCtl { int done; int namb; int pad[62]; };       // 256 bytes, followed by counts_acc[K]

// Phase stamps of the assignment kernels (diagnostic build only, tools/diag/vq_stamps.hip): VQ_ST(i) adds the ticks since the previous
// stamp to slot i of the wave.  A kernel that stamps declares vq_ts, t_prev, t_begin and w_begin under the same #ifdef.
#ifdef VQ_STAMPS
__device__ unsigned long long* vq_dbg;
#define VQ_ST(i) do { const unsigned long long t_now = __builtin_amdgcn_s_memtime(); if (lane == 0) vq_ts[wave][i] += t_now - t_prev; t_prev = t_now; } while (0)
#else
#define VQ_ST(i) do { } while (0)
#endif

// exact squared distances of row n to the codes k0 and k1 (k1 < 0: only k0) in float64; operands rounded to T first, as everywhere
// in this file.  16-byte loads, four chunks in flight: the caller is one lane per candidate pair, the latency of the loads is all
// there is to hide.
template <typename T, int U = 4>
__device__ __forceinline__ void vq_exact_pair(const T* __restrict__ Z, const float* __restrict__ E, int64_t n, int k0, int k1, int d,
                                              double& d0, double& d1) {
  const T* zr = Z + n * (int64_t)d;
  const float* e0 = E + (int64_t)k0 * d;
  const float* e1 = E + (int64_t)(k1 >= 0 ? k1 : k0) * d;
  double s0 = 0.0, s1 = 0.0;
  if ((d & 7) == 0) {
#pragma unroll U
    for (int j = 0; j < d; j += 8) {
      float zv[8];
      if constexpr (sizeof(T) == 2) {
        Vec<T>::load(zr + j, zv);
      } else {
        Vec<T>::load(zr + j, zv);
        Vec<T>::load(zr + j + 4, zv + 4);
      }
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(e0 + j), a1 = *reinterpret_cast<const f32x4*>(e0 + j + 4);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(e1 + j), b1 = *reinterpret_cast<const f32x4*>(e1 + j + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const double zz = (double)zv[e];
        const double da = zz - (double)to_f32(from_f32<T>(e < 4 ? a0[e & 3] : a1[e & 3]));
        const double db = zz - (double)to_f32(from_f32<T>(e < 4 ? b0[e & 3] : b1[e & 3]));
        s0 = __builtin_fma(da, da, s0);
        s1 = __builtin_fma(db, db, s1);
      }
    }
  } else {
    for (int j = 0; j < d; ++j) {
      const double zz = (double)to_f32(zr[j]);
      const double da = zz - (double)to_f32(from_f32<T>(e0[j])), db = zz - (double)to_f32(from_f32<T>(e1[j]));
      s0 = __builtin_fma(da, da, s0);
      s1 = __builtin_fma(db, db, s1);
    }
  }
  d0 = s0;
  d1 = s1;
}

template <typename T>
__device__ __forceinline__ double vq_exact_one(const T* __restrict__ Z, const float* __restrict__ E, int64_t n, int k, int d) {
  double d0, d1;
  vq_exact_pair<T, 4>(Z, E, n, k, -1, d, d0, d1);        // (k1 < 0: the second row folds away; two 16-byte chunks in flight)
  return d0;
}

// The same float64 distance with both operands taken from LDS (bf16 rows with d = 4 q): z from the parked-row copy, e from the packed
// image (e rounded to bf16 = -0.5 x the packed -2e, exact).  Same channel order and arithmetic as vq_exact_pair: same bits.
template <int NF>
__device__ __forceinline__ double vq_exact_lds(const bf16* __restrict__ zrow, const bf16x8* __restrict__ wl, int code, int d) {
  constexpr int q = NF * 8;
  double s0 = 0.0;
  for (int j = 0; j < d; j += 8) {
    const bf16x8 zv = *reinterpret_cast<const bf16x8*>(zrow + j);
    const bf16x8 pv = wl[((code >> 4) * NF + ((j % q) >> 3)) * 64 + (code & 15) + 16 * (j / q)];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const double da = (double)(float)zv[e] - (double)(-0.5f * (float)pv[e]);
      s0 = __builtin_fma(da, da, s0);
    }
  }
  return s0;
}

// Workgroup barrier of the batch loop: orders LDS traffic only.  __syncthreads() also drains the vector-memory queue, i.e. the first
// barrier behind the epilogue waited for every z_q / index store of the batch to reach memory before the parked rows were looked at.
#define VQ_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// ---------------------------------------------------------------------------------------------
// Tails shared by the assignment kernels.  Each states the order it guarantees: first index on ties, NaN rows to code 0 and
// bit-reproducible statistics rest on them.
// ---------------------------------------------------------------------------------------------

// Ambiguity threshold, relative part: two scores closer than thr_rel * (||z|| + enroot)^2 are re-evaluated in float64.
struct VqThr { float thr_rel, enroot; };
__device__ __forceinline__ VqThr vq_thresholds(int q, float enmax) {
  const float err_rel = (float)(4 * q + 8) * 1.1920929e-7f;            // (d_pad+8) * 2^-23: f32 accumulation of exact products
  const float thr_rel = (3.0517578125e-5f + 2.f * err_rel) * 1.001953125f;   // 2^-15: key truncation of both scores, + 2*err, + margin
  return VqThr{thr_rel, sqrtf(enmax)};
}
// The threshold of one row of a lane-quarter tile: ||z||^2 is one fmaf chain over the lane's channels (fragment s, element e, in that
// order), then the quarters 16 and 32 lanes away are added, in that order; every lane of the row gets the same bits.
template <typename T, int NF>
__device__ __forceinline__ float vq_row_threshold(const LQTile<T, NF>& z, VqThr th) {
  float zn = 0.f;
#pragma unroll
  for (int s = 0; s < NF; ++s)
#pragma unroll
    for (int e = 0; e < DT<T>::FE; ++e) { const float v = lq_get<T, NF>(z, s, e); zn = fmaf(v, v, zn); }
  zn += __shfl_xor(zn, 16, 64);
  zn += __shfl_xor(zn, 32, 64);
  const float sroot = sqrtf(zn) + th.enroot;                       // |score| and every partial sum <= (||z|| + ||e||max)^2
  return sroot * sroot * th.thr_rel + 1e-37f;
}

// z_q of one resolved row for this lane's channel quarter (the codebook row rounded to T, per channel, guarded by d) and the squared
// error against the tile, added to sq_acc as one fmaf chain in channel order.
template <typename T, int NF>
__device__ __forceinline__ void vq_write_row(const LQTile<T, NF>& z, const float* E, T* zq_out, int64_t row, int code,
                                             int d, int kc, float& sq_acc) {
  constexpr int FE = DT<T>::FE, q = NF * FE;
  const float* er = E + (int64_t)code * d + q * kc;
  T* zo = zq_out + row * (int64_t)d + q * kc;
#pragma unroll
  for (int s = 0; s < NF * FE; ++s) {
    if (q * kc + s < d) {
      const float ev = to_f32(from_f32<T>(er[s]));
      zo[s] = from_f32<T>(ev);
      const float df = lq_get<T, NF>(z, s / FE, s % FE) - ev;
      sq_acc = fmaf(df, df, sq_acc);
    }
  }
}

// Exact arg-min of the rows of one 16-row tile over the code blocks [mb0, mb1), by the wave that holds the tile (lane-quarter fragments
// z): the tile is re-scored on the matrix cores against `frags` / `norms` (the packed image and ||e||^2, in LDS or global memory), every
// code < K of a lane with `mine` whose score is <= the row's limit lm is evaluated in float64 in-lane -- up to two pending per lane,
// flushed together by exact(p0, p1, d0, d1) (p1 < 0: only p0) as soon as one lane has both slots taken.  Smallest distance, among equal
// distances the smallest code, within the lane and then over the four lane quarters (16, then 32 lanes away).  A row without any
// candidate (NaN row) returns k = 0x7fffffff: the caller maps k >= K to code 0 once no further merge follows.
struct VqBest { double d; int k; };
template <typename T, int NF, typename Exact>
__device__ __forceinline__ VqBest vq_resolve_inlane(const LQTile<T, NF>& z, const typename DT<T>::frag_t* __restrict__ frags,
                                                    const float* __restrict__ norms, int mb0, int mb1, int K, int lane, bool mine, float lm,
                                                    Exact exact) {
  const int kc = lane >> 4;
  double bestd = 1.0e300;
  int bk = 0x7fffffff, p0 = -1, p1 = -1;
  auto flush = [&]() {
    if (p0 >= 0) {
      double d0, d1;
      exact(p0, p1, d0, d1);
      if (d0 < bestd || (d0 == bestd && p0 < bk)) { bestd = d0; bk = p0; }
      if (p1 >= 0 && (d1 < bestd || (d1 == bestd && p1 < bk))) { bestd = d1; bk = p1; }
    }
    p0 = p1 = -1;
  };
  for (int mb = mb0; mb < mb1; ++mb) {
    f32x4 acc = *reinterpret_cast<const f32x4*>(norms + mb * 16 + 4 * kc);
#pragma unroll
    for (int s = 0; s < NF; ++s) acc = mfma16(frags[(size_t)(mb * NF + s) * 64 + lane], z.f[s], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int code = mb * 16 + 4 * kc + r;
      const bool hit = mine && acc[r] <= lm && code < K;
      if (__builtin_amdgcn_ballot_w64(hit && p1 >= 0) != 0ull) flush();       // a lane with both slots taken: evaluate all pending
      if (hit) { if (p0 < 0) p0 = code; else p1 = code; }
    }
  }
  flush();
#pragma unroll
  for (int off = 16; off <= 32; off <<= 1) {
    const double ob = __shfl_xor(bestd, off, 64);
    const int okk = __shfl_xor(bk, off, 64);
    if (ob < bestd || (ob == bestd && okk < bk)) { bestd = ob; bk = okk; }
  }
  return VqBest{bestd, bk};
}

// The workgroup's LDS histogram to the global accumulator: one integer atomic per used code (order-independent).
template <int NW>
__device__ __forceinline__ void vq_flush_hist(const int* __restrict__ hist, int32_t* __restrict__ counts_acc, int K, int tid) {
  for (int k = tid; k < K; k += NW * 64) {
    const int h = hist[k];
    if (h) atomicAdd(&counts_acc[k], h);
  }
}

// Statistics fold of the one-launch kernels, by the workgroup that took the last ticket (all NW waves call it): the float32 wave partials
// of the squared error and p log p of the histogram are summed in double -- thread i takes the entries i, i + 64 NW, .. in that order,
// wave_sum_d, then thread 0 adds the wave sums in wave order -- so stats do not depend on which workgroup folds.  lane / wave are those
// of tid (passed in: the callers hold them already).  Writes counts_out and
// stats_out = {sum ||z - z_q||^2, perplexity, rows re-evaluated, mean squared error} (and the same four floats to stats_copy when given) and re-arms the control block (histogram
// accumulator, namb, done) for the next call.  red: 2 NW doubles of LDS.
template <int NW>
__device__ __forceinline__ void vq_fold_stats(double* red, int tid, int lane, int wave, const float* partial, int npartial, VqCtl* ctl, int K, int64_t N, int d,
                                              int32_t* __restrict__ counts_out, float* __restrict__ stats_out, float* __restrict__ stats_copy) {
  int32_t* counts_acc = reinterpret_cast<int32_t*>(ctl + 1);
  double sp = 0.0;
  for (int i = tid; i < npartial; i += NW * 64) sp += (double)__hip_atomic_load(&partial[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  double hp = 0.0;
  for (int k = tid; k < K; k += NW * 64) {
    const int c = __hip_atomic_load(&counts_acc[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    counts_out[k] = c;
    __hip_atomic_store(&counts_acc[k], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // clean for the next call
    const double p = (double)c / (double)N;
    hp += p * log(p + 1e-10);
  }
  sp = wave_sum_d(sp);
  hp = wave_sum_d(hp);
  if (lane == 0) { red[wave] = sp; red[NW + wave] = hp; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < NW; ++w) { red[0] += red[w]; red[NW] += red[NW + w]; }     // fixed order
    const float st[4] = {(float)red[0], (float)exp(-red[NW]), (float)__hip_atomic_load(&ctl->namb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                         (float)(red[0] / ((double)N * (double)d))};   // [3]: mean squared error (the two VQ loss terms)
#pragma unroll
    for (int i = 0; i < 4; ++i) stats_out[i] = st[i];
    if (stats_copy) {                                            // the record a second time, for a caller that differentiates its own copy
#pragma unroll
      for (int i = 0; i < 4; ++i) stats_copy[i] = st[i];
    }
    __hip_atomic_store(&ctl->namb, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&ctl->done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Order-independent sum of non-negative float32 values: v = m * 2^(e - 149) with a 24-bit integer m is added as the integer
// m << (e % 32), its low 32 bits to bin e / 32 and the rest to the bin above, so that bin b counts units of 2^(32 b - 149).  Integer
// additions commute, and a bin takes 2^31 values before it can overflow: the sum is exact and the same whatever the order.  inf and
// NaN go to *nonfinite by a float64 atomic (any order gives inf or NaN alike).  vq_sq_bins_value reads the bins from the top down.
__device__ __forceinline__ void vq_sq_bins_add(unsigned long long* bins, double* nonfinite, float v) {
  const unsigned u = __float_as_uint(v);
  const unsigned ex = (u >> 23) & 0xffu;
  if (ex == 0xffu || (u >> 31)) { atomicAdd(nonfinite, (double)v); return; }      // (a negative value cannot occur; kept out of the bins)
  const unsigned m = ex ? ((u & 0x7fffffu) | 0x800000u) : (u & 0x7fffffu);
  if (m == 0u) return;
  const unsigned e = ex ? ex - 1u : 0u;
  const unsigned long long w = (unsigned long long)m << (e & 31u);
  atomicAdd(&bins[e >> 5], w & 0xffffffffull);
  if (w >> 32) atomicAdd(&bins[(e >> 5) + 1], w >> 32);
}
__device__ __forceinline__ double vq_sq_bins_value(const unsigned long long* bins) {
  double s = 0.0;
#pragma unroll
  for (int b = VQ_SQ_BINS - 1; b >= 0; --b) s = s * 4294967296.0 + (double)bins[b];      // (Horner in steps of 2^32; the scalings are exact)
  return s * 0x1p-149;
}
