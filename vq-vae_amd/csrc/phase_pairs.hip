// Phase pair mining for the phase soft-neighbourhood chain:
//   build_phase_pairs  frl/losses/phase_pairs.py:74-253 -- per anchor the k nearest anchors of its own sample in spectral space (L2),
//   never itself; a neighbour stays when the two pixels share at least min_overlap distinct ysfc values, an anchor stays when at least
//   min_pairs of its neighbours do; the pair weight is exp(-|spec_i - spec_j|_2 / sigma).
// The reference runs once per sample on an [N, N] torch.cdist, a topk and an [N, classes] float presence matrix times its transpose.
// Here every sample of a batch is one segment of the rows and one launch serves them all, with the layout of knn_kernel
// (csrc/pairs.hip): one wave per anchor, its squared distances to the segment in LDS, k rounds of a wave-wide arg-min by
// (distance, index).  Lane r then owns neighbour r: the ysfc presence sets are 256-bit masks (one tiny kernel ahead of the main one), the
// overlap is a popcount of the AND, the anchor's survival a popcount of the ballot.  Nothing N x N or N x classes is written.
#include "frl_common.hpp"
#include "frl_host.hpp"

#define PP_WAVES 4

// ysfc [N][T] float32 -> masks [N][4]: bit v of a row is set iff trunc(value) == v somewhere in T (what ysfc.long() and scatter_ give).
// A NaN, an infinity, a negative value or a value of 256 or more sets no bit and raises *flag.
__global__ __launch_bounds__(256) void phase_mask_kernel(const float* __restrict__ ysfc, int N, int T, unsigned long long* __restrict__ masks,
                                                         int* __restrict__ flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  unsigned long long m[4] = {0ull, 0ull, 0ull, 0ull};
  bool bad = false;
  for (int t = 0; t < T; ++t) {
    const float v = ysfc[(size_t)i * T + t];
    if (!(v >= 0.f) || !(v < 256.f)) { bad = true; continue; }
    const int c = (int)v;                                                        // truncation, as .long()
#pragma unroll
    for (int w = 0; w < 4; ++w)
      if ((c >> 6) == w) m[w] |= 1ull << (c & 63);
  }
#pragma unroll
  for (int w = 0; w < 4; ++w) masks[(size_t)i * 4 + w] = m[w];
  if (bad) atomicOr(flag, 1);
}

// LDS as in knn_kernel: q [PP_WAVES][D] | tile [64][D + 4] | dist [PP_WAVES][n].  blockIdx.y is the segment, blockIdx.x the group of four
// anchors within it (the grid is as wide as the longest segment needs; the surplus workgroups of shorter ones leave at once), so all four
// waves of a workgroup share the segment whose rows they stage: 64-row tiles, fetched once per workgroup with coalesced 16-byte loads,
// two tiles in flight (one wave per SIMD is resident next to the distance rows: nobody else hides the latency).
template <int D4PT>   // float4 pieces of a 64-row tile per thread = 64 * (D / 4) / 256
__global__ __launch_bounds__(64 * PP_WAVES) void phase_pairs_kernel(const float* __restrict__ spec, int N, int D, const int* __restrict__ seg,
                                                                    const unsigned long long* __restrict__ masks, int k, int min_overlap,
                                                                    int min_pairs, float sigma, int* __restrict__ knn_idx,
                                                                    int* __restrict__ overlap, uint8_t* __restrict__ keep,
                                                                    uint8_t* __restrict__ keep_overlap, float* __restrict__ weight,
                                                                    float* __restrict__ l2, uint8_t* __restrict__ anchor_ok,
                                                                    int* __restrict__ counters) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int s0 = seg[blockIdx.y], s1 = seg[blockIdx.y + 1];
  s0 = s0 < 0 ? 0 : (s0 > N ? N : s0);                                           // the host has checked the offsets; never leave the rows
  s1 = s1 < s0 ? s0 : (s1 > N ? N : s1);
  const int n = s1 - s0;
  if ((int)blockIdx.x * PP_WAVES >= n) return;                                   // workgroup-uniform, ahead of every barrier
  const float* feat = spec + (size_t)s0 * D;
  constexpr int d4 = 4 * D4PT;                                                   // D / 4: the host dispatches on D = 16 * D4PT
  const int pitch = D + 4;
  float* qall = reinterpret_cast<float*>(smem);
  float* tile = qall + (size_t)PP_WAVES * D;
  float* dist = tile + (size_t)64 * pitch + (size_t)wave * n;
  const int iq = blockIdx.x * PP_WAVES + wave;
  const bool live = iq < n;
  const int i = live ? iq : n - 1;                                               // surplus waves shadow the last anchor (no stores)
  float* q = qall + (size_t)wave * D;
  for (int d = lane; d < D; d += 64) q[d] = feat[(size_t)i * D + d];
  const float inf = __builtin_inff();
  const f32x4* q4 = reinterpret_cast<const f32x4*>(q);
  const int ntiles = (n + 63) >> 6;
  f32x4 preA[D4PT], preB[D4PT];
  auto fetch = [&](f32x4 (&pre)[D4PT], int tix) {                                // piece p of the tile: row p / d4, float4 column p % d4
#pragma unroll
    for (int u = 0; u < D4PT; ++u) {
      const int p = tid + 256 * u;
      int row = tix * 64 + p / d4;
      if (row >= n) row = n - 1;
      pre[u] = *reinterpret_cast<const f32x4*>(feat + (size_t)row * D + 4 * (p % d4));
    }
  };
  auto step = [&](f32x4 (&pre)[D4PT], int tix) {
    __syncthreads();                                                             // everyone is done with the previous tile (and q is written)
#pragma unroll
    for (int u = 0; u < D4PT; ++u) {
      const int p = tid + 256 * u;
      *reinterpret_cast<f32x4*>(tile + (size_t)(p / d4) * pitch + 4 * (p % d4)) = pre[u];
    }
    __syncthreads();
    if (tix + 2 < ntiles) fetch(pre, tix + 2);
    const int j = tix * 64 + lane;
    const f32x4* x4 = reinterpret_cast<const f32x4*>(tile + (size_t)lane * pitch);
    float s = 0.f;
#pragma unroll 8
    for (int d = 0; d < d4; ++d) {
      const f32x4 a = q4[d], b = x4[d];
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float t = a[e] - b[e]; s = fmaf(t, t, s); }
    }
    if (j < n) dist[j] = j == i ? inf : s;                                       // never itself
  };
  fetch(preA, 0);
  if (ntiles > 1) fetch(preB, 1);
  for (int tix = 0; tix < ntiles; tix += 2) {
    step(preA, tix);
    if (tix + 1 < ntiles) step(preB, tix + 1);
  }
  __builtin_amdgcn_wave_barrier();
  // ---- k selection rounds, as in knn_kernel: lane l owns the entries j = l, l + 64, ...; a round takes the wave-wide arg-min by
  // (distance, index), retires the winner, and the 64 lanes together rescan the winner's owner.  Lane r keeps the winner of round r.
  auto wave_argmin = [&](float& v, int& jx) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(v, off, 64);
      const int oj = __shfl_xor(jx, off, 64);
      if (ov < v || (ov == v && oj < jx)) { v = ov; jx = oj; }
    }
  };
  float lbest = inf;
  int lj = 0x7fffffff;
  {
    int j = lane;
    for (; j + 7 * 64 < n; j += 8 * 64) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = dist[j + 64 * u];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (v[u] < lbest) { lbest = v[u]; lj = j + 64 * u; }                     // ascending j per lane: first index wins ties
    }
    for (; j < n; j += 64) {
      const float v = dist[j];
      if (v < lbest) { lbest = v; lj = j; }
    }
  }
  int my_j = -1;
  float my_d2 = 0.f;
  for (int r = 0; r < k; ++r) {
    float best = lbest;
    int bj = lj;
    wave_argmin(best, bj);
    if (!(best < inf)) break;                                                    // wave-uniform: the segment has no further anchor
    if (lane == r) { my_j = bj; my_d2 = best; }
    const int owner = bj & 63;
    if (lane == owner) dist[bj] = inf;                                           // retire the winner
    __builtin_amdgcn_wave_barrier();
    float cb = inf;
    int cj = 0x7fffffff;
    for (int j = owner + 64 * lane; j < n; j += 64 * 64) {
      const float v = dist[j];
      if (v < cb) { cb = v; cj = j; }
    }
    wave_argmin(cb, cj);
    if (lane == owner) { lbest = cb; lj = cb < inf ? cj : 0x7fffffff; }
  }
  // ---- overlap, filters and weights: lane r owns neighbour r (k <= 64)
  const unsigned long long* mi = masks + (size_t)(s0 + i) * 4;
  int ov = 0;
  if (my_j >= 0) {
    const unsigned long long* mj = masks + (size_t)(s0 + my_j) * 4;
#pragma unroll
    for (int w = 0; w < 4; ++w) ov += __popcll(mi[w] & mj[w]);
  }
  const bool kov = my_j >= 0 && ov >= min_overlap;
  const int ncand = __popcll(__ballot(my_j >= 0));
  const int cnt = __popcll(__ballot(kov));
  const bool ok = cnt >= min_pairs;
  if (!live) return;
  if (lane < k) {
    const size_t o = (size_t)(s0 + i) * k + lane;
    const float d = sqrtf(my_d2);
    knn_idx[o] = my_j >= 0 ? s0 + my_j : -1;
    overlap[o] = ov;
    keep_overlap[o] = kov ? 1 : 0;
    keep[o] = kov && ok ? 1 : 0;
    l2[o] = my_j >= 0 ? d : 0.f;
    weight[o] = my_j >= 0 ? expf(-d / sigma) : 0.f;
  }
  if (lane == 0) {
    anchor_ok[s0 + i] = ok ? 1 : 0;
    int* c = counters + (size_t)blockIdx.y * 4;
    if (ncand) atomicAdd(c + 0, ncand);
    if (cnt) atomicAdd(c + 1, cnt);
    if (ok && cnt) atomicAdd(c + 2, cnt);
    if (ok) atomicAdd(c + 3, 1);
  }
}

static size_t pp_lds_bytes(int n, int D) {
  return ((size_t)PP_WAVES * D + (size_t)64 * (D + 4) + (size_t)PP_WAVES * n) * sizeof(float);
}

template <int D4PT, class... A>
static int pp_launch(dim3 grid, size_t lds, hipStream_t stream, A... args) {
  auto kern = phase_pairs_kernel<D4PT>;
  if (lds > 64 * 1024) FRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  FRL_LAUNCH_AS("phase_pairs_kernel", kern, grid, dim3(64 * PP_WAVES), lds, stream, args...);
  return 0;
}

extern "C" {

size_t frl_phase_pairs_max_points(int D) {
  if (D <= 0) return 0;
  const size_t lds = 160 * 1024, fixed = pp_lds_bytes(0, D);
  return lds > fixed ? (lds - fixed) / (PP_WAVES * sizeof(float)) : 0;
}

// See include/frl_hip.h.
int frl_phase_pairs(const float* spec, const float* ysfc, int N, int D, int T, const int32_t* seg_host, const int32_t* seg, int S, int k,
                    int min_overlap, int min_pairs, float sigma, uint64_t* masks, int32_t* knn_idx, int32_t* overlap, uint8_t* keep,
                    uint8_t* keep_overlap, float* weight, float* dist, uint8_t* anchor_ok, int32_t* counters, int32_t* flag,
                    hipStream_t stream) {
  if (N <= 0 || D <= 0 || T <= 0 || S <= 0) return frl_fail(-2, "phase_pairs: N, D, T and the segment count must be positive");
  if (k < 1 || k > 64) return frl_fail(-2, "phase_pairs: k must be in 1..64 (one lane per neighbour)");
  if (!(sigma > 0.f)) return frl_fail(-2, "phase_pairs: sigma must be positive");
  if ((D & 15) || D > 256) return frl_fail(-2, "phase_pairs: the feature width must be a multiple of 16, at most 256 (pad with zeros)");
  if (S > 65535) return frl_fail(-2, "phase_pairs: at most 65535 segments");
  if (!spec || !ysfc || !seg_host || !seg || !masks || !knn_idx || !overlap || !keep || !keep_overlap || !weight || !dist || !anchor_ok ||
      !counters || !flag)
    return frl_fail(-2, "phase_pairs: null pointer");
  int longest = 0;
  if (seg_host[0] != 0 || seg_host[S] != N) return frl_fail(-2, "phase_pairs: segment offsets must rise from 0 to N");
  for (int s = 0; s < S; ++s) {
    const int n = seg_host[s + 1] - seg_host[s];
    if (n < 0) return frl_fail(-2, "phase_pairs: segment offsets must rise from 0 to N");
    longest = n > longest ? n : longest;
  }
  if ((size_t)longest > frl_phase_pairs_max_points(D))
    return frl_fail(-3, "phase_pairs: the distance rows of four anchors of the longest segment do not fit the LDS");
  FRL_LAUNCH(phase_mask_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, ysfc, N, T, (unsigned long long*)masks, flag);
  const size_t lds = pp_lds_bytes(longest, D);
  const dim3 grid((longest + PP_WAVES - 1) / PP_WAVES, S);
  const unsigned long long* m = (const unsigned long long*)masks;
  int rc;
#define PP_CASE(W)                                                                                                                       \
  case W:                                                                                                                                \
    rc = pp_launch<W>(grid, lds, stream, spec, N, D, seg, m, k, min_overlap, min_pairs, sigma, knn_idx, overlap, keep, keep_overlap,     \
                      weight, dist, anchor_ok, counters);                                                                                \
    break
  switch (D / 16) {   // D4PT = 64 * (D / 4) / 256 = D / 16
    PP_CASE(1);
    PP_CASE(2);
    PP_CASE(3);
    PP_CASE(4);
    PP_CASE(6);
    PP_CASE(8);
    PP_CASE(16);
    default: return frl_fail(-2, "phase_pairs: feature width must be 16, 32, 48, 64, 96, 128 or 256");
  }
#undef PP_CASE
  if (rc) return rc;
  return frl_check_launch("phase_pairs");
}

}  // extern "C"
