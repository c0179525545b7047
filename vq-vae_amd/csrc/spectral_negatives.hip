// The middle of the global spectral InfoNCE block (frl/training/representation/step.py:707-812), between pairs_mutual_knn_chunked
// (pairs.hip) and contrastive_loss (contrastive.hip):
//   * cross-patch negatives (step.py:743-773): the reference loops over all ordered patch pairs (pi, pj), pi != pj, draws n_per anchors of
//     each with two torch.randint calls per pair (2 S (S - 1) launches), concatenates, gathers both spectral rows, takes the norm of the
//     difference and turns it into the false-negative weight clamp(1 - exp(-d / tau), min_w, 1).  Here one launch does all of it: negative
//     q lies in block b = q / n_per of the reference's loop order, pi = b / (S - 1), r = b % (S - 1), pj = r + (r >= pi), and its two
//     anchors are offsets[p] + ((uint64) draw * count_p >> 31) for the two draws of q: uniform over the patch to within count / 2^31, and
//     below count for every draw in [0, 2^31).
//   * the kernel-sizing diagnostic (step.py:798-807, and the per-pair similarities of :569-574): sims[t] = -|emb[a] - emb[b]|^2 / D with
//     their mean and unbiased standard deviation.  The sums are kept in double: per-workgroup partials in the caller's workspace, then one
//     workgroup adds them in index order.  No float atomics and no arrival counter, so the result is bit-reproducible.
// Both kernels give one 16-lane group to a pair, as pair_logits_kernel of contrastive.hip: 16-byte row loads when the width is a multiple
// of four and the rows are 16-byte aligned, one element per lane otherwise; lane-strided partial sums (channels ascending within a lane),
// then the 16-lane butterfly.  Out-of-range input follows the sparse-op convention (ops.index_errors): it is clamped and ORs a bit into the
// caller's flag word, and no address outside the arrays is ever formed.
#include "frl_common.hpp"
#include "frl_host.hpp"
#include "frl_loss.hpp"
#include <math.h>

#define SPN_BLOCK 256
#define SPN_GROUPS (SPN_BLOCK / 16)
#define SPN_GRID_MAX 2048
#define SPN_MAX_WIDTH 256

// sum_c (a[c] - b[c])^2 over one 16-lane group; every lane of the group returns the sum
template <bool VEC>
__device__ __forceinline__ float group16_sqdist(const float* __restrict__ a, const float* __restrict__ b, int C, int l) {
  float s = 0.f;
  if constexpr (VEC) {
    const f32x4* a4 = reinterpret_cast<const f32x4*>(a);
    const f32x4* b4 = reinterpret_cast<const f32x4*>(b);
    for (int j = l; j < (C >> 2); j += 16) {
      const f32x4 av = a4[j], bv = b4[j];
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float df = av[e] - bv[e]; s = fmaf(df, df, s); }
    }
  } else {
    for (int j = l; j < C; j += 16) { const float df = a[j] - b[j]; s = fmaf(df, df, s); }
  }
  return group16_sum(s);
}

// ---------------------------------------------------------------------------------------------------------------------------
// negative q -> (i, j), |spec[i] - spec[j]|, weight.  flag bits: 1 a negative draw (taken as 0), 2 patch bounds that are not
// 0 <= offsets[p] < offsets[p + 1] <= N (clamped to a non-empty range inside the array)
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t spn_pick(const int32_t* __restrict__ offsets, int p, int draw, int64_t N, int& bad) {
  int64_t lo = offsets[p], hi = offsets[p + 1];
  if (lo < 0 || hi > N || hi <= lo) {
    bad |= 2;
    lo = lo < 0 ? 0 : (lo > N - 1 ? N - 1 : lo);
    hi = hi > N ? N : hi;
    if (hi <= lo) hi = lo + 1;
  }
  if (draw < 0) { bad |= 1; draw = 0; }
  return lo + (int64_t)(((uint64_t)draw * (uint64_t)(hi - lo)) >> 31);
}

template <bool VEC>
__global__ __launch_bounds__(SPN_BLOCK) void spectral_negatives_kernel(const float* __restrict__ spec, int64_t N, int C,
                                                                      const int32_t* __restrict__ offsets, int S, int n_per,
                                                                      const int32_t* __restrict__ draws, int64_t Q, float tau, float min_w,
                                                                      int64_t* __restrict__ pairs, float* __restrict__ dist,
                                                                      float* __restrict__ weights, int* __restrict__ flag) {
  const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
  int bad = 0;
  for (int64_t q = (int64_t)blockIdx.x * SPN_GROUPS + g; q < Q; q += (int64_t)gridDim.x * SPN_GROUPS) {
    const uint32_t b = (uint32_t)q / (uint32_t)n_per;                // Q < 2^31: 32-bit divisions
    const int pi = (int)(b / (uint32_t)(S - 1)), r = (int)(b % (uint32_t)(S - 1));
    const int pj = r + (r >= pi ? 1 : 0);
    const int64_t i = spn_pick(offsets, pi, draws[2 * q], N, bad);
    const int64_t j = spn_pick(offsets, pj, draws[2 * q + 1], N, bad);
    const float d = sqrtf(group16_sqdist<VEC>(spec + i * C, spec + j * C, C, l));
    if (l == 0) {
      const float w = 1.f - expf(-d / tau);
      pairs[2 * q] = i;
      pairs[2 * q + 1] = j;
      dist[q] = d;
      weights[q] = w < min_w ? min_w : (w > 1.f ? 1.f : w);          // (a NaN stays a NaN, as torch.clamp)
    }
  }
  if (bad && l == 0 && flag != nullptr) atomicOr(flag, bad);
}

// ---------------------------------------------------------------------------------------------------------------------------
// sims[t] = -|emb[a_t] - emb[b_t]|^2 / D; with `partial` the workgroup's sum and sum of squares of its sims in double (groups added in
// index order).  Rows in [-N, 0) wrap, any other row outside [0, N) is clamped and ORs 1 into *flag.
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t ps_row(int64_t v, int64_t N, int& bad) {
  if (v < 0) v += N;
  if (v < 0 || v >= N) { bad = 1; v = v < 0 ? 0 : N - 1; }
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(SPN_BLOCK) void pair_sims_kernel(const float* __restrict__ emb, int64_t N, int D, const int64_t* __restrict__ pairs,
                                                             int64_t T, float* __restrict__ sims, double* __restrict__ partial,
                                                             int* __restrict__ flag) {
  __shared__ double red[SPN_GROUPS][2];
  const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
  int bad = 0;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t t = (int64_t)blockIdx.x * SPN_GROUPS + g; t < T; t += (int64_t)gridDim.x * SPN_GROUPS) {
    const int64_t a = ps_row(pairs[2 * t], N, bad), b = ps_row(pairs[2 * t + 1], N, bad);
    const float sim = -group16_sqdist<VEC>(emb + a * D, emb + b * D, D, l) / (float)D;
    if (l == 0) sims[t] = sim;
    s1 += (double)sim;
    s2 += (double)sim * (double)sim;
  }
  if (bad && l == 0 && flag != nullptr) atomicOr(flag, 1);
  if (partial == nullptr) return;
  if (l == 0) { red[g][0] = s1; red[g][1] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t1 = 0.0, t2 = 0.0;
    for (int k = 0; k < SPN_GROUPS; ++k) { t1 += red[k][0]; t2 += red[k][1]; }
    partial[2 * blockIdx.x] = t1;
    partial[2 * blockIdx.x + 1] = t2;
  }
}

// stats = (T, mean, unbiased standard deviation, 0) from the nb workgroup partials: one workgroup, fixed order.  The sims are float32
// values, so a spread below 6e-8 |mean| is not resolved by the data itself; the cancellation in sum(x^2) - sum(x)^2 / T, 1e-16 mean^2 in
// double, lies below that.
__global__ __launch_bounds__(SPN_BLOCK) void pair_sims_finish_kernel(const double* __restrict__ partial, int nb, int64_t T, double* __restrict__ stats) {
  __shared__ double red[SPN_BLOCK][2];
  double t1 = 0.0, t2 = 0.0;
  for (int i = threadIdx.x; i < nb; i += SPN_BLOCK) { t1 += partial[2 * i]; t2 += partial[2 * i + 1]; }
  red[threadIdx.x][0] = t1;
  red[threadIdx.x][1] = t2;
  __syncthreads();
  for (int o = SPN_BLOCK / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) { red[threadIdx.x][0] += red[threadIdx.x + o][0]; red[threadIdx.x][1] += red[threadIdx.x + o][1]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double n = (double)T, mean = red[0][0] / n;
    const double m2 = red[0][1] - red[0][0] * mean;
    stats[0] = n;
    stats[1] = mean;
    stats[2] = T < 2 ? (double)NAN : sqrt((m2 > 0.0 ? m2 : 0.0) / (n - 1.0));   // torch.std of one value is NaN
    stats[3] = 0.0;
  }
}

static unsigned spn_grid(int64_t work) { return frl_grid(work, SPN_GROUPS, SPN_GRID_MAX); }

static bool spn_vec_ok(const void* rows, int width) { return (width & 3) == 0 && ((uintptr_t)rows & 15) == 0; }

extern "C" {

int frl_spectral_negatives(const float* spec, int64_t N, int C, const int32_t* offsets, int S, int n_per, const int32_t* draws, int64_t Q,
                           float tau, float min_w, int64_t* pairs, float* dist, float* weights, int32_t* index_flag, hipStream_t stream) {
  if (C < 1 || C > SPN_MAX_WIDTH) return frl_fail(-2, "spectral_negatives: C must be in 1..256");
  if (Q < 0) return frl_fail(-2, "spectral_negatives: Q < 0");
  if (Q == 0) return 0;
  if (S < 2) return frl_fail(-2, "spectral_negatives: negatives need at least two patches");
  if (Q >= ((int64_t)1 << 31)) return frl_fail(-2, "spectral_negatives: Q must be below 2^31");
  if (n_per < 1 || (int64_t)n_per * S * (S - 1) != Q) return frl_fail(-2, "spectral_negatives: Q must be n_per * S * (S - 1), n_per >= 1");
  if (N < 1) return frl_fail(-2, "spectral_negatives: no anchors to draw from");
  if (!(tau > 0.f)) return frl_fail(-2, "spectral_negatives: tau must be positive");
  if (spec == nullptr || offsets == nullptr || draws == nullptr || pairs == nullptr || dist == nullptr || weights == nullptr)
    return frl_fail(-1, "spectral_negatives: null pointer");
  int* flag = reinterpret_cast<int*>(index_flag);
  if (spn_vec_ok(spec, C))
    FRL_LAUNCH((spectral_negatives_kernel<true>), dim3(spn_grid(Q)), dim3(SPN_BLOCK), 0, stream, spec, N, C, offsets, S, n_per, draws, Q, tau, min_w,
               pairs, dist, weights, flag);
  else
    FRL_LAUNCH((spectral_negatives_kernel<false>), dim3(spn_grid(Q)), dim3(SPN_BLOCK), 0, stream, spec, N, C, offsets, S, n_per, draws, Q, tau, min_w,
               pairs, dist, weights, flag);
  return frl_check_launch("spectral_negatives");
}

size_t frl_pair_sims_workspace_bytes(int64_t T) { return T > 0 ? (size_t)spn_grid(T) * 2 * sizeof(double) : 0; }

int frl_pair_sims(const float* emb, int64_t N, int D, const int64_t* pairs, int64_t T, float* sims, double* stats, int32_t* index_flag, void* ws,
                  size_t ws_bytes, hipStream_t stream) {
  if (D < 1 || D > SPN_MAX_WIDTH) return frl_fail(-2, "pair_sims: D must be in 1..256");
  if (T < 0) return frl_fail(-2, "pair_sims: T < 0");
  if (T == 0) return 0;
  if (N < 1) return frl_fail(-2, "pair_sims: pairs over an empty embedding matrix");
  if (emb == nullptr || pairs == nullptr || sims == nullptr) return frl_fail(-1, "pair_sims: null pointer");
  if (stats != nullptr && (ws == nullptr || ws_bytes < frl_pair_sims_workspace_bytes(T) || ((uintptr_t)ws & 7) != 0))
    return frl_fail(-3, "pair_sims: statistics need an 8-byte aligned workspace of frl_pair_sims_workspace_bytes(T)");
  double* partial = stats != nullptr ? reinterpret_cast<double*>(ws) : nullptr;
  int* flag = reinterpret_cast<int*>(index_flag);
  const unsigned nb = spn_grid(T);
  if (spn_vec_ok(emb, D))
    FRL_LAUNCH((pair_sims_kernel<true>), dim3(nb), dim3(SPN_BLOCK), 0, stream, emb, N, D, pairs, T, sims, partial, flag);
  else
    FRL_LAUNCH((pair_sims_kernel<false>), dim3(nb), dim3(SPN_BLOCK), 0, stream, emb, N, D, pairs, T, sims, partial, flag);
  if (stats != nullptr)
    FRL_LAUNCH(pair_sims_finish_kernel, dim3(1), dim3(SPN_BLOCK), 0, stream, (const double*)partial, (int)nb, T, stats);
  return frl_check_launch("pair_sims");
}

}  // extern "C"
