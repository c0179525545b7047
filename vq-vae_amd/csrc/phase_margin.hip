// Phase margin losses of the reference's cross-batch phase block (frl/training/representation/step.py:969-1006): the recovery
// discrimination loss (frl/losses/triplet_phase.py:352-426) and the phase spread ranking (frl/losses/phase_neighborhood.py:637-740).
// Both are, per item, all pairwise L2 distances d = |a_t - a_t'|_2 of at most 32 short rows under a mask, folded into one scalar.
//   recovery discrimination, per pixel n of z [N][T][D] with ysfc [N][T] (NaN / negative = invalid):
//       low[t] = valid && ysfc <= low_max, high[t] = valid && ysfc >= high_min, pairs = {(tl, th): low[tl] && high[th]}
//       d = sqrt(max(|z_tl - z_th|^2, 1e-12)),  loss = sum over pixels and pairs of softplus(margin - d) / n_pairs   (0 without pairs)
//       d z_tl += -g sigmoid(margin - d) / n_pairs (z_tl - z_th) / d, z_th the negative; 0 where the sum of squares is under the clamp
//   spread ranking, per valid pair b with the self-distance blocks of its two pixels and the mask t, t' < K_b, t != t':
//       n_b = max(1, unmasked entries), spread_i = sum mask d_i / n_b, spread_j likewise, r_b = dynamism_ref[i] - dynamism_ref[j]
//       term_b = softplus(spread_j - spread_i + margin) [r_b > delta] + softplus(spread_i - spread_j + margin) [r_b < -delta]
//       loss = sum_b term_b / B;   c_b = d term_b / d spread_i = -sigmoid(..) [r_b > delta] + sigmoid(..) [r_b < -delta] = -d term_b / d spread_j
//     matrix form: the blocks d_i, d_j, mask [B][M][M] from memory, any M, gradient +-g c_b / (B n_b) on the unmasked entries;
//     gathered form: the blocks are formed on chip from rows of emb [R][D]; the backward kernel writes per-(role, pair, position) rows
//       d a_t = +-g c_b / B (2 / n_b) sum_{t' != t} (a_t - a_t') / d[t, t']   (0 where d = 0, beyond K_b and for c_b = 0)
//     which the caller folds into d emb with frl_segment_sum_rows.
// Mapping: an item (a pixel; a (pair, role)) is one wave, up to four items per workgroup, each with its rows staged in its own slice of
// LDS at an odd pitch (lanes over t' read distinct banks) and, backward, a T x 33 block of per-pair coefficients.  Distances come from
// exact differences with the compensated sum of squares of frl_loss.hpp.  Reduction order is fixed (lanes strided over the
// pairs of an item, a butterfly inside the wave, items strided over one workgroup in f64): no float atomics, bit-reproducible.
#include "frl_common.hpp"
#include "frl_host.hpp"
#include "frl_loss.hpp"
#include <math.h>

#define PM_MAX_T 32                                               // rows per item (T, M)
#define PM_MAX_W 256                                              // row width D
#define PM_HP 33                                                  // pitch of the on-chip coefficient block
#define PM_LDS_BUDGET (60 * 1024)                                 // dynamic LDS a workgroup may ask for without an attribute

// torch's softplus (beta 1, threshold 20) and its derivative
__device__ __forceinline__ float pm_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float pm_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// ---------------------------------------------------------------------------------------------------------------------------
// recovery discrimination: wave = pixel.  FWD writes partial [N][2] = sum of softplus, pair count.  BWD writes grad [N][T][D], every row.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void pm_recovery_kernel(const T* __restrict__ z, const float* __restrict__ ysfc, int64_t N, int Tn, int D,
                                                          float margin, float low_max, float high_min, float* __restrict__ partial,
                                                          const float* __restrict__ out2, const float* __restrict__ gup, T* __restrict__ grad) {
  extern __shared__ float pm_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int pitch = D | 1;
  float* A = pm_lds + (size_t)wave * (Tn * pitch + (BWD ? Tn * PM_HP : 0));
  float* H = A + Tn * pitch;
  const int64_t n = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  const bool inside = n < N;
  bool lo = false, hi = false;
  if (inside && lane < Tn) {
    const float y = ysfc[n * Tn + lane];
    const bool valid = fabsf(y) < INFINITY && y >= 0.f;           // false for NaN and the infinities
    lo = valid && y <= low_max;
    hi = valid && y >= high_min;
  }
  const uint32_t lom = (uint32_t)__ballot(lo), him = (uint32_t)__ballot(hi);
  bool active = lom != 0u && him != 0u;                           // uniform over the wave
  float sc = 0.f;
  if (BWD) {
    const float np = out2[1];
    sc = (active && np > 0.f) ? -gup[0] / np : 0.f;
    active = active && sc != 0.f;
  }
  const int64_t base = n * (int64_t)Tn * D;
  if (active)
    for (int i = lane; i < Tn * D; i += 64) {
      const int t = i / D, c = i - t * D;
      A[t * pitch + c] = to_f32(z[base + i]);
    }
  __syncthreads();
  if (!BWD) {
    float s = 0.f;
    int cnt = 0;
    if (active)
      for (int e = lane; e < Tn * Tn; e += 64) {
        const int tl = e / Tn, th = e - tl * Tn;
        if (((lom >> tl) & 1u) && ((him >> th) & 1u)) {
          const float d = sqrtf(fmaxf(sumsq_diff(A + tl * pitch, A + th * pitch, D), 1e-12f));
          s += pm_softplus(margin - d);
          cnt += 1;
        }
      }
    s = wave_sum(s);
    cnt = wave_sum_i(cnt);
    if (inside && lane == 0) { partial[2 * n] = s; partial[2 * n + 1] = (float)cnt; }
  } else {
    if (active)
      for (int e = lane; e < Tn * Tn; e += 64) {
        const int tl = e / Tn, th = e - tl * Tn;
        float h = 0.f;
        if (((lom >> tl) & 1u) && ((him >> th) & 1u)) {
          const float ss = sumsq_diff(A + tl * pitch, A + th * pitch, D);
          if (ss > 1e-12f) {
            const float d = sqrtf(ss);
            h = sc * pm_sigmoid(margin - d) / d;
          }
        }
        H[tl * PM_HP + th] = h;
      }
    __syncthreads();
    if (inside)
      for (int i = lane; i < Tn * D; i += 64) {
        float v = 0.f;
        if (active) {
          const int t = i / D, c = i - t * D;
          const float at = A[t * pitch + c];
          for (int u = 0; u < Tn; ++u) v = fmaf(H[t * PM_HP + u] + H[u * PM_HP + t], at - A[u * pitch + c], v);   // t as low, t as high
        }
        grad[base + i] = from_f32<T>(v);
      }
  }
}

// partial [N][2] -> out2 [2] = loss, n_pairs; stats [4] (f64) = loss, n_pairs, active pixels, 0.  One workgroup, as sn_reduce_kernel.
__global__ __launch_bounds__(1024) void pm_recovery_reduce_kernel(const float* __restrict__ partial, int64_t N, float* __restrict__ out2,
                                                                  double* __restrict__ stats) {
  __shared__ double red[16][3];
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t n = threadIdx.x; n < N; n += 1024) {
    const float cnt = partial[2 * n + 1];
    if (cnt > 0.f) { s[0] += (double)partial[2 * n]; s[1] += (double)cnt; s[2] += 1.0; }
  }
  block_sum_d<3, 16>(s, red);
  if (threadIdx.x == 0) {
    const double* v = red[0];
    const float loss = v[1] > 0.0 ? (float)(v[0] / v[1]) : 0.f;
    out2[0] = loss;
    out2[1] = (float)v[1];
    stats[0] = (double)loss;
    stats[1] = v[1];
    stats[2] = v[2];
    stats[3] = 0.0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// spread ranking.  pairstat [B][3] = spread_i, spread_j, n_b.  The per-pair tail is shared by the reduction and both backward kernels.
// ---------------------------------------------------------------------------------------------------------------------------
struct PmTerm { float term, coef; int ci, cj, sat; };

__device__ __forceinline__ PmTerm pm_spread_term(float si, float sj, float r, float margin, float delta) {
  PmTerm o = {0.f, 0.f, 0, 0, 0};
  if (r > delta) {
    const float x = sj - si + margin;
    o.term = pm_softplus(x);
    o.coef = -pm_sigmoid(x);
    o.ci = 1;
    o.sat = (si - sj) > margin;
  } else if (r < -delta) {
    const float x = si - sj + margin;
    o.term = pm_softplus(x);
    o.coef = pm_sigmoid(x);
    o.cj = 1;
    o.sat = (sj - si) > margin;
  }
  return o;
}

// matrix form: wave = pair, lanes strided over the M * M entries
__global__ __launch_bounds__(256) void pm_spread_matrix_fwd_kernel(const float* __restrict__ di, const float* __restrict__ dj,
                                                                   const unsigned char* __restrict__ mask, int64_t B, int M,
                                                                   float* __restrict__ pairstat) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int64_t mm = (int64_t)M * M, ro = b * mm;
  float si = 0.f, sj = 0.f;
  int cnt = 0;
  for (int64_t e = lane; e < mm; e += 64)
    if (mask[ro + e]) { si += di[ro + e]; sj += dj[ro + e]; cnt += 1; }
  si = wave_sum(si);
  sj = wave_sum(sj);
  cnt = wave_sum_i(cnt);
  if (lane == 0) {
    const float nb = (float)(cnt > 1 ? cnt : 1);
    pairstat[3 * b] = si / nb;
    pairstat[3 * b + 1] = sj / nb;
    pairstat[3 * b + 2] = nb;
  }
}

// grad_i = g c_b / (B n_b) on the unmasked entries, grad_j its negative
__global__ __launch_bounds__(256) void pm_spread_matrix_bwd_kernel(const unsigned char* __restrict__ mask, const float* __restrict__ pairstat,
                                                                   const float* __restrict__ ref_diff, const float* __restrict__ gup, int64_t B,
                                                                   int64_t mm, float margin, float delta, float* __restrict__ gi,
                                                                   float* __restrict__ gj) {
  const float g = gup[0] / (float)B;
  const int64_t total = B * mm;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / mm;
    float v = 0.f;
    if (mask[i]) {
      const float* ps = pairstat + 3 * b;
      const float c = pm_spread_term(ps[0], ps[1], ref_diff[b], margin, delta).coef;
      v = c != 0.f ? g * c / ps[2] : 0.f;
    }
    gi[i] = v;
    gj[i] = -v;
  }
}

// gathered form: wave = (pair, role); role 0 gathers rows_i, role 1 rows_j.  FWD writes the role's spread (role 0 also n_b); BWD
// writes the role's gradient rows grows [2][B][M][D].
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void pm_spread_gathered_kernel(const T* __restrict__ emb, int D, const int64_t* __restrict__ rows_i,
                                                                 const int64_t* __restrict__ rows_j, const int64_t* __restrict__ lengths,
                                                                 const float* __restrict__ ref_diff, int64_t B, int M, float margin, float delta,
                                                                 float* __restrict__ pairstat, const float* __restrict__ gup,
                                                                 float* __restrict__ grows) {
  extern __shared__ float pm_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int pitch = D | 1;
  float* A = pm_lds + (size_t)wave * (M * pitch + (BWD ? M * PM_HP : 0));
  float* H = A + M * pitch;
  const int64_t item = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  const bool inside = item < 2 * B;
  const int64_t b = inside ? item >> 1 : 0;
  const int role = (int)(item & 1);
  int K = 0;
  if (inside) {
    const int64_t len = lengths[b];
    K = (int)(len < 0 ? 0 : (len > M ? M : len));
  }
  const int nb = K > 1 ? K * (K - 1) : 1;
  float sc = 0.f;
  if (BWD && inside) {
    const float* ps = pairstat + 3 * b;
    const float c = pm_spread_term(ps[0], ps[1], ref_diff[b], margin, delta).coef;
    sc = c != 0.f ? (role ? -2.f : 2.f) * (gup[0] / (float)B) * c / (float)nb : 0.f;
  }
  const bool active = K > 1 && (!BWD || sc != 0.f);               // uniform over the wave; a single position has no off-diagonal entry
  if (active) {
    const int64_t* rows = (role ? rows_j : rows_i) + b * M;
    const long long mine = lane < K ? (long long)rows[lane] : 0ll;
    for (int t = 0; t < K; ++t) {
      const int64_t r = (int64_t)__shfl(mine, t, 64);
      for (int c = lane; c < D; c += 64) A[t * pitch + c] = to_f32(emb[r * D + c]);
    }
  }
  __syncthreads();
  if (!BWD) {
    float s = 0.f;
    if (active)
      for (int e = lane; e < K * K; e += 64) {
        const int t = e / K, u = e - t * K;
        if (t != u) s += sqrtf(sumsq_diff(A + t * pitch, A + u * pitch, D));
      }
    s = wave_sum(s);
    if (inside && lane == 0) {
      pairstat[3 * b + role] = s / (float)nb;
      if (role == 0) pairstat[3 * b + 2] = (float)nb;
    }
  } else {
    if (active)
      for (int e = lane; e < K * K; e += 64) {
        const int t = e / K, u = e - t * K;
        float h = 0.f;
        if (t != u) {
          const float d = sqrtf(sumsq_diff(A + t * pitch, A + u * pitch, D));
          h = d > 0.f ? 1.f / d : 0.f;
        }
        H[t * PM_HP + u] = h;
      }
    __syncthreads();
    if (inside) {
      float* out = grows + ((int64_t)role * B + b) * (int64_t)M * D;
      for (int i = lane; i < M * D; i += 64) {
        const int t = i / D, c = i - t * D;
        float v = 0.f;
        if (active && t < K) {
          const float at = A[t * pitch + c];
          for (int u = 0; u < K; ++u) v = fmaf(H[t * PM_HP + u], at - A[u * pitch + c], v);
          v *= sc;
        }
        out[i] = v;
      }
    }
  }
}

// pairstat, ref_diff -> out2 [2] = loss, B; stats [8] (f64) = loss, constrained i, constrained j, satisfied, sum spread_i, sum spread_j,
// sum |r_b|, B.  One workgroup, pairs strided over its threads in f64.
__global__ __launch_bounds__(1024) void pm_spread_reduce_kernel(const float* __restrict__ pairstat, const float* __restrict__ ref_diff, int64_t B,
                                                                float margin, float delta, float* __restrict__ out2,
                                                                double* __restrict__ stats) {
  __shared__ double red[16][7];
  double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t b = threadIdx.x; b < B; b += 1024) {
    const float* ps = pairstat + 3 * b;
    const float r = ref_diff[b];
    const PmTerm t = pm_spread_term(ps[0], ps[1], r, margin, delta);
    s[0] += (double)t.term;
    s[1] += (double)t.ci;
    s[2] += (double)t.cj;
    s[3] += (double)t.sat;
    s[4] += (double)ps[0];
    s[5] += (double)ps[1];
    s[6] += (double)fabsf(r);
  }
  block_sum_d<7, 16>(s, red);
  if (threadIdx.x == 0) {
    const float loss = (float)(red[0][0] / (double)B);
    out2[0] = loss;
    out2[1] = (float)B;
    stats[0] = (double)loss;
    for (int k = 1; k < 7; ++k) stats[k] = red[0][k];
    stats[7] = (double)B;
  }
}

// items (waves) per workgroup: up to four, fewer when the rows of four do not fit the LDS budget
static int pm_items_per_block(int rows, int D, bool bwd, size_t* item_bytes) {
  *item_bytes = ((size_t)rows * (D | 1) + (bwd ? (size_t)rows * PM_HP : 0)) * sizeof(float);
  int ipb = (int)(PM_LDS_BUDGET / *item_bytes);
  return ipb > 4 ? 4 : (ipb < 1 ? 1 : ipb);
}

static int pm_check_recovery(int64_t N, int T, int D, int dtype) {
  if (N < 1 || N > 0x3fffffff) return frl_fail(-2, "recovery_disc: needs 1 <= N < 2^30 pixels");
  if (T < 1 || T > PM_MAX_T) return frl_fail(-2, "recovery_disc: supports 1 <= T <= 32");
  if (D < 1 || D > PM_MAX_W) return frl_fail(-2, "recovery_disc: supports 1 <= D <= 256");
  if (dtype != FRL_F32 && dtype != FRL_BF16) return frl_fail(-2, "recovery_disc: dtype must be FRL_F32 or FRL_BF16");
  return 0;
}

static int pm_check_spread_gathered(int64_t B, int M, int D, int dtype) {
  if (B < 1 || B > 0x3fffffff) return frl_fail(-2, "spread_rank_gathered: needs 1 <= B < 2^30 pairs");
  if (M < 1 || M > PM_MAX_T) return frl_fail(-2, "spread_rank_gathered: supports 1 <= M <= 32");
  if (D < 1 || D > PM_MAX_W) return frl_fail(-2, "spread_rank_gathered: supports 1 <= D <= 256");
  if (dtype != FRL_F32 && dtype != FRL_BF16) return frl_fail(-2, "spread_rank_gathered: emb dtype must be FRL_F32 or FRL_BF16");
  return 0;
}

template <typename T, bool BWD>
static void pm_launch_recovery(const void* z, const float* ysfc, int64_t N, int Tn, int D, float margin, float low_max, float high_min,
                               float* partial, const float* out2, const float* gup, void* grad, hipStream_t st) {
  size_t item;
  const int ipb = pm_items_per_block(Tn, D, BWD, &item);
  auto kern = pm_recovery_kernel<T, BWD>;
  FRL_LAUNCH_AS(BWD ? "pm_recovery_bwd_kernel" : "pm_recovery_fwd_kernel", kern, dim3((unsigned)((N + ipb - 1) / ipb)),
                dim3(64 * ipb), ipb * item, st, (const T*)z, ysfc, N, Tn, D, margin, low_max, high_min, partial, out2, gup, (T*)grad);
}

template <typename T, bool BWD>
static void pm_launch_spread(const void* emb, int D, const int64_t* rows_i, const int64_t* rows_j, const int64_t* lengths, const float* ref_diff,
                             int64_t B, int M, float margin, float delta, float* pairstat, const float* gup, float* grows, hipStream_t st) {
  size_t item;
  const int ipb = pm_items_per_block(M, D, BWD, &item);
  auto kern = pm_spread_gathered_kernel<T, BWD>;
  FRL_LAUNCH_AS(BWD ? "pm_spread_gathered_bwd_kernel" : "pm_spread_gathered_fwd_kernel", kern, dim3((unsigned)((2 * B + ipb - 1) / ipb)), dim3(64 * ipb), ipb * item, st, (const T*)emb, D, rows_i, rows_j, lengths, ref_diff, B, M,
                margin, delta, pairstat, gup, grows);
}

extern "C" {

// z [N][T][D] (dtype 0 = float32, 1 = bfloat16), ysfc [N][T] f32 (NaN / negative = invalid).  Outputs: partial [N][2] (sum of softplus,
// pairs), out2 [2] = loss, n_pairs, stats [4] f64 = loss, n_pairs, active pixels, 0.  T <= 32, D <= 256.
int frl_recovery_disc_fwd(const void* z, int dtype, const float* ysfc, int64_t N, int T, int D, float margin, float low_ysfc_max,
                          float high_ysfc_min, float* partial, float* out2, double* stats, hipStream_t stream) {
  int rc = pm_check_recovery(N, T, D, dtype);
  if (rc) return rc;
  if (!z || !ysfc || !partial || !out2 || !stats) return frl_fail(-2, "recovery_disc_fwd: NULL argument");
  FRL_BY_DTYPE(dtype, Tz,
               pm_launch_recovery<Tz, false>(z, ysfc, N, T, D, margin, low_ysfc_max, high_ysfc_min, partial, nullptr, nullptr, nullptr, stream));
  FRL_LAUNCH(pm_recovery_reduce_kernel, dim3(1), dim3(1024), 0, stream, (const float*)partial, N, out2, stats);
  return frl_check_launch("recovery_disc_fwd");
}

// grad [N][T][D] in z's dtype = gup[0] * d loss / d z, every row written once (zeros for inactive pixels and when n_pairs = 0)
int frl_recovery_disc_bwd(const void* z, int dtype, const float* ysfc, int64_t N, int T, int D, float margin, float low_ysfc_max,
                          float high_ysfc_min, const float* out2, const float* gup, void* grad, hipStream_t stream) {
  int rc = pm_check_recovery(N, T, D, dtype);
  if (rc) return rc;
  if (!z || !ysfc || !out2 || !gup || !grad) return frl_fail(-2, "recovery_disc_bwd: NULL argument");
  FRL_BY_DTYPE(dtype, Tz, pm_launch_recovery<Tz, true>(z, ysfc, N, T, D, margin, low_ysfc_max, high_ysfc_min, nullptr, out2, gup, grad, stream));
  return frl_check_launch("recovery_disc_bwd");
}

// d_i, d_j [B][M][M] f32, mask [B][M][M] bytes, ref_diff [B] f32 = r_b.  Outputs: pairstat [B][3] = spread_i, spread_j, n_b, out2 [2] =
// loss, B, stats [8] f64 (see pm_spread_reduce_kernel).  Any M >= 1.
int frl_spread_rank_fwd(const float* d_i, const float* d_j, const unsigned char* mask, const float* ref_diff, int64_t B, int M, float margin,
                        float delta, float* pairstat, float* out2, double* stats, hipStream_t stream) {
  if (B < 1 || M < 1 || B > 0x3fffffff) return frl_fail(-2, "spread_rank_fwd: needs 1 <= B < 2^30 pairs and M >= 1");
  if (!d_i || !d_j || !mask || !ref_diff || !pairstat || !out2 || !stats) return frl_fail(-2, "spread_rank_fwd: NULL argument");
  FRL_LAUNCH(pm_spread_matrix_fwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, stream, d_i, d_j, mask, B, M, pairstat);
  FRL_LAUNCH(pm_spread_reduce_kernel, dim3(1), dim3(1024), 0, stream, (const float*)pairstat, ref_diff, B, margin, delta, out2, stats);
  return frl_check_launch("spread_rank_fwd");
}

// grad_i [B][M][M] = gup[0] * c_b / (B n_b) on the unmasked entries (0 elsewhere), grad_j = -grad_i
int frl_spread_rank_bwd(const unsigned char* mask, const float* pairstat, const float* ref_diff, const float* gup, int64_t B, int M,
                        float margin, float delta, float* grad_i, float* grad_j, hipStream_t stream) {
  if (B < 1 || M < 1 || B > 0x3fffffff) return frl_fail(-2, "spread_rank_bwd: needs 1 <= B < 2^30 pairs and M >= 1");
  if (!mask || !pairstat || !ref_diff || !gup || !grad_i || !grad_j) return frl_fail(-2, "spread_rank_bwd: NULL argument");
  const int64_t mm = (int64_t)M * M;
  FRL_LAUNCH(pm_spread_matrix_bwd_kernel, dim3(frl_grid(B * mm, 256, 4096)), dim3(256), 0, stream, mask, pairstat, ref_diff, gup, B, mm, margin, delta,
             grad_i, grad_j);
  return frl_check_launch("spread_rank_bwd");
}

// emb [R][D] (dtype 0 = float32, 1 = bfloat16), rows_i, rows_j [B][M] int64 already inside [0, R), lengths [B] int64 (K_b, clamped into
// [0, M]); mask = t, t' < K_b and t != t'.  Outputs as frl_spread_rank_fwd.  M <= 32, D <= 256.
int frl_spread_rank_gathered_fwd(const void* emb, int D, int emb_dtype, const int64_t* rows_i, const int64_t* rows_j, const int64_t* lengths,
                                 const float* ref_diff, int64_t B, int M, float margin, float delta, float* pairstat, float* out2,
                                 double* stats, hipStream_t stream) {
  int rc = pm_check_spread_gathered(B, M, D, emb_dtype);
  if (rc) return rc;
  if (!emb || !rows_i || !rows_j || !lengths || !ref_diff || !pairstat || !out2 || !stats)
    return frl_fail(-2, "spread_rank_gathered_fwd: NULL argument");
  FRL_BY_DTYPE(emb_dtype, T,
               pm_launch_spread<T, false>(emb, D, rows_i, rows_j, lengths, ref_diff, B, M, margin, delta, pairstat, nullptr, nullptr, stream));
  FRL_LAUNCH(pm_spread_reduce_kernel, dim3(1), dim3(1024), 0, stream, (const float*)pairstat, ref_diff, B, margin, delta, out2, stats);
  return frl_check_launch("spread_rank_gathered_fwd");
}

// grad_rows [2][B][M][D] f32: role i then role j, scaled by gup[0] / B; zeros where d = 0, beyond K_b and for unconstrained pairs
int frl_spread_rank_gathered_bwd(const void* emb, int D, int emb_dtype, const int64_t* rows_i, const int64_t* rows_j, const int64_t* lengths,
                                 const float* ref_diff, int64_t B, int M, float margin, float delta, const float* pairstat, const float* gup,
                                 float* grad_rows, hipStream_t stream) {
  int rc = pm_check_spread_gathered(B, M, D, emb_dtype);
  if (rc) return rc;
  if (!emb || !rows_i || !rows_j || !lengths || !ref_diff || !pairstat || !gup || !grad_rows)
    return frl_fail(-2, "spread_rank_gathered_bwd: NULL argument");
  FRL_BY_DTYPE(emb_dtype, T,
               pm_launch_spread<T, true>(emb, D, rows_i, rows_j, lengths, ref_diff, B, M, margin, delta, const_cast<float*>(pairstat), gup,
                                         grad_rows, stream));
  return frl_check_launch("spread_rank_gathered_bwd");
}

}  // extern "C"
