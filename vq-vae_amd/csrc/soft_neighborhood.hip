// Soft-neighbourhood matching loss (frl/losses/soft_neighborhood.py:46-208; the two terms of phase_neighborhood_loss,
// frl/losses/phase_neighborhood.py:458-630, caller frl/training/representation/step.py:948): a masked row-softmax KL divergence between a
// reference distance block and a learned one, per pair b and row t over the unmasked entries t' of that row only
//     lp = log_softmax(-d_ref / tau_ref), lq = log_softmax(-d_learned / tau_learned), p = exp(lp), q = exp(lq)
//     kl[b,t] = sum_t' p (lp - lq)                 rows with fewer than min_valid unmasked entries are skipped
//     L_b     = sum_t kl[b,t] / rows_b             rows_b = contributing rows; a pair with none is inactive
//     loss    = sum_b w_b L_b / sum_b w_b          over active pairs; 0 when there is none or the weights sum to 0
//     d loss / d d_learned[b,t,t'] = w_b / (rows_b sum_w) (p - q) / tau_learned
// (the reference fills masked logits with -1e9, which gives p = q = 0 exactly there: skipping them is the same function).
//   * matrix form:   d_ref, d_learned, mask [B][M][M] from memory, any M; one workgroup per pair, a group of 16 / 32 / 64 lanes per row, lanes over columns.
//   * gathered form: the blocks are never in memory.  One workgroup per pair gathers the M rows of each role from ref [R][C] / emb [R][D]
//     into LDS, forms d[t][t'] = |a_t - b_t'|_2 on chip (exact differences, as torch.cdist without the matmul route; the sum of squares is
//     compensated, so d is good to an ulp at any width) and evaluates the same
//     rows; the backward kernel recomputes the blocks and writes per-(role, pair, position) gradient rows
//         d a_t = sum_t' g[t,t'] (a_t - b_t') / d[t,t'],   d b_t' = -sum_t g[t,t'] (a_t - b_t') / d[t,t']     (0 where d = 0: torch.cdist's
//     convention, met on the diagonal of the (i, i) self-pairs), which the caller folds into d emb with frl_segment_sum_rows.
// Reduction order is fixed everywhere (butterflies inside a row, rows in order inside a pair, pairs strided over one workgroup in f64):
// no float atomics, loss and gradients are bit-reproducible.
#include "frl_common.hpp"
#include "frl_host.hpp"
#include "frl_loss.hpp"
#include <math.h>

#define SN_MAX_M 32                                               // gathered form: positions per pair
#define SN_MAX_W 256                                              // gathered form: row width (C and D)
#define SN_DP 33                                                  // pitch of the on-chip M x M blocks
enum { SN_L = 0, SN_ROWS, SN_OVERLAP, SN_ENT_P, SN_ENT_Q, SN_KL, SN_NSTAT };   // columns of pairstat [B][6]

struct SnRow { float kl, ep, eq, cnt; };

__device__ __forceinline__ float sn_gsum(float v, int gw) {
  for (int o = gw >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float sn_gmax(float v, int gw) {
  for (int o = gw >> 1; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// One row by an aligned group of gw lanes (j = lane in the group), columns c = j, j + gw, ... < n.  ld(c, d_ref, d_learned) -> unmasked?;
// st(c, (p - q) / tau_learned) receives every column (0 on masked entries and on skipped rows).  All lanes return the row's sums.
template <typename Ld, typename St>
__device__ __forceinline__ SnRow sn_row(int j, int gw, int n, float itr, float itl, int min_valid, Ld ld, St st) {
  float mr = -INFINITY, ml = -INFINITY, cnt = 0.f, dr, dl;
  for (int c = j; c < n; c += gw)
    if (ld(c, dr, dl)) { mr = fmaxf(mr, -dr * itr); ml = fmaxf(ml, -dl * itl); cnt += 1.f; }
  mr = sn_gmax(mr, gw);
  ml = sn_gmax(ml, gw);
  cnt = sn_gsum(cnt, gw);
  SnRow r = {0.f, 0.f, 0.f, cnt};
  if (cnt < (float)min_valid) {
    for (int c = j; c < n; c += gw) st(c, 0.f);
    return r;
  }
  float sr = 0.f, sl = 0.f;
  for (int c = j; c < n; c += gw)
    if (ld(c, dr, dl)) { sr += expf(-dr * itr - mr); sl += expf(-dl * itl - ml); }
  const float lsr = logf(sn_gsum(sr, gw)), lsl = logf(sn_gsum(sl, gw));
  for (int c = j; c < n; c += gw) {
    float g = 0.f;
    if (ld(c, dr, dl)) {
      const float lp = -dr * itr - mr - lsr, lq = -dl * itl - ml - lsl;
      const float p = expf(lp), q = expf(lq);
      r.kl = fmaf(p, lp - lq, r.kl);
      r.ep = fmaf(-p, lp, r.ep);
      r.eq = fmaf(-q, lq, r.eq);
      g = (p - q) * itl;
    }
    st(c, g);
  }
  r.kl = sn_gsum(r.kl, gw);
  r.ep = sn_gsum(r.ep, gw);
  r.eq = sn_gsum(r.eq, gw);
  return r;
}

__device__ __forceinline__ void sn_write_pairstat(float* ps, float kl, float rows, float ov, float ep, float eq) {
  ps[SN_L] = rows > 0.f ? kl / rows : 0.f;
  ps[SN_ROWS] = rows;
  ps[SN_OVERLAP] = ov;
  ps[SN_ENT_P] = ep;
  ps[SN_ENT_Q] = eq;
  ps[SN_KL] = kl;
}

// ---------------------------------------------------------------------------------------------------------------------------
// matrix form: workgroup = pair, a row per group of 16 (M <= 16), 32 (M <= 32) or 64 lanes, lane = column (strided when M > 64).
// coef (optional) [B][M][M] = (p - q) / tau_learned, not yet divided by rows_b.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sn_matrix_fwd_kernel(const float* __restrict__ dref, const float* __restrict__ dlrn,
                                                            const unsigned char* __restrict__ mask, int M, float itr, float itl, int min_valid,
                                                            float* __restrict__ pairstat, float* __restrict__ coef) {
  __shared__ float part[16][5];
  const int64_t b = blockIdx.x;
  const int gw = M <= 16 ? 16 : M <= 32 ? 32 : 64, ng = 256 / gw;  // a row per group of 16 / 32 / 64 lanes: 16 / 8 / 4 rows at a time
  const int g = threadIdx.x / gw, j = threadIdx.x - g * gw;
  float kl = 0.f, ep = 0.f, eq = 0.f, ov = 0.f, rows = 0.f;
  for (int t = g; t < M; t += ng) {
    const int64_t ro = (b * M + t) * (int64_t)M;
    const SnRow r = sn_row(j, gw, M, itr, itl, min_valid,
                           [&](int c, float& a, float& d) {
                             if (!mask[ro + c]) return false;
                             a = dref[ro + c];
                             d = dlrn[ro + c];
                             return true;
                           },
                           [&](int c, float v) { if (coef != nullptr) coef[ro + c] = v; });
    if (r.cnt >= (float)min_valid) { kl += r.kl; ep += r.ep; eq += r.eq; ov += r.cnt; rows += 1.f; }
  }
  if (j == 0) { part[g][0] = kl; part[g][1] = ep; part[g][2] = eq; part[g][3] = ov; part[g][4] = rows; }
  __syncthreads();
  if (threadIdx.x == 0) {
    kl = ep = eq = ov = rows = 0.f;
    for (int w = 0; w < ng; ++w) { kl += part[w][0]; ep += part[w][1]; eq += part[w][2]; ov += part[w][3]; rows += part[w][4]; }
    sn_write_pairstat(pairstat + b * SN_NSTAT, kl, rows, ov, ep, eq);
  }
}

// grad = coef * upstream * w_b / (sum_w * rows_b)
__global__ __launch_bounds__(256) void sn_matrix_bwd_kernel(const float* __restrict__ coef, const float* __restrict__ pairstat,
                                                            const float* __restrict__ weights, const float* __restrict__ out2,
                                                            const float* __restrict__ gup, int64_t total, int64_t mm, float* __restrict__ grad) {
  const float sumw = out2[1], g = gup[0];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / mm;
    const float rows = pairstat[b * SN_NSTAT + SN_ROWS];
    const float sc = (rows > 0.f && sumw > 0.f) ? g * (weights ? weights[b] : 1.f) / (sumw * rows) : 0.f;
    grad[i] = sc != 0.f ? sc * coef[i] : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// pairs -> loss.  One workgroup of 1024 threads: pairs strided over the threads (f64 partials), butterfly per wave, the 16 wave sums
// added in order.  out2 [2] = loss, sum of the active pairs' weights; stats [8] (f64) = loss, sum_w, active pairs, contributing rows,
// sum of their unmasked counts, sum of H(p), sum of H(q), 0.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void sn_reduce_kernel(const float* __restrict__ pairstat, const float* __restrict__ weights, int64_t B,
                                                         float* __restrict__ out2, double* __restrict__ stats) {
  __shared__ double red[16][7];
  double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};           // sum w L | sum w | active | rows | overlap | H(p) | H(q)
  for (int64_t b = threadIdx.x; b < B; b += 1024) {
    const float* ps = pairstat + b * SN_NSTAT;
    if (ps[SN_ROWS] > 0.f) {
      const double w = weights ? (double)weights[b] : 1.0;
      s[0] += w * (double)ps[SN_L];
      s[1] += w;
      s[2] += 1.0;
      s[3] += (double)ps[SN_ROWS];
      s[4] += (double)ps[SN_OVERLAP];
      s[5] += (double)ps[SN_ENT_P];
      s[6] += (double)ps[SN_ENT_Q];
    }
  }
  block_sum_d<7, 16>(s, red);
  if (threadIdx.x == 0) {
    const double sw = red[0][1];
    const float loss = sw > 0.0 ? (float)(red[0][0] / sw) : 0.f;
    out2[0] = loss;
    out2[1] = (float)sw;
    stats[0] = (double)loss;
    stats[1] = sw;
    for (int k = 2; k < 7; ++k) stats[k] = red[0][k];
    stats[7] = 0.0;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// gathered form: workgroup = pair.  LDS: the gathered rows of both roles (pitch odd: a lane per row walks the columns conflict-free),
// the two K x K blocks, per-row results.  Rows are evaluated by groups of 16 lanes (K <= 16) or 32 lanes, a lane per column.
// BWD: the learned block's slot of d_ref is overwritten with g / d and the gradient rows are formed from the staged embedding rows.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename S>
__device__ __forceinline__ void sn_stage(float* __restrict__ A, float* __restrict__ Bm, int pitch, const S* __restrict__ src, int W,
                                         const int64_t* ia, const int64_t* ib, int K) {
  for (int i = threadIdx.x; i < K * W; i += 256) {
    const int t = i / W, c = i - t * W;
    A[t * pitch + c] = to_f32(src[ia[t] * (int64_t)W + c]);
    Bm[t * pitch + c] = to_f32(src[ib[t] * (int64_t)W + c]);
  }
}

__device__ __forceinline__ void sn_dist(float* __restrict__ dm, const float* __restrict__ A, const float* __restrict__ Bm, int pitch, int W, int K) {
  for (int e = threadIdx.x; e < K * K; e += 256) {
    const int t = e / K, u = e - t * K;
    dm[t * SN_DP + u] = sqrtf(sumsq_diff(A + t * pitch, Bm + u * pitch, W));
  }
}

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void sn_gathered_kernel(const float* __restrict__ ref, int C, const T* __restrict__ emb, int D,
                                                          const int64_t* __restrict__ rra, const int64_t* __restrict__ rrb,
                                                          const int64_t* __restrict__ era, const int64_t* __restrict__ erb,
                                                          const int64_t* __restrict__ lengths, const float* __restrict__ weights, int64_t B, int M,
                                                          int excl, float itr, float itl, int min_valid, float* __restrict__ pairstat,
                                                          const float* __restrict__ out2, const float* __restrict__ gup, float* __restrict__ grows) {
  extern __shared__ float sn_rows[];
  __shared__ float dR[SN_MAX_M * SN_DP], dL[SN_MAX_M * SN_DP];
  __shared__ float rowres[SN_MAX_M][4];
  __shared__ int64_t idx[4][SN_MAX_M];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const int pitch = (C > D ? C : D) | 1;
  float* A = sn_rows;
  float* Bm = sn_rows + M * pitch;
  int64_t len = lengths[b];
  const int K = (int)(len < 0 ? 0 : (len > M ? M : len));
  if (tid < 4 * K) {
    const int r = tid / K, t = tid - r * K;
    const int64_t* src = r == 0 ? rra : r == 1 ? rrb : r == 2 ? era : erb;
    idx[r][t] = src[b * M + t];
  }
  __syncthreads();
  sn_stage(A, Bm, pitch, ref, C, idx[0], idx[1], K);
  __syncthreads();
  sn_dist(dR, A, Bm, pitch, C, K);
  __syncthreads();
  sn_stage(A, Bm, pitch, emb, D, idx[2], idx[3], K);
  __syncthreads();
  sn_dist(dL, A, Bm, pitch, D, K);
  __syncthreads();
  const int gw = K <= 16 ? 16 : 32, ng = 256 / gw;
  const int g = tid / gw, j = tid - g * gw;
  for (int t = g; t < K; t += ng) {
    const SnRow r = sn_row(j, gw, K, itr, itl, min_valid,
                           [&](int c, float& a, float& d) {
                             if (excl && c == t) return false;
                             a = dR[t * SN_DP + c];
                             d = dL[t * SN_DP + c];
                             return true;
                           },
                           [&](int c, float v) {
                             if (BWD) { const float d = dL[t * SN_DP + c]; dR[t * SN_DP + c] = d > 0.f ? v / d : 0.f; }
                           });
    if (j == 0) { rowres[t][0] = r.kl; rowres[t][1] = r.ep; rowres[t][2] = r.eq; rowres[t][3] = r.cnt; }
  }
  __syncthreads();
  if (!BWD) {
    if (tid == 0) {
      float kl = 0.f, ep = 0.f, eq = 0.f, ov = 0.f, rows = 0.f;
      for (int t = 0; t < K; ++t)
        if (rowres[t][3] >= (float)min_valid) { kl += rowres[t][0]; ep += rowres[t][1]; eq += rowres[t][2]; ov += rowres[t][3]; rows += 1.f; }
      sn_write_pairstat(pairstat + b * SN_NSTAT, kl, rows, ov, ep, eq);
    }
  } else {
    const float rows = pairstat[b * SN_NSTAT + SN_ROWS], sumw = out2[1];
    const float sc = (rows > 0.f && sumw > 0.f) ? gup[0] * (weights ? weights[b] : 1.f) / (sumw * rows) : 0.f;
    float* ga_out = grows + b * (int64_t)M * D;
    float* gb_out = grows + (B + b) * (int64_t)M * D;
    for (int i = tid; i < M * D; i += 256) {
      const int t = i / D, c = i - t * D;
      float ga = 0.f, gb = 0.f;
      if (t < K && sc != 0.f) {
        const float at = A[t * pitch + c], bt = Bm[t * pitch + c];
        for (int u = 0; u < K; ++u) {
          ga = fmaf(dR[t * SN_DP + u], at - Bm[u * pitch + c], ga);
          gb = fmaf(-dR[u * SN_DP + t], A[u * pitch + c] - bt, gb);
        }
        ga *= sc;
        gb *= sc;
      }
      ga_out[i] = ga;
      gb_out[i] = gb;
    }
  }
}

static int sn_check_matrix(int64_t B, int M, float itr, float itl, int min_valid) {
  if (B < 1 || M < 1 || B > 0x7fffffff) return frl_fail(-2, "soft_nbr: needs 1 <= B < 2^31 pairs and M >= 1");
  if (!(itr > 0.f) || !(itl > 0.f)) return frl_fail(-2, "soft_nbr: temperatures must be positive");
  if (min_valid < 2) return frl_fail(-2, "soft_nbr: min_valid_per_row must be >= 2");
  return 0;
}

static int sn_check_gathered(int64_t B, int M, int C, int D, int dtype, float itr, float itl, int min_valid) {
  int rc = sn_check_matrix(B, M, itr, itl, min_valid);
  if (rc) return rc;
  if (M > SN_MAX_M) return frl_fail(-2, "soft_nbr_gathered: supports M <= 32");
  if (C < 1 || C > SN_MAX_W || D < 1 || D > SN_MAX_W) return frl_fail(-2, "soft_nbr_gathered: supports 1 <= C <= 256 and 1 <= D <= 256");
  if (dtype != FRL_F32 && dtype != FRL_BF16) return frl_fail(-2, "soft_nbr_gathered: emb dtype must be FRL_F32 or FRL_BF16");
  return 0;
}

template <typename T, bool BWD>
static int sn_launch_gathered(const float* ref, int C, const void* emb, int D, const int64_t* rra, const int64_t* rrb, const int64_t* era,
                              const int64_t* erb, const int64_t* lengths, const float* weights, int64_t B, int M, int excl, float itr, float itl,
                              int min_valid, float* pairstat, const float* out2, const float* gup, float* grows, hipStream_t st) {
  auto kern = sn_gathered_kernel<T, BWD>;
  const size_t lds = (size_t)2 * M * ((C > D ? C : D) | 1) * sizeof(float);
  // with the 10 KB of static LDS the widest shapes pass the 64 KB a kernel gets by default; asked for at every such launch (a function
  // attribute, not a stream operation), so it holds on whichever device and thread the call runs
  if (lds > 48 * 1024) FRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  FRL_LAUNCH_AS(BWD ? "sn_gathered_bwd_kernel" : "sn_gathered_fwd_kernel", kern, dim3((unsigned)B), dim3(256), lds, st, ref, C, (const T*)emb, D,
                rra, rrb, era, erb, lengths, weights, B, M, excl, itr, itl, min_valid, pairstat, out2, gup, grows);
  return 0;
}

extern "C" {

// d_ref, d_learned [B][M][M] f32, mask [B][M][M] bytes, weights [B] or NULL; inv_tau_* = 1 / temperature.  Outputs: pairstat [B][6]
// (L_b, rows_b, sum of unmasked counts, sum H(p), sum H(q), sum kl over the contributing rows), coef [B][M][M] = (p - q) / tau_learned or
// NULL (no gradient wanted), out2 [2] = loss, sum_w, stats [8] f64 (see sn_reduce_kernel).
int frl_soft_nbr_fwd(const float* d_ref, const float* d_learned, const unsigned char* mask, const float* weights, int64_t B, int M,
                     float inv_tau_ref, float inv_tau_learned, int min_valid, float* pairstat, float* coef, float* out2, double* stats,
                     hipStream_t stream) {
  int rc = sn_check_matrix(B, M, inv_tau_ref, inv_tau_learned, min_valid);
  if (rc) return rc;
  if (!d_ref || !d_learned || !mask || !pairstat || !out2 || !stats) return frl_fail(-2, "soft_nbr_fwd: NULL argument");
  FRL_LAUNCH(sn_matrix_fwd_kernel, dim3((unsigned)B), dim3(256), 0, stream, d_ref, d_learned, mask, M, inv_tau_ref, inv_tau_learned, min_valid,
             pairstat, coef);
  FRL_LAUNCH(sn_reduce_kernel, dim3(1), dim3(1024), 0, stream, (const float*)pairstat, weights, B, out2, stats);
  return frl_check_launch("soft_nbr_fwd");
}

// grad [B][M][M] = gup[0] * w_b / (sum_w * rows_b) * coef  (zeros for inactive pairs and when sum_w <= 0)
int frl_soft_nbr_bwd(const float* coef, const float* pairstat, const float* weights, const float* out2, const float* gup, int64_t B, int M,
                     float* grad, hipStream_t stream) {
  if (B < 1 || M < 1) return frl_fail(-2, "soft_nbr_bwd: needs B >= 1 and M >= 1");
  if (!coef || !pairstat || !out2 || !gup || !grad) return frl_fail(-2, "soft_nbr_bwd: NULL argument");
  const int64_t mm = (int64_t)M * M;
  FRL_LAUNCH(sn_matrix_bwd_kernel, dim3(frl_grid(B * mm, 256, 4096)), dim3(256), 0, stream, coef, pairstat, weights, out2, gup, B * mm, mm, grad);
  return frl_check_launch("soft_nbr_bwd");
}

// ref [R][C] f32, emb [R][D] (dtype 0 = float32, 1 = bfloat16), four [B][M] int64 row-index arrays already inside [0, R), lengths [B] int64
// (K_b, clamped into [0, M]); mask = t < K_b and t' < K_b, minus the diagonal when exclude_diagonal.  M <= 32, C, D <= 256.
int frl_soft_nbr_gathered_fwd(const float* ref, int C, const void* emb, int D, int emb_dtype, const int64_t* ref_rows_a, const int64_t* ref_rows_b,
                              const int64_t* emb_rows_a, const int64_t* emb_rows_b, const int64_t* lengths, const float* weights, int64_t B, int M,
                              int exclude_diagonal, float inv_tau_ref, float inv_tau_learned, int min_valid, float* pairstat, float* out2,
                              double* stats, hipStream_t stream) {
  int rc = sn_check_gathered(B, M, C, D, emb_dtype, inv_tau_ref, inv_tau_learned, min_valid);
  if (rc) return rc;
  if (!ref || !emb || !ref_rows_a || !ref_rows_b || !emb_rows_a || !emb_rows_b || !lengths || !pairstat || !out2 || !stats)
    return frl_fail(-2, "soft_nbr_gathered_fwd: NULL argument");
  FRL_BY_DTYPE(emb_dtype, T,
               rc = sn_launch_gathered<T, false>(ref, C, emb, D, ref_rows_a, ref_rows_b, emb_rows_a, emb_rows_b, lengths, weights, B, M,
                                                 exclude_diagonal, inv_tau_ref, inv_tau_learned, min_valid, pairstat, nullptr, nullptr, nullptr,
                                                 stream));
  if (rc) return rc;
  FRL_LAUNCH(sn_reduce_kernel, dim3(1), dim3(1024), 0, stream, (const float*)pairstat, weights, B, out2, stats);
  return frl_check_launch("soft_nbr_gathered_fwd");
}

// grad_rows [2][B][M][D] f32: role a (emb_rows_a) then role b, scaled by gup[0] * w_b / (sum_w * rows_b); zeros beyond K_b.
int frl_soft_nbr_gathered_bwd(const float* ref, int C, const void* emb, int D, int emb_dtype, const int64_t* ref_rows_a, const int64_t* ref_rows_b,
                              const int64_t* emb_rows_a, const int64_t* emb_rows_b, const int64_t* lengths, const float* weights, int64_t B, int M,
                              int exclude_diagonal, float inv_tau_ref, float inv_tau_learned, int min_valid, const float* pairstat,
                              const float* out2, const float* gup, float* grad_rows, hipStream_t stream) {
  int rc = sn_check_gathered(B, M, C, D, emb_dtype, inv_tau_ref, inv_tau_learned, min_valid);
  if (rc) return rc;
  if (!ref || !emb || !ref_rows_a || !ref_rows_b || !emb_rows_a || !emb_rows_b || !lengths || !pairstat || !out2 || !gup || !grad_rows)
    return frl_fail(-2, "soft_nbr_gathered_bwd: NULL argument");
  FRL_BY_DTYPE(emb_dtype, T,
               rc = sn_launch_gathered<T, true>(ref, C, emb, D, ref_rows_a, ref_rows_b, emb_rows_a, emb_rows_b, lengths, weights, B, M,
                                                exclude_diagonal, inv_tau_ref, inv_tau_learned, min_valid, const_cast<float*>(pairstat), out2,
                                                gup, grad_rows, stream));
  if (rc) return rc;
  return frl_check_launch("soft_nbr_gathered_bwd");
}

}  // extern "C"
