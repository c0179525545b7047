// Diagonal-covariance Gaussian mixtures (sklearn.mixture.GaussianMixture(covariance_type="diag"), as the reference's
// frl/training/fit_gmm_clusters.py and fit_landscape_categories.py use it) and the phase summary of the latter.
//
// One EM iteration reads X [N][D] once.  With y = x - p (p = the column mean of X, frl_gmm_pivot, once per fit) and m = mu - p,
//   lp[n][k] = a_k + sum_d y^2 A_kd + sum_d y B_kd,   A = -1/2 / var,  B = m / var,
//   a_k = log pi_k - 1/2 (D log 2 pi + sum_d log var_kd + sum_d m_kd^2 / var_kd)          (a_k in double, rounded once)
// which is a [rows] x [K x 2D] product, and the moments  S0 = sum w r,  S1 = sum w r y,  S2 = sum w r y^2  are r^T x [y | y^2].
// Both run on v_mfma_f32_16x16x4_f32 (exact float32, an fmaf chain in k order).  A workgroup of four waves walks 64-row tiles in a
// grid-stride loop: a tile is staged once in LDS (pivot subtracted), each wave forms lp, the softmax and w r for its 16 rows and
// parks w r in LDS transposed; then the waves share out the (K/16) x (2D/16) moment blocks, whose accumulators stay in registers
// for the whole loop (the moment half is the scheme of frl_moments.hpp).  Responsibilities never reach memory.  Each workgroup writes one
// slab of partial sums; frl_gmm_m_step adds the slabs in the order of moment_slab_sum and forms the parameters, the lower bound and the
// convergence flag on the device, so the host can enqueue iterations blind.  No float atomics anywhere: results are bit-identical run to run.
//
// The state the iteration carries is (pi, m = mu - p, var): mu itself is only an output, so data far from the origin loses nothing
// to the rounding of mu.
#include "frl_common.hpp"
#include "frl_host.hpp"
#include "frl_moments.hpp"

#define GMM_MAX_K 128
#define GMM_MAX_D 128
#define GMM_MAX_KD 8192
#define GMM_RS 68          // row stride of the transposed w r tile [Kp][64]: lanes (k, row) hit 64 distinct banks
#define GMM_LDS_MAX (160 * 1024)
#define GMM_PIVOT_WG 256
// 1: the variants with at most 8 moment blocks per wave are compiled for two waves per SIMD (two workgroups per CU), which costs a few
// spilled registers and hides the barriers and LDS latency of one workgroup behind the other: measured 1.6x on the E pass at
// N = 500 000, D = 64, K = 50 and no change at K = 5 (tools/gmm_bench.py).  -DGMM_FORCE_OCC=0 builds the one-wave variants for an A/B.
#ifndef GMM_FORCE_OCC
#define GMM_FORCE_OCC 1
#endif

enum { GMM_SOFT = 0, GMM_HARD = 1, GMM_SCORE = 2 };
enum { GMM_M_EM = 0, GMM_M_LLOYD = 1, GMM_M_INIT = 2 };

namespace {

struct GmmDims {
  int KB, DB, Kp, Dp, NS, ys, nblk, slabF;
  size_t lds;
};

GmmDims gmm_dims(int D, int K) {
  GmmDims g;
  g.KB = (K + 15) / 16;
  g.DB = (D + 15) / 16;
  g.Kp = 16 * g.KB;
  g.Dp = 16 * g.DB;
  g.NS = 4 * g.DB;
  const int ys = g.ys = frl_tile_stride(g.Dp);
  g.nblk = g.KB * 2 * g.DB;
  g.slabF = g.nblk * 256 + g.Kp;
  g.lds = sizeof(float) * ((size_t)2 * g.Kp * g.Dp + g.Kp + g.Dp + (size_t)MOMENT_ROWS * ys + (size_t)g.Kp * GMM_RS + MOMENT_ROWS);
  return g;
}

int gmm_grid(int64_t N, const GmmDims& g, int workgroups) {
  if (workgroups > 0) return workgroups;
  const int64_t ntiles = (N + MOMENT_ROWS - 1) / MOMENT_ROWS;
  const int64_t cap = g.lds <= 80 * 1024 ? 512 : 256;                            // two workgroups per CU where LDS allows
  return (int)(ntiles < cap ? ntiles : cap);
}

// workspace: dsl [G][2] double | red [slabF] double | pivot partials / slabs [G][slabF] float
struct GmmWs {
  double* dsl;
  double* red;
  float* slabs;
  size_t bytes;
};
GmmWs gmm_ws(void* ws, int G, const GmmDims& g) {
  GmmWs o;
  o.dsl = (double*)ws;
  o.red = o.dsl + 2 * (size_t)G;
  o.slabs = (float*)(o.red + g.slabF);
  o.bytes = sizeof(double) * (2 * (size_t)G + g.slabF) + sizeof(float) * (size_t)G * g.slabF;
  return o;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------
// the pivot: column means of X, in double, chunk by chunk in a fixed order
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gmm_pivot_partial_kernel(const float* __restrict__ X, int N, int D, int rows_per_wg,
                                                                double* __restrict__ part) {
  __shared__ double hi[GMM_MAX_D];
  const int c = threadIdx.x & 127, rg = threadIdx.x >> 7;
  const int r0 = blockIdx.x * rows_per_wg;
  const int r1 = r0 + rows_per_wg < N ? r0 + rows_per_wg : N;
  double s = 0.0;
  if (c < D)
    for (int r = r0 + rg; r < r1; r += 2) s += (double)X[(size_t)r * D + c];
  if (rg == 1 && c < D) hi[c] = s;
  __syncthreads();
  if (rg == 0 && c < D) part[(size_t)blockIdx.x * D + c] = s + hi[c];
}

__global__ __launch_bounds__(128) void gmm_pivot_final_kernel(const double* __restrict__ part, int G, int N, int D, float* __restrict__ pivot) {
  const int c = threadIdx.x;
  if (c >= D) return;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += part[(size_t)g * D + c];
  pivot[c] = (float)(s / (double)N);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// E step (soft | hard) and scoring.  KBM: register capacity in 16-component blocks, NBM: moment blocks per wave.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int KBM, int NBM, int MODE>
__global__ __launch_bounds__(256, (GMM_FORCE_OCC && NBM <= 8 ? 2 : 1)) void gmm_e_kernel(const float* __restrict__ X, const float* __restrict__ w, int N, int D, int K, int KB,
                                                    int DB, int ys, int vec, const float* __restrict__ pivot, const float* __restrict__ pi,
                                                    const float* __restrict__ mc, const float* __restrict__ var,
                                                    const int* __restrict__ state, float* __restrict__ slabs, double* __restrict__ dsl,
                                                    float* __restrict__ lse_out, int* __restrict__ labels, float* __restrict__ resp) {
  if (MODE != GMM_SCORE && state[1]) return;                                     // converged: nothing is touched any more
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double dred[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
  const int Kp = 16 * KB, Dp = 16 * DB, NS = 4 * DB;
  float* PA = reinterpret_cast<float*>(smem);                                    // [KB][NS][64] fragments of A (k = lane & 15, d = 4 s + lane >> 4)
  float* PB = PA + Kp * Dp;
  float* ak = PB + Kp * Dp;                                                      // [Kp], -inf beyond K
  float* piv = ak + Kp;                                                          // [Dp]
  float* yt = piv + Dp;                                                          // [64][ys]
  float* rT = yt + MOMENT_ROWS * ys;                                             // [Kp][GMM_RS]
  float* wrow = rT + Kp * GMM_RS;                                                // [64]

  for (int i = tid; i < Kp * Dp; i += 256) {
    const int l = i & 63, fs = i >> 6, s = fs % NS, kb = fs / NS;
    const int k = kb * 16 + (l & 15), d = 4 * s + (l >> 4);
    float a = 0.f, b = 0.f;
    if (k < K && d < D) {
      const float iv = 1.f / var[k * D + d];
      a = -0.5f * iv;
      b = mc[k * D + d] * iv;
    }
    PA[i] = a;
    PB[i] = b;
  }
  for (int k = tid; k < Kp; k += 256) {
    float a = -__builtin_inff();
    if (k < K) {
      double s = 0.0;
      for (int d = 0; d < D; ++d) {
        const double v = (double)var[k * D + d], m = (double)mc[k * D + d];
        s += log(v) + m * m / v;
      }
      a = (float)(log((double)pi[k]) - 0.5 * ((double)D * 1.8378770664093453 + s));
    }
    ak[k] = a;
  }
  for (int d = tid; d < Dp; d += 256) piv[d] = d < D ? pivot[d] : 0.f;
  for (int i = tid; i < MOMENT_ROWS * ys; i += 256) yt[i] = 0.f;                // the padding columns stay zero

  f32x4 macc[NBM];
  float s0[KBM][4];
#pragma unroll
  for (int i = 0; i < NBM; ++i) macc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < KBM; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) s0[kb][r] = 0.f;
  double dl = 0.0, dw = 0.0;

  const int ntiles = (N + MOMENT_ROWS - 1) / MOMENT_ROWS, tileF = MOMENT_ROWS * D;
  f32x4 pre[8];
  float wpre = 0.f;
  auto fetch = [&](int tile) {
    const int row0 = tile * MOMENT_ROWS;
    const int valid = (N - row0 < MOMENT_ROWS ? N - row0 : MOMENT_ROWS) * D;    // floats of the tile that exist
    const float* base = X + (size_t)row0 * D;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int e0 = (c * 256 + tid) * 4;
      pre[c] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (e0 >= tileF) continue;
      if (vec && e0 + 4 <= valid) pre[c] = *reinterpret_cast<const f32x4*>(base + e0);
      else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (e0 + j < valid) pre[c][j] = base[e0 + j];
      }
    }
    if (tid < MOMENT_ROWS) wpre = row0 + tid < N ? (w ? w[row0 + tid] : 1.f) : 0.f;
  };
  auto commit = [&](int tile) {
    const int row0 = tile * MOMENT_ROWS;
    const int valid = (N - row0 < MOMENT_ROWS ? N - row0 : MOMENT_ROWS) * D;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int e0 = (c * 256 + tid) * 4;
      if (e0 >= tileF) continue;
      if (vec) {                                                                 // D % 4 == 0: the four floats share a row
        const int row = e0 / D, col = e0 - row * D;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (e0 < valid) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = pre[c][j] - piv[col + j];
        }
        *reinterpret_cast<f32x4*>(yt + row * ys + col) = v;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = e0 + j;
          if (e < tileF) {
            const int row = e / D, col = e - row * D;
            yt[row * ys + col] = e < valid ? pre[c][j] - piv[col] : 0.f;
          }
        }
      }
    }
    if (tid < MOMENT_ROWS) wrow[tid] = wpre;
  };

  if ((int)blockIdx.x < ntiles) fetch(blockIdx.x);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    __syncthreads();                                                             // the previous tile is consumed (and the prologue is written)
    commit(tile);
    __syncthreads();
    if (tile + (int)gridDim.x < ntiles) fetch(tile + gridDim.x);

    // ---- lp of this wave's 16 rows: acc[kb][r] is component 16 kb + 4 lg + r of row lr
    f32x4 acc[KBM];
#pragma unroll
    for (int kb = 0; kb < KBM; ++kb) acc[kb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* yrow = yt + (wave * 16 + lr) * ys + lg;
#pragma unroll 4
    for (int s = 0; s < NS; ++s) {                                               // NS = 4 DB: whole groups of four, their LDS reads in flight together
      const float yv = yrow[4 * s], y2 = yv * yv;
#pragma unroll
      for (int kb = 0; kb < KBM; ++kb)
        if (kb < KB) {
          acc[kb] = mfma16(PA[(kb * NS + s) * 64 + lane], y2, acc[kb]);
          acc[kb] = mfma16(PB[(kb * NS + s) * 64 + lane], yv, acc[kb]);
        }
    }
    float best = -__builtin_inff();
    int bestk = 0x7fffffff;
#pragma unroll
    for (int kb = 0; kb < KBM; ++kb)
      if (kb < KB) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = kb * 16 + 4 * lg + r;
          const float v = acc[kb][r] + ak[k];
          acc[kb][r] = v;
          if (v > best) { best = v; bestk = k; }                                 // ascending k: the lowest k of equal values stays
        }
      }
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float ov = __shfl_xor(best, o, 64);
      const int ok = __shfl_xor(bestk, o, 64);
      if (ov > best || (ov == best && ok < bestk)) { best = ov; bestk = ok; }
    }
    const int rl = wave * 16 + lr;                                               // row within the tile
    const float wr = wrow[rl];
    float lse = best, inv = 1.f;
    if (MODE != GMM_HARD) {
      float sum = 0.f;
#pragma unroll
      for (int kb = 0; kb < KBM; ++kb)
        if (kb < KB) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float e = expf(acc[kb][r] - best);
            acc[kb][r] = e;
            sum += e;
          }
        }
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      lse = best + logf(sum);
      inv = 1.f / sum;
    }
    if (MODE == GMM_SCORE) {
      const int64_t row = (int64_t)tile * MOMENT_ROWS + rl;
      if (row < N) {
        if (lg == 0) {
          lse_out[row] = lse;
          labels[row] = bestk;
        }
        if (resp) {
#pragma unroll
          for (int kb = 0; kb < KBM; ++kb)
            if (kb < KB) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int k = kb * 16 + 4 * lg + r;
                if (k < K) resp[row * K + k] = acc[kb][r] * inv;
              }
            }
        }
      }
      continue;                                                                  // (uniform: MODE is a template argument)
    }
#pragma unroll
    for (int kb = 0; kb < KBM; ++kb)
      if (kb < KB) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = kb * 16 + 4 * lg + r;
          const float rw = MODE == GMM_HARD ? (k == bestk ? wr : 0.f) : acc[kb][r] * inv * wr;
          s0[kb][r] += rw;
          rT[k * GMM_RS + rl] = rw;
        }
      }
    if (lg == 0) {
      dl += (double)wr * (double)lse;
      dw += (double)wr;
    }
    __syncthreads();

    // ---- moments: block b = wave + 4 i is components 16 kb.. x columns 16 cb.. of [y | y^2]
    const int nb2 = 2 * DB, nblk = KB * nb2;
#pragma unroll
    for (int i = 0; i < NBM; ++i) {
      const int b = wave + 4 * i;
      if (b < nblk) {
        const int kb = b / nb2, cb = b - kb * nb2;
        const bool sq = cb >= DB;
        const float* ap = rT + (kb * 16 + lr) * GMM_RS + lg;
        const float* vp = yt + lg * ys + (sq ? cb - DB : cb) * 16 + lr;
#pragma unroll 4
        for (int st = 0; st < MOMENT_ROWS / 4; ++st) {
          float v = vp[4 * st * ys];
          if (sq) v *= v;
          macc[i] = mfma16(ap[4 * st], v, macc[i]);
        }
      }
    }
  }
  if (MODE == GMM_SCORE) return;

  // ---- the slab of this workgroup: moment blocks in fragment order | S0 [Kp]; sum w lse, sum w in dsl
  const int nblk = KB * 2 * DB, slabF = nblk * 256 + Kp;
  float* slab = slabs + (size_t)blockIdx.x * slabF;
#pragma unroll
  for (int i = 0; i < NBM; ++i) {                                                // (written out: DESIGN 6v)
    const int b = wave + 4 * i;
    if (b < nblk) *reinterpret_cast<f32x4*>(slab + ((size_t)b * 64 + lane) * 4) = macc[i];
  }
  __syncthreads();                                                               // rT is free: it carries the per-wave S0 now
#pragma unroll
  for (int kb = 0; kb < KBM; ++kb)
    if (kb < KB) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = s0[kb][r];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
        if (lr == 0) rT[wave * Kp + kb * 16 + 4 * lg + r] = v;
      }
    }
  dl = wave_sum_d(dl);
  dw = wave_sum_d(dw);
  if (lane == 0) {
    dred[2 * wave] = dl;
    dred[2 * wave + 1] = dw;
  }
  __syncthreads();
  for (int k = tid; k < Kp; k += 256) slab[nblk * 256 + k] = ((rT[k] + rT[Kp + k]) + rT[2 * Kp + k]) + rT[3 * Kp + k];
  if (tid == 0) {
    dsl[2 * (size_t)blockIdx.x] = ((dred[0] + dred[2]) + dred[4]) + dred[6];
    dsl[2 * (size_t)blockIdx.x + 1] = ((dred[1] + dred[3]) + dred[5]) + dred[7];
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// M step: the slabs added in double (moment_slab_sum), then one workgroup forms the parameters, the lower bound and the flag
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gmm_m_reduce_kernel(const float* __restrict__ slabs, int G, int slabF, const int* __restrict__ state,
                                                           double* __restrict__ red) {
  if (state[1]) return;
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);
  const double sum = moment_slab_sum(slabs, G, slabF, e, e < slabF);             // the S0 tail of a slab need not fill 64 elements
  if (threadIdx.x < 64 && e < slabF) red[e] = sum;
}

__global__ __launch_bounds__(256) void gmm_m_final_kernel(const double* __restrict__ red, const double* __restrict__ dsl, int G, int D, int K,
                                                          int KB, int DB, const float* __restrict__ pivot, float* __restrict__ pi,
                                                          float* __restrict__ mu, float* __restrict__ mc, float* __restrict__ var,
                                                          double reg_covar, double tol, int mode, double* __restrict__ history,
                                                          int max_iter, int* __restrict__ state) {
  if (state[1]) return;
  __shared__ double nk[GMM_MAX_K];
  __shared__ double pl[256], pw[256];
  __shared__ double tot;
  const int tid = threadIdx.x, nb2 = 2 * DB, nblk = KB * nb2;
  if (tid < K) nk[tid] = red[nblk * 256 + tid] + (mode == GMM_M_LLOYD ? 0.0 : 10.0 * 2.220446049250313e-16);
  double sl = 0.0, sw = 0.0;
  for (int g = tid; g < G; g += 256) {
    sl += dsl[2 * (size_t)g];
    sw += dsl[2 * (size_t)g + 1];
  }
  pl[tid] = sl;
  pw[tid] = sw;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int k = 0; k < K; ++k) t += nk[k];
    tot = t;
  }
  __syncthreads();
  for (int e = tid; e < K * D; e += 256) {
    const int k = e / D, d = e - k * D;
    const size_t i1 = moment_frag_index((k >> 4) * nb2 + (d >> 4), k & 15, d & 15), i2 = i1 + (size_t)DB * 256;   // y | y^2 are DB blocks apart
    const double n = nk[k];
    if (mode == GMM_M_LLOYD) {
      if (n > 0.0) {                                                             // a centre without a row keeps its value
        const double m = red[i1] / n;
        mc[e] = (float)m;
        mu[e] = (float)((double)pivot[d] + m);
      }
    } else {
      const double m = red[i1] / n;
      mc[e] = (float)m;
      mu[e] = (float)((double)pivot[d] + m);
      var[e] = (float)(red[i2] / n - m * m + reg_covar);
    }
  }
  if (mode != GMM_M_LLOYD && tid < K) pi[tid] = (float)(nk[tid] / tot);
  if (mode == GMM_M_EM && tid == 0) {
    double L = 0.0, W = 0.0;
    for (int t = 0; t < 256; ++t) {
      L += pl[t];
      W += pw[t];
    }
    const double lb = L / W;
    const int it = state[0];
    if (it < max_iter) {
      const bool conv = it >= 1 && fabs(lb - history[it - 1]) < tol;
      history[it] = lb;
      state[0] = it + 1;
      if (conv) state[1] = 1;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// phase summary: four rows per workgroup, lane d of a wave owns channel d
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void phase_summary_kernel(const float* __restrict__ z, const float* __restrict__ ysfc, int64_t N, int T, int D,
                                                            float low_max, float high_min, float* __restrict__ summary,
                                                            float* __restrict__ tvar) {
  const int d = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;                                                            // whole waves leave together
  const float* zp = z + (size_t)n * T * D + d;
  const float* yp = ysfc + (size_t)n * T;
  double sa = 0.0, sd = 0.0, sr = 0.0;
  int cd = 0, cr = 0;
  const bool on = d < D;
  for (int t = 0; t < T; ++t) {
    const float y = yp[t];
    const float v = on ? zp[(size_t)t * D] : 0.f;
    const bool fin = fabsf(y) < __builtin_inff();                                // false for NaN and for the infinities
    sa += v;
    if (fin && y <= low_max) { sd += v; ++cd; }
    if (fin && y >= high_min) { sr += v; ++cr; }
  }
  const double mean = sa / (double)T;
  double q = 0.0;
  if (on)
    for (int t = 0; t < T; ++t) {
      const double c = (double)zp[(size_t)t * D] - mean;
      q += c * c;
    }
  const float vard = on ? (float)(q / (double)(T - 1)) : 0.f;                    // 0 / 0 = NaN at T = 1, as torch.var gives
  const float tv = wave_sum(vard) / (float)D;
  if (on) {
    float* o = summary + (size_t)n * 3 * D;
    o[d] = cd ? (float)(sd / (double)cd) : (float)mean;
    o[D + d] = cr ? (float)(sr / (double)cr) : (float)mean;
    o[2 * D + d] = (float)mean;
  }
  if (d == 0) tvar[n] = tv;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

int gmm_check(const char* what, int64_t N, int D, int K) {
  const char* why = nullptr;
  if (K < 1 || K > GMM_MAX_K) why = "1 <= K <= 128 components";
  else if (D < 1 || D > GMM_MAX_D) why = "1 <= D <= 128 columns";
  else if ((int64_t)K * D > GMM_MAX_KD) why = "K * D <= 8192";
  else if (N < K) why = "N >= K rows";
  else if (N > 0x7fffffffll) why = "N < 2^31 rows";
  return why ? frl_failf(-2, "%s: needs %s", what, why) : 0;
}

typedef void (*gmm_e_fn)(const float*, const float*, int, int, int, int, int, int, int, const float*, const float*, const float*, const float*,
                         const int*, float*, double*, float*, int*, float*);

template <int MODE> gmm_e_fn gmm_pick(int KB, int NB) {
  if (MODE == GMM_SCORE) return KB <= 2 ? gmm_e_kernel<2, 1, MODE> : KB <= 4 ? gmm_e_kernel<4, 1, MODE> : gmm_e_kernel<8, 1, MODE>;
  if (KB <= 2) return NB <= 2 ? gmm_e_kernel<2, 2, MODE> : NB <= 8 ? gmm_e_kernel<2, 8, MODE> : gmm_e_kernel<2, 22, MODE>;
  if (KB <= 4) return NB <= 8 ? gmm_e_kernel<4, 8, MODE> : gmm_e_kernel<4, 22, MODE>;
  return NB <= 2 ? gmm_e_kernel<8, 2, MODE> : NB <= 8 ? gmm_e_kernel<8, 8, MODE> : gmm_e_kernel<8, 22, MODE>;
}

int gmm_launch_e(int mode, const float* X, const float* w, int64_t N, int D, int K, const float* pivot, const float* pi, const float* mc,
                 const float* var, const int* state, int G, float* slabs, double* dsl, float* lse, int* labels, float* resp,
                 hipStream_t stream) {
  const GmmDims g = gmm_dims(D, K);
  const int NB = (g.nblk + 3) / 4;
  if (g.lds > GMM_LDS_MAX || NB > 22) return frl_fail(-2, "gmm: K and D need more LDS or registers than a workgroup has");
  gmm_e_fn kern = mode == GMM_SCORE ? gmm_pick<GMM_SCORE>(g.KB, NB) : mode == GMM_HARD ? gmm_pick<GMM_HARD>(g.KB, NB) : gmm_pick<GMM_SOFT>(g.KB, NB);
  if (g.lds > 64 * 1024) FRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));
  const int vec = (D & 3) == 0 && ((uintptr_t)X & 15) == 0;
  FRL_LAUNCH_AS("gmm_e_kernel", kern, dim3((unsigned)G), dim3(256), g.lds, stream, X, w, (int)N, D, K, g.KB, g.DB, g.ys, vec, pivot, pi, mc, var,
                state, slabs, dsl, lse, labels, resp);
  return 0;
}

}  // namespace

extern "C" {

// See include/frl_hip.h.
size_t frl_gmm_workspace_bytes(int64_t N, int D, int K, int workgroups) {
  if (N < 1 || D < 1 || D > GMM_MAX_D || K < 1 || K > GMM_MAX_K || !frl_wg_in_range(workgroups)) return 0;
  const GmmDims g = gmm_dims(D, K);
  const size_t em = gmm_ws(nullptr, gmm_grid(N, g, workgroups), g).bytes;
  const size_t pv = sizeof(double) * GMM_PIVOT_WG * (size_t)D;
  return em > pv ? em : pv;
}

int frl_gmm_pivot(const float* X, int64_t N, int D, float* pivot, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (N < 1 || N > 0x7fffffffll) return frl_fail(-2, "gmm_pivot: needs 1 <= N < 2^31 rows");
  if (D < 1 || D > GMM_MAX_D) return frl_fail(-2, "gmm_pivot: needs 1 <= D <= 128 columns");
  if (!X || !pivot) return frl_fail(-2, "gmm_pivot: null pointer");
  if (!ws || ((uintptr_t)ws & 7) || ws_bytes < sizeof(double) * GMM_PIVOT_WG * (size_t)D) return frl_fail(-4, "gmm_pivot: workspace too small");
  const int rows = (int)((N + GMM_PIVOT_WG - 1) / GMM_PIVOT_WG), G = (int)((N + rows - 1) / rows);
  FRL_LAUNCH(gmm_pivot_partial_kernel, dim3((unsigned)G), dim3(256), 0, stream, X, (int)N, D, rows, (double*)ws);
  FRL_LAUNCH(gmm_pivot_final_kernel, dim3(1), dim3(128), 0, stream, (const double*)ws, G, (int)N, D, pivot);
  return frl_check_launch("gmm_pivot");
}

int frl_gmm_em_step(const float* X, const float* w, int64_t N, int D, int K, const float* pivot, const float* weights, const float* means_c,
                    const float* vars, int hard, int workgroups, const int* state, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (int rc = gmm_check("gmm_em_step", N, D, K)) return rc;
  if (int rc = frl_check_workgroups("gmm_em_step", workgroups)) return rc;
  if (!X || !pivot || !weights || !means_c || !vars || !state) return frl_fail(-2, "gmm_em_step: null pointer");
  const GmmDims g = gmm_dims(D, K);
  const int G = gmm_grid(N, g, workgroups);
  const GmmWs o = gmm_ws(ws, G, g);
  if (int rc = frl_check_workspace("gmm_em_step", ws, ws_bytes, o.bytes)) return rc;
  if (int rc = gmm_launch_e(hard ? GMM_HARD : GMM_SOFT, X, w, N, D, K, pivot, weights, means_c, vars, state, G, o.slabs, o.dsl, nullptr, nullptr,
                            nullptr, stream))
    return rc;
  return frl_check_launch("gmm_em_step");
}

int frl_gmm_m_step(int64_t N, int D, int K, const float* pivot, float* weights, float* means, float* means_c, float* vars, double reg_covar,
                   double tol, int mode, double* history, int max_iter, int* state, int workgroups, void* ws, size_t ws_bytes,
                   hipStream_t stream) {
  if (int rc = gmm_check("gmm_m_step", N, D, K)) return rc;
  if (int rc = frl_check_workgroups("gmm_m_step", workgroups)) return rc;
  if (mode < GMM_M_EM || mode > GMM_M_INIT) return frl_fail(-2, "gmm_m_step: mode must be 0 (EM), 1 (Lloyd) or 2 (initial parameters)");
  if (!pivot || !weights || !means || !means_c || !vars || !state) return frl_fail(-2, "gmm_m_step: null pointer");
  if (mode == GMM_M_EM && (!history || max_iter < 1)) return frl_fail(-2, "gmm_m_step: the EM mode needs history [max_iter], max_iter >= 1");
  const GmmDims g = gmm_dims(D, K);
  const int G = gmm_grid(N, g, workgroups);
  const GmmWs o = gmm_ws(ws, G, g);
  if (int rc = frl_check_workspace("gmm_m_step", ws, ws_bytes, o.bytes)) return rc;
  FRL_LAUNCH(gmm_m_reduce_kernel, dim3((unsigned)((g.slabF + 63) / 64)), dim3(256), 0, stream, (const float*)o.slabs, G, g.slabF,
             (const int*)state, o.red);
  FRL_LAUNCH(gmm_m_final_kernel, dim3(1), dim3(256), 0, stream, (const double*)o.red, (const double*)o.dsl, G, D, K, g.KB, g.DB, pivot, weights,
             means, means_c, vars, reg_covar, tol, mode, history, max_iter, state);
  return frl_check_launch("gmm_m_step");
}

int frl_gmm_score(const float* X, int64_t N, int D, int K, const float* pivot, const float* weights, const float* means_c, const float* vars,
                  float* lse, int* labels, float* resp, hipStream_t stream) {
  if (K < 1 || K > GMM_MAX_K || D < 1 || D > GMM_MAX_D || (int64_t)K * D > GMM_MAX_KD) return gmm_check("gmm_score", GMM_MAX_K, D, K);
  if (N < 1 || N > 0x7fffffffll) return frl_fail(-2, "gmm_score: needs 1 <= N < 2^31 rows");
  if (!X || !pivot || !weights || !means_c || !vars || !lse || !labels) return frl_fail(-2, "gmm_score: null pointer");
  const int64_t ntiles = (N + MOMENT_ROWS - 1) / MOMENT_ROWS;
  const int G = (int)(ntiles < FRL_MAX_WG ? ntiles : FRL_MAX_WG);
  if (int rc = gmm_launch_e(GMM_SCORE, X, nullptr, N, D, K, pivot, weights, means_c, vars, nullptr, G, nullptr, nullptr, lse, labels, resp, stream))
    return rc;
  return frl_check_launch("gmm_score");
}

int frl_phase_summary(const float* z_phase, const float* ysfc, int64_t N, int T, int D, float low_max, float high_min, float* summary,
                      float* temporal_var, hipStream_t stream) {
  if (N < 1 || N > 0x7fffffffll) return frl_fail(-2, "phase_summary: needs 1 <= N < 2^31 rows");
  if (T < 1 || T > 64) return frl_fail(-2, "phase_summary: needs 1 <= T <= 64 timesteps");
  if (D < 1 || D > 64) return frl_fail(-2, "phase_summary: needs 1 <= D <= 64 channels");
  if (!z_phase || !ysfc || !summary || !temporal_var) return frl_fail(-2, "phase_summary: null pointer");
  FRL_LAUNCH(phase_summary_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, stream, z_phase, ysfc, N, T, D, low_max, high_min, summary,
             temporal_var);
  return frl_check_launch("phase_summary");
}

}  // extern "C"
