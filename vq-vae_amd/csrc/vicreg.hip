// VICReg variance-covariance loss over rows X [N][D] (frl/losses/variance_covariance.py:14-88; callers
// frl/training/representation/step.py:551,623):
//   mu = mean_rows(X), Xc = X - mu, cov = Xc^T Xc / (N-1), std_j = sqrt(cov_jj + eps)
//   variance_loss = mean_j relu(target - std_j), covariance_loss = sum_{j != k} cov_jk^2 / D, total = vw * variance + cw * covariance
// Forward = moments kernel -> fixed-order slab sum (frl_reduce.hpp) -> one-workgroup finalise:
//   * the moments are taken about a PIVOT p = the mean of the first min(N, 64) rows (every workgroup forms it itself, in the same order:
//     identical bits everywhere; a single outlying row moves it by 1/64 of its distance):  S_j = sum_n (x_nj - p_j),
//     G_jk = sum_n (x_nj - p_j)(x_nk - p_k), so that cov = (G - S S^T / N) / (N-1) cancels only |mu - p| (a fraction of one std)
//     against std, never |mu| -- one pass over the rows, no f32 loss when |mu| >> std.  The difference x - p is formed in f32 (exact for bf16 rows and, for f32 rows, up
//     to one rounding of a value of the size of the spread), so BOTH row dtypes run the f32 MFMA 16x16x4: a centred value is not a bf16
//     number, and rounding it to one costs 2^-9 of every product, far outside the f32 bound the loss is held to;
//   * each workgroup reduces a contiguous row range into a private f32 slab [D*D Gram | D sums]; no float atomics: loss and gradient
//     are bit-reproducible call to call.
// Backward = ONE kernel:  dX = ((X - p) - delta) A,  delta = mu - p (p and delta are saved by the forward: centre [2][D]),
//   A = (4 cwe / (D (N-1))) offdiag(cov) - diag(vwe 1[std_j < target] / (D (N-1) std_j)),   cwe = g_total cw + g_cov,  vwe = g_total vw + g_var
// (the centring Jacobian drops out because the rows of Xc sum to zero).  Every workgroup builds A in LDS from cov and the three upstream
// scalars, which are read on the device: no host sync, a captured step replays it.
#include "frl_common.hpp"
#include "frl_host.hpp"
#include "frl_reduce.hpp"
#include <math.h>

#define VC_KP 64          // rows per staged tile
#ifndef VC_MAX_WGS
#define VC_MAX_WGS 1024   // slabs of the moments kernel / workgroups of the backward (A/B tools/vicreg_bench.py: 1024 beats 512 at all three shapes)
#endif

// pivot[c] = mean of column c over the first min(N, VC_KP) rows, summed in row order (the same bits in every workgroup); 0 for c >= D
template <typename T>
__device__ __forceinline__ void vc_pivot(const T* __restrict__ X, int64_t N, int D, int DP, float* __restrict__ piv, int tid) {
  const int nr = N < VC_KP ? (int)N : VC_KP;
  for (int c = tid; c < DP; c += 256) {
    float s = 0.f;
    if (c < D) {
#pragma unroll 16
      for (int r = 0; r < VC_KP; ++r) s += r < nr ? to_f32(X[(int64_t)r * D + c]) : 0.f;   // (independent loads, summed in row order)
    }
    piv[c] = s / (float)nr;
  }
}

// ---- staging of a 64-row tile, centred about the pivot, as f32 [VC_KP][pitch] in LDS --------------------------------------------
// vec: D % 4 == 0 -> 4-element accesses (16 B of f32 rows, 8 B of bf16 rows) prefetched into registers behind the MFMAs of the tile in
// flight; otherwise element by element.  Columns D..DP-1 of the image are zeroed once and never written again.
template <typename T, int DB>
struct VcStage {
  static constexpr int DP = DB * 16;
  static constexpr int NV = (VC_KP * DP / 4 + 255) / 256;   // 4-element vectors per thread and tile
  float r[NV][4];

  __device__ __forceinline__ void fetch(const T* __restrict__ X, int64_t p0, int64_t p_end, int D, int tid) {
    const int vpr = D >> 2;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int i = tid + u * 256;
      const int row = i / vpr, c0 = (i - row * vpr) * 4;
      const bool ok = row < VC_KP && p0 + row < p_end;
      const T* src = X + (ok ? (p0 + row) * (int64_t)D + c0 : 0);
      if constexpr (sizeof(T) == 2) {
        bf16x4 v = *reinterpret_cast<const bf16x4*>(src);
#pragma unroll
        for (int e = 0; e < 4; ++e) r[u][e] = (float)v[e];
      } else {
        f32x4 v = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
        for (int e = 0; e < 4; ++e) r[u][e] = v[e];
      }
    }
  }
  // piv: pivot row in LDS [DP]; sub: second subtrahend (delta, backward) or nullptr
  __device__ __forceinline__ void commit(float* __restrict__ tile, int pitch, const float* __restrict__ piv, const float* __restrict__ sub,
                                         int64_t p0, int64_t p_end, int D, int tid) const {
    const int vpr = D >> 2;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int i = tid + u * 256;
      const int row = i / vpr, c0 = (i - row * vpr) * 4;
      if (row >= VC_KP) continue;
      const bool ok = p0 + row < p_end;
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float d = r[u][e] - piv[c0 + e];
        if (sub != nullptr) d -= sub[c0 + e];
        v[e] = ok ? d : 0.f;
      }
      *reinterpret_cast<f32x4*>(tile + row * pitch + c0) = v;
    }
  }
  // element-wise path (D not a multiple of 4)
  static __device__ __forceinline__ void stage_scalar(float* __restrict__ tile, int pitch, const float* __restrict__ piv,
                                                      const float* __restrict__ sub, const T* __restrict__ X, int64_t p0, int64_t p_end,
                                                      int D, int tid) {
    for (int i = tid; i < VC_KP * D; i += 256) {
      const int row = i / D, c = i - row * D;
      float d = 0.f;
      if (p0 + row < p_end) {
        d = to_f32(X[(p0 + row) * (int64_t)D + c]) - piv[c];
        if (sub != nullptr) d -= sub[c];
      }
      tile[row * pitch + c] = d;
    }
  }
};

// ---------------------------------------------------------------------------------------------------------------------------------
// moments: slab[wg] = [D*D] G | [D] S over the workgroup's rows.  4 waves; wave w owns the Gram row blocks w*OBW .. w*OBW+OBW-1.
// LDS pitch DP + 16: the fragment read [row kc][column r16] puts the two rows of a 32-lane half 16 banks apart.
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T, int DB>
__global__ __launch_bounds__(256) void vicreg_moments_kernel(const T* __restrict__ X, float* __restrict__ slab, int64_t N, int D,
                                                             int64_t rows_per_wg) {
  constexpr int DP = DB * 16, OBW = (DB + 3) / 4, pitch = DP + 16;
  __shared__ __attribute__((aligned(16))) float tile[VC_KP * pitch];
  __shared__ float piv[DP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, kc = lane >> 4;

  for (int i = tid; i < VC_KP * pitch; i += 256) tile[i] = 0.f;
  vc_pivot<T>(X, N, D, DP, piv, tid);

  f32x4 acc[OBW][DB], accs[OBW];
#pragma unroll
  for (int o = 0; o < OBW; ++o) {
    accs[o] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < DB; ++i) acc[o][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int64_t p_begin = (int64_t)blockIdx.x * rows_per_wg;
  int64_t p_end = p_begin + rows_per_wg;
  if (p_end > N) p_end = N;
  const bool vec = (D & 3) == 0 && ((uintptr_t)X & 15) == 0;   // 4-element accesses need aligned row starts
  VcStage<T, DB> st;
  if (vec && p_begin < p_end) st.fetch(X, p_begin, p_end, D, tid);
  const float ones = (r16 == 0) ? 1.f : 0.f;

  for (int64_t p0 = p_begin; p0 < p_end; p0 += VC_KP) {
    __syncthreads();                                           // (first pass: the zero fill and the pivot; later: the MFMAs of the last tile)
    if (vec) st.commit(tile, pitch, piv, nullptr, p0, p_end, D, tid);
    else VcStage<T, DB>::stage_scalar(tile, pitch, piv, nullptr, X, p0, p_end, D, tid);
    __syncthreads();
    if (vec && p0 + VC_KP < p_end) st.fetch(X, p0 + VC_KP, p_end, D, tid);
    if (wave * OBW < DB) {                                     // wave-uniform: waves without a row block (D <= 48) only stage
#pragma unroll 4
      for (int ks = 0; ks < VC_KP / 4; ++ks) {
        const float* rowp = tile + (ks * 4 + kc) * pitch + r16;
        float bf[DB];
#pragma unroll
        for (int i = 0; i < DB; ++i) bf[i] = rowp[i * 16];
#pragma unroll
        for (int o = 0; o < OBW; ++o) {
          const int ab = wave * OBW + o;
          if (ab < DB) {
            const float af = rowp[ab * 16];
#pragma unroll
            for (int i = 0; i < DB; ++i) acc[o][i] = mfma16(af, bf[i], acc[o][i]);
            accs[o] = mfma16(af, ones, accs[o]);               // column 0 of the product with a "ones" column = the column sums
          }
        }
      }
    }
  }
  float* my = slab + (int64_t)blockIdx.x * ((int64_t)D * D + D);
#pragma unroll
  for (int o = 0; o < OBW; ++o) {
    const int ab = wave * OBW + o;
    if (ab >= DB) continue;
#pragma unroll
    for (int i = 0; i < DB; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = ab * 16 + kc * 4 + r, k = i * 16 + r16;
        if (j < D && k < D) my[(int64_t)j * D + k] = acc[o][i][r];
      }
    if (r16 == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = ab * 16 + kc * 4 + r;
        if (j < D) my[(int64_t)D * D + j] = accs[o][r];
      }
    }
  }
}

// fixed-order sum of 256 doubles (one workgroup); every thread returns the total
__device__ __forceinline__ double vc_block_sum(double v, double* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// finalise (one workgroup): m = [D*D] G | [D] S  ->  losses [3] = total, variance, covariance;  cov [D*D] and centre [2][D] = p | mu - p
// when a gradient is wanted (cov != nullptr).  The combination runs in double: it is D*D values, and G - S S^T / N is the one subtraction of
// the scheme.
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void vicreg_finalise_kernel(const T* __restrict__ X, const float* __restrict__ m, int64_t N, int D, float vw,
                                                              float cw, float target, float eps, float* __restrict__ losses,
                                                              float* __restrict__ cov, float* __restrict__ centre) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const float* S = m + (int64_t)D * D;
  const double n = (double)N, inv = 1.0 / (n - 1.0);
  double sq = 0.0, hinge = 0.0;
  for (int i = tid; i < D * D; i += 256) {
    const int j = i / D, k = i - j * D;
    const double c = ((double)m[i] - (double)S[j] * (double)S[k] / n) * inv;
    if (cov != nullptr) cov[i] = (float)c;
    if (j != k) sq += c * c;
    else {
      const double h = (double)target - sqrt((c > 0.0 ? c : 0.0) + (double)eps);     // (rounding can leave a variance just below zero)
      hinge += h > 0.0 ? h : 0.0;
    }
  }
  if (centre != nullptr) {
    vc_pivot<T>(X, N, D, D, centre, tid);
    for (int j = tid; j < D; j += 256) centre[D + j] = (float)((double)S[j] / n);
  }
  const double cl = vc_block_sum(sq, red) / (double)D;
  const double vl = vc_block_sum(hinge, red) / (double)D;
  if (tid == 0) {
    losses[0] = (float)((double)vw * vl + (double)cw * cl);
    losses[1] = (float)vl;
    losses[2] = (float)cl;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// backward: dX[p][k] = sum_j Xc[p][j] A[j][k], computed transposed (A is symmetric): MFMA rows = output columns, MFMA columns = the 16
// pixels of the wave, so a lane ends with 4 CONSECUTIVE output columns of one pixel -> 16-byte (f32) / 8-byte (bf16) stores.
// Both operands are read as [row r16][column kc]: pitch DP + 4 spreads the 64 lanes over the 64 banks.
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T, int DB>
__global__ __launch_bounds__(256) void vicreg_bwd_kernel(const T* __restrict__ X, const float* __restrict__ cov, const float* __restrict__ centre,
                                                         const float* __restrict__ g3, int64_t N, int D, float vw, float cw, float target,
                                                         float eps, T* __restrict__ dX, int64_t rows_per_wg) {
  constexpr int DP = DB * 16, pitch = DP + 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tile = reinterpret_cast<float*>(smem);                // [VC_KP][pitch]
  float* As = tile + VC_KP * pitch;                            // [DP][pitch]
  float* piv = As + DP * pitch;                                // [DP]
  float* del = piv + DP;                                       // [DP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, kc = lane >> 4;

  const int64_t p_begin = (int64_t)blockIdx.x * rows_per_wg;
  int64_t p_end = p_begin + rows_per_wg;
  if (p_end > N) p_end = N;
  if (p_begin >= p_end) return;                                // (block-uniform)

  {
    const float g0 = g3[0], gv = g3[1], gc = g3[2];
    const float cwe = g0 * cw + gc, vwe = g0 * vw + gv;
    const float dn = (float)D * (float)(N - 1);
    const float coff = 4.f * cwe / dn;
    for (int i = tid; i < DP * pitch; i += 256) {
      const int j = i / pitch, k = i - j * pitch;
      float a = 0.f;
      if (j < D && k < D) {
        const float c = cov[j * D + k];
        if (j != k) a = coff * c;
        else {
          const float sd = sqrtf(fmaxf(c, 0.f) + eps);
          a = sd < target ? -vwe / (dn * sd) : 0.f;
        }
      }
      As[i] = a;
    }
    for (int i = tid; i < VC_KP * pitch; i += 256) tile[i] = 0.f;
    for (int i = tid; i < DP; i += 256) {
      piv[i] = i < D ? centre[i] : 0.f;
      del[i] = i < D ? centre[D + i] : 0.f;
    }
  }
  const bool vec = (D & 3) == 0 && (((uintptr_t)X | (uintptr_t)dX) & 15) == 0;
  VcStage<T, DB> st;
  if (vec) st.fetch(X, p_begin, p_end, D, tid);

  for (int64_t p0 = p_begin; p0 < p_end; p0 += VC_KP) {
    __syncthreads();
    if (vec) st.commit(tile, pitch, piv, del, p0, p_end, D, tid);
    else VcStage<T, DB>::stage_scalar(tile, pitch, piv, del, X, p0, p_end, D, tid);
    __syncthreads();
    if (vec && p0 + VC_KP < p_end) st.fetch(X, p0 + VC_KP, p_end, D, tid);
    f32x4 acc[DB];
#pragma unroll
    for (int i = 0; i < DB; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* xr = tile + (wave * 16 + r16) * pitch + kc;
    const float* ar = As + r16 * pitch + kc;
#pragma unroll 4
    for (int js = 0; js < DP / 4; ++js) {
      const float bf = xr[js * 4];
#pragma unroll
      for (int i = 0; i < DB; ++i) acc[i] = mfma16(ar[i * 16 * pitch + js * 4], bf, acc[i]);
    }
    const int64_t p = p0 + wave * 16 + r16;
    if (p < p_end) {
      T* dst = dX + p * (int64_t)D;
#pragma unroll
      for (int i = 0; i < DB; ++i) {
        const int c0 = i * 16 + kc * 4;
        if (vec) {
          if (c0 < D) {
            if constexpr (sizeof(T) == 2) {
              *reinterpret_cast<bf16x4*>(dst + c0) = bf16x4{(bf16)acc[i][0], (bf16)acc[i][1], (bf16)acc[i][2], (bf16)acc[i][3]};
            } else {
              *reinterpret_cast<f32x4*>(dst + c0) = acc[i];
            }
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (c0 + r < D) dst[c0 + r] = from_f32<T>(acc[i][r]);
        }
      }
    }
  }
}

static int vc_nwg(int64_t N) { return frl_moment_wgs(N, VC_KP, VC_MAX_WGS); }
static int64_t vc_rows_per_wg(int64_t N) { return frl_moment_rows_per_wg(N, VC_KP, VC_MAX_WGS); }

template <typename T, int DB>
static void vc_launch_moments(const void* x, float* slab, int64_t N, int D, hipStream_t st) {
  FRL_LAUNCH((vicreg_moments_kernel<T, DB>), dim3(vc_nwg(N)), dim3(256), 0, st, (const T*)x, slab, N, D, vc_rows_per_wg(N));
}

template <typename T, int DB>
static int vc_launch_bwd(const void* x, const float* cov, const float* centre, const float* g3, int64_t N, int D, float vw, float cw,
                         float target, float eps, void* dx, hipStream_t st) {
  constexpr int DP = DB * 16, pitch = DP + 4;
  const size_t lds = (size_t)((VC_KP + DP) * pitch + 2 * DP) * sizeof(float);
  auto kern = vicreg_bwd_kernel<T, DB>;
  static bool lds_set = false;                                 // per instantiation: once, not on every launch of a captured step
  if (lds > 64 * 1024 && !lds_set) {
    FRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    lds_set = true;
  }
  FRL_LAUNCH_AS("vicreg_bwd_kernel", kern, dim3(vc_nwg(N)), dim3(256), lds, st, (const T*)x, cov, centre, g3, N, D, vw, cw, target, eps, (T*)dx,
                vc_rows_per_wg(N));
  return 0;
}

static int vc_check(const char* what, const void* x, int64_t N, int D, int dtype) {
  (void)what;
  if (x == nullptr) return frl_fail(-2, "vicreg: NULL rows");
  if (N < 2) return frl_fail(-2, "vicreg: needs N >= 2 rows (the caller returns zeros for fewer)");
  if (D < 1 || D > 128) return frl_fail(-2, "vicreg: supports 1 <= D <= 128");
  if (dtype != FRL_F32 && dtype != FRL_BF16) return frl_fail(-2, "vicreg: dtype must be FRL_F32 or FRL_BF16");
  return 0;
}

extern "C" {

// slabs of the moments kernel plus the summed moments: (workgroups + 1) * (D*D + D) floats
size_t frl_vicreg_workspace_bytes(int64_t N, int D) {
  if (N < 1 || D < 1) return 0;
  return (size_t)(vc_nwg(N) + 1) * ((size_t)D * D + D) * sizeof(float);
}

int frl_vicreg_fwd(const void* x, int64_t N, int D, int dtype, float variance_weight, float covariance_weight, float variance_target,
                   float eps, float* losses, float* cov, float* centre, void* ws, size_t ws_bytes, hipStream_t stream) {
  int rc = vc_check("fwd", x, N, D, dtype);
  if (rc) return rc;
  if (losses == nullptr || (cov == nullptr) != (centre == nullptr)) return frl_fail(-2, "vicreg_fwd: losses is required; cov and centre go together");
  if (ws == nullptr || ws_bytes < frl_vicreg_workspace_bytes(N, D)) return frl_fail(-4, "vicreg_fwd: workspace too small");
  const int nwg = vc_nwg(N);
  const int64_t n = (int64_t)D * D + D;
  float* slab = (float*)ws;
  float* mom = slab + (int64_t)nwg * n;
  const int db = (D + 15) / 16;
#define VC_CASE(B) vc_launch_moments<T, B>(x, slab, N, D, stream)
  FRL_BY_DTYPE(dtype, T, if (db <= 1) VC_CASE(1); else if (db <= 2) VC_CASE(2); else if (db <= 4) VC_CASE(4); else VC_CASE(8));
#undef VC_CASE
  launch_slab_reduce<float, CopyEpi>(slab, nwg, n, CopyEpi{mom}, stream);
  if (dtype == FRL_F32)                                        // (written out: the type's spelling keys the timing report)
    FRL_LAUNCH(vicreg_finalise_kernel<float>, dim3(1), dim3(256), 0, stream, (const float*)x, (const float*)mom, N, D, variance_weight,
               covariance_weight, variance_target, eps, losses, cov, centre);
  else
    FRL_LAUNCH(vicreg_finalise_kernel<bf16>, dim3(1), dim3(256), 0, stream, (const bf16*)x, (const float*)mom, N, D, variance_weight,
               covariance_weight, variance_target, eps, losses, cov, centre);
  return frl_check_launch("vicreg_fwd");
}

// g3 [3] device floats: upstream gradients of (total, variance_loss, covariance_loss); dx in the dtype of x
int frl_vicreg_bwd(const void* x, const float* cov, const float* centre, const float* g3, int64_t N, int D, int dtype, float variance_weight,
                   float covariance_weight, float variance_target, float eps, void* dx, hipStream_t stream) {
  int rc = vc_check("bwd", x, N, D, dtype);
  if (rc) return rc;
  if (cov == nullptr || centre == nullptr || g3 == nullptr || dx == nullptr) return frl_fail(-2, "vicreg_bwd: NULL argument");
  const int db = (D + 15) / 16;
#define VC_CASE(B) rc = vc_launch_bwd<T, B>(x, cov, centre, g3, N, D, variance_weight, covariance_weight, variance_target, eps, dx, stream)
  FRL_BY_DTYPE(dtype, T, if (db <= 1) VC_CASE(1); else if (db <= 2) VC_CASE(2); else if (db <= 4) VC_CASE(4); else VC_CASE(8));
#undef VC_CASE
  if (rc) return rc;
  return frl_check_launch("vicreg_bwd");
}

}  // extern "C"
