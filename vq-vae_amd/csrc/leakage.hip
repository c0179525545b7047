// Phase-type leakage loss (frl/training/representation/step.py:1015-1021): the Frobenius norm of the cross-covariance between the
// pre-FiLM bottleneck rows h [N][P] and the stop-gradient type embedding z [N][Dz]:
//   h_c = h - mean_rows(h), z_c = z - mean_rows(z), C = h_c^T z_c / max(N-1, 1), loss = sqrt(sum C^2)
// A cousin of the VICReg term (csrc/vicreg.hip) with the same structure.  Forward = moments kernel -> fixed-order slab sum
// (frl_reduce.hpp) -> one-workgroup finalise:
//   * the moments are taken about a PIVOT p = the mean of the first min(N, 64) rows, formed as row 0 plus the mean of the differences
//     from row 0 in row order (the same bits in every workgroup; a constant column gives exactly its constant):
//     Sh_p = sum_n (h_np - ph_p), Sz_d = sum_n (z_nd - pz_d), G_pd = sum_n (h_np - ph_p)(z_nd - pz_d), so that
//     C = (G - Sh Sz^T / N) / max(N-1, 1) cancels only |mean - pivot| against the spread, never |mean|;
//   * each workgroup reduces a contiguous row range into a private f32 slab [P*Dz cross | P | Dz]; no float atomics: loss and gradient
//     are bit-reproducible call to call.  The work is tiny (2 N P Dz flop) and launch-bound: plain FMAs.
// Backward = ONE kernel:  dh[n][p] = g * sum_d z_c[n][d] C[p][d] / (max(N-1, 1) * loss)  (the centring Jacobian drops out because the
// rows of z_c sum to zero: sum_n z_c[n][d] = 0, so the -mean(h) term contributes nothing).  g is read on the device.  Where loss == 0
// (N = 1, constant columns, exact orthogonality) the gradient is ZERO; the reference's autograd gives NaN there (sqrt' at 0).
#include "frl_common.hpp"
#include "frl_host.hpp"
#include "frl_reduce.hpp"
#include <math.h>

#define LK_ROWS 64        // rows per staged tile
#define LK_MAX_P 64
#define LK_MAX_DZ 128
#define LK_MAX_WGS 256    // slabs of the moments kernel

// piv[c] = X[0][c] + (sum_{r < nr} (X[r][c] - X[0][c])) / nr, nr = min(N, LK_ROWS), summed in row order
template <typename T>
__device__ __forceinline__ float lk_pivot(const T* __restrict__ X, int64_t N, int D, int c) {
  const int nr = N < LK_ROWS ? (int)N : LK_ROWS;
  const float x0 = to_f32(X[c]);
  float s = 0.f;
  for (int r = 1; r < nr; ++r) s += to_f32(X[(int64_t)r * D + c]) - x0;
  return x0 + s / (float)nr;
}

// slot of column p of h in a staged row: thread half (p & 1) owns the PU consecutive slots of p = half, half + 2, ...
template <int PU> __device__ __forceinline__ int lk_hslot(int p) { return (p & 1) * PU + (p >> 1); }

// ---------------------------------------------------------------------------------------------------------------------------------
// moments: slab[wg] = [P*Dz] G | [P] Sh | [Dz] Sz over the workgroup's rows.  Thread t owns column d = t & 127 of z and the PU columns
// p = (t >> 7), (t >> 7) + 2, ... of h; a row of h is read as PU / 4 broadcast 16-byte LDS reads.
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename TH, typename TZ, int PU>
__global__ __launch_bounds__(256) void leakage_moments_kernel(const TH* __restrict__ h, const TZ* __restrict__ z, float* __restrict__ slab, int64_t N,
                                                              int P, int Dz, int64_t rows_per_wg) {
  __shared__ __attribute__((aligned(16))) float ht[LK_ROWS][2 * PU];
  __shared__ float zt[LK_ROWS][LK_MAX_DZ];
  __shared__ float piv[LK_MAX_P + LK_MAX_DZ];
  const int tid = threadIdx.x, d = tid & 127, half = tid >> 7;
  if (tid < P) piv[tid] = lk_pivot<TH>(h, N, P, tid);
  else if (tid - P < Dz) piv[LK_MAX_P + tid - P] = lk_pivot<TZ>(z, N, Dz, tid - P);
  for (int i = tid; i < LK_ROWS * 2 * PU; i += 256) (&ht[0][0])[i] = 0.f;       // slots of columns >= P stay zero
  float acc[PU];
#pragma unroll
  for (int u = 0; u < PU; ++u) acc[u] = 0.f;
  float sz = 0.f, sh = 0.f;
  const int64_t p_begin = (int64_t)blockIdx.x * rows_per_wg;
  int64_t p_end = p_begin + rows_per_wg;
  if (p_end > N) p_end = N;
  for (int64_t p0 = p_begin; p0 < p_end; p0 += LK_ROWS) {
    __syncthreads();                                                             // (first pass: the zero fill and the pivot; later: the last tile's reads)
    const int rows = p_end - p0 < LK_ROWS ? (int)(p_end - p0) : LK_ROWS;
    for (int i = tid; i < LK_ROWS * P; i += 256) {                               // the tile of h is LK_ROWS * P contiguous elements
      const int r = i / P, p = i - r * P;
      ht[r][lk_hslot<PU>(p)] = r < rows ? to_f32(h[p0 * P + i]) - piv[p] : 0.f;
    }
    for (int i = tid; i < LK_ROWS * Dz; i += 256) {
      const int r = i / Dz, c = i - r * Dz;
      zt[r][c] = r < rows ? to_f32(z[p0 * Dz + i]) - piv[LK_MAX_P + c] : 0.f;
    }
    __syncthreads();
    if (d < Dz) {
#pragma unroll 4
      for (int r = 0; r < LK_ROWS; ++r) {
        const float zv = zt[r][d];
        if (half == 0) sz += zv;
        const f32x4* hv = reinterpret_cast<const f32x4*>(&ht[r][half * PU]);
#pragma unroll
        for (int u4 = 0; u4 < PU / 4; ++u4) {
          const f32x4 a = hv[u4];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[4 * u4 + e] = fmaf(a[e], zv, acc[4 * u4 + e]);
        }
      }
    }
    if (tid < P) {
      const int slot = lk_hslot<PU>(tid);
      for (int r = 0; r < LK_ROWS; ++r) sh += ht[r][slot];
    }
  }
  float* my = slab + (int64_t)blockIdx.x * ((int64_t)P * Dz + P + Dz);
  if (d < Dz) {
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      const int p = half + 2 * u;
      if (p < P) my[(int64_t)p * Dz + d] = acc[u];
    }
    if (half == 0) my[(int64_t)P * Dz + P + d] = sz;
  }
  if (tid < P) my[(int64_t)P * Dz + tid] = sh;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// finalise (one workgroup): m = [P*Dz] G | [P] Sh | [Dz] Sz  ->  stats [2] = loss, 1 / (max(N-1, 1) * loss) (0 where loss == 0: the
// backward then writes zeros); cmat [P*Dz] = C and centre [2][Dz] = pz | mean_z - pz when a gradient is wanted.  The combination runs in
// double: it is P*Dz values, and G - Sh Sz^T / N is the one subtraction of the scheme.
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename TZ>
__global__ __launch_bounds__(256) void leakage_finalise_kernel(const TZ* __restrict__ z, const float* __restrict__ m, int64_t N, int P, int Dz,
                                                               float* __restrict__ stats, float* __restrict__ cmat, float* __restrict__ centre) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const float* Sh = m + (int64_t)P * Dz;
  const float* Sz = Sh + P;
  const double n = (double)N, den = N > 1 ? n - 1.0 : 1.0;
  double sq = 0.0;
  for (int i = tid; i < P * Dz; i += 256) {
    const int p = i / Dz, d = i - p * Dz;
    const double c = ((double)m[i] - (double)Sh[p] * (double)Sz[d] / n) / den;
    if (cmat != nullptr) cmat[i] = (float)c;
    sq += c * c;
  }
  if (centre != nullptr)
    for (int c = tid; c < Dz; c += 256) {
      centre[c] = lk_pivot<TZ>(z, N, Dz, c);
      centre[Dz + c] = (float)((double)Sz[c] / n);
    }
  red[tid] = sq;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {                                            // fixed-order sum
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const double loss = sqrt(red[0]);
    stats[0] = (float)loss;
    stats[1] = loss > 0.0 ? (float)(1.0 / (den * loss)) : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// backward: a workgroup owns 64 rows = 64 P contiguous elements of dh; C [P][Dz] and the centred tile of z are in LDS (pitch Dz + 1:
// the lanes of a wave walk p fastest, so their rows of C sit on different banks; the row of z is a broadcast).
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename TZ, typename TH>
__global__ __launch_bounds__(256) void leakage_bwd_kernel(const TZ* __restrict__ z, const float* __restrict__ cmat, const float* __restrict__ centre,
                                                          const float* __restrict__ stats, const float* __restrict__ g, int64_t N, int P, int Dz,
                                                          TH* __restrict__ dh) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int pitch = Dz + 1;
  float* Cs = reinterpret_cast<float*>(smem);                                    // [P][pitch]
  float* zt = Cs + P * pitch;                                                    // [LK_ROWS][pitch]
  const int tid = threadIdx.x;
  const int64_t p0 = (int64_t)blockIdx.x * LK_ROWS;
  const int rows = N - p0 < LK_ROWS ? (int)(N - p0) : LK_ROWS;
  const float scale = g[0] * stats[1];
  for (int i = tid; i < P * Dz; i += 256) {
    const int p = i / Dz, d = i - p * Dz;
    Cs[p * pitch + d] = cmat[i];
  }
  for (int i = tid; i < rows * Dz; i += 256) {
    const int r = i / Dz, c = i - r * Dz;
    zt[r * pitch + c] = (to_f32(z[p0 * Dz + i]) - centre[c]) - centre[Dz + c];
  }
  __syncthreads();
  for (int e = tid; e < rows * P; e += 256) {
    const int r = e / P, p = e - r * P;
    const float* zr = zt + r * pitch;
    const float* cr = Cs + p * pitch;
    float s = 0.f;
    for (int d = 0; d < Dz; ++d) s = fmaf(zr[d], cr[d], s);
    dh[p0 * P + e] = from_f32<TH>(scale * s);
  }
}

static int lk_nwg(int64_t N) { return frl_moment_wgs(N, LK_ROWS, LK_MAX_WGS); }
static size_t lk_slab_floats(int P, int Dz) { return (size_t)P * Dz + P + Dz; }

template <typename TH, typename TZ>
static void lk_launch_moments(const void* h, const void* z, float* slab, int64_t N, int P, int Dz, hipStream_t st) {
  const int nwg = lk_nwg(N);
  const int64_t rows = frl_moment_rows_per_wg(N, LK_ROWS, LK_MAX_WGS);
  if (P <= 16) FRL_LAUNCH((leakage_moments_kernel<TH, TZ, 8>), dim3(nwg), dim3(256), 0, st, (const TH*)h, (const TZ*)z, slab, N, P, Dz, rows);
  else if (P <= 32) FRL_LAUNCH((leakage_moments_kernel<TH, TZ, 16>), dim3(nwg), dim3(256), 0, st, (const TH*)h, (const TZ*)z, slab, N, P, Dz, rows);
  else FRL_LAUNCH((leakage_moments_kernel<TH, TZ, 32>), dim3(nwg), dim3(256), 0, st, (const TH*)h, (const TZ*)z, slab, N, P, Dz, rows);
}

template <typename TZ, typename TH>
static int lk_launch_bwd(const void* z, const float* cmat, const float* centre, const float* stats, const float* g, int64_t N, int P, int Dz,
                         void* dh, hipStream_t st) {
  const size_t lds = (size_t)(P + LK_ROWS) * (Dz + 1) * sizeof(float);          // at most 128 * 129 * 4 = 66048 bytes
  auto kern = leakage_bwd_kernel<TZ, TH>;
  static bool lds_set = false;                                                   // per instantiation: once, not on every launch of a captured step
  if (lds > 64 * 1024 && !lds_set) {
    FRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    lds_set = true;
  }
  FRL_LAUNCH_AS("leakage_bwd_kernel", kern, dim3((unsigned)((N + LK_ROWS - 1) / LK_ROWS)), dim3(256), lds, st, (const TZ*)z, cmat, centre, stats,
                g, N, P, Dz, (TH*)dh);
  return 0;
}

static int lk_check(const void* z, int64_t N, int P, int Dz, int h_dtype, int z_dtype) {
  if (z == nullptr) return frl_fail(-2, "leakage: NULL rows");
  if (N < 1 || N > ((int64_t)0x7fffffff) * LK_ROWS) return frl_fail(-2, "leakage: needs 1 <= N <= 64 * (2^31 - 1) rows");
  if (P < 1 || P > LK_MAX_P) return frl_fail(-2, "leakage: supports 1 <= P <= 64 columns of h");
  if (Dz < 1 || Dz > LK_MAX_DZ) return frl_fail(-2, "leakage: supports 1 <= Dz <= 128 columns of z");
  if ((h_dtype != FRL_F32 && h_dtype != FRL_BF16) || (z_dtype != FRL_F32 && z_dtype != FRL_BF16))
    return frl_fail(-2, "leakage: dtypes must be FRL_F32 or FRL_BF16");
  return 0;
}

extern "C" {

// slabs of the moments kernel plus the summed moments: (workgroups + 1) * (P*Dz + P + Dz) floats
size_t frl_leakage_workspace_bytes(int64_t N, int P, int Dz) {
  if (N < 1 || P < 1 || Dz < 1) return 0;
  return (size_t)(lk_nwg(N) + 1) * lk_slab_floats(P, Dz) * sizeof(float);
}

int frl_leakage_fwd(const void* h, int h_dtype, const void* z, int z_dtype, int64_t N, int P, int Dz, float* stats, float* cmat, float* centre,
                    void* ws, size_t ws_bytes, hipStream_t stream) {
  int rc = lk_check(z, N, P, Dz, h_dtype, z_dtype);
  if (rc) return rc;
  if (h == nullptr || stats == nullptr || (cmat == nullptr) != (centre == nullptr))
    return frl_fail(-2, "leakage_fwd: h and stats are required; cmat and centre go together");
  if (ws == nullptr || ws_bytes < frl_leakage_workspace_bytes(N, P, Dz)) return frl_fail(-4, "leakage_fwd: workspace too small");
  const int nwg = lk_nwg(N);
  const int64_t n = (int64_t)lk_slab_floats(P, Dz);
  float* slab = (float*)ws;
  float* mom = slab + (int64_t)nwg * n;
  FRL_BY_DTYPE(h_dtype, TH, FRL_BY_DTYPE(z_dtype, TZ, lk_launch_moments<TH, TZ>(h, z, slab, N, P, Dz, stream)));
  launch_slab_reduce<float, CopyEpi>(slab, nwg, n, CopyEpi{mom}, stream);
  if (z_dtype == FRL_F32)
    FRL_LAUNCH(leakage_finalise_kernel<float>, dim3(1), dim3(256), 0, stream, (const float*)z, (const float*)mom, N, P, Dz, stats, cmat, centre);
  else
    FRL_LAUNCH(leakage_finalise_kernel<bf16>, dim3(1), dim3(256), 0, stream, (const bf16*)z, (const float*)mom, N, P, Dz, stats, cmat, centre);
  return frl_check_launch("leakage_fwd");
}

// stats [2], cmat [P][Dz] and centre [2][Dz] as frl_leakage_fwd wrote them; g [1] device float: the upstream gradient; dh in h_dtype
int frl_leakage_bwd(const void* z, int z_dtype, const float* cmat, const float* centre, const float* stats, const float* g, int64_t N, int P,
                    int Dz, void* dh, int h_dtype, hipStream_t stream) {
  int rc = lk_check(z, N, P, Dz, h_dtype, z_dtype);
  if (rc) return rc;
  if (cmat == nullptr || centre == nullptr || stats == nullptr || g == nullptr || dh == nullptr) return frl_fail(-2, "leakage_bwd: NULL argument");
  FRL_BY_DTYPE(z_dtype, TZ, FRL_BY_DTYPE(h_dtype, TH, rc = lk_launch_bwd<TZ, TH>(z, cmat, centre, stats, g, N, P, Dz, dh, stream)));
  if (rc) return rc;
  return frl_check_launch("leakage_bwd");
}

}  // extern "C"
