// Vector-quantisation step: nearest-codebook assignment, straight-through / commitment gradients,
// EMA codebook statistics.  The reference no longer ships a quantizer; the definition implemented here
// is SURVEY.md section 8a row a11 (constants: frl/config/frl_model_v0.yaml:29-35,
// frl/config/frl_bindings_v0.yaml:887-891, scripts/train_vqvae.py:410-436).
//
// vq_assign: for every row z_n find argmin_k ||z_n - e_k||^2 (first index on ties), bit-exact against a
// float64 evaluation, while running the -2 z.e term on the matrix cores:
//   * codebook chunk (<= 512 codes) staged once per workgroup in LDS as packed MFMA A fragments holding
//     -2*e, plus ||e||^2; z streams from HBM as lane-quarter B fragments (16 vectors per tile, 16 B / lane);
//   * the accumulator starts at ||e_k||^2, so the MFMA result is the score ||e_k||^2 - 2 z.e_k (no batch bias); key = (f32 bits & ~127) |
//     index inside a group of 128 codes, ordered as FLOATS: v_min_f32 / v_min3_f32 track the running arg-min, v_med3_f32 the runner-up;
//     groups are folded into (best, runner-up, group), min-reduce over the 4 lane quarters by __shfl_xor at the end;
//   * rows whose runner-up is within the rigorous rounding + truncation bound of the minimum are flagged
//     (idx = -1 - provisional) and re-evaluated exactly in float64 (<1 % of rows): inside the kernel when the codebook is resident,
//     by vq_fixup_tile_kernel (16 rows per wave, candidates screened on the matrix cores) on the multi-chunk path;
//   * z_q gather, squared-error partial sums and the per-workgroup code histogram are fused in.
// Roofline: HBM for K <= 1024 (algorithmic bytes/vector = 2*d*s + 4), MFMA for K = 8192.
// One translation unit: the kernels live in vq_prepare.hpp, vq_assign_chunked.hpp (multi-chunk route, fixup, finalize),
// vq_assign_resident.hpp, vq_assign_stream.hpp and vq_bwd.hpp (backward, EMA, revive); what they share is in vq_common.hpp.  This file
// keeps the host side and the C ABI.
#include "frl_common.hpp"
#include "frl_host.hpp"
#include "vq_common.hpp"
#include "vq_prepare.hpp"
#include "vq_assign_chunked.hpp"
#include "vq_assign_resident.hpp"
#include "vq_assign_stream.hpp"
#include "vq_bwd.hpp"
#include "frl_pack.hpp"
#include <stdlib.h>

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static int vq_chunk(int K, int d_pad, size_t esize) {
  const size_t cap = 64 * 1024;                              // <= 64 KB of codes so that two workgroups fit a CU
  int kc = VQ_MAX_CHUNK;
  while (kc > 16 && (size_t)kc * d_pad * esize > cap) kc >>= 1;
  const int kpad = (K + 15) / 16 * 16;
  if (kc > kpad) kc = kpad;
  return kc;
}
// Large batches (d <= 64): 8-wave workgroups, two per CU (four waves per SIMD, two 16-vector tiles per wave inside the 128-register
// budget); the two workgroups of a CU drift apart, so one streams z / writes z_q while the other is in its MFMA loop.  Else 4 waves x 4 tiles.
static int vq_waves(int64_t N, int d) { return (d <= 64 && N >= (int64_t)256 * 8 * 2 * 16) ? 8 : 4; }
static int vq_grid(int64_t N, int d) {
  const int nw = vq_waves(N, d), NT = nw == 8 ? 2 : 4;
  const int64_t nb = (N + nw * NT * 16 - 1) / (nw * NT * 16);
  const int cap = 512;
  return (int)(nb < cap ? (nb < 1 ? 1 : nb) : cap);
}
#define VQ_FIX_WAVES 1024
#define VQ_BWD_WGS 256

// "prepared codebook": [||e||^2: kpad floats (3e38 beyond K)][packed -2e fragments of kpad codes]; kpad = K rounded up to whole chunks
struct VqPrep { size_t ctl, en, pack, total; int Kc, kpad, npk; };
template <typename T, int NF>
static VqPrep vq_prep_layout(int64_t N, int K, int d) {
  VqPrep P;
  const int d_pad = NF * DT<T>::FE * 4;
  P.Kc = vq_chunk(K, d_pad, sizeof(T));
  P.kpad = (K + P.Kc - 1) / P.Kc * P.Kc;
  P.npk = (P.kpad / 16) * NF * 64;
  P.ctl = 0;                                                        // VqCtl + counts_acc[K] (kpad >= 64 always holds the 64 header ints)
  P.en = (sizeof(VqCtl) + (size_t)K * 4 + 255) / 256 * 256;
  P.pack = P.en + ((size_t)P.kpad * 4 + 255) / 256 * 256;
  P.total = P.pack + (size_t)P.npk * sizeof(typename DT<T>::frag_t);
  return P;
}
static size_t vq_prep_bytes_max(int K) {
  return (sizeof(VqCtl) + (size_t)K * 4 + 255) / 256 * 256 + ((size_t)(K + VQ_MAX_CHUNK) * 4 + 255) / 256 * 256 +
         (size_t)((K + 15) / 16 + 64) * 16 * 128 * 4;
}

struct VqLayout { size_t hdr, counts_fix, partial, amb, amb_lim, prep, total; int grid; };
static VqLayout vq_layout(int64_t N, int K, int d) {
  VqLayout L;
  L.grid = vq_grid(N, d);
  size_t o = 0;
  L.hdr = o; o += 256;
  L.counts_fix = o; o += ((size_t)K * 4 + 255) / 256 * 256;       // [hdr, counts_fix / counts_acc] are zeroed every call
  L.partial = o; o += ((size_t)L.grid * 16 * 4 + 255) / 256 * 256;
  L.amb = o; o += ((size_t)N * 4 + 255) / 256 * 256;
  L.amb_lim = o; o += ((size_t)N * 4 + 255) / 256 * 256;
  L.prep = o; o += vq_prep_bytes_max(K);                           // prepared codebook of the one-call entry point
  L.total = o;
  return L;
}

template <typename T, int NF>
static int launch_vq_prepare(const float* E, int64_t N, int K, int d, char* prep, hipStream_t st) {
  typedef typename DT<T>::frag_t frag_t;
  const VqPrep P = vq_prep_layout<T, NF>(N, K, d);
  const int npack_blocks = (P.npk + 255) / 256;
  const int kz = P.kpad > 64 ? P.kpad : 64;                         // the norms blocks also zero the 64 header ints of the control block
  FRL_LAUNCH((vq_prepare_kernel<T, NF>), dim3(npack_blocks + (kz + 255) / 256), dim3(256), 0, st, E, K, d, (float*)(prep + P.en), P.kpad,
             (frag_t*)(prep + P.pack), P.npk, npack_blocks, (int*)(prep + P.ctl));
  return frl_check_launch("vq_prepare");
}

static int g_vq_stream_tiles = -1;    // frl_vq_stream_tiles(): -1 = the FRL_VQ_STREAM environment variable, else VQ_STREAM_DEFAULT
static int vq_stream_tiles();
#ifndef VQ_STREAM_DEFAULT
#define VQ_STREAM_DEFAULT 2   // tiles per wave and batch of the streaming kernel when FRL_VQ_STREAM is unset (0: resident kernel)
#endif
static int vq_stream_tiles() {
  if (g_vq_stream_tiles >= 0) return g_vq_stream_tiles;
  static const int env = [] { const char* e = getenv("FRL_VQ_STREAM"); return e ? atoi(e) : VQ_STREAM_DEFAULT; }();
  return env;
}
#ifndef VQ_RES_NT
#define VQ_RES_NT 4        // 16-row tiles per wave and batch of the resident kernel
#endif
// launch of an assignment kernel: every generation is timed under the one key "vq_assign_kernel"
template <typename... P, typename... A>
static int vq_launch_assign(void (*kern)(P...), int grid, int threads, size_t lds, hipStream_t st, A... args) {
  if (lds > 64 * 1024) FRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  FRL_LAUNCH_AS("vq_assign_kernel", kern, dim3(grid), dim3(threads), lds, st, args...);
  return 0;
}
template <typename T, int NF>
static int launch_vq(const void* z, const float* E, char* prep, int64_t N, int K, int d, int32_t* idx, void* zq, float* stats,
                     float* stats_copy, int32_t* counts, char* ws, hipStream_t st) {
  typedef typename DT<T>::frag_t frag_t;
  const VqLayout L = vq_layout(N, K, d);
  const VqPrep P = vq_prep_layout<T, NF>(N, K, d);
  const int nw = vq_waves(N, d);
  const int Kc = P.Kc;
  VqHeader* hdr = (VqHeader*)(ws + L.hdr);
  const bool resident = P.kpad == Kc;                                // the whole codebook is one LDS chunk
  if (!resident) FRL_HIP(hipMemsetAsync(ws, 0, L.partial, st));      // header + counts_fix of the multi-chunk path
  if (prep == nullptr) {                                             // one-call entry point: prepare into the workspace first
    const int rc = launch_vq_prepare<T, NF>(E, N, K, d, ws + L.prep, st);
    if (rc) return rc;
    prep = ws + L.prep;
  }
  const float* en = (const float*)(prep + P.en);
  const frag_t* pk = (const frag_t*)(prep + P.pack);
  if constexpr (sizeof(T) == 2 && NF == 2) {
    // streaming form (one 16-wave workgroup per CU, no workgroup barrier in the batch loop); FRL_VQ_STREAM=0 selects the older kernel,
    // FRL_VQ_STREAM=1 / 2 / 4 the 16-row tiles per wave and batch (A/B hook, read once)
    const int stream_nt = vq_stream_tiles();
    int nt = stream_nt >= 4 ? 4 : (stream_nt >= 2 ? 2 : 1);
    while (nt > 1 && N % (VQS_NW * nt * 16) != 0) nt >>= 1;          // whole batches only: fewer tiles per wave when the row count asks for it
    const int batch = VQS_NW * nt * 16;
    if (resident && stream_nt > 0 && d == 64 && (Kc & 15) == 0 && N % batch == 0 && N < ((int64_t)1 << 32)) {   // whole batches only: no row guards in the kernel
      const int64_t nb = (N + batch - 1) / batch;
      const int grid_s = (int)(nb < 256 ? nb : 256);
      const size_t lds = (size_t)(Kc / 16) * NF * 64 * sizeof(frag_t) + (size_t)Kc * 4 + (size_t)((K + 3) & ~3) * 4 + 64 * 4 +
                         (size_t)VQ_FAST_ROWS * 16 + (size_t)VQS_NW * VQS_CAP * 8 + (size_t)VQS_CAND * 4 +
                         (size_t)VQS_NW * (VQS_CAP + 16) * VQS_ZP * sizeof(T);
      if (lds > 160 * 1024) return frl_fail(-3, "vq_assign: LDS budget exceeded");
      const auto kern = nt == 4 ? vq_assign_stream_kernel<4> : nt == 2 ? vq_assign_stream_kernel<2> : vq_assign_stream_kernel<1>;
      const int rc = vq_launch_assign(kern, grid_s, 64 * VQS_NW, lds, st, (const bf16*)z, en, N, K, Kc, idx, (bf16*)zq, (float*)(ws + L.partial),
                                      (const bf16x8*)pk, (VqCtl*)(prep + P.ctl), counts, stats, (unsigned*)(ws + L.amb), (float*)(ws + L.amb_lim),
                                      stats_copy);
      return rc ? rc : frl_check_launch("vq_assign");
    }
  }
  if (resident) {
    // image | norms | histogram | per-row minima | parked rows | candidates | misc; the statistics fold of the last workgroup reuses the front
    const int nwr = (nw == 8 && NF <= (sizeof(T) == 2 ? 2 : 4)) ? 8 : 4;  // 8 waves x 4 tiles only where the tiles fit the 128-register budget
    const int batch = nwr * VQ_RES_NT * 16;
    const int64_t nb = (N + batch - 1) / batch;
    const int grid_r = (int)(nb < L.grid ? nb : L.grid);
    size_t lds = (size_t)(Kc / 16) * NF * 64 * sizeof(frag_t) + (size_t)Kc * 4 + (size_t)((K + 1) & ~1) * 4 + (size_t)VQ_FAST_ROWS * 12 +
                 (size_t)2 * batch * 4 + (size_t)nwr * 64 * 4 + 32 * 4 + (size_t)VQ_PZ_CAP * d * sizeof(T);
    const size_t fold = (size_t)2 * nwr * 64 * sizeof(double);
    if (lds < fold) lds = fold;
    if (lds > 160 * 1024) return frl_fail(-3, "vq_assign: LDS budget exceeded");
    auto kern = vq_assign_resident_kernel<T, NF, VQ_RES_NT, 4>;
    if constexpr (NF <= (sizeof(T) == 2 ? 2 : 4)) {                  // (the 8-wave form is not instantiated for wider tiles)
      if (nwr == 8) kern = vq_assign_resident_kernel<T, NF, VQ_RES_NT, 8>;
    }
    const int rc = vq_launch_assign(kern, grid_r, 64 * nwr, lds, st, (const T*)z, E, en, N, K, d, Kc, idx, (T*)zq, (float*)(ws + L.partial), pk,
                                    (VqCtl*)(prep + P.ctl), counts, stats, stats_copy);
    return rc ? rc : frl_check_launch("vq_assign");
  }
  // multi-chunk: two half-size chunk buffers (fragments + norms each), so that two workgroups still fit a CU
  const int Kc2 = Kc >= 32 ? Kc / 2 : Kc;
  const size_t lds = 2 * ((size_t)(Kc2 / 16) * NF * 64 * sizeof(frag_t) + (size_t)Kc2 * 4) + 64 + (K <= 2048 ? (size_t)K * 4 : 0);
  if (((Kc2 / 16) * NF * 64 * sizeof(frag_t)) % 1024 != 0 || (Kc2 & 63) != 0) return frl_fail(-3, "vq_assign: chunk is not a whole number of DMA pieces");
  const auto kern = nw == 8 ? vq_assign_kernel<T, NF, 2, 8> : vq_assign_kernel<T, NF, 4, 4>;
  const int rc = vq_launch_assign(kern, L.grid, 64 * nw, lds, st, (const T*)z, E, en, N, K, d, Kc2, idx, (T*)zq, (float*)(ws + L.partial),
                                  (int32_t*)(ws + L.counts_fix), hdr, (int32_t*)(ws + L.amb), (float*)(ws + L.amb_lim), pk);
  if (rc) return rc;
  FRL_LAUNCH_AS("vq_fixup_tile_kernel", (vq_fixup_tile_kernel<T, NF>), dim3(1024), dim3(64 * VQ_FIXT_WAVES), 0, st, (const T*)z, E, en, pk, K, P.kpad, d,
                (const int32_t*)(ws + L.amb), (const float*)(ws + L.amb_lim), hdr, idx, (T*)zq, (int32_t*)(ws + L.counts_fix));
  FRL_LAUNCH(vq_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)(ws + L.partial), L.grid * nw, (const VqHeader*)hdr,
             (const int32_t*)(ws + L.counts_fix), counts, K, N, d, stats, stats_copy);
  return frl_check_launch("vq_assign");
}

static int vq_bwd_chunk(int K, int d) {
  int kc = K;
  while ((size_t)kc * d * 4 > 96 * 1024 && kc > 1) kc = (kc + 1) / 2;
  return kc;
}

// frl_vq_bwd and frl_vq_bwd_scalars: g_cm / g_cb = device scalars, the upstream gradients of L_commit / L_codebook (null: 1), on top of
// the host factors cz_factor / ce_factor (0 for a term that receives no gradient: its coefficient is then formed as c * 0)
extern "C" size_t frl_vq_workspace_bytes(int64_t N, int K, int d);
static int vq_bwd_impl(const void* g_out, const void* z, const void* zq, const float* E, const int32_t* idx, const int32_t* counts,
                       const float* g_cm, const float* g_cb, float cz_factor, float ce_factor, float beta, int64_t N, int K, int d, void* g_z_out,
                       float* g_E_out, float* sums_out, int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (N <= 0 || K <= 0 || d <= 0) return frl_fail(-2, "vq_bwd: empty input");
  if (dtype != FRL_F32 && dtype != FRL_BF16) return frl_fail(-2, "vq_bwd: bad dtype");
  // the widest matrix-core instance covers 128 channels (as the forward); the float32 kernel is generic in d up to one code per LDS chunk
  if (dtype == FRL_BF16 && d > 128) return frl_fail(-2, "vq_bwd: d > 128 unsupported in bf16");
  if (ws_bytes < frl_vq_workspace_bytes(N, K, d)) return frl_fail(-4, "vq_bwd: workspace too small");
  const int Kc = vq_bwd_chunk(K, d);
  const size_t lds = (size_t)Kc * d * 4;
  if (dtype == FRL_F32 && lds > 96 * 1024) return frl_fail(-2, "vq_bwd: one code row exceeds the LDS chunk");
  const int64_t rows = (N + VQ_BWD_WGS - 1) / VQ_BWD_WGS;
  const float cz = beta * 2.f / ((float)N * (float)d) * cz_factor, ce = 2.f / ((float)N * (float)d) * ce_factor;
  float* slab = (float*)ws;
  if (dtype == FRL_F32) {
    auto kern = vq_bwd_kernel<float>;
    if (lds > 64 * 1024) FRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    FRL_LAUNCH_AS("vq_bwd_kernel", kern, dim3(VQ_BWD_WGS), dim3(256), lds, stream, (const float*)g_out, (const float*)z, E, idx, g_cm,
                       cz, N, K, d, Kc, rows, (float*)g_z_out, slab);
    launch_slab_reduce_deferrable<float, CodeEpi>((const float*)slab, VQ_BWD_WGS, (int64_t)K * d, CodeEpi{E, counts, g_cb, ce, d, 0, g_E_out, sums_out}, stream, sums_out == nullptr);
  } else if (dtype == FRL_BF16) {
    const int64_t rows64 = (rows + 63) / 64 * 64;
    if (d <= 32) {
      FRL_LAUNCH((vq_bwd_mfma_kernel<4, 2, 8>), dim3(VQ_BWD_WGS), dim3(512), (size_t)64 * 40 * 2 + 256, stream, (const bf16*)g_out, (const bf16*)z, (const bf16*)zq, E, idx,
                 g_cm, cz, N, K, d, rows64, (bf16*)g_z_out, slab);
    } else if (d <= 64) {
      FRL_LAUNCH((vq_bwd_mfma_kernel<4, 4, 8>), dim3(VQ_BWD_WGS), dim3(512), (size_t)64 * 72 * 2 + 256, stream, (const bf16*)g_out, (const bf16*)z, (const bf16*)zq, E, idx,
                 g_cm, cz, N, K, d, rows64, (bf16*)g_z_out, slab);
    } else {
      FRL_LAUNCH((vq_bwd_mfma_kernel<2, 8, 8>), dim3(VQ_BWD_WGS), dim3(512), (size_t)64 * 136 * 2 + 256, stream, (const bf16*)g_out, (const bf16*)z, (const bf16*)zq, E, idx,
                 g_cm, cz, N, K, d, rows64, (bf16*)g_z_out, slab);
    }
    launch_slab_reduce_deferrable<float, CodeEpi>((const float*)slab, VQ_BWD_WGS, (int64_t)K * d, CodeEpi{E, counts, g_cb, ce, d, 1, g_E_out, sums_out}, stream, sums_out == nullptr);
  } else return frl_fail(-2, "vq_bwd: bad dtype");
  return frl_check_launch("vq_bwd");
}

// the prepared image as a FRL_PACK_VQ job (frl_pack.hpp) of a weight-image cache: see frl_pack_cache_add_vq
template <typename T, int NF>
static int vq_pack_job(int handle, const float* E, int K, int d, int dtype, char* prep) {
  const VqPrep P = vq_prep_layout<T, NF>(0, K, d);
  const int kz = P.kpad > 64 ? P.kpad : 64;
  FrlPackJob j;
  j.W = E; j.dst = prep; j.so = (long long)P.en; j.si = (long long)P.pack; j.kind = FRL_PACK_VQ; j.dtype = dtype; j.NF = NF;
  j.Cout = K; j.Cin = d; j.MB = P.kpad; j.tap_rev = P.npk; j.nfrag = P.npk + kz;
  return frl_pack_cache_add_job(handle, j);
}

extern "C" {

// A/B hook: 16-row tiles per wave and batch of the streaming assignment kernel (1, 2 or 4), 0 = the resident kernel of round 2,
// -1 = back to the default (FRL_VQ_STREAM, else the built-in choice).  Returns the previous setting.  Results are identical either way.
int frl_vq_stream_tiles(int nt) {
  const int prev = g_vq_stream_tiles;
  g_vq_stream_tiles = nt < 0 ? -1 : nt;
  return prev;
}

size_t frl_vq_workspace_bytes(int64_t N, int K, int d) {
  const VqLayout L = vq_layout(N, K, d);
  const size_t bwd = (size_t)VQ_BWD_WGS * K * d * 4 + (size_t)K * d * 4;
  return L.total > bwd ? L.total : bwd;
}

// Dispatch on (dtype, d) to the fragment count NF of the kernels.
#define VQ_DISPATCH(dtype, d, CALL)                                              \
  do {                                                                          \
    if ((dtype) == FRL_F32) {                                                   \
      if ((d) <= 16) return CALL(float, 4);                                     \
      if ((d) <= 32) return CALL(float, 8);                                     \
      if ((d) <= 64) return CALL(float, 16);                                    \
      return CALL(float, 32);                                                   \
    } else if ((dtype) == FRL_BF16) {                                           \
      if ((d) <= 32) return CALL(bf16, 1);                                      \
      if ((d) <= 64) return CALL(bf16, 2);                                      \
      return CALL(bf16, 4);                                                     \
    }                                                                           \
    return frl_fail(-2, "vq: bad dtype");                                       \
  } while (0)

// Prepared codebook: ||e||^2 + the packed MFMA fragment image of -2 e.  It depends on the codebook only, so a caller that keeps the
// codebook fixed over several assignments (inference), or knows when it changes (once per optimizer step), builds it once with
// frl_vq_prepare and hands it to frl_vq_assign_fwd_prepared: the assignment is then ONE kernel launch (plus a memset node).
// N only selects the kernel variant (workgroup shape); pass the row count the assignments will use.
size_t frl_vq_prepared_bytes(int K, int d) { return (K > 0 && d > 0 && d <= 128) ? vq_prep_bytes_max(K) : 0; }

int frl_vq_prepare(const float* E, int64_t N, int K, int d, int dtype, void* prep, size_t prep_bytes, hipStream_t stream) {
  if (N <= 0 || K <= 0 || d <= 0) return frl_fail(-2, "vq_prepare: empty input");
  if (d > 128) return frl_fail(-2, "vq_prepare: d > 128 unsupported");
  if (prep == nullptr || prep_bytes < frl_vq_prepared_bytes(K, d)) return frl_fail(-4, "vq_prepare: buffer too small");
#define VQ_CALL_PREP(T_, NF_) launch_vq_prepare<T_, NF_>(E, N, K, d, (char*)prep, stream)
  VQ_DISPATCH(dtype, d, VQ_CALL_PREP);
#undef VQ_CALL_PREP
}

// The image as a job of a weight-image cache's refresh launch (frl_pack.hpp: FRL_PACK_VQ): frl_pack_cache_refresh(handle) then rewrites
// `prep` from E -- norms, fragments and the zeroed control block, by vq_prepare_kernel's own device functions -- together with the weight
// images, and a caller that refreshes right behind every codebook update needs no frl_vq_prepare launch of its own.  E and prep must
// outlive the cache; no assignment may be in flight on the image when the refresh runs.
int frl_pack_cache_add_vq(int handle, const float* E, int K, int d, int dtype, void* prep, size_t prep_bytes) {
  if (K <= 0 || d <= 0 || d > 128 || E == nullptr) return frl_fail(-2, "pack_cache_add_vq: bad codebook shape");
  if (prep == nullptr || prep_bytes < frl_vq_prepared_bytes(K, d)) return frl_fail(-4, "pack_cache_add_vq: buffer too small");
#define VQ_CALL_JOB(T_, NF_) vq_pack_job<T_, NF_>(handle, E, K, d, dtype, (char*)prep)
  VQ_DISPATCH(dtype, d, VQ_CALL_JOB);
#undef VQ_CALL_JOB
}

// z [N][d] (dtype), E [K][d] f32 master codebook.  Outputs: idx_out [N] int32, zq_out [N][d] (dtype, the
// codebook rows rounded to dtype), stats_out [4] f32 = {sum ||z - z_q||^2, perplexity, #rows re-evaluated in
// float64, mean squared error = sum / (N d)}, counts_out [K] int32 code usage.  In bf16 mode distances are taken to the bf16-rounded codebook.
// prep: NULL, or the image frl_vq_prepare wrote for THIS codebook content, dtype and row count class.  The image carries the kernel's
// arrival counter and histogram accumulator (zeroed by frl_vq_prepare, left zeroed by every call): one call in flight per image.
// stats_copy (optional, [4] f32): the kernel that writes stats_out stores the record there as well.
int frl_vq_assign_fwd_stats2(const void* z, const float* E, void* prep, int64_t N, int K, int d, int32_t* idx_out, void* zq_out,
                             float* stats_out, float* stats_copy, int32_t* counts_out, int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (N <= 0 || K <= 0 || d <= 0) return frl_fail(-2, "vq_assign: empty input");
  if (d > 128) return frl_fail(-2, "vq_assign: d > 128 unsupported");
  if (ws_bytes < frl_vq_workspace_bytes(N, K, d)) return frl_fail(-4, "vq_assign: workspace too small");
#define VQ_CALL_FWD(T_, NF_) launch_vq<T_, NF_>(z, E, (char*)prep, N, K, d, idx_out, zq_out, stats_out, stats_copy, counts_out, (char*)ws, stream)
  VQ_DISPATCH(dtype, d, VQ_CALL_FWD);
#undef VQ_CALL_FWD
}

int frl_vq_assign_fwd_prepared(const void* z, const float* E, void* prep, int64_t N, int K, int d, int32_t* idx_out, void* zq_out,
                               float* stats_out, int32_t* counts_out, int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
  return frl_vq_assign_fwd_stats2(z, E, prep, N, K, d, idx_out, zq_out, stats_out, nullptr, counts_out, dtype, ws, ws_bytes, stream);
}

int frl_vq_assign_fwd(const void* z, const float* E, int64_t N, int K, int d, int32_t* idx_out, void* zq_out,
                      float* stats_out, int32_t* counts_out, int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
  return frl_vq_assign_fwd_prepared(z, E, nullptr, N, K, d, idx_out, zq_out, stats_out, counts_out, dtype, ws, ws_bytes, stream);
}

// g_z = g_out + gscale[0] * beta * 2/(N d) * (z - e_idx);  g_E[k] = gscale[1] * 2/(N d) * (n_k e_k - sum_{idx=k} z)
// gscale: device float[2] = upstream gradients of {L_commit, L_codebook}, may be null (= {1, 1}).
// zq (optional): the forward's z_q rows; when given the bf16 path reads it instead of gathering codebook rows.  g_out may be null (=0).
// g_z / g_E may be null to skip.  sums_out (optional, [K][d] f32) receives the per-code sums of z.
// frl_vq_bwd_scalars: the two upstream gradients as two device scalars, g_commit for L_commit and g_codebook for L_codebook; a null one
// means NO gradient arrives for that term (its factor is cz * 0 or ce * 0, the bits a zero scalar gives) -- not 1 as a null gscale does.
int frl_vq_bwd(const void* g_out, const void* z, const void* zq, const float* E, const int32_t* idx, const int32_t* counts,
               const float* gscale, float beta, int64_t N, int K, int d, void* g_z_out, float* g_E_out,
               float* sums_out, int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
  return vq_bwd_impl(g_out, z, zq, E, idx, counts, gscale, gscale ? gscale + 1 : nullptr, 1.f, 1.f, beta, N, K, d, g_z_out, g_E_out, sums_out, dtype,
                     ws, ws_bytes, stream);
}

int frl_vq_bwd_scalars(const void* g_out, const void* z, const void* zq, const float* E, const int32_t* idx, const int32_t* counts,
                       const float* g_commit, const float* g_codebook, float beta, int64_t N, int K, int d, void* g_z_out, float* g_E_out,
                       float* sums_out, int dtype, void* ws, size_t ws_bytes, hipStream_t stream) {
  return vq_bwd_impl(g_out, z, zq, E, idx, counts, g_commit, g_codebook, g_commit ? 1.f : 0.f, g_codebook ? 1.f : 0.f, beta, N, K, d, g_z_out,
                     g_E_out, sums_out, dtype, ws, ws_bytes, stream);
}

// EMA codebook update from this batch's assignments: counts [K] int32 and per-code sums [K][d] f32
// (both produced by frl_vq_assign_fwd / frl_vq_bwd(sums_out)).  Updates ema_count, ema_sum, E in place.
int frl_vq_ema_update(const float* sums, const int32_t* counts, int K, int d, float decay, float eps, float* ema_count,
                      float* ema_sum, float* E, const float* ok, hipStream_t stream) {
  FRL_LAUNCH(vq_ema_kernel, dim3(1), dim3(256), 0, stream, sums, counts, K, d, decay, eps, ema_count, ema_sum, E, ok);
  return frl_check_launch("vq_ema_update");
}

// E [K][d] float32 codebook (updated in place), window_counts [K] int64, z [N][d] rows of `dtype`, m / v optional AdamW moment
// rows of the codebook, revived: device int32 incremented by the number of re-seeded codes.
int frl_vq_revive_dead_codes(float* E, const int64_t* window_counts, int64_t min_count, const void* z, int64_t N, int K, int d,
                             uint64_t seed, float* m, float* v, int32_t* revived, int dtype, hipStream_t stream) {
  if (K <= 0 || d <= 0) return frl_fail(-2, "vq_revive_dead_codes: bad codebook shape");
  if (N <= 0) return frl_fail(-2, "vq_revive_dead_codes: no candidate rows");
  if (dtype == FRL_F32)
    FRL_LAUNCH((vq_revive_kernel<float>), dim3(K), dim3(64), 0, stream, E, (const long long*)window_counts, (long long)min_count,
               (const float*)z, (long long)N, K, d, (unsigned long long)seed, m, v, revived);
  else if (dtype == FRL_BF16)
    FRL_LAUNCH((vq_revive_kernel<bf16>), dim3(K), dim3(64), 0, stream, E, (const long long*)window_counts, (long long)min_count,
               (const bf16*)z, (long long)N, K, d, (unsigned long long)seed, m, v, revived);
  else return frl_fail(-2, "vq_revive_dead_codes: dtype must be FRL_F32 or FRL_BF16");
  return frl_check_launch("vq_revive_dead_codes");
}

}  // extern "C"
