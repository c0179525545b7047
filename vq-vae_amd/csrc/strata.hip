// EVT-stratified diagnostics (the reference's frl/training/compare_gmm_evt.py, phase_evt_diagnostics.py and ysfc_evt_histograms.py):
// every valid pixel of a split is keyed by its EVT code, and counts or first and second moments are accumulated per key.
//
// An observation is (b, t, p) as in probe.hip.  Its key comes from codes [B][P] (int32 or float32), looked up in vocab [G] (int32,
// strictly increasing), which every workgroup keeps in LDS and searches by bisection.  A code is valid when it is finite and > 0 (the
// reference's np.isfinite(evt_grid) & (evt_grid > 0)); a valid float code is truncated as astype(np.int32) does.  An observation with
// an invalid code is skipped, one with a valid code that vocab does not hold is skipped and counted in `unmatched`.
//
// frl_strata_contingency: table [R][G] (int64) += 1 at (rows[b][t][p], column of codes[b][p]).  One thread per observation in a
// grid-stride loop.  Up to 8192 cells a workgroup counts into an int32 table in LDS (LDS integer atomics) and adds its non-zero cells
// to the table with one 64-bit integer atomic each; beyond that every observation is one 64-bit integer atomic in memory.  Integer adds
// commute: the table is exact whatever the order.
//
// frl_strata_moments: per group of a window [g0, g0 + Gc) of the vocabulary and per column, count, S1 = sum y, S2 = sum y^2 of
// y = x - pivot (and SW, the sum of the per-pixel variances over t, in the temporal mode): the staged-tile scheme of frl_moments.hpp over
// tiles of 64 consecutive pixels, the product being onehot^T [y | y^2 | w] (exact float32, an fmaf chain in row order; the one-hot operand
// is formed in registers from the 64 group indices of the tile, y^2 from y).  A tile whose 64 mask bytes are zero, or none of whose pixels
// falls into the window, is skipped before anything of X is read.  The slabs are added in the order of moment_slab_sum.  Counts are
// integers: an LDS table per workgroup, one 64-bit integer atomic per group.  No float atomics: two runs give the same bits.
#include "strata_keys.hpp"

#define STRATA_MAX_R 4096
#define STRATA_MAX_CELLS (1 << 24)
#define STRATA_LDS_CELLS 8192
#define STRATA_MAX_GC 128
#define STRATA_MAX_D 128
#define STRATA_MAX_GD 8192

namespace {

struct StrataMom {
  StrataKeys k;
  const float* X;
  const float* pivot;
  int D, DB, NQ, g0, Gc, ys, PT, ntiles, vec;
};

struct StrataDims {
  int DB, GB, NQ, nblk, ys, slabF;
  size_t lds;
};

StrataDims strata_dims(int Gc, int D, int temporal, int G) {
  StrataDims g;
  g.DB = (D + 15) / 16;
  g.GB = (Gc + 15) / 16;
  g.NQ = temporal ? 3 : 2;
  g.nblk = g.GB * g.NQ * g.DB;
  const int ys = g.ys = frl_tile_stride(16 * g.DB);
  g.slabF = g.nblk * 256;
  // y [64][ys] | w [64][ys] (temporal) | pivot [16 DB] | vocab [G] | group of each row [64] | counts [Gc]
  g.lds = sizeof(float) * ((size_t)MOMENT_ROWS * ys * (temporal ? 2 : 1) + 16 * g.DB) + sizeof(int) * ((size_t)G + MOMENT_ROWS + Gc);
  return g;
}

int strata_mom_cap(const StrataDims& g) { return g.nblk <= 16 ? 1024 : g.nblk <= 64 ? 512 : 256; }

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------------
// the contingency table
// ---------------------------------------------------------------------------------------------------------------------------------
template <bool LDS_TAB>
__global__ __launch_bounds__(256) void strata_table_kernel(StrataKeys q, const int* __restrict__ rows, int Tr, int R,
                                                           unsigned long long* __restrict__ table, unsigned long long* __restrict__ unmatched,
                                                           unsigned long long* __restrict__ rejected) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* vl = reinterpret_cast<int*>(smem);                                        // [G]
  int* tab = vl + q.G;                                                           // [R G] where it fits
  const int tid = threadIdx.x, lane = tid & 63, cells = R * q.G;
  for (int i = tid; i < q.G; i += 256) vl[i] = q.vocab[i];
  if (LDS_TAB)
    for (int i = tid; i < cells; i += 256) tab[i] = 0;
  __syncthreads();
  const unsigned N = (unsigned)q.B * (unsigned)q.T * (unsigned)q.P, stride = gridDim.x * 256u;   // N < 2^31, stride <= 2^20
  int unm = 0, rej = 0;
  for (unsigned i = blockIdx.x * 256u + tid; i < N; i += stride) {
    const unsigned bt = i / (unsigned)q.P, p = i - bt * (unsigned)q.P, b = bt / (unsigned)q.T, t = bt - b * (unsigned)q.T;
    if (q.mask && !q.mask[((size_t)b * q.Tm + (q.Tm > 1 ? t : 0u)) * q.P + p]) continue;
    int code;
    if (!strata_code(q, (size_t)b * q.P + p, code)) continue;
    const int g = strata_find(vl, q.G, code);
    if (g < 0) {
      ++unm;
      continue;
    }
    const int r = rows[((size_t)b * Tr + (Tr > 1 ? t : 0u)) * q.P + p];
    if (r < 0 || r >= R) {
      ++rej;
      continue;
    }
    if (LDS_TAB) atomicAdd(&tab[r * q.G + g], 1);
    else atomicAdd(&table[(size_t)r * q.G + g], 1ull);
  }
  unm = wave_sum_i(unm);
  rej = wave_sum_i(rej);
  if (lane == 0 && unm) atomicAdd(unmatched, (unsigned long long)unm);
  if (lane == 0 && rej) atomicAdd(rejected, (unsigned long long)rej);
  if (LDS_TAB) {
    __syncthreads();
    for (int i = tid; i < cells; i += 256) {
      const int v = tab[i];
      if (v) atomicAdd(&table[i], (unsigned long long)v);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// grouped moments.  NBM: 16 x 16 blocks per wave; block (gb, kind, db) = 16 groups x 16 columns of y (kind 0), y^2 (1) or w (2)
// ---------------------------------------------------------------------------------------------------------------------------------
// stages V consecutive columns of one row: y = x - pivot, or in the temporal mode the mean over t of y (summed in t order) and the
// population variance over t
template <int V, bool TEMPORAL>
__device__ __forceinline__ void strata_stage_row(const StrataMom& q, const float* __restrict__ px, const float* pv, float* yo, float* wo) {
  float y[V];
  if (!TEMPORAL) {
    if (V == 4) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(px);
#pragma unroll
      for (int j = 0; j < V; ++j) y[j] = x[j] - pv[j];
    } else {
      y[0] = px[0] - pv[0];
    }
  } else {
    const size_t st = (size_t)q.k.P * q.D;
    const int T = q.k.T;
    const float fT = (float)T;
    float s[V], w[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = w[j] = 0.f;
    for (int t = 0; t < T; ++t) {
      if (V == 4) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(px + t * st);
#pragma unroll
        for (int j = 0; j < V; ++j) s[j] += x[j] - pv[j];
      } else {
        s[0] += px[t * st] - pv[0];
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) y[j] = s[j] / fT;
    for (int t = 0; t < T; ++t) {                                                // the second read of the tile comes from the cache
      if (V == 4) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(px + t * st);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float d = (x[j] - pv[j]) - y[j];
          w[j] = fmaf(d, d, w[j]);
        }
      } else {
        const float d = (px[t * st] - pv[0]) - y[0];
        w[0] = fmaf(d, d, w[0]);
      }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) wo[j] = w[j] / fT;
  }
#pragma unroll
  for (int j = 0; j < V; ++j) yo[j] = y[j];
}

template <int NBM, bool TEMPORAL>
__global__ __launch_bounds__(256, (NBM <= 4 ? 4 : NBM <= 8 ? 2 : 1)) void strata_mom_kernel(StrataMom q, float* __restrict__ slabs,
                                                                                         unsigned long long* __restrict__ count,
                                                                                         unsigned long long* __restrict__ unmatched) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lg = lane >> 4;
  const int D = q.D, ys = q.ys, DB = q.DB, NQ = q.NQ, Gc = q.Gc, G = q.k.G, P = q.k.P, T = q.k.T;
  const int nblk = ((Gc + 15) >> 4) * NQ * DB, tsz = MOMENT_ROWS * ys;
  float* vt = reinterpret_cast<float*>(smem);                                    // [64][ys]: y
  float* wt = vt + (TEMPORAL ? tsz : 0);                                         // [64][ys]: w
  float* piv = wt + tsz;                                                         // [16 DB]
  int* vl = reinterpret_cast<int*>(piv + 16 * DB);                               // [G]
  int* gl = vl + G;                                                              // [64]: the tile's group in the window, or -1
  int* cl = gl + MOMENT_ROWS;                                                    // [Gc]
  for (int d = tid; d < 16 * DB; d += 256) piv[d] = d < D ? q.pivot[d] : 0.f;
  for (int i = tid; i < (TEMPORAL ? 2 : 1) * tsz; i += 256) vt[i] = 0.f;         // the padding columns stay zero
  for (int i = tid; i < G; i += 256) vl[i] = q.k.vocab[i];
  for (int i = tid; i < Gc; i += 256) cl[i] = 0;
  __syncthreads();

  f32x4 acc[NBM];
  int gsel[NBM], boff[NBM], kind[NBM];
#pragma unroll
  for (int i = 0; i < NBM; ++i) {
    acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int blk = wave + 4 * i < nblk ? wave + 4 * i : 0;
    const int db = blk % DB, gk = blk / DB;
    kind[i] = __builtin_amdgcn_readfirstlane(gk % NQ);
    gsel[i] = (gk / NQ) * 16 + lr;
    boff[i] = lg * ys + db * 16 + lr;
  }
  long long unm = 0;

  for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
    int b, t, p0;
    moment_tile(tile, q.PT, TEMPORAL ? 1 : T, b, t, p0);                         // the temporal mode walks (b, p0): t = 0
    bool on = lane < moment_tile_rows(P, p0);
    if (on && q.k.mask) on = q.k.mask[((size_t)b * q.k.Tm + (q.k.Tm > 1 ? t : 0)) * P + p0 + lane] != 0;
    if (__ballot(on) == 0ull) continue;                                          // uniform: every wave sees the same 64 mask bytes
    int gi = -1, code = 0;
    if (on && strata_code(q.k, (size_t)b * P + p0 + lane, code)) {
      const int g = strata_find(vl, G, code);
      if (g < 0) gi = -2;
      else if (g >= q.g0 && g < q.g0 + Gc) gi = g - q.g0;
    }
    const unsigned long long rows = __ballot(gi >= 0);
    if (wave == 0) {
      unm += __popcll(__ballot(gi == -2));
      if (gi >= 0) atomicAdd(&cl[gi], 1);
    }
    if (rows == 0ull) continue;                                                  // uniform
    __syncthreads();                                                             // the previous tile is consumed
    if (wave == 0) gl[lane] = gi >= 0 ? gi : -1;
    const float* base = q.X + ((size_t)((int64_t)b * T + t) * P + p0) * D;
    if (q.vec) {
      const int q4 = D >> 2, n4 = MOMENT_ROWS * q4;
      for (int e = tid; e < n4; e += 256) {
        const int row = e / q4, c = (e - row * q4) * 4;
        float y[4] = {0.f, 0.f, 0.f, 0.f}, w[4] = {0.f, 0.f, 0.f, 0.f};
        if ((rows >> row) & 1ull) strata_stage_row<4, TEMPORAL>(q, base + (size_t)row * D + c, piv + c, y, w);
        *reinterpret_cast<f32x4*>(vt + row * ys + c) = f32x4{y[0], y[1], y[2], y[3]};
        if (TEMPORAL) *reinterpret_cast<f32x4*>(wt + row * ys + c) = f32x4{w[0], w[1], w[2], w[3]};
      }
    } else {
      const int n = MOMENT_ROWS * D;
      for (int e = tid; e < n; e += 256) {
        const int row = e / D, c = e - row * D;
        float y[1] = {0.f}, w[1] = {0.f};
        if ((rows >> row) & 1ull) strata_stage_row<1, TEMPORAL>(q, base + (size_t)row * D + c, piv + c, y, w);
        vt[row * ys + c] = y[0];
        if (TEMPORAL) wt[row * ys + c] = w[0];
      }
    }
    __syncthreads();
    int gq[MOMENT_ROWS / 4];
#pragma unroll
    for (int st = 0; st < MOMENT_ROWS / 4; ++st) gq[st] = gl[4 * st + lg];
#pragma unroll
    for (int i = 0; i < NBM; ++i) {
      if (wave + 4 * i < nblk) {
        const float* bp = (kind[i] == 2 ? wt : vt) + boff[i];
        const bool sq = kind[i] == 1;
#pragma unroll
        for (int st = 0; st < MOMENT_ROWS / 4; ++st) {
          float bv = bp[4 * st * ys];
          if (sq) bv *= bv;
          acc[i] = mfma16(gq[st] == gsel[i] ? 1.f : 0.f, bv, acc[i]);
        }
      }
    }
  }
  moment_store_slab<NBM>(slabs + (size_t)blockIdx.x * nblk * 256, acc, wave, lane, nblk);
  __syncthreads();
  for (int g = tid; g < Gc; g += 256) {
    const int v = cl[g];
    if (v) atomicAdd(&count[q.g0 + g], (unsigned long long)v);
  }
  if (tid == 0 && unmatched && unm) atomicAdd(unmatched, (unsigned long long)unm);
}

// the slabs added in double (moment_slab_sum), 64 elements per workgroup, into S1 / S2 / SW [G][D]
__global__ __launch_bounds__(256) void strata_mom_reduce_kernel(const float* __restrict__ slabs, int nslab, int slabF, int DB, int NQ, int D, int g0,
                                                                int Gc, double* __restrict__ S1, double* __restrict__ S2, double* __restrict__ SW) {
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);
  const double sum = moment_slab_sum(slabs, nslab, slabF, e, true);
  if (threadIdx.x < 64) {
    int blk, row, col;
    moment_frag_decode(e, blk, row, col);
    const int db = blk % DB, gk = blk / DB, kind = gk % NQ, gb = gk / NQ;
    const int g = gb * 16 + row, c = db * 16 + col;
    if (g < Gc && c < D) {
      double* out = kind == 0 ? S1 : kind == 1 ? S2 : SW;
      out[(size_t)(g0 + g) * D + c] += sum;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

template <bool TEMPORAL>
int strata_mom_launch(const StrataMom& q, const StrataDims& g, int grid, float* slabs, unsigned long long* count, unsigned long long* unmatched,
                      hipStream_t stream) {
  const int NB = (g.nblk + 3) / 4;
#define STRATA_GO(N)                                                                                                                       \
  do {                                                                                                                                     \
    auto kern = strata_mom_kernel<N, TEMPORAL>;                                                                                            \
    if (g.lds > 64 * 1024) FRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));        \
    FRL_LAUNCH_AS("strata_mom_kernel", kern, dim3((unsigned)grid), dim3(256), g.lds, stream, q, slabs, count, unmatched);                  \
  } while (0)
  if (NB <= 2) STRATA_GO(2);
  else if (NB <= 8) STRATA_GO(8);
  else if (NB <= 16) STRATA_GO(16);
  else STRATA_GO(32);
#undef STRATA_GO
  return 0;
}

}  // namespace

extern "C" {

// See include/frl_hip.h.
size_t frl_strata_workspace_bytes(int Gc, int D, int temporal, int workgroups) {
  if (Gc < 1 || Gc > STRATA_MAX_GC || D < 1 || D > STRATA_MAX_D || Gc * D > STRATA_MAX_GD || !frl_wg_in_range(workgroups)) return 0;
  // enough for every window of at most Gc groups: a shorter window has smaller slabs but may run more workgroups
  size_t most = 0;
  for (int gc = 1; gc <= Gc; ++gc) {
    const StrataDims g = strata_dims(gc, D, temporal, 1);
    const size_t wg = workgroups > 0 ? workgroups : strata_mom_cap(g);
    most = wg * g.slabF > most ? wg * g.slabF : most;
  }
  return sizeof(float) * most;
}

int frl_strata_contingency(const int32_t* rows, int Tr, const void* codes, int codes_float, const unsigned char* mask, int Tm, const int32_t* vocab,
                           int G, int B, int T, int64_t P, int R, int workgroups, int64_t* table, int64_t* unmatched, int64_t* rejected,
                           hipStream_t stream) {
  StrataKeys k;
  if (int rc = strata_check_keys("strata_contingency", codes, codes_float, mask, Tm, vocab, G, B, T, P, workgroups, k)) return rc;
  if (!rows || !table || !unmatched || !rejected) return frl_fail(-2, "strata_contingency: null pointer");
  if (Tr != 1 && Tr != T) return frl_fail(-2, "strata_contingency: needs Tr 1 or T");
  if (R < 1 || R > STRATA_MAX_R || (int64_t)R * G > STRATA_MAX_CELLS) return frl_fail(-2, "strata_contingency: needs 1 <= R <= 4096 and R * G <= 2^24 cells");
  const int64_t N = (int64_t)B * T * P;
  const bool in_lds = R * G <= STRATA_LDS_CELLS;
  const int grid = workgroups > 0 ? workgroups : (int)frl_grid(N, 256 * 8, in_lds ? 512 : 2048);
  const size_t lds = sizeof(int) * ((size_t)G + (in_lds ? (size_t)R * G : 0));
  unsigned long long* tb = reinterpret_cast<unsigned long long*>(table);
  unsigned long long* um = reinterpret_cast<unsigned long long*>(unmatched);
  unsigned long long* rj = reinterpret_cast<unsigned long long*>(rejected);
  if (in_lds) FRL_LAUNCH(strata_table_kernel<true>, dim3((unsigned)grid), dim3(256), lds, stream, k, (const int*)rows, Tr, R, tb, um, rj);
  else FRL_LAUNCH(strata_table_kernel<false>, dim3((unsigned)grid), dim3(256), lds, stream, k, (const int*)rows, Tr, R, tb, um, rj);
  return frl_check_launch("strata_contingency");
}

int frl_strata_moments(const float* X, const void* codes, int codes_float, const unsigned char* mask, int Tm, const int32_t* vocab, int G, int g0,
                       int Gc, int B, int T, int64_t P, int D, const float* pivot, int temporal, int workgroups, int64_t* count, double* S1,
                       double* S2, double* SW, int64_t* unmatched, void* ws, size_t ws_bytes, hipStream_t stream) {
  StrataMom q;
  if (int rc = strata_check_keys("strata_moments", codes, codes_float, mask, temporal ? 1 : Tm, vocab, G, B, T, P, workgroups, q.k)) return rc;
  if (!X || !pivot || !count || !S1 || !S2 || (temporal && !SW)) return frl_fail(-2, "strata_moments: null pointer");
  if (temporal != 0 && temporal != 1) return frl_fail(-2, "strata_moments: temporal must be 0 or 1");
  if (temporal && mask && Tm != 1) return frl_fail(-2, "strata_moments: the temporal mode takes a mask [B][1][P]");
  if (D < 1 || D > STRATA_MAX_D || Gc < 1 || Gc > STRATA_MAX_GC || Gc * D > STRATA_MAX_GD)
    return frl_fail(-2, "strata_moments: needs 1 <= D <= 128, 1 <= Gc <= 128 and Gc * D <= 8192");
  if (g0 < 0 || g0 + Gc > G) return frl_fail(-2, "strata_moments: the window [g0, g0 + Gc) must lie in the vocabulary");
  const StrataDims g = strata_dims(Gc, D, temporal, G);
  if (g.nblk > 128) return frl_fail(-2, "strata_moments: more than 128 blocks of 16 x 16");
  q.X = X; q.pivot = pivot;
  q.D = D; q.DB = g.DB; q.NQ = g.NQ; q.g0 = g0; q.Gc = Gc; q.ys = g.ys;
  q.ntiles = frl_moment_tiles(B, temporal ? 1 : T, P, q.PT);
  q.vec = (D & 3) == 0 && ((uintptr_t)X & 15) == 0;
  const int cap = workgroups > 0 ? workgroups : strata_mom_cap(g);
  const int grid = workgroups > 0 ? workgroups : (q.ntiles < cap ? q.ntiles : cap);
  const size_t need = sizeof(float) * (size_t)grid * g.slabF;
  if (int rc = frl_check_workspace("strata_moments", ws, ws_bytes, need)) return rc;
  float* slabs = (float*)ws;
  unsigned long long* cn = reinterpret_cast<unsigned long long*>(count);
  unsigned long long* um = reinterpret_cast<unsigned long long*>(unmatched);
  if (int rc = temporal ? strata_mom_launch<true>(q, g, grid, slabs, cn, um, stream) : strata_mom_launch<false>(q, g, grid, slabs, cn, um, stream)) return rc;
  FRL_LAUNCH(strata_mom_reduce_kernel, dim3((unsigned)(g.slabF / 64)), dim3(256), 0, stream, (const float*)slabs, grid, g.slabF, g.DB, g.NQ, D, g0, Gc,
             S1, S2, SW);
  return frl_check_launch("strata_moments");
}

}  // extern "C"
