// Exact grouped quantiles by radix select (the per-bin quartiles of the reference's frl/training/phase_recovery_curves.py, the medians of
// ysfc_evt_histograms.py, compute_stats of representation/step.py and the robust statistics of data/stats), over every observation.
//
// Key.  quant_key(x) is a uint32 whose unsigned order is the order of x: -0.0 is folded into +0.0, a negative float has all its bits
// flipped, any other its sign bit set; every NaN maps to the largest key.  quant_value undoes it.
//
// Select.  The k-th smallest key of a (cell, column) is found in four passes of 8-bit digits from the most significant one.  A pass counts
// the digit of every key that matches the prefix found so far into a histogram of 256 bins; quant_pick_kernel then walks the 256 bins, picks
// the digit that holds the rank and takes the bins below it off the rank.  Pass 1 has one histogram per slot (cell, column) and every
// element takes part; its totals give the count of every cell, from which the 2 Q ranks of a cell (k and min(k + 1, n - 1) of
// v = (n - 1) q in double) are formed on the device.  Passes 2 to 4 have one histogram per (cell, column, rank): ranks that share pass 1
// may part afterwards.
//
// quant_hist_lds_kernel counts into a window of QUANT_WIN slots in LDS and adds the window's non-zero bins to memory once per workgroup;
// blockIdx.y walks the windows of a longer slot list, blockIdx.x the elements in a grid-stride loop.  Pass 1 always runs so.  A later pass
// runs so up to QUANT_LDS_WINDOWS windows; beyond that few elements match a prefix and quant_hist_direct_kernel adds them to memory in one
// sweep, the lanes of a wave that share a bin adding once.  All counts are 32-bit integer atomics (fewer than 2^31 elements): the
// histograms, hence the order statistics, are exact and do not depend on the order of the elements or of the workgroups.  No float atomics.
//
// Elements are either records (cells [n], keys [D][capacity], n = min(*cursor, capacity) read on the device: what quant_append_kernel
// wrote) or rows of X [N][D] keyed on the fly, all in cell 0 (mask [N] optional); D = 1 rows are read four at a time.
// quant_append_kernel keys observations as strata_table_kernel does, skips rows with a value that is not finite, and takes the slots of a
// workgroup's records (1024 observations per step) with one add to the cursor.
#include "strata_keys.hpp"

#define QUANT_MAX_D 16
#define QUANT_MAX_Q 8
#define QUANT_MAX_C 65535
#define QUANT_MAX_SLOTS (1 << 23)
#define QUANT_BINS 256
#define QUANT_WIN 48                                                             // slots of 256 bins a workgroup counts in LDS: 48 KiB
#define QUANT_LDS_WINDOWS 4                                                      // passes 2 to 4 count in LDS up to this many windows

namespace {

struct QuantSrc {
  const int* cells;
  const unsigned* keys;
  const unsigned long long* cursor;
  const float* X;
  const unsigned char* mask;
  unsigned cap, N;
  int D, C;
};

struct QuantProbs {
  double p[QUANT_MAX_Q];
};

}  // namespace

__device__ __forceinline__ unsigned quant_key(float x) {
  unsigned u = __float_as_uint(x);
  if (x != x) return 0xffffffffu;
  if ((u << 1) == 0u) u = 0u;
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ float quant_value(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

__device__ __forceinline__ unsigned quant_n(const QuantSrc& s) {
  if (s.X) return s.N;
  const unsigned long long c = *s.cursor;
  return c < s.cap ? (unsigned)c : s.cap;
}

// the cell of element i, or -1 where it does not count (a masked row; a record of a cell beyond C)
__device__ __forceinline__ int quant_cell(const QuantSrc& s, unsigned i) {
  if (s.X) return s.mask && !s.mask[i] ? -1 : 0;
  const int c = s.cells[i];
  return (unsigned)c < (unsigned)s.C ? c : -1;
}

__device__ __forceinline__ unsigned quant_load_key(const QuantSrc& s, unsigned i, int d) {
  return s.X ? quant_key(s.X[(size_t)i * s.D + d]) : s.keys[(size_t)d * s.cap + i];
}

// the bits above the digit at `shift`
__device__ __forceinline__ unsigned quant_himask(int shift) { return shift == 24 ? 0u : ~0u << (shift + 8); }

// ---------------------------------------------------------------------------------------------------------------------------------
// histograms
// ---------------------------------------------------------------------------------------------------------------------------------
// element i of cell c into the window [w0, w1) of slots: slot (c D + d) J + j counts the digit where the key matches pl[slot - w0]
__device__ __forceinline__ void quant_count_elem(const QuantSrc& s, unsigned i, unsigned c, int J, unsigned w0, unsigned w1, int shift, unsigned himask,
                                                 const unsigned* pl, unsigned* hl) {
  const unsigned DJ = (unsigned)(s.D * J), s0 = c * DJ;
  if (s0 + DJ <= w0 || s0 >= w1) return;
  for (int d = 0; d < s.D; ++d) {
    const unsigned a = s0 + (unsigned)(d * J);
    if (a + J <= w0 || a >= w1) continue;
    const unsigned key = quant_load_key(s, i, d);
    for (int j = 0; j < J; ++j) {
      const unsigned sl = a + j;
      if (sl < w0 || sl >= w1) continue;
      if ((key & himask) == pl[sl - w0]) atomicAdd(&hl[(sl - w0) * QUANT_BINS + ((key >> shift) & 255u)], 1u);
    }
  }
}

// V = 4: rows of X [N][1] (16-byte aligned, mask 4-byte aligned), four per thread and step; V = 1: anything
template <int V>
__global__ __launch_bounds__(256) void quant_hist_lds_kernel(QuantSrc s, int J, int shift, unsigned nslots, int win, const unsigned* __restrict__ prefix,
                                                             unsigned* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned* hl = reinterpret_cast<unsigned*>(smem);                              // [win][256]
  unsigned* pl = hl + win * QUANT_BINS;                                          // [win]: the prefix of every slot of the window
  const int tid = threadIdx.x;
  const unsigned n = quant_n(s), himask = quant_himask(shift), ngroups = (n + V - 1) / V, stride = gridDim.x * 256u;
  const unsigned W = (nslots + win - 1) / win;
  for (unsigned w = blockIdx.y; w < W; w += gridDim.y) {
    const unsigned w0 = w * win, w1 = w0 + win < nslots ? w0 + win : nslots, nb = (w1 - w0) * QUANT_BINS;
    for (unsigned i = tid; i < nb; i += 256) hl[i] = 0u;
    for (unsigned i = tid; i < w1 - w0; i += 256) pl[i] = prefix[w0 + i] & himask;
    __syncthreads();
    for (unsigned g = blockIdx.x * 256u + tid; g < ngroups; g += stride) {
      const unsigned i0 = g * V;
      if (V == 4 && i0 + 4 <= n) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(s.X + i0);
        const unsigned m = s.mask ? *reinterpret_cast<const unsigned*>(s.mask + i0) : 0x01010101u;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (!((m >> (8 * e)) & 255u)) continue;
          const unsigned key = quant_key(x[e]);
          for (int j = 0; j < J; ++j)                                            // C = 1, D = 1: slot j; the host keeps this path to one window
            if ((key & himask) == pl[j]) atomicAdd(&hl[j * QUANT_BINS + ((key >> shift) & 255u)], 1u);
        }
      } else {
        for (int e = 0; e < V; ++e) {
          const unsigned i = i0 + e;
          if (i >= n) break;
          const int c = quant_cell(s, i);
          if (c >= 0) quant_count_elem(s, i, (unsigned)c, J, w0, w1, shift, himask, pl, hl);
        }
      }
    }
    __syncthreads();
    for (unsigned i = tid; i < nb; i += 256) {
      const unsigned v = hl[i];
      if (v) atomicAdd(&hist[(size_t)w0 * QUANT_BINS + i], v);
    }
    __syncthreads();
  }
}

// passes 2 to 4 over many slots: one sweep, the matching elements added to memory; lanes of a wave that share a bin add once
__global__ __launch_bounds__(256) void quant_hist_direct_kernel(QuantSrc s, int J, int shift, const unsigned* __restrict__ prefix,
                                                                unsigned* __restrict__ hist) {
  const int tid = threadIdx.x, lane = tid & 63;
  const unsigned n = quant_n(s), himask = quant_himask(shift), stride = gridDim.x * 256u;
  for (unsigned i0 = blockIdx.x * 256u + (tid & ~63); i0 < n; i0 += stride) {     // uniform in the wave
    const unsigned i = i0 + lane;
    const int c = i < n ? quant_cell(s, i) : -1;
    for (int d = 0; d < s.D; ++d) {
      const unsigned key = c >= 0 ? quant_load_key(s, i, d) : 0u;
      for (int j = 0; j < J; ++j) {
        const unsigned sj = c >= 0 ? ((unsigned)c * s.D + d) * J + j : 0u;
        const bool hit = c >= 0 && (key & himask) == prefix[sj];
        const unsigned idx = sj * QUANT_BINS + ((key >> shift) & 255u);
        unsigned long long todo = __ballot(hit);
        while (todo) {                                                           // uniform in the wave
          const int leader = __ffsll((long long)todo) - 1;
          const unsigned lidx = __shfl(idx, leader, 64);
          const unsigned long long same = __ballot(hit && idx == lidx);
          if (lane == leader) atomicAdd(&hist[lidx], (unsigned)__popcll(same));
          todo &= ~same;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// counts, ranks and the digit of a rank
// ---------------------------------------------------------------------------------------------------------------------------------
// after pass 1: count [C] from the histogram of column 0, frac [C][Q]
__global__ __launch_bounds__(256) void quant_count_kernel(const unsigned* __restrict__ hist, int C, int D, int Q, QuantProbs pr, long long* __restrict__ count,
                                                          double* __restrict__ frac) {
#pragma clang fp contract(off)                                                    // v - floor(v) of the rounded product, not an fma
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const unsigned* row = hist + (size_t)c * D * QUANT_BINS;
  long long n = 0;
  for (int b = 0; b < QUANT_BINS; ++b) n += row[b];
  count[c] = n;
  for (int q = 0; q < Q; ++q) {
    const double v = (double)(n - 1) * pr.p[q];
    frac[(size_t)c * Q + q] = n > 0 ? v - floor(v) : 0.0;
  }
}

// one thread per (cell, column, rank j = 2 q + side): the bin of this pass's histogram that holds the rank; the prefix gains the digit,
// the rank loses the bins below it; after the last pass the prefix is the key of the order statistic
__global__ __launch_bounds__(256) void quant_pick_kernel(const unsigned* __restrict__ hist, unsigned* __restrict__ prefix, unsigned* __restrict__ rank,
                                                         const long long* __restrict__ count, QuantProbs pr, int C, int D, int Q, int shift,
                                                         float* __restrict__ lo, float* __restrict__ hi) {
  const unsigned sj = blockIdx.x * 256u + threadIdx.x, J = 2u * Q;
  if (sj >= (unsigned)C * D * J) return;
  const unsigned j = sj % J, sl = sj / J, c = sl / D, q = j >> 1;
  float* out = (j & 1u ? hi : lo) + (size_t)sl * Q + q;
  const long long n = count[c];
  if (n == 0) {
    if (shift == 0) *out = __uint_as_float(0x7fc00000u);
    return;
  }
  const bool first = shift == 24;
  unsigned r;
  if (first) {
    const long long k = (long long)floor((double)(n - 1) * pr.p[q]);
    r = (unsigned)((j & 1u) && k + 1 < n ? k + 1 : k);
  } else {
    r = rank[sj];
  }
  const unsigned* row = hist + (size_t)(first ? sl : sj) * QUANT_BINS;
  unsigned cum = 0, bin = QUANT_BINS - 1;
  for (unsigned b = 0; b < QUANT_BINS; ++b) {
    const unsigned h = row[b];
    if (r < cum + h) {
      bin = b;
      break;
    }
    cum += h;
  }
  const unsigned pfx = (first ? 0u : prefix[sj]) | (bin << shift);
  prefix[sj] = pfx;
  rank[sj] = r - cum;
  if (shift == 0) *out = quant_value(pfx);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the streaming front end
// ---------------------------------------------------------------------------------------------------------------------------------
#define QUANT_APPEND_ITEMS 4                                                     // observations per lane and cursor add: 1024 per workgroup

// the tests of observation i in order -> whether it survives, and its cell; counts what is skipped.  VX = 4: D a multiple of 4 and X
// 16-byte aligned
template <int VX>
__device__ __forceinline__ bool quant_observe(const StrataKeys& q, const int* vl, const int* __restrict__ rows, int Tr, int R, const float* __restrict__ X,
                                              int D, unsigned i, int& cell, int& unm, int& rej, int& nf) {
  const unsigned bt = i / (unsigned)q.P, p = i - bt * (unsigned)q.P, b = bt / (unsigned)q.T, t = bt - b * (unsigned)q.T;
  if (q.mask && !q.mask[((size_t)b * q.Tm + (q.Tm > 1 ? t : 0u)) * q.P + p]) return false;
  int code, r = 0;
  if (!strata_code(q, (size_t)b * q.P + p, code)) return false;
  const int g = strata_find(vl, q.G, code);
  if (g < 0) {
    ++unm;
    return false;
  }
  if (rows) {
    r = rows[((size_t)b * Tr + (Tr > 1 ? t : 0u)) * q.P + p];
    if (r < 0 || r >= R) {
      ++rej;
      return false;
    }
  }
  const float* px = X + (size_t)i * D;
  bool fin = true;
  for (int d = 0; d < D; d += VX) {
    if (VX == 4) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(px + d);
#pragma unroll
      for (int e = 0; e < 4; ++e) fin = fin && (__float_as_uint(x[e]) & 0x7fffffffu) < 0x7f800000u;
    } else {
      fin = fin && (__float_as_uint(px[d]) & 0x7fffffffu) < 0x7f800000u;
    }
  }
  if (!fin) {
    ++nf;
    return false;
  }
  cell = r * q.G + g;
  return true;
}

// A workgroup takes 1024 consecutive observations per step, four per lane: the waves count their survivors, thread 0 takes the slots of
// all of them with one add to the cursor, and every survivor stores its record at the base of its wave plus its place among the
// survivors of its wave.  Returning adds on one address serialise, hence one per 1024 observations and not one per wave.
template <int VX>
__global__ __launch_bounds__(256) void quant_append_kernel(StrataKeys q, const int* __restrict__ rows, int Tr, int R, const float* __restrict__ X, int D,
                                                           int* __restrict__ cells, unsigned* __restrict__ keys, unsigned cap,
                                                           unsigned long long* __restrict__ cursor, unsigned long long* __restrict__ unmatched,
                                                           unsigned long long* __restrict__ rejected, unsigned long long* __restrict__ nonfinite,
                                                           unsigned long long* __restrict__ dropped) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* bl = reinterpret_cast<unsigned long long*>(smem);          // [1]: the first slot of the workgroup's step
  int* wl = reinterpret_cast<int*>(smem + 8);                                    // [4]: survivors of every wave
  int* vl = wl + 4;                                                              // [G]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < q.G; i += 256) vl[i] = q.vocab[i];
  __syncthreads();
  const unsigned N = (unsigned)q.B * (unsigned)q.T * (unsigned)q.P, per = 256u * QUANT_APPEND_ITEMS, stride = gridDim.x * per;   // N < 2^31, stride <= 2^22
  int unm = 0, rej = 0, nf = 0, drp = 0;
  for (unsigned i0 = blockIdx.x * per; i0 < N; i0 += stride) {                    // uniform in the workgroup
    bool live[QUANT_APPEND_ITEMS];
    int cell[QUANT_APPEND_ITEMS];
    unsigned long long who[QUANT_APPEND_ITEMS];
    int wcnt = 0;
#pragma unroll
    for (int e = 0; e < QUANT_APPEND_ITEMS; ++e) {
      const unsigned i = i0 + e * 256u + tid;
      cell[e] = 0;
      live[e] = i < N && quant_observe<VX>(q, vl, rows, Tr, R, X, D, i, cell[e], unm, rej, nf);
      who[e] = __ballot(live[e]);
      wcnt += __popcll(who[e]);
    }
    if (lane == 0) wl[wave] = wcnt;
    __syncthreads();
    if (tid == 0) {
      const int tot = wl[0] + wl[1] + wl[2] + wl[3];
      *bl = tot ? atomicAdd(cursor, (unsigned long long)tot) : 0ull;
    }
    __syncthreads();
    unsigned long long base = *bl;
    for (int w = 0; w < wave; ++w) base += (unsigned long long)wl[w];
#pragma unroll
    for (int e = 0; e < QUANT_APPEND_ITEMS; ++e) {
      if (live[e]) {
        const unsigned long long slot = base + (unsigned long long)__popcll(who[e] & ((1ull << lane) - 1ull));
        if (slot < cap) {
          const float* px = X + (size_t)(i0 + e * 256u + tid) * D;               // the second read of the row comes from the cache
          cells[slot] = cell[e];
          for (int d = 0; d < D; d += VX) {
            if (VX == 4) {
              const f32x4 x = *reinterpret_cast<const f32x4*>(px + d);
#pragma unroll
              for (int c = 0; c < 4; ++c) keys[(size_t)(d + c) * cap + slot] = quant_key(x[c]);
            } else {
              keys[(size_t)d * cap + slot] = quant_key(px[d]);
            }
          }
        } else {
          ++drp;
        }
      }
      base += (unsigned long long)__popcll(who[e]);
    }
    __syncthreads();                                                             // wl and bl are rewritten by the next step
  }
  unm = wave_sum_i(unm);
  rej = wave_sum_i(rej);
  nf = wave_sum_i(nf);
  drp = wave_sum_i(drp);
  if (lane == 0 && unm) atomicAdd(unmatched, (unsigned long long)unm);
  if (lane == 0 && rej) atomicAdd(rejected, (unsigned long long)rej);
  if (lane == 0 && nf) atomicAdd(nonfinite, (unsigned long long)nf);
  if (lane == 0 && drp) atomicAdd(dropped, (unsigned long long)drp);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

// the bins of all slots are indexed in 32 bits: C D 2Q <= 2^23 slots
bool quant_dims_ok(int C, int D, int Q) {
  return C >= 1 && C <= QUANT_MAX_C && D >= 1 && D <= QUANT_MAX_D && Q >= 1 && Q <= QUANT_MAX_Q && (int64_t)C * D * 2 * Q <= QUANT_MAX_SLOTS;
}

// hist [C D 2Q][256] | prefix [C D 2Q] | rank [C D 2Q], all uint32
size_t quant_ws_bytes(int C, int D, int Q) { return sizeof(unsigned) * (size_t)C * D * 2 * Q * (QUANT_BINS + 2); }

// one histogram pass over nslots = C D J slots
void quant_hist_launch(const QuantSrc& s, int vec, int J, int shift, unsigned nslots, int64_t nmax, int workgroups, const unsigned* prefix, unsigned* hist,
                       hipStream_t stream) {
  const int win = nslots < QUANT_WIN ? (int)nslots : QUANT_WIN;
  const unsigned W = (nslots + win - 1) / win;
  const int budget = workgroups > 0 ? workgroups : 2048;
  if (shift == 24 || W <= QUANT_LDS_WINDOWS) {
    const unsigned gy = W < (unsigned)budget ? W : (unsigned)budget;
    const unsigned gx = frl_grid(nmax, 256 * 4 * (vec ? 4 : 1), (int)(budget / gy));
    const size_t lds = sizeof(unsigned) * (size_t)win * (QUANT_BINS + 1);
    if (vec && W == 1) FRL_LAUNCH(quant_hist_lds_kernel<4>, dim3(gx, gy), dim3(256), lds, stream, s, J, shift, nslots, win, prefix, hist);
    else FRL_LAUNCH(quant_hist_lds_kernel<1>, dim3(gx, gy), dim3(256), lds, stream, s, J, shift, nslots, win, prefix, hist);
  } else {
    const unsigned gx = workgroups > 0 ? (unsigned)workgroups : frl_grid(nmax, 256 * 4, 2048);
    FRL_LAUNCH(quant_hist_direct_kernel, dim3(gx), dim3(256), 0, stream, s, J, shift, prefix, hist);
  }
}

}  // namespace

extern "C" {

// See include/frl_hip.h.
size_t frl_quantile_workspace_bytes(int C, int D, int Q) { return quant_dims_ok(C, D, Q) ? quant_ws_bytes(C, D, Q) : 0; }

int frl_quantile_append(const float* X, const void* codes, int codes_float, const int32_t* rows, int Tr, const unsigned char* mask, int Tm,
                        const int32_t* vocab, int G, int B, int T, int64_t P, int D, int R, int workgroups, int32_t* cells, uint32_t* keys,
                        int64_t capacity, int64_t* cursor, int64_t* unmatched, int64_t* rejected, int64_t* nonfinite, int64_t* dropped,
                        hipStream_t stream) {
  StrataKeys k;
  if (int rc = strata_check_keys("quantile_append", codes, codes_float, mask, Tm, vocab, G, B, T, P, workgroups, k)) return rc;
  if (!X || !cells || !keys || !cursor || !unmatched || !rejected || !nonfinite || !dropped) return frl_fail(-2, "quantile_append: null pointer");
  if (rows && Tr != 1 && Tr != T) return frl_fail(-2, "quantile_append: needs Tr 1 or T");
  if (D < 1 || D > QUANT_MAX_D) return frl_fail(-2, "quantile_append: needs 1 <= D <= 16 columns");
  if (R < 1 || (int64_t)R * G > QUANT_MAX_C || (!rows && R != 1)) return frl_fail(-2, "quantile_append: needs R >= 1 (1 without rows) and R * G <= 65535 cells");
  if (capacity < 1 || capacity > 0x7fffffffll) return frl_fail(-2, "quantile_append: needs 1 <= capacity < 2^31 records");
  const int64_t N = (int64_t)B * T * P;
  const int grid = workgroups > 0 ? workgroups : (int)frl_grid(N, 256 * QUANT_APPEND_ITEMS, 2048);
  const size_t lds = 8 + sizeof(int) * (4 + (size_t)G);                         // first slot | survivors per wave | vocab
  unsigned long long* cu = reinterpret_cast<unsigned long long*>(cursor);
  unsigned long long* um = reinterpret_cast<unsigned long long*>(unmatched);
  unsigned long long* rj = reinterpret_cast<unsigned long long*>(rejected);
  unsigned long long* nf = reinterpret_cast<unsigned long long*>(nonfinite);
  unsigned long long* dr = reinterpret_cast<unsigned long long*>(dropped);
  if ((D & 3) == 0 && ((uintptr_t)X & 15) == 0)
    FRL_LAUNCH(quant_append_kernel<4>, dim3((unsigned)grid), dim3(256), lds, stream, k, (const int*)rows, Tr, R, X, D, (int*)cells, (unsigned*)keys,
               (unsigned)capacity, cu, um, rj, nf, dr);
  else
    FRL_LAUNCH(quant_append_kernel<1>, dim3((unsigned)grid), dim3(256), lds, stream, k, (const int*)rows, Tr, R, X, D, (int*)cells, (unsigned*)keys,
               (unsigned)capacity, cu, um, rj, nf, dr);
  return frl_check_launch("quantile_append");
}

int frl_quantile_select(const int32_t* cells, const uint32_t* keys, int64_t capacity, const int64_t* cursor, const float* X,
                        const unsigned char* mask, int64_t N, int C, int D, const double* probs, int Q, int workgroups, int64_t* count, float* lo,
                        float* hi, double* frac, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (!quant_dims_ok(C, D, Q)) return frl_fail(-2, "quantile_select: needs 1 <= D <= 16, 1 <= Q <= 8, 1 <= C <= 65535 and C * D * 2Q <= 2^23");
  if (!probs || !count || !lo || !hi || !frac) return frl_fail(-2, "quantile_select: null pointer");
  if (int rc = frl_check_workgroups("quantile_select", workgroups)) return rc;
  QuantProbs pr;
  for (int q = 0; q < QUANT_MAX_Q; ++q) {
    pr.p[q] = q < Q ? probs[q] : 0.0;
    if (!(pr.p[q] >= 0.0 && pr.p[q] <= 1.0)) return frl_fail(-2, "quantile_select: probabilities must lie in [0, 1]");
  }
  QuantSrc s;
  s.cells = cells; s.keys = keys; s.cursor = reinterpret_cast<const unsigned long long*>(cursor); s.X = X; s.mask = mask; s.D = D; s.C = C;
  s.cap = 0; s.N = 0;
  int64_t nmax;
  if (X) {
    if (cells || keys || cursor) return frl_fail(-2, "quantile_select: takes either records or X");
    if (C != 1) return frl_fail(-2, "quantile_select: X goes into a single cell (C = 1)");
    if (N < 1 || N > 0x7fffffffll) return frl_fail(-2, "quantile_select: needs 1 <= N < 2^31 rows");
    s.N = (unsigned)N;
    nmax = N;
  } else {
    if (!cells || !keys || !cursor || mask) return frl_fail(-2, "quantile_select: records need cells, keys and cursor, and take no mask");
    if (capacity < 1 || capacity > 0x7fffffffll) return frl_fail(-2, "quantile_select: needs 1 <= capacity < 2^31 records");
    s.cap = (unsigned)capacity;
    nmax = capacity;
  }
  const size_t need = quant_ws_bytes(C, D, Q);
  if (int rc = frl_check_workspace("quantile_select", ws, ws_bytes, need)) return rc;
  const int J = 2 * Q;
  const unsigned S = (unsigned)C * D, SJ = S * J;
  unsigned* hist = (unsigned*)ws;
  unsigned* prefix = hist + (size_t)SJ * QUANT_BINS;
  unsigned* rank = prefix + SJ;
  const int vec = X && D == 1 && ((uintptr_t)X & 15) == 0 && ((uintptr_t)mask & 3) == 0;
  const size_t hist_bytes = sizeof(unsigned) * (size_t)SJ * QUANT_BINS;
  FRL_HIP(hipMemsetAsync(ws, 0, need, stream));
  quant_hist_launch(s, vec, 1, 24, S, nmax, workgroups, prefix, hist, stream);
  FRL_LAUNCH(quant_count_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, stream, (const unsigned*)hist, C, D, Q, pr, (long long*)count, frac);
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (shift < 24) {
      FRL_HIP(hipMemsetAsync(hist, 0, hist_bytes, stream));
      quant_hist_launch(s, vec, J, shift, SJ, nmax, workgroups, prefix, hist, stream);
    }
    FRL_LAUNCH(quant_pick_kernel, dim3((SJ + 255) / 256), dim3(256), 0, stream, (const unsigned*)hist, prefix, rank, (const long long*)count, pr, C, D, Q,
               shift, lo, hi);
  }
  return frl_check_launch("quantile_select");
}

}  // extern "C"
