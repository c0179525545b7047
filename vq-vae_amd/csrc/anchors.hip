// Anchor sampling (frl/data/sampling/anchor_sampling.py): per sample the jittered grid points on valid pixels, a supplement of up to 1024
// valid pixels drawn without replacement (uniformly or in proportion to a weight map), and the inverse-frequency weight map.  The reference
// does this with a dozen small torch ops and two host reads per sample; here one workgroup serves a sample and a launch serves the batch.
// The supplement is an exponential race: the caller supplies one Exp(1) variate per pixel, the key of an eligible pixel is noise / weight
// (noise alone without weights), and the picks are the pixels with the smallest (key, pixel index) in ascending order.  A radix select
// over the key's 32-bit pattern (non-negative floats order as unsigned integers) finds the key at the cut in four 8-bit passes; one
// more pass, in pixel order, collects everything below the cut and the first ties at it; a bitonic sort in LDS orders the winners.
// The keys are formed once and kept in a workspace that every pass re-reads, at every size: there is one path.
// Masks enter as the packed words of frl_spatial_pack_mask (spatial_pairs.hip).
#include "frl_common.hpp"
#include "frl_host.hpp"

#define AN_MAX_HW 1024
#define AN_MAX_SEG 4096
#define AN_MAX_SUP 1024
#define AN_MAX_GRID 16384
#define AN_MAX_DISTINCT 4096
#define AN_SLOTS 8192                     // hash table slots: at most half full
#define AN_EMPTY 0xffffffffu              // a NaN pattern: never the pattern of a finite value
#define AN_SEL_THREADS 1024
#define AN_GRID_THREADS 256

#define AN_FLAG_JITTER 1
#define AN_FLAG_WEIGHT 2
#define AN_FLAG_NOISE 4
#define AN_FLAG_DISTINCT 8

__device__ __forceinline__ bool an_bit(const uint32_t* __restrict__ sbits, int nw, int r, int c) {
  return (sbits[(size_t)r * nw + (c >> 5)] >> (c & 31)) & 1u;
}

// the number of i >= 0 with start + i * stride < end
__host__ __device__ __forceinline__ int an_steps(int start, int end, int stride) {
  return start < end ? (end - start + stride - 1) / stride : 0;
}

// ---- grid ----------------------------------------------------------------------------------------------------------------------------
// One workgroup per sample.  Grid point q = i * nc + j (row-major) is (r0 + i * stride, c0 + j * stride); the kept ones are compacted in
// that order: a ballot and a popcount within the wave, the waves' totals through LDS, a running prefix over the rounds of 256 points.
__global__ __launch_bounds__(AN_GRID_THREADS) void anchor_grid_kernel(const uint32_t* __restrict__ bits, int H, int W, int nw, int stride,
                                                                      int border, int radius, const int* __restrict__ jitter, int gmax,
                                                                      int* __restrict__ grid_rc, int* __restrict__ counts,
                                                                      int* __restrict__ flag) {
  __shared__ int wtot[2][AN_GRID_THREADS / 64];
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* sbits = bits + (size_t)s * H * nw;
  int* out = grid_rc + (size_t)s * gmax * 2;
  const int jr = jitter[2 * s], jc = jitter[2 * s + 1];
  const bool ok = jr >= -radius && jr <= radius && jc >= -radius && jc <= radius;         // block-uniform
  if (!ok && tid == 0) atomicOr(flag, AN_FLAG_JITTER);
  const int r0 = border + jr, c0 = border + jc;                                            // >= 0: border >= radius
  const int nr = ok ? an_steps(r0, H - border, stride) : 0, nc = ok ? an_steps(c0, W - border, stride) : 0;
  const int total = nr * nc;                                                               // <= gmax: the extreme jitter bounds it
  int run = 0;
  for (int base = 0, it = 0; base < total; base += AN_GRID_THREADS, ++it) {
    const int q = base + tid;
    int r = 0, c = 0;
    bool keep = false;
    if (q < total) {
      r = r0 + (q / nc) * stride;
      c = c0 + (q % nc) * stride;
      keep = an_bit(sbits, nw, r, c);
    }
    const unsigned long long b = __ballot(keep);
    if (lane == 0) wtot[it & 1][wave] = __popcll(b);
    __syncthreads();
    int pos = run + __popcll(b & ((1ull << lane) - 1ull));
    for (int u = 0; u < AN_GRID_THREADS / 64; ++u) {
      const int t = wtot[it & 1][u];
      if (u < wave) pos += t;
      run += t;
    }
    if (keep && pos < gmax) {
      out[2 * pos] = r;
      out[2 * pos + 1] = c;
    }
  }
  for (int p = run + tid; p < gmax; p += AN_GRID_THREADS) {
    out[2 * p] = -1;
    out[2 * p + 1] = -1;
  }
  if (tid == 0) counts[s] = run;
}

// ---- supplement ----------------------------------------------------------------------------------------------------------------------
#define AN_NOKEY 0xffffffffu             // not a valid pixel
#define AN_MASKED 0xfffffffeu            // a valid pixel whose weight is not positive

// One workgroup of 1024 threads per sample.  Pass 0 visits every pixel once (mask bit, weight, noise, the one division) and leaves the
// key's pattern in keys [S][H][W]: the later passes read 4 bytes per pixel, coalesced, and every thread only ever reads what it wrote
// itself (pixel idx belongs to thread idx % 1024 in every pass).  The key's pattern: noise, or noise / w rounded to nearest, with the
// sign bit dropped (-0 is 0; a negative or NaN noise is flagged), so an eligible pixel has a pattern of at most 0x7fffffff.
__global__ __launch_bounds__(AN_SEL_THREADS) void anchor_supplement_kernel(const uint32_t* __restrict__ bits, int H, int W, int nw,
                                                                           const float* __restrict__ weights,
                                                                           const float* __restrict__ noise, int n_sup,
                                                                           uint32_t* __restrict__ keys, int* __restrict__ sup_rc,
                                                                           int* __restrict__ counts, int* __restrict__ n_valid,
                                                                           int* __restrict__ flag) {
  __shared__ unsigned long long win[AN_MAX_SUP];
  __shared__ int hist[256];
  __shared__ int wtot[2][AN_SEL_THREADS / 64];
  __shared__ int sh_valid, sh_pos, sh_flag, sh_bin, sh_before, sh_ties, sh_less;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HW = H * W;
  const uint32_t* sbits = bits + (size_t)s * H * nw;
  const float* sw = weights ? weights + (size_t)s * HW : nullptr;
  const float* sn = noise ? noise + (size_t)s * HW : nullptr;
  uint32_t* sk = keys ? keys + (size_t)s * HW : nullptr;                                  // NULL only with n_sup == 0
  if (tid == 0) { sh_valid = 0; sh_pos = 0; sh_flag = 0; sh_less = 0; }
  __syncthreads();

  // pass 0: valid pixels, pixels of positive weight, bad inputs, the keys
  {
    int nv = 0, np = 0, f = 0;
    const int dr = AN_SEL_THREADS / W, dc = AN_SEL_THREADS - dr * W;                       // one round moves a thread by 1024 pixels
    int r = tid / W, c = tid - r * W;
    for (int base = tid; base < HW; base += 4 * AN_SEL_THREADS) {                         // four pixels per round: their loads go out together
      bool mk[4];
      float w[4], nz[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = base + u * AN_SEL_THREADS;
        const bool in = idx < HW;
        mk[u] = in && an_bit(sbits, nw, r, c);
        w[u] = (in && sw) ? sw[idx] : 1.f;
        nz[u] = (in && n_sup > 0) ? sn[idx] : 0.f;
        c += dc;
        r += dr;
        if (c >= W) { c -= W; ++r; }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = base + u * AN_SEL_THREADS;
        uint32_t key = AN_NOKEY;
        if (mk[u]) {                                                                     // what lies outside the mask is never looked at
          ++nv;
          if (!(fabsf(w[u]) <= 3.402823466e38f)) f |= AN_FLAG_WEIGHT;                     // inf or NaN
          if (!(nz[u] >= 0.f)) f |= AN_FLAG_NOISE;                                       // negative or NaN
          key = AN_MASKED;
          if (w[u] > 0.f) {
            ++np;
            key = __float_as_uint(sw ? __fdiv_rn(nz[u], w[u]) : nz[u]) & 0x7fffffffu;
          }
        }
        if (sk && idx < HW) sk[idx] = key;
      }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
      nv += __shfl_down(nv, off, 64);
      np += __shfl_down(np, off, 64);
      f |= __shfl_down(f, off, 64);
    }
    if (lane == 0) {
      if (nv) atomicAdd(&sh_valid, nv);
      if (np) atomicAdd(&sh_pos, np);
      if (f) atomicOr(&sh_flag, f);
    }
  }
  __syncthreads();
  const int valid = sh_valid;
  const bool fallback = sh_pos == 0;                                                     // no positive weight: uniform over the valid pixels
  const int eligible = fallback ? valid : sh_pos;
  const int m = n_sup < eligible ? n_sup : eligible;
  if (tid == 0) {
    counts[s] = m;
    n_valid[s] = valid;
    if (sh_flag) atomicOr(flag, sh_flag);
  }
  int* out = sup_rc + (size_t)s * n_sup * 2;
  if (m == 0) {                                                                          // block-uniform
    for (int p = tid; p < n_sup; p += AN_SEL_THREADS) {
      out[2 * p] = -1;
      out[2 * p + 1] = -1;
    }
    return;
  }
  if (fallback) {                                                                        // block-uniform: the key is the noise alone
    for (int idx = tid; idx < HW; idx += AN_SEL_THREADS)
      if (sk[idx] == AN_MASKED) sk[idx] = __float_as_uint(sn[idx]) & 0x7fffffffu;
  }

  // radix select: cut = the key of rank m (from 1) among the eligible pixels, need = how many pixels with exactly that key are taken
  uint32_t cut = 0xffffffffu;                                                            // every key is below it: take all
  int need = 0, ties = 0;
  if (m < eligible) {
    uint32_t prefix = 0;
    int remaining = m;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (int base = tid; base < HW; base += 8 * AN_SEL_THREADS) {                       // eight loads in flight
        uint32_t k[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int idx = base + u * AN_SEL_THREADS;
          k[u] = idx < HW ? sk[idx] : AN_NOKEY;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (k[u] <= 0x7fffffffu && (pass == 0 || (k[u] >> (shift + 8)) == prefix)) atomicAdd(&hist[(k[u] >> shift) & 255u], 1);
      }
      __syncthreads();
      if (wave == 0) {                                                                   // lane l owns bins 4 l .. 4 l + 3
        const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
        const int v = h0 + h1 + h2 + h3;
        int inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int t = __shfl_up(inc, off, 64);
          if (lane >= off) inc += t;
        }
        const int before = inc - v;                                                      // keys in the bins below mine
        if (before < remaining && remaining <= inc) {                                    // exactly one lane
          int b = 0, acc = before;
          if (acc + h0 < remaining) { acc += h0; b = 1;
            if (acc + h1 < remaining) { acc += h1; b = 2;
              if (acc + h2 < remaining) { acc += h2; b = 3; } } }
          sh_bin = 4 * lane + b;
          sh_before = acc;
          sh_ties = b == 0 ? h0 : b == 1 ? h1 : b == 2 ? h2 : h3;                          // after the last pass: the pixels with the cut's key
        }
      }
      __syncthreads();
      prefix = (prefix << 8) | (uint32_t)sh_bin;
      remaining -= sh_before;
    }
    cut = prefix;
    need = remaining;                                                                    // >= 1
    ties = sh_ties;                                                                      // >= need
  }
  const int less = m - need;                                                             // pixels with a key below the cut: all taken

  // collection.  Every pixel at the cut is taken (always so for distinct keys): whoever is at or below the cut takes a free slot, the sort
  // orders them.
  if (ties == need) {                                                                    // block-uniform
    for (int base = tid; base < HW; base += 8 * AN_SEL_THREADS) {
      uint32_t k[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int idx = base + u * AN_SEL_THREADS;
        k[u] = idx < HW ? sk[idx] : AN_NOKEY;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k[u] <= 0x7fffffffu && k[u] <= cut) {
          const int slot = atomicAdd(&sh_less, 1);
          if (slot < AN_MAX_SUP) win[slot] = ((unsigned long long)k[u] << 32) | (unsigned)(base + u * AN_SEL_THREADS);
        }
    }
    need = 0;
  }
  // Otherwise the cut falls inside a group of equal keys, and the walk is in pixel order: keys below the cut take any free slot in
  // [0, less), ties at the cut take the slots less + rank for the first `need` of them by pixel index
  const bool ordered = need > 0;                                                         // block-uniform
  int run = 0;
  for (int base = 0, it = 0; ordered && base < HW; base += AN_SEL_THREADS, ++it) {
    const int idx = base + tid;
    bool below = false, tie = false;
    uint32_t key = 0;
    if (idx < HW) {
      key = sk[idx];
      below = key <= 0x7fffffffu && key < cut;
      tie = key == cut;                                                                  // the cut is an eligible key or 0xffffffff with need == 0
    }
    if (below) {
      const int slot = atomicAdd(&sh_less, 1);
      if (slot < AN_MAX_SUP) win[slot] = ((unsigned long long)key << 32) | (unsigned)idx;
    }
    if (need == 0) continue;                                                             // block-uniform: the last tie is in
    const unsigned long long b = __ballot(tie);
    if (lane == 0) wtot[it & 1][wave] = __popcll(b);
    __syncthreads();
    int rank = run + __popcll(b & ((1ull << lane) - 1ull));
    for (int u = 0; u < AN_SEL_THREADS / 64; ++u) {
      const int t = wtot[it & 1][u];
      if (u < wave) rank += t;
      run += t;
    }
    if (tie && rank < need) win[less + rank] = ((unsigned long long)key << 32) | (unsigned)idx;   // less + rank < m <= 1024
    if (run >= need) {                                                                   // block-uniform: the remaining ties lose
      need = 0;
    }
  }
  __syncthreads();

  // bitonic sort of the m winners, padded to a power of two with the largest value
  int P = 2;
  while (P < m) P <<= 1;
  if (tid >= m && tid < P) win[tid] = ~0ull;
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      const int o = tid ^ j;
      if (tid < P && o > tid) {
        const unsigned long long a = win[tid], c = win[o];
        const bool up = (tid & k) == 0;
        if ((a > c) == up) {
          win[tid] = c;
          win[o] = a;
        }
      }
    }
  }
  __syncthreads();
  for (int p = tid; p < n_sup; p += AN_SEL_THREADS) {
    int r = -1, c = -1;
    if (p < m) {
      const int idx = (int)(win[p] & 0xffffffffull);
      r = idx / W;
      c = idx - r * W;
    }
    out[2 * p] = r;
    out[2 * p + 1] = c;
  }
}

// ---- inverse frequency ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool an_listed(const int* __restrict__ list, int n, float v) {
  const float r = rintf(v);                                                              // half to even
  if (!(fabsf(r) < 2147483648.f)) return false;
  const int code = (int)r;
  int a = 0, b = n;
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (list[mid] < code) a = mid + 1; else b = mid;
  }
  return a < n && list[a] == code;
}

__device__ __forceinline__ uint32_t an_hash(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x & (AN_SLOTS - 1);
}

// One workgroup per sample, two passes: count the eligible values in an LDS hash table keyed by the value's pattern (-0 as 0), then write
// 1 / count.  The table has twice AN_MAX_DISTINCT slots; the value that is one too many raises the flag (the counts stay right until the
// table is full; a pixel that finds no slot gets 0).
__global__ __launch_bounds__(AN_SEL_THREADS) void anchor_invfreq_kernel(const float* __restrict__ data, const uint32_t* __restrict__ bits, int H,
                                                                        int W, int nw, const int* __restrict__ list, int n_list,
                                                                        float* __restrict__ out, int* __restrict__ flag) {
  __shared__ uint32_t keys[AN_SLOTS];
  __shared__ int cnt[AN_SLOTS];
  __shared__ int sh_distinct, sh_elig, sh_over;
  const int s = blockIdx.x, tid = threadIdx.x;
  const int HW = H * W;
  const uint32_t* sbits = bits + (size_t)s * H * nw;
  const float* sd = data + (size_t)s * HW;
  float* so = out + (size_t)s * HW;
  for (int i = tid; i < AN_SLOTS; i += AN_SEL_THREADS) {
    keys[i] = AN_EMPTY;
    cnt[i] = 0;
  }
  if (tid == 0) { sh_distinct = 0; sh_elig = 0; sh_over = 0; }
  __syncthreads();
  const int dr = AN_SEL_THREADS / W, dc = AN_SEL_THREADS - dr * W;                         // one round moves a thread by 1024 pixels
  int r = tid / W, c = tid - r * W;
  for (int idx = tid; idx < HW; idx += AN_SEL_THREADS) {
    const bool masked = an_bit(sbits, nw, r, c);
    c += dc;
    r += dr;
    if (c >= W) { c -= W; ++r; }
    if (!masked) continue;
    const float v = sd[idx];
    if (!(fabsf(v) <= 3.402823466e38f)) continue;
    if (list && !an_listed(list, n_list, v)) continue;
    sh_elig = 1;                                                                         // every writer stores the same value
    const uint32_t pat = v == 0.f ? 0u : __float_as_uint(v);
    uint32_t h = an_hash(pat);
    bool placed = false;
    for (int probe = 0; probe < AN_SLOTS; ++probe) {
      uint32_t cur = keys[h];
      if (cur == AN_EMPTY) {
        cur = atomicCAS(&keys[h], AN_EMPTY, pat);                                        // another thread may have taken the slot meanwhile
        if (cur == AN_EMPTY) {
          cur = pat;
          if (atomicAdd(&sh_distinct, 1) >= AN_MAX_DISTINCT) sh_over = 1;                // one distinct value too many
        }
      }
      if (cur == pat) {
        atomicAdd(&cnt[h], 1);
        placed = true;
        break;
      }
      h = (h + 1) & (AN_SLOTS - 1);
    }
    if (!placed) sh_over = 1;
  }
  __syncthreads();
  const bool none = sh_elig == 0;
  if (tid == 0 && sh_over) atomicOr(flag, AN_FLAG_DISTINCT);
  r = tid / W;
  c = tid - r * W;
  for (int idx = tid; idx < HW; idx += AN_SEL_THREADS) {
    const bool masked = an_bit(sbits, nw, r, c);
    c += dc;
    r += dr;
    if (c >= W) { c -= W; ++r; }
    float wgt = 0.f;
    if (none) {
      wgt = masked ? 1.f : 0.f;
    } else if (masked) {
      const float v = sd[idx];
      if (fabsf(v) <= 3.402823466e38f && (!list || an_listed(list, n_list, v))) {
        const uint32_t pat = v == 0.f ? 0u : __float_as_uint(v);
        uint32_t h = an_hash(pat);
        for (int probe = 0; probe < AN_SLOTS; ++probe) {
          const uint32_t cur = keys[h];
          if (cur == pat) { wgt = __fdiv_rn(1.f, (float)cnt[h]); break; }
          if (cur == AN_EMPTY) break;
          h = (h + 1) & (AN_SLOTS - 1);
        }
      }
    }
    so[idx] = wgt;
  }
}

static int an_check(int S, int H, int W) {
  if (S <= 0 || S > AN_MAX_SEG) return frl_fail(-2, "anchors: the sample count must be in 1..4096");
  if (H <= 0 || W <= 0 || H > AN_MAX_HW || W > AN_MAX_HW) return frl_fail(-3, "anchors: H and W must be in 1..1024");
  return 0;
}

extern "C" {

// See include/frl_hip.h.
int frl_anchor_grid_max(int H, int W, int stride, int border, int jitter_radius) {
  if (H <= 0 || W <= 0 || H > AN_MAX_HW || W > AN_MAX_HW) return frl_fail(-3, "anchor_grid: H and W must be in 1..1024");
  if (stride < 1 || jitter_radius < 0 || border < jitter_radius || border > AN_MAX_HW)
    return frl_fail(-2, "anchor_grid: stride >= 1 and 0 <= jitter_radius <= border <= 1024 are required");
  const long long g = (long long)an_steps(border - jitter_radius, H - border, stride) * an_steps(border - jitter_radius, W - border, stride);
  if (g > AN_MAX_GRID) return frl_fail(-3, "anchor_grid: at most 16384 grid points per sample");
  return (int)g;
}

int frl_anchor_grid(const uint32_t* bits, int S, int H, int W, int stride, int border, int jitter_radius, const int32_t* jitter, int gmax,
                    int32_t* grid_rc, int32_t* counts, int32_t* flag, hipStream_t stream) {
  const int rc = an_check(S, H, W);
  if (rc) return rc;
  const int g = frl_anchor_grid_max(H, W, stride, border, jitter_radius);
  if (g < 0) return g;
  if (gmax < g) return frl_fail(-2, "anchor_grid: gmax is below frl_anchor_grid_max");
  if (!bits || !jitter || !counts || !flag || (gmax > 0 && !grid_rc)) return frl_fail(-2, "anchor_grid: null pointer");
  FRL_LAUNCH(anchor_grid_kernel, dim3(S), dim3(AN_GRID_THREADS), 0, stream, bits, H, W, (W + 31) / 32, stride, border, jitter_radius, jitter,
             gmax, grid_rc, counts, flag);
  return frl_check_launch("anchor_grid");
}

int frl_anchor_supplement(const uint32_t* bits, int S, int H, int W, const float* weights, const float* noise, int supplement_n,
                          uint32_t* keys, int32_t* sup_rc, int32_t* counts, int32_t* n_valid, int32_t* flag, hipStream_t stream) {
  const int rc = an_check(S, H, W);
  if (rc) return rc;
  if (supplement_n < 0 || supplement_n > AN_MAX_SUP) return frl_fail(-2, "anchor_supplement: supplement_n must be in 0..1024");
  if (!bits || !counts || !n_valid || !flag || (supplement_n > 0 && (!noise || !sup_rc || !keys))) return frl_fail(-2, "anchor_supplement: null pointer");
  FRL_LAUNCH(anchor_supplement_kernel, dim3(S), dim3(AN_SEL_THREADS), 0, stream, bits, H, W, (W + 31) / 32, weights, noise, supplement_n,
             supplement_n > 0 ? keys : nullptr, sup_rc, counts, n_valid, flag);
  return frl_check_launch("anchor_supplement");
}

int frl_anchor_inverse_frequency(const float* data, const uint32_t* bits, int S, int H, int W, const int32_t* valid_values, int n_values,
                                 float* out, int32_t* flag, hipStream_t stream) {
  const int rc = an_check(S, H, W);
  if (rc) return rc;
  if (n_values < 0 || n_values > AN_MAX_DISTINCT) return frl_fail(-2, "anchor_inverse_frequency: at most 4096 listed values");
  if (!data || !bits || !out || !flag || (n_values > 0 && !valid_values)) return frl_fail(-2, "anchor_inverse_frequency: null pointer");
  FRL_LAUNCH(anchor_invfreq_kernel, dim3(S), dim3(AN_SEL_THREADS), 0, stream, data, bits, H, W, (W + 31) / 32, valid_values, n_values, out, flag);
  return frl_check_launch("anchor_inverse_frequency");
}

}  // extern "C"
