// Spatial InfoNCE pair mining (frl/training/representation/step.py:323-401 with frl/utils/spatial.py:176-332): per anchor pixel the
// offset k nearest valid neighbours, n far negatives drawn uniformly without replacement from the valid pixels at a distance in
// [min, max], the map of all those coordinates onto their sorted unique list, and the spectral pair weights.
// The reference forms, per anchor, the float distance to every valid pixel of the patch (65 536 for a 256 x 256 mask), a where and a
// randperm.  Here everything lives on the H x W grid: the mask is packed to one bit per pixel, the candidates of an anchor in a mask row
// are the set bits inside at most two column intervals (integer square roots of lo - dy^2 and hi - dy^2), their number is a popcount, the
// candidate of a given rank is found by a search in the prefix sums of the row counts and a bit select, and the index of a coordinate in
// the sorted unique list is the number of set bits below its key in a bitmap of the marked pixels.  Nothing with one element per valid
// pixel is written.  Every kernel serves all segments (samples) of a batch: blockIdx.y is the segment.
#include "frl_common.hpp"
#include "frl_host.hpp"

#define SP_WAVES 4
#define SP_MAX_HW 1024
#define SP_MAX_SEG 4096

// masks [S][H][W] bytes -> bits [S][H][nw] words, bit c % 32 of word c / 32 = pixel (r, c); one thread per pixel of the padded row,
// one ballot per 64 of them (nw * 32 is a multiple of 32: a wave covers two whole words).
__global__ __launch_bounds__(256) void spatial_pack_kernel(const uint8_t* __restrict__ mask, long long total, int W, int nw,
                                                           uint32_t* __restrict__ bits) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  bool v = false;
  if (idx < total) {
    const int c = (int)(idx % (nw * 32));
    const long long row = idx / (nw * 32);
    v = c < W && mask[row * W + c] != 0;
  }
  const unsigned long long b = __ballot(v);
  const int lane = threadIdx.x & 63;
  if (idx < total && (lane & 31) == 0) bits[idx >> 5] = (uint32_t)(lane ? b >> 32 : b);
}

// floor(sqrt(v)) for 0 <= v < 2^22, integers only
__device__ __forceinline__ int sp_isqrt(int v) {
  int r = 0;
#pragma unroll
  for (int b = 1 << 10; b; b >>= 1) {
    const int t = r | b;
    if (t * t <= v) r = t;
  }
  return r;
}

struct SpIv { int a0, a1, b0, b1; };   // the columns a0..a1 and b0..b1 (a before b); an interval with x0 > x1 is empty

// The columns x of mask row y with lo <= (y - r)^2 + (x - c)^2 <= hi: |x - c| in [a, b], a = ceil(sqrt(lo - dy^2)), b = floor(sqrt(hi - dy^2)).
__device__ __forceinline__ SpIv sp_row_intervals(int r, int c, int y, int lo, int hi, int W) {
  SpIv iv = {0, -1, 0, -1};
  const int dy = y - r, dy2 = dy * dy;
  const int t1 = hi - dy2, t0 = lo - dy2;
  if (t1 < 0) return iv;
  const int b = sp_isqrt(t1);
  const int a = t0 <= 0 ? 0 : sp_isqrt(t0 - 1) + 1;
  if (a > b) return iv;
  iv.a0 = max(c - b, 0);
  if (a == 0) { iv.a1 = min(c + b, W - 1); return iv; }
  iv.a1 = c - a;                                                                 // below c < W; negative: empty
  iv.b0 = c + a;                                                                 // W or more: empty
  iv.b1 = min(c + b, W - 1);
  return iv;
}

// the bits of word j that lie in columns x0..x1, for (x0 >> 5) <= j <= (x1 >> 5)
__device__ __forceinline__ uint32_t sp_word_mask(int j, int x0, int x1) {
  uint32_t m = 0xffffffffu;
  if (j == (x0 >> 5)) m &= 0xffffffffu << (x0 & 31);
  if (j == (x1 >> 5)) m &= 0xffffffffu >> (31 - (x1 & 31));
  return m;
}

__device__ __forceinline__ int sp_count(const uint32_t* __restrict__ row, int x0, int x1) {
  int n = 0;
  if (x0 > x1) return 0;
  for (int j = x0 >> 5; j <= (x1 >> 5); ++j) n += __popc(row[j] & sp_word_mask(j, x0, x1));
  return n;
}

// the column of the set bit of rank q (from 0) among columns x0..x1; -1 when there are not that many
__device__ __forceinline__ int sp_select(const uint32_t* __restrict__ row, int x0, int x1, int q) {
  if (x0 > x1) return -1;
  for (int j = x0 >> 5; j <= (x1 >> 5); ++j) {
    uint32_t w = row[j] & sp_word_mask(j, x0, x1);
    const int n = __popc(w);
    if (q < n) {
      for (; q > 0; --q) w &= w - 1;
      return j * 32 + __ffs(w) - 1;
    }
    q -= n;
  }
  return -1;
}

__device__ __forceinline__ void sp_segment(const int* __restrict__ seg, int N, int& s0, int& n) {
  int a = seg[blockIdx.y], b = seg[blockIdx.y + 1];
  a = a < 0 ? 0 : (a > N ? N : a);                                               // the host has checked the offsets; never leave the rows
  b = b < a ? a : (b > N ? N : b);
  s0 = a;
  n = b - a;
}

// Far negatives.  One wave per anchor, four anchors per workgroup, no workgroup barrier.  Pass 1: lane l counts the candidates of rows
// l, l + 64, ... and a wave scan leaves pre[y] = candidates in rows above y in LDS (pre[H] = cnt).  Pass 2 (wave-uniform, lane l keeps
// the l-th smallest pick so far): draw j -> q = draw * (cnt - j) >> 31, the rank among the remaining candidates; the rank among all
// candidates is q + t with t the number of earlier picks s_0 < s_1 < ... with s_i - i <= q (s_i - i does not decrease, so these are
// exactly the picks that the rule "ascending, while q >= pick: q += 1" passes).  Pass 3: lane j locates its pick: row by a binary search
// in pre, column by a bit select.
__global__ __launch_bounds__(64 * SP_WAVES) void spatial_neg_kernel(const uint32_t* __restrict__ bits, int H, int W, int nw,
                                                                    const int* __restrict__ anchors, int N, const int* __restrict__ seg,
                                                                    int lo, int hi, int n_per, const int* __restrict__ draws,
                                                                    int* __restrict__ neg_rc, int* __restrict__ neg_count,
                                                                    int* __restrict__ counters, int* __restrict__ flag) {
  __shared__ int pre_all[SP_WAVES][SP_MAX_HW + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int s0, n;
  sp_segment(seg, N, s0, n);
  const int iq = blockIdx.x * SP_WAVES + wave;
  if (iq >= n) return;                                                           // wave-uniform
  const int i = s0 + iq;
  const int r = anchors[2 * i], c = anchors[2 * i + 1];
  const bool inside = r >= 0 && r < H && c >= 0 && c < W;
  int* pre = pre_all[wave];
  const uint32_t* sbits = bits + (size_t)blockIdx.y * H * nw;
  int cnt = 0;
  if (inside && lo <= hi) {
    int base = 0;
    for (int y0 = 0; y0 < H; y0 += 64) {
      const int y = y0 + lane;
      int v = 0;
      if (y < H) {
        const SpIv iv = sp_row_intervals(r, c, y, lo, hi, W);
        const uint32_t* row = sbits + (size_t)y * nw;
        v = sp_count(row, iv.a0, iv.a1) + sp_count(row, iv.b0, iv.b1);
      }
      int inc = v;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
      }
      if (y < H) pre[y] = base + inc - v;
      base += __shfl(inc, 63, 64);
    }
    cnt = base;
    if (lane == 0) pre[H] = cnt;
  }
  __builtin_amdgcn_wave_barrier();
  const int m = n_per < cnt ? n_per : cnt;
  const int myd = lane < n_per ? draws[(size_t)i * n_per + lane] : 0;
  const bool bad = __ballot(myd < 0) != 0ull;                                    // a draw outside [0, 2^31)
  int sorted = 0x7fffffff, mine = -1;
  for (int j = 0; j < m; ++j) {
    const unsigned long long d = (unsigned long long)(__shfl(myd, j, 64) & 0x7fffffff);
    const int q = (int)((d * (unsigned long long)(cnt - j)) >> 31);
    const int t = __popcll(__ballot(lane < j && sorted - lane <= q));
    const int v = q + t;
    const int up = __shfl_up(sorted, 1, 64);
    sorted = lane < t ? sorted : (lane == t ? v : up);
    if (lane == j) mine = v;
  }
  if (lane < n_per) {
    int y = -1, x = -1;
    if (lane < m) {
      int a = 0, b = H;                                                          // pre[a] <= mine < pre[b]
      while (b - a > 1) {
        const int mid = (a + b) >> 1;
        if (pre[mid] <= mine) a = mid; else b = mid;
      }
      const SpIv iv = sp_row_intervals(r, c, a, lo, hi, W);
      const uint32_t* row = sbits + (size_t)a * nw;
      const int rr = mine - pre[a], na = sp_count(row, iv.a0, iv.a1);
      x = rr < na ? sp_select(row, iv.a0, iv.a1, rr) : sp_select(row, iv.b0, iv.b1, rr - na);
      y = x < 0 ? -1 : a;
    }
    int* o = neg_rc + ((size_t)i * n_per + lane) * 2;
    o[0] = y;
    o[1] = x;
  }
  if (lane == 0) {
    neg_count[i] = m;
    if (m) atomicAdd(counters + blockIdx.y, m);
    const int f = (inside ? 0 : 1) | (bad ? 2 : 0);
    if (f) atomicOr(flag, f);
  }
}

// Offset neighbours: one thread per (anchor, offset).
__global__ __launch_bounds__(256) void spatial_knn_kernel(const uint32_t* __restrict__ bits, int H, int W, int nw, const int* __restrict__ anchors,
                                                          int N, const int* __restrict__ seg, const int* __restrict__ offs, int k,
                                                          int* __restrict__ pos_rc, uint8_t* __restrict__ pos_valid,
                                                          int* __restrict__ counters, int* __restrict__ flag) {
  int s0, n;
  sp_segment(seg, N, s0, n);
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  bool ok = false;
  if (t < (long long)n * k) {
    const int i = s0 + (int)(t / k), slot = (int)(t % k);
    const int r = anchors[2 * i], c = anchors[2 * i + 1];
    const bool inside = r >= 0 && r < H && c >= 0 && c < W;
    int y = -1, x = -1;
    if (inside) {
      y = r + offs[2 * slot];
      x = c + offs[2 * slot + 1];
      if (y >= 0 && y < H && x >= 0 && x < W) ok = (bits[((size_t)blockIdx.y * H + y) * nw + (x >> 5)] >> (x & 31)) & 1u;
    } else if (slot == 0) {
      atomicOr(flag, 1);
    }
    const size_t o = (size_t)i * k + slot;
    pos_rc[2 * o] = y;
    pos_rc[2 * o + 1] = x;
    pos_valid[o] = ok ? 1 : 0;
  }
  const int nv = __popcll(__ballot(ok));
  if ((threadIdx.x & 63) == 0 && nv) atomicAdd(counters + blockIdx.y, nv);
}

// The key r * W + c of slot `slot` of anchor i (0: the anchor, 1..k: its neighbours, k + 1..k + n_per: its negatives), or -1 when the
// slot holds nothing (an invalid neighbour, a negative beyond neg_count, anything of an anchor outside the grid).
__device__ __forceinline__ int sp_slot_key(int i, int slot, int H, int W, const int* __restrict__ anchors, const int* __restrict__ pos_rc,
                                           const uint8_t* __restrict__ pos_valid, int k, const int* __restrict__ neg_rc,
                                           const int* __restrict__ neg_count, int n_per) {
  const int r = anchors[2 * i], c = anchors[2 * i + 1];
  if (r < 0 || r >= H || c < 0 || c >= W) return -1;
  int y = r, x = c;
  if (slot >= 1 && slot <= k) {
    const size_t o = (size_t)i * k + slot - 1;
    if (!pos_valid[o]) return -1;
    y = pos_rc[2 * o];
    x = pos_rc[2 * o + 1];
  } else if (slot > k) {
    const int j = slot - 1 - k;
    if (j >= neg_count[i]) return -1;
    const size_t o = (size_t)i * n_per + j;
    y = neg_rc[2 * o];
    x = neg_rc[2 * o + 1];
  }
  if (y < 0 || y >= H || x < 0 || x >= W) return -1;
  return y * W + x;
}

__global__ __launch_bounds__(256) void spatial_mark_kernel(int H, int W, int nwb, const int* __restrict__ anchors, int N, const int* __restrict__ seg,
                                                           const int* __restrict__ pos_rc, const uint8_t* __restrict__ pos_valid, int k,
                                                           const int* __restrict__ neg_rc, const int* __restrict__ neg_count, int n_per,
                                                           uint32_t* __restrict__ bitmap) {
  int s0, n;
  sp_segment(seg, N, s0, n);
  const int slots = 1 + k + n_per;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)n * slots) return;
  const int key = sp_slot_key(s0 + (int)(t / slots), (int)(t % slots), H, W, anchors, pos_rc, pos_valid, k, neg_rc, neg_count, n_per);
  if (key >= 0) atomicOr(bitmap + (size_t)blockIdx.y * nwb + (key >> 5), 1u << (key & 31));
}

// One workgroup per segment: wordpre[w] = set bits in the words below w, totals[s] = set bits of the segment.
__global__ __launch_bounds__(256) void spatial_scan_kernel(const uint32_t* __restrict__ bitmap, int nwb, int* __restrict__ wordpre,
                                                           int* __restrict__ totals) {
  __shared__ int wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* bm = bitmap + (size_t)blockIdx.x * nwb;
  int* wp = wordpre + (size_t)blockIdx.x * nwb;
  const int chunk = (nwb + 255) / 256;
  const int w0 = tid * chunk, w1 = min(w0 + chunk, nwb);
  int v = 0;
  for (int w = w0; w < w1; ++w) v += __popc(bm[w]);
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int run = inc - v;
  for (int u = 0; u < wave; ++u) run += wsum[u];
  for (int w = w0; w < w1; ++w) {
    wp[w] = run;
    run += __popc(bm[w]);
  }
  if (tid == 255) totals[blockIdx.x] = run;
}

__global__ void spatial_offsets_kernel(const int* __restrict__ totals, int S, int* __restrict__ unique_seg) {
  if (threadIdx.x || blockIdx.x) return;
  int run = 0;
  for (int s = 0; s < S; ++s) {
    unique_seg[s] = run;
    run += totals[s];
  }
  unique_seg[S] = run;
}

// One thread per bitmap word: the coordinates of its set bits, ascending, at unique_seg[s] + wordpre[w] + rank.
__global__ __launch_bounds__(256) void spatial_emit_kernel(const uint32_t* __restrict__ bitmap, int nwb, int W, const int* __restrict__ wordpre,
                                                           const int* __restrict__ unique_seg, long long cap, int* __restrict__ unique_rc) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= nwb) return;
  uint32_t b = bitmap[(size_t)blockIdx.y * nwb + w];
  long long pos = (long long)unique_seg[blockIdx.y] + wordpre[(size_t)blockIdx.y * nwb + w];
  while (b && pos < cap) {
    const int key = w * 32 + __ffs(b) - 1;
    unique_rc[2 * pos] = key / W;
    unique_rc[2 * pos + 1] = key % W;
    b &= b - 1;
    ++pos;
  }
}

// One thread per (anchor, slot): the index of the slot's coordinate in the unique list (shifted by the segment's unique offset) and, for
// the pair slots, d = |f_anchor - f_other|_2 over the C channels of feat [S][C][H][W] and the weights.
__global__ __launch_bounds__(256) void spatial_index_kernel(int H, int W, int nwb, const int* __restrict__ anchors, int N, const int* __restrict__ seg,
                                                            const int* __restrict__ pos_rc, const uint8_t* __restrict__ pos_valid, int k,
                                                            const int* __restrict__ neg_rc, const int* __restrict__ neg_count, int n_per,
                                                            const uint32_t* __restrict__ bitmap, const int* __restrict__ wordpre,
                                                            const int* __restrict__ unique_seg, const float* __restrict__ feat, int C, float tau,
                                                            float min_w, int* __restrict__ anchor_idx, int* __restrict__ pos_idx,
                                                            int* __restrict__ neg_idx, float* __restrict__ pos_w, float* __restrict__ pos_d,
                                                            float* __restrict__ neg_w, float* __restrict__ neg_d) {
  int s0, n;
  sp_segment(seg, N, s0, n);
  const int slots = 1 + k + n_per;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)n * slots) return;
  const int i = s0 + (int)(t / slots), slot = (int)(t % slots);
  const int key = sp_slot_key(i, slot, H, W, anchors, pos_rc, pos_valid, k, neg_rc, neg_count, n_per);
  int idx = -1;
  if (key >= 0) {
    const size_t w = (size_t)blockIdx.y * nwb + (key >> 5);
    idx = unique_seg[blockIdx.y] + wordpre[w] + __popc(bitmap[w] & ((1u << (key & 31)) - 1u));
  }
  if (slot == 0) { anchor_idx[i] = idx; return; }
  float d = 0.f, wgt = 0.f;
  if (key >= 0) {
    const size_t hw = (size_t)H * W;
    const float* fa = feat + (size_t)blockIdx.y * C * hw + (size_t)anchors[2 * i] * W + anchors[2 * i + 1];
    const float* fb = feat + (size_t)blockIdx.y * C * hw + key;
    float s = 0.f;
    for (int ch = 0; ch < C; ++ch) {
      const float e = fa[ch * hw] - fb[ch * hw];
      s = fmaf(e, e, s);
    }
    d = sqrtf(s);
    const float e = expf(-d / tau);
    wgt = fminf(fmaxf(slot <= k ? e : 1.f - e, min_w), 1.f);
  }
  if (slot <= k) {
    const size_t o = (size_t)i * k + slot - 1;
    pos_idx[o] = idx;
    pos_w[o] = wgt;
    pos_d[o] = d;
  } else {
    const size_t o = (size_t)i * n_per + slot - 1 - k;
    neg_idx[o] = idx;
    neg_w[o] = wgt;
    neg_d[o] = d;
  }
}

// the checks every entry point shares -> the longest segment, or a negative code
static int sp_check(int S, int H, int W, int N, const int32_t* seg_host) {
  if (S <= 0 || S > SP_MAX_SEG) return frl_fail(-2, "spatial_pairs: the segment count must be in 1..4096");
  if (H <= 0 || W <= 0 || H > SP_MAX_HW || W > SP_MAX_HW) return frl_fail(-3, "spatial_pairs: H and W must be in 1..1024");
  if (N <= 0 || N > (1 << 24)) return frl_fail(-2, "spatial_pairs: N must be in 1..2^24");
  if (!seg_host) return frl_fail(-2, "spatial_pairs: null pointer");
  if (seg_host[0] != 0 || seg_host[S] != N) return frl_fail(-2, "spatial_pairs: segment offsets must rise from 0 to N");
  int longest = 0;
  for (int s = 0; s < S; ++s) {
    const int n = seg_host[s + 1] - seg_host[s];
    if (n < 0) return frl_fail(-2, "spatial_pairs: segment offsets must rise from 0 to N");
    longest = n > longest ? n : longest;
  }
  return longest;
}

extern "C" {

int frl_spatial_pairs_max_hw(void) { return SP_MAX_HW; }

// See include/frl_hip.h.
int frl_spatial_pack_mask(const uint8_t* mask, int S, int H, int W, uint32_t* bits, hipStream_t stream) {
  if (S <= 0 || S > SP_MAX_SEG) return frl_fail(-2, "spatial_pack_mask: the segment count must be in 1..4096");
  if (H <= 0 || W <= 0 || H > SP_MAX_HW || W > SP_MAX_HW) return frl_fail(-3, "spatial_pack_mask: H and W must be in 1..1024");
  if (!mask || !bits) return frl_fail(-2, "spatial_pack_mask: null pointer");
  const int nw = (W + 31) / 32;
  const long long total = (long long)S * H * nw * 32;
  FRL_LAUNCH(spatial_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, mask, total, W, nw, bits);
  return frl_check_launch("spatial_pack_mask");
}

int frl_spatial_knn(const uint32_t* bits, int S, int H, int W, const int32_t* anchors, int N, const int32_t* seg_host, const int32_t* seg,
                    const int32_t* offsets, int k, int32_t* pos_rc, uint8_t* pos_valid, int32_t* counters, int32_t* flag, hipStream_t stream) {
  const int longest = sp_check(S, H, W, N, seg_host);
  if (longest < 0) return longest;
  if (k < 1 || k > 64) return frl_fail(-2, "spatial_knn: the offset count must be in 1..64");
  if (!bits || !anchors || !seg || !offsets || !pos_rc || !pos_valid || !counters || !flag) return frl_fail(-2, "spatial_knn: null pointer");
  if (longest == 0) return 0;
  const dim3 grid((unsigned)(((long long)longest * k + 255) / 256), S);
  FRL_LAUNCH(spatial_knn_kernel, grid, dim3(256), 0, stream, bits, H, W, (W + 31) / 32, anchors, N, seg, offsets, k, pos_rc, pos_valid, counters,
             flag);
  return frl_check_launch("spatial_knn");
}

int frl_spatial_negatives(const uint32_t* bits, int S, int H, int W, const int32_t* anchors, int N, const int32_t* seg_host, const int32_t* seg,
                          int lo, int hi, int n_per_anchor, const int32_t* draws, int32_t* neg_rc, int32_t* neg_count, int32_t* counters,
                          int32_t* flag, hipStream_t stream) {
  const int longest = sp_check(S, H, W, N, seg_host);
  if (longest < 0) return longest;
  if (n_per_anchor < 1 || n_per_anchor > 64) return frl_fail(-2, "spatial_negatives: n_per_anchor must be in 1..64");
  if (!bits || !anchors || !seg || !draws || !neg_rc || !neg_count || !counters || !flag)
    return frl_fail(-2, "spatial_negatives: null pointer");
  if (longest == 0) return 0;
  const int top = (H - 1) * (H - 1) + (W - 1) * (W - 1);                        // no pair of pixels is farther apart
  if (lo < 0) lo = 0;
  if (hi > top) hi = top;
  if (lo > top) { lo = 1; hi = 0; }                                              // empty for every anchor
  const dim3 grid((longest + SP_WAVES - 1) / SP_WAVES, S);
  FRL_LAUNCH(spatial_neg_kernel, grid, dim3(64 * SP_WAVES), 0, stream, bits, H, W, (W + 31) / 32, anchors, N, seg, lo, hi, n_per_anchor, draws,
             neg_rc, neg_count, counters, flag);
  return frl_check_launch("spatial_negatives");
}

int frl_spatial_pair_index(int S, int H, int W, const int32_t* anchors, int N, const int32_t* seg_host, const int32_t* seg, const int32_t* pos_rc,
                           const uint8_t* pos_valid, int k, const int32_t* neg_rc, const int32_t* neg_count, int n_per_anchor, const float* feat,
                           int C, float tau, float min_w, uint32_t* bitmap, int32_t* wordpre, int32_t* unique_seg, int32_t* unique_rc,
                           int32_t* anchor_idx, int32_t* pos_idx, int32_t* neg_idx, float* pos_w, float* pos_d, float* neg_w, float* neg_d,
                           hipStream_t stream) {
  const int longest = sp_check(S, H, W, N, seg_host);
  if (longest < 0) return longest;
  if (k < 1 || k > 64 || n_per_anchor < 1 || n_per_anchor > 64)
    return frl_fail(-2, "spatial_pair_index: the offset count and n_per_anchor must be in 1..64");
  if (C < 1 || C > 256) return frl_fail(-2, "spatial_pair_index: C must be in 1..256");
  if (!(tau > 0.f)) return frl_fail(-2, "spatial_pair_index: tau must be positive");
  if (!anchors || !seg || !pos_rc || !pos_valid || !neg_rc || !neg_count || !feat || !bitmap || !wordpre || !unique_seg || !unique_rc ||
      !anchor_idx || !pos_idx || !neg_idx || !pos_w || !pos_d || !neg_w || !neg_d)
    return frl_fail(-2, "spatial_pair_index: null pointer");
  const int nwb = (H * W + 31) / 32, slots = 1 + k + n_per_anchor;
  int* totals = wordpre + (size_t)S * nwb;
  FRL_HIP(hipMemsetAsync(bitmap, 0, (size_t)S * nwb * sizeof(uint32_t), stream));
  const dim3 grid((unsigned)(((long long)longest * slots + 255) / 256), S);
  if (longest)
    FRL_LAUNCH(spatial_mark_kernel, grid, dim3(256), 0, stream, H, W, nwb, anchors, N, seg, pos_rc, pos_valid, k, neg_rc, neg_count, n_per_anchor,
               bitmap);
  FRL_LAUNCH(spatial_scan_kernel, dim3(S), dim3(256), 0, stream, (const uint32_t*)bitmap, nwb, wordpre, totals);
  FRL_LAUNCH(spatial_offsets_kernel, dim3(1), dim3(64), 0, stream, (const int*)totals, S, unique_seg);
  FRL_LAUNCH(spatial_emit_kernel, dim3((nwb + 255) / 256, S), dim3(256), 0, stream, (const uint32_t*)bitmap, nwb, W, (const int*)wordpre,
             (const int*)unique_seg, (long long)N * slots, unique_rc);
  if (longest)
    FRL_LAUNCH(spatial_index_kernel, grid, dim3(256), 0, stream, H, W, nwb, anchors, N, seg, pos_rc, pos_valid, k, neg_rc, neg_count, n_per_anchor,
               (const uint32_t*)bitmap, (const int*)wordpre, (const int*)unique_seg, feat, C, tau, min_w, anchor_idx, pos_idx, neg_idx, pos_w, pos_d,
               neg_w, neg_d);
  return frl_check_launch("spatial_pair_index");
}

}  // extern "C"
