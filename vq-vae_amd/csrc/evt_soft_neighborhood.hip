// EVT soft-neighbourhood loss (frl/losses/evt_soft_neighborhood.py:266-440, caller frl/training/representation/step.py:540): per sample
// (a "segment" of anchor rows) the weighted mean over anchors of a row KL between the softmax of diffusion distances in the EVT confusion
// graph and the softmax of embedding distances, all pairs of the segment, with no [M, M] array in memory.
//   emb [N][D] f32 | bf16 (upcast on load), idx [N] int32 code index (-1 = unknown code), S [K][K] f32 diffused similarity (NOT symmetric:
//   a power of a row-normalised matrix), w [K] f32 inverse-frequency weights, seg [nseg + 1] int32 row offsets.
//   anchor i valid        iff idx[i] >= 0 (an idx >= K is treated as unknown and flagged)
//   pair (i, j) in mask   iff both valid, i != j and idx[i] != idx[j]   (i != j follows from idx[i] != idx[j])
//   row i active          iff it has >= 2 pairs in the mask
//   a_ij = -(1 - S[idx_i][idx_j]) / tau_ref,  b_ij = -|e_i - e_j|_2 / tau_learned,  p = softmax_j(a),  q = softmax_j(b) over the mask
//   KL_i = sum_j p_ij (log p_ij - log q_ij),  loss = sum_i w[idx_i] active_i KL_i / sum_i w[idx_i] active_i
//   a segment with fewer than min_valid_anchors valid anchors, or whose weights sum to nothing, has loss 0 and gradient 0.
// For finite inputs this is the reference's function: it filters the valid anchors, compares raw codes (the same test among valid anchors:
// the code -> index map is injective) and fills the excluded logits with -1e9, whose softmax terms are exactly 0 in float32 and float64, so
// leaving them out is the same sum.  1 - S is formed in float32, as the reference's d_ref is.
//
// Forward: a workgroup of 256 threads owns 32 rows of one segment (blockIdx.y = segment, blockIdx.x = row tile) and streams the segment's
// rows 64 at a time through LDS.  Thread (r = tid / 8, cl = tid % 8) holds row r against columns cl, cl + 8, .. of the tile: squared
// distances from float32 differences (never the Gram form |a|^2 + |b|^2 - 2ab, which cancels at small distances), chunks of 16 channels
// summed plainly and the chunks folded with a two-sum, so d is good to an ulp at D = 256.  Online state per row, relative to the running
// maximum m of b (u = b - m <= 0; a is bounded by [-1 / tau_ref, 0] and needs no maximum):
//   sb = sum e^u, sbb = sum e^u u, sa = sum e^a, saa = sum e^a a, sab = sum e^a (a - u), the mask count, and the confused-pair diagnostics
// (m drops out of KL_i = sab / sa - log sa + log sb, so no large terms cancel).  The 8 partial states of a row are merged by a butterfly;
// lane cl = 0 writes the row, so the order of the merges is fixed.
// Per row: KL, log sa, m, log sb, H(p), H(q), count, confused count, sum of d over confused / non-confused pairs (confused: d_ref < 1 - 1e-6).
// evt_reduce_kernel then sums the rows of a segment in a fixed order in f64.
//
// Backward: the same tiling, recomputing d.  With c_i = up_s w[idx_i] active_i / W_s:  G_ij = -c_i (q_ij - p_ij) / tau_learned and
//   d e_i = sum_j (G_ij + G_ji) (e_i - e_j) / d_ij        (0 where d_ij = 0: torch.cdist's convention, as in soft_neighborhood.hip)
// The owner of row i forms G_ji itself from row j's saved log-sum-exps and S[idx_j][idx_i] (the transposed entry: S is not symmetric), so a
// gradient row is written once, by one workgroup, in a fixed order: no float atomics, bit-identical from run to run.
#include "frl_common.hpp"
#include "frl_host.hpp"
#include "frl_loss.hpp"
#include <math.h>
#include <stdio.h>

#define EV_TR 32                                                 // rows per workgroup
#define EV_TC 64                                                  // columns per LDS tile
#define EV_CL 8                                                   // lanes per row; a lane takes EV_TC / EV_CL = 8 columns of a tile
#define EV_HP (EV_TC + 1)                                         // pitch of the backward's coefficient tile
#define EV_MAX_D 256
enum { EV_KL = 0, EV_LSEA, EV_MB, EV_LOGSB, EV_HP_ENT, EV_HQ_ENT, EV_CNT, EV_NCF, EV_DCF, EV_DNC, EV_NROW };     // columns of rowstat [N][10]
enum { EV_NSEG = 12 };                                            // doubles per segment in segstat

__device__ __forceinline__ int ev_code(int v, int K) { return (v < 0 || v >= K) ? -1 : v; }

// rows [first, first + n) of emb -> dst [rows][pitch], zeros beyond n; the tile's code indices -> didx
template <typename T>
__device__ __forceinline__ void ev_stage(float* __restrict__ dst, int* __restrict__ didx, int rows, int pitch, const T* __restrict__ emb,
                                         const int* __restrict__ idx, int64_t first, int n, int D, int K) {
  for (int i = threadIdx.x; i < rows * D; i += 256) {
    const int t = i / D, c = i - t * D;
    dst[t * pitch + c] = t < n ? to_f32(emb[(first + t) * (int64_t)D + c]) : 0.f;
  }
  if ((int)threadIdx.x < rows) didx[threadIdx.x] = (int)threadIdx.x < n ? ev_code(idx[first + threadIdx.x], K) : -1;
}

// |er - ec_k|_2 for the lane's 8 columns (ec = the first, the others 8 tile rows apart)
__device__ __forceinline__ void ev_dist(const float* __restrict__ er, const float* __restrict__ ec, int pitch, int D, float* __restrict__ d) {
  float s[8], lo[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = lo[k] = 0.f;
  for (int c0 = 0; c0 < D; c0 += 16) {
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    const int c1 = c0 + 16 < D ? c0 + 16 : D;
    for (int c = c0; c < c1; ++c) {
      const float a = er[c];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float df = a - ec[k * EV_CL * pitch + c];
        acc[k] = fmaf(df, df, acc[k]);
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {                                 // two-sum of the chunk into (s, lo)
      const float n = s[k] + acc[k], bp = n - s[k];
      lo[k] += (s[k] - (n - bp)) + (acc[k] - bp);
      s[k] = n;
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) d[k] = sqrtf(s[k] + lo[k]);
}

struct EvState { float m, sb, sbb, sa, saa, sab, cnt, ncf, dcf, dnc; };

// the state of x and y's columns together.  After the butterfly every lane of a row holds the merge of all eight (the compiler may
// contract the two-product sums differently for the two operand orders, so lanes can differ in the last bit: lane cl = 0 alone writes)
__device__ __forceinline__ EvState ev_merge(const EvState& x, const EvState& y) {
  EvState o;
  o.m = fmaxf(x.m, y.m);
  const float dx = x.cnt > 0.f ? o.m - x.m : 0.f, dy = y.cnt > 0.f ? o.m - y.m : 0.f;
  const float ex = expf(-dx), ey = expf(-dy);
  o.sb = x.sb * ex + y.sb * ey;
  o.sbb = (x.sbb - dx * x.sb) * ex + (y.sbb - dy * y.sb) * ey;
  o.sab = (x.sab + dx * x.sa) + (y.sab + dy * y.sa);
  o.sa = x.sa + y.sa;
  o.saa = x.saa + y.saa;
  o.cnt = x.cnt + y.cnt;
  o.ncf = x.ncf + y.ncf;
  o.dcf = x.dcf + y.dcf;
  o.dnc = x.dnc + y.dnc;
  return o;
}

template <typename T>
__global__ __launch_bounds__(256) void evt_fwd_kernel(const T* __restrict__ emb, int D, const int* __restrict__ idx, const float* __restrict__ S,
                                                      int K, const int* __restrict__ seg, float itr, float itl, float* __restrict__ rowstat,
                                                      int* __restrict__ flag) {
  extern __shared__ float ev_lds[];
  __shared__ int ridx[EV_TR], cidx[EV_TC];
  const int s0 = seg[blockIdx.y], len = seg[blockIdx.y + 1] - s0, r0 = blockIdx.x * EV_TR;
  if (r0 >= len) return;
  const int pitch = D | 1, nr = len - r0 < EV_TR ? len - r0 : EV_TR;
  float* Er = ev_lds;
  float* Ec = ev_lds + EV_TR * pitch;
  const int r = threadIdx.x / EV_CL, cl = threadIdx.x % EV_CL;
  ev_stage(Er, ridx, EV_TR, pitch, emb, idx, (int64_t)s0 + r0, nr, D, K);
  if ((int)threadIdx.x < nr && flag != nullptr && idx[s0 + r0 + threadIdx.x] >= K) *flag = 1;
  const float confused_below = (float)(1.0 - 1e-6);
  EvState st = {-INFINITY, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int c0 = 0; c0 < len; c0 += EV_TC) {
    __syncthreads();                                              // the previous tile is consumed (first pass: the rows are staged)
    ev_stage(Ec, cidx, EV_TC, pitch, emb, idx, (int64_t)s0 + c0, len - c0 < EV_TC ? len - c0 : EV_TC, D, K);
    __syncthreads();
    const int ii = ridx[r];
    if (ii < 0) continue;
    float d[8];
    ev_dist(Er + r * pitch, Ec + cl * pitch, pitch, D, d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int cj = cidx[cl + EV_CL * k];
      if (cj < 0 || cj == ii) continue;
      const float dref = 1.f - S[(int64_t)ii * K + cj];
      const float a = -dref * itr, b = -d[k] * itl, ea = expf(a);
      if (b > st.m) {                                             // a new maximum: re-base the sums kept relative to it
        if (st.cnt > 0.f) {
          const float dm = b - st.m, e = expf(-dm);
          st.sbb = (st.sbb - dm * st.sb) * e;
          st.sb *= e;
          st.sab = fmaf(dm, st.sa, st.sab);
        }
        st.m = b;
      }
      const float u = b - st.m, eu = expf(u);
      st.sb += eu;
      st.sbb = fmaf(eu, u, st.sbb);
      st.sa += ea;
      st.saa = fmaf(ea, a, st.saa);
      st.sab = fmaf(ea, a - u, st.sab);
      st.cnt += 1.f;
      if (dref < confused_below) { st.ncf += 1.f; st.dcf += d[k]; } else st.dnc += d[k];
    }
  }
#pragma unroll
  for (int o = 1; o < EV_CL; o <<= 1) {
    EvState y;
    y.m = __shfl_xor(st.m, o, 64);     y.sb = __shfl_xor(st.sb, o, 64);   y.sbb = __shfl_xor(st.sbb, o, 64);
    y.sa = __shfl_xor(st.sa, o, 64);   y.saa = __shfl_xor(st.saa, o, 64); y.sab = __shfl_xor(st.sab, o, 64);
    y.cnt = __shfl_xor(st.cnt, o, 64); y.ncf = __shfl_xor(st.ncf, o, 64); y.dcf = __shfl_xor(st.dcf, o, 64);
    y.dnc = __shfl_xor(st.dnc, o, 64);
    st = ev_merge(st, y);
  }
  if (cl == 0 && r < nr) {
    float* rs = rowstat + ((int64_t)s0 + r0 + r) * EV_NROW;
    const bool active = st.cnt >= 2.f;
    const float lsa = active ? logf(st.sa) : 0.f, lsb = active ? logf(st.sb) : 0.f;
    rs[EV_KL] = active ? st.sab / st.sa - lsa + lsb : 0.f;
    rs[EV_LSEA] = lsa;
    rs[EV_MB] = active ? st.m : 0.f;
    rs[EV_LOGSB] = lsb;
    rs[EV_HP_ENT] = active ? lsa - st.saa / st.sa : 0.f;
    rs[EV_HQ_ENT] = active ? lsb - st.sbb / st.sb : 0.f;
    rs[EV_CNT] = st.cnt;
    rs[EV_NCF] = st.ncf;
    rs[EV_DCF] = st.dcf;
    rs[EV_DNC] = st.dnc;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// rows -> segment.  One workgroup of 256 threads per segment: rows strided over the threads (f64 partials), butterfly per wave, the 4 wave
// sums added in order.  segout [nseg][2] = loss, W (the active rows' weight; 0 = the segment contributes nothing, which the backward reads);
// segstat [nseg][12] f64 = loss, live, valid anchors, active rows, sum H(p), sum H(q), confused pairs of active rows, confused pairs,
// sum d over confused pairs, sum d over the other pairs, the other pairs, W.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void evt_reduce_kernel(const float* __restrict__ rowstat, const int* __restrict__ idx, const float* __restrict__ w,
                                                         int K, const int* __restrict__ seg, int min_valid, float* __restrict__ segout,
                                                         double* __restrict__ segstat) {
  __shared__ double red[4][11];
  const int s0 = seg[blockIdx.x], len = seg[blockIdx.x + 1] - s0;
  double s[11];                                                   // sum w kl | sum w | valid | active | H(p) | H(q) | ncf active | ncf | dcf | dnc | nnc
#pragma unroll
  for (int k = 0; k < 11; ++k) s[k] = 0.0;
  for (int i = threadIdx.x; i < len; i += 256) {
    const int v = ev_code(idx[s0 + i], K);
    if (v < 0) continue;
    const float* rs = rowstat + ((int64_t)s0 + i) * EV_NROW;
    const double cnt = rs[EV_CNT], ncf = rs[EV_NCF];
    s[2] += 1.0;
    s[7] += ncf;
    s[8] += (double)rs[EV_DCF];
    s[9] += (double)rs[EV_DNC];
    s[10] += cnt - ncf;
    if (cnt >= 2.0) {
      const double wi = w[v];
      s[0] += wi * (double)rs[EV_KL];
      s[1] += wi;
      s[3] += 1.0;
      s[4] += (double)rs[EV_HP_ENT];
      s[5] += (double)rs[EV_HQ_ENT];
      s[6] += ncf;
    }
  }
  block_sum_d<11, 4>(s, red);
  if (threadIdx.x == 0) {
    const double W = red[0][1];
    const bool live = red[0][2] >= (double)min_valid && W > 0.0;
    const float loss = live ? (float)(red[0][0] / W) : 0.f;
    segout[2 * blockIdx.x] = loss;
    segout[2 * blockIdx.x + 1] = live ? (float)W : 0.f;
    double* o = segstat + (int64_t)blockIdx.x * EV_NSEG;
    o[0] = (double)loss;
    o[1] = live ? 1.0 : 0.0;
    for (int k = 2; k < 11; ++k) o[k] = red[0][k];
    o[11] = W;
  }
}

// c_i = up w[idx_i] / W for an active row of a live segment, else 0
__device__ __forceinline__ float ev_coef(int code, const float* __restrict__ rs, const float* __restrict__ w, float up, float W) {
  return (code >= 0 && rs[EV_CNT] >= 2.f) ? up * (w[code] / W) : 0.f;
}

template <typename T>
__global__ __launch_bounds__(256) void evt_bwd_kernel(const T* __restrict__ emb, int D, const int* __restrict__ idx, const float* __restrict__ S,
                                                      const float* __restrict__ w, int K, const int* __restrict__ seg, float itr, float itl,
                                                      const float* __restrict__ rowstat, const float* __restrict__ segout,
                                                      const float* __restrict__ gup, const float* __restrict__ segw, T* __restrict__ grad) {
  extern __shared__ float ev_lds[];
  __shared__ int ridx[EV_TR], cidx[EV_TC];
  __shared__ float ccoef[EV_TC], clsa[EV_TC], cmb[EV_TC], clsb[EV_TC];
  const int s0 = seg[blockIdx.y], len = seg[blockIdx.y + 1] - s0, r0 = blockIdx.x * EV_TR;
  if (r0 >= len) return;
  const int pitch = D | 1, nr = len - r0 < EV_TR ? len - r0 : EV_TR;
  float* Er = ev_lds;
  float* Ec = Er + EV_TR * pitch;
  float* G = Ec + EV_TC * pitch;
  float* H = G + EV_TR * pitch;
  const int r = threadIdx.x / EV_CL, cl = threadIdx.x % EV_CL;
  const float W = segout[2 * blockIdx.y + 1], up = gup[blockIdx.y] * (segw != nullptr ? segw[blockIdx.y] : 1.f);
  T* grow = grad + ((int64_t)s0 + r0) * D;
  if (!(W > 0.f)) {                                               // the segment contributes nothing: zero rows
    for (int i = threadIdx.x; i < nr * D; i += 256) grow[i] = from_f32<T>(0.f);
    return;
  }
  ev_stage(Er, ridx, EV_TR, pitch, emb, idx, (int64_t)s0 + r0, nr, D, K);
  for (int i = threadIdx.x; i < EV_TR * pitch; i += 256) G[i] = 0.f;
  __syncthreads();
  const int ii = ridx[r];
  const float* rsi = rowstat + ((int64_t)s0 + r0 + (r < nr ? r : 0)) * EV_NROW;
  const float ci = ev_coef(ii, rsi, w, up, W), lsa_i = rsi[EV_LSEA], mb_i = rsi[EV_MB], lsb_i = rsi[EV_LOGSB];
  for (int c0 = 0; c0 < len; c0 += EV_TC) {
    const int nc = len - c0 < EV_TC ? len - c0 : EV_TC;
    __syncthreads();                                              // the previous tile is consumed
    ev_stage(Ec, cidx, EV_TC, pitch, emb, idx, (int64_t)s0 + c0, nc, D, K);
    if ((int)threadIdx.x < EV_TC) {
      const int j = threadIdx.x;
      const float* rs = rowstat + ((int64_t)s0 + c0 + (j < nc ? j : 0)) * EV_NROW;
      ccoef[j] = j < nc ? ev_coef(ev_code(idx[s0 + c0 + j], K), rs, w, up, W) : 0.f;
      clsa[j] = rs[EV_LSEA];
      cmb[j] = rs[EV_MB];
      clsb[j] = rs[EV_LOGSB];
    }
    __syncthreads();
    float d[8];
    if (ii >= 0) ev_dist(Er + r * pitch, Ec + cl * pitch, pitch, D, d);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int j = cl + EV_CL * k, cj = cidx[j];
      float h = 0.f;
      if (ii >= 0 && cj >= 0 && cj != ii && d[k] > 0.f) {
        const float b = -d[k] * itl, cjc = ccoef[j];
        float g = 0.f;
        if (ci != 0.f) {
          const float a = -(1.f - S[(int64_t)ii * K + cj]) * itr;
          g = ci * (expf((b - mb_i) - lsb_i) - expf(a - lsa_i));
        }
        if (cjc != 0.f) {                                         // G_ji: row j's distribution, the transposed entry of S
          const float a = -(1.f - S[(int64_t)cj * K + ii]) * itr;
          g = fmaf(cjc, expf((b - cmb[j]) - clsb[j]) - expf(a - clsa[j]), g);
        }
        h = -itl * g / d[k];
      }
      H[r * EV_HP + j] = h;
    }
    __syncthreads();
    for (int c = cl; c < D; c += EV_CL) {                         // element (r, c) of G belongs to this thread alone
      const float er = Er[r * pitch + c];
      float s = 0.f;
      for (int j = 0; j < nc; ++j) s = fmaf(H[r * EV_HP + j], er - Ec[j * pitch + c], s);
      G[r * pitch + c] += s;
    }
  }
  if (r < nr)
    for (int c = cl; c < D; c += EV_CL) grow[r * D + c] = from_f32<T>(G[r * pitch + c]);
}

static size_t ev_lds_bytes(int D, bool bwd) {
  const size_t pitch = (size_t)(D | 1);
  return sizeof(float) * (bwd ? (2 * EV_TR + EV_TC) * pitch + EV_TR * EV_HP : (EV_TR + EV_TC) * pitch);
}

// host-side validation: sizes, and the segment offsets (a host copy: 0 = seg[0] <= seg[1] <= .. <= seg[nseg] = N) -> the longest segment
static int ev_check(const char* what, const void* emb, int dtype, int64_t N, int D, const int* idx, const float* S, const float* w, int K,
                    const int* seg, const int* seg_host, int nseg, float itr, float itl, int* maxlen) {
  static thread_local char msg[160];
  const char* err = nullptr;
  if (!emb || !idx || !S || !w || !seg || !seg_host) err = "NULL argument";
  else if (dtype != FRL_F32 && dtype != FRL_BF16) err = "emb dtype must be FRL_F32 or FRL_BF16";
  else if (D < 1 || D > EV_MAX_D) err = "supports 1 <= D <= 256";
  else if (N < 1 || N > 0x7fffffff) err = "needs 1 <= N < 2^31 rows";
  else if (K < 1) err = "needs K >= 1 codes";
  else if (nseg < 1 || nseg > 65535) err = "needs 1 <= segments <= 65535";
  else if (!(itr > 0.f) || !(itl > 0.f)) err = "temperatures must be positive";
  else {
    *maxlen = 0;
    if (seg_host[0] != 0 || (int64_t)seg_host[nseg] != N) err = "segment offsets must start at 0 and end at N";
    for (int s = 0; s < nseg && !err; ++s) {
      const int len = seg_host[s + 1] - seg_host[s];
      if (len < 0) err = "segment offsets must not decrease";
      else if (len > *maxlen) *maxlen = len;
    }
  }
  if (!err) return 0;
  snprintf(msg, sizeof(msg), "%s: %s", what, err);
  return frl_fail(-2, msg);
}

template <typename T>
static int ev_launch_fwd(const void* emb, int D, const int* idx, const float* S, int K, const int* seg, int nseg, int maxlen, float itr, float itl,
                         float* rowstat, int* flag, hipStream_t st) {
  auto kern = evt_fwd_kernel<T>;
  const size_t lds = ev_lds_bytes(D, false);
  if (lds > 48 * 1024) FRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const unsigned tiles = (unsigned)((maxlen + EV_TR - 1) / EV_TR);
  FRL_LAUNCH_AS("evt_fwd_kernel", kern, dim3(tiles < 1 ? 1 : tiles, (unsigned)nseg), dim3(256), lds, st, (const T*)emb, D, idx, S, K, seg, itr, itl,
                rowstat, flag);
  return 0;
}

template <typename T>
static int ev_launch_bwd(const void* emb, int D, const int* idx, const float* S, const float* w, int K, const int* seg, int nseg, int maxlen,
                         float itr, float itl, const float* rowstat, const float* segout, const float* gup, const float* segw, void* grad,
                         hipStream_t st) {
  auto kern = evt_bwd_kernel<T>;
  const size_t lds = ev_lds_bytes(D, true);
  if (lds > 48 * 1024) FRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const unsigned tiles = (unsigned)((maxlen + EV_TR - 1) / EV_TR);
  FRL_LAUNCH_AS("evt_bwd_kernel", kern, dim3(tiles < 1 ? 1 : tiles, (unsigned)nseg), dim3(256), lds, st, (const T*)emb, D, idx, S, w, K, seg, itr,
                itl, rowstat, segout, gup, segw, (T*)grad);
  return 0;
}

extern "C" {

// emb [N][D] (dtype 0 = float32, 1 = bfloat16), idx [N] int32 (-1 = unknown; >= K is treated as unknown and sets *flag, NULL = not
// wanted), S [K][K], w [K], seg [nseg + 1] int32 on the device and the same offsets on the host (validated there), inv_tau_* = 1 /
// temperature.  Outputs: rowstat [N][10], segout [nseg][2] = loss, W, segstat [nseg][12] f64 (see evt_reduce_kernel).
int frl_evt_soft_nbr_fwd(const void* emb, int emb_dtype, int64_t N, int D, const int* idx, const float* S, const float* w, int K, const int* seg,
                         const int* seg_host, int nseg, float inv_tau_ref, float inv_tau_learned, int min_valid_anchors, float* rowstat,
                         float* segout, double* segstat, int* flag, hipStream_t stream) {
  int maxlen = 0;
  int rc = ev_check("evt_soft_nbr_fwd", emb, emb_dtype, N, D, idx, S, w, K, seg, seg_host, nseg, inv_tau_ref, inv_tau_learned, &maxlen);
  if (rc) return rc;
  if (!rowstat || !segout || !segstat) return frl_fail(-2, "evt_soft_nbr_fwd: NULL argument");
  FRL_BY_DTYPE(emb_dtype, T, rc = ev_launch_fwd<T>(emb, D, idx, S, K, seg, nseg, maxlen, inv_tau_ref, inv_tau_learned, rowstat, flag, stream));
  if (rc) return rc;
  FRL_LAUNCH(evt_reduce_kernel, dim3((unsigned)nseg), dim3(256), 0, stream, (const float*)rowstat, idx, w, K, seg, min_valid_anchors, segout,
             segstat);
  return frl_check_launch("evt_soft_nbr_fwd");
}

// grad [N][D] in emb's dtype = sum over segments of gup[s] * seg_weights[s] (NULL = 1) * d loss_s / d emb, every row written once.
int frl_evt_soft_nbr_bwd(const void* emb, int emb_dtype, int64_t N, int D, const int* idx, const float* S, const float* w, int K, const int* seg,
                         const int* seg_host, int nseg, float inv_tau_ref, float inv_tau_learned, const float* rowstat, const float* segout,
                         const float* gup, const float* seg_weights, void* grad, hipStream_t stream) {
  int maxlen = 0;
  int rc = ev_check("evt_soft_nbr_bwd", emb, emb_dtype, N, D, idx, S, w, K, seg, seg_host, nseg, inv_tau_ref, inv_tau_learned, &maxlen);
  if (rc) return rc;
  if (!rowstat || !segout || !gup || !grad) return frl_fail(-2, "evt_soft_nbr_bwd: NULL argument");
  FRL_BY_DTYPE(emb_dtype, T, rc = ev_launch_bwd<T>(emb, D, idx, S, w, K, seg, nseg, maxlen, inv_tau_ref, inv_tau_learned, rowstat, segout, gup,
                                                   seg_weights, grad, stream));
  if (rc) return rc;
  return frl_check_launch("evt_soft_nbr_bwd");
}

}  // extern "C"
