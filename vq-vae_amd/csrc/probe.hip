// Closed-form linear probes (the reference's frl/training/fit_linear_probe.py and fit_phase_linear_probe.py): streamed masked moments
// for a ridge fit, and a fused prediction + error-sum pass.
//
// An observation is (b, t, p): sample, timestep, pixel.  Its feature columns come from one or two row-major float32 sources
// A [B][Ta][P][Da], Bs [B][Tb][P][Db] (T_s = 1: the row is shared by all t), its targets from Y [B][Ty][P][Cy], and mask [B][P] (uint8,
// shared over t) says whether it counts.  With v = [x - p_x | y - p_y | m] (p: a fixed pivot near the column means, subtracted in
// float32; the whole row is zero where m = 0) one product v^T v holds everything a ridge fit needs: the scatter, the column sums and,
// in its last entry, the count.  frl_probe_accumulate forms it by the staged-tile scheme of frl_moments.hpp over tiles of 64 consecutive
// pixels of one (b, t), the product being the 16 x 16 blocks of the upper triangle (exact float32, an fmaf chain in row order).  A tile
// whose 64 mask bytes are zero is skipped before anything of it is read.  The slabs are added in the order of moment_slab_sum into the
// running state, which is then mirrored.  The count is a sum of popcounts in int64.  No float atomics: two runs give the same bits.
// frl_probe_pivot forms the masked column means the same way (tiles staged in LDS, column sums in double, workgroups added in a
// fixed order).  frl_probe_evaluate stages the tile with the next one's loads already in registers, gives lane = pixel and
// wave = targets w, w + 4, .., and runs pred = bc + (x - p) Wc as a float32 fmaf chain in d order with SSE, sum (y - q) and
// sum (y - q)^2 in double per lane.
#include "probe_common.hpp"

#define PROBE_PIVOT_WG 1024
#define PROBE_EVAL_WG 1024

namespace {

struct ProbeDims {
  int D, C, C1, CB, ys, nblk, slabF;
  size_t lds;
};

ProbeDims probe_dims(int D, int Cy) {
  ProbeDims g;
  g.D = D;
  g.C = D + Cy;
  g.C1 = g.C + 1;
  g.CB = (g.C1 + 15) / 16;
  const int ys = g.ys = frl_tile_stride(16 * g.CB);
  g.nblk = g.CB * (g.CB + 1) / 2;
  g.slabF = g.nblk * 256;
  g.lds = sizeof(float) * ((size_t)MOMENT_ROWS * ys + 16 * g.CB);
  return g;
}

int probe_acc_grid(int64_t ntiles, const ProbeDims& g, int workgroups) {
  if (workgroups > 0) return workgroups;
  const int64_t cap = g.nblk <= 16 ? 1024 : 512;
  return (int)(ntiles < cap ? ntiles : cap);
}

}  // namespace

// block b of the upper triangle, rows first: (0,0) (0,1) .. (0,CB-1) (1,1) ..
__device__ __forceinline__ void probe_block(int b, int CB, int& ib, int& jb) {
  ib = 0;
  while (b >= CB - ib) {
    b -= CB - ib;
    ++ib;
  }
  jb = ib + b;
}

// A tile on its way from memory to LDS in the pivot and evaluate kernels.  Where every feature source is rows of whole, 16-byte
// aligned float4 (q.fast) the loads of a tile are issued into registers together (probe_fetch), in the evaluate kernel while the
// previous tile is still being consumed, and written to LDS later (probe_commit); elsewhere probe_commit stages straight from memory.
// (The accumulate kernel stages straight from memory at five waves per SIMD: with the prefetch registers it fits two, and measured
// 220 us against 145 us at 16 x 256 x 256, D = 64.)  Chunk c < nA = ceil(Da / 16) is float4 number tid + 256 c of
// A's part of the tile, the chunks after it are Bs's: ceil(Da / 16) + ceil(Db / 16) <= 9 for Da + Db <= 128.
#define PROBE_CHUNKS 9
struct ProbeRegs {
  f32x4 v[PROBE_CHUNKS];
  float y[4];
  unsigned long long rows, live;                                                 // unmasked pixels; pixels that are staged
  int b, t, p0;
};

// where a thread's chunks sit, the same for every tile: row of the tile (-1: no such chunk), offset in the source's part of the
// tile, offset in LDS
struct ProbeMap {
  int row[PROBE_CHUNKS], goff[PROBE_CHUNKS], loff[PROBE_CHUNKS];
  int yrow[4], yloff[4];
  int nA;
};

__device__ __forceinline__ void probe_map(const ProbeIn& q, int ys, int tid, ProbeMap& M) {
  const int qa = q.Da >> 2, qb = q.Db >> 2;
  M.nA = (q.Da + 15) >> 4;
#pragma unroll
  for (int c = 0; c < PROBE_CHUNKS; ++c) {
    const bool isA = c < M.nA;
    const int qq = isA ? qa : qb, e = tid + 256 * (isA ? c : c - M.nA);
    M.row[c] = -1;
    M.goff[c] = M.loff[c] = 0;
    if (q.fast && e < MOMENT_ROWS * qq) {
      const int row = e / qq, c4 = e - row * qq;
      M.row[c] = row;
      M.goff[c] = row * 4 * qq + 4 * c4;
      M.loff[c] = row * ys + (isA ? 0 : q.Da) + 4 * c4;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = tid + 256 * j;
    M.yrow[j] = -1;
    M.yloff[j] = 0;
    if (q.fast && e < MOMENT_ROWS * q.Cy) {
      const int row = e / q.Cy;
      M.yrow[j] = row;
      M.yloff[j] = row * ys + q.Da + q.Db + (e - row * q.Cy);
    }
  }
}

__device__ __forceinline__ void probe_fetch(const ProbeIn& q, const ProbeMap& M, int tile, int tid, int lane, bool all, ProbeRegs& R) {
  moment_tile(tile, q.PT, q.T, R.b, R.t, R.p0);
  R.rows = probe_mask_bits(q, R.b, R.p0, lane);
  const int valid = moment_tile_rows(q.P, R.p0);
  R.live = all ? (valid == MOMENT_ROWS ? ~0ull : (1ull << valid) - 1ull) : R.rows;
  if (R.live == 0ull || !q.fast) return;
  const float* baseA = q.A + ((size_t)((int64_t)R.b * q.Ta + (q.Ta > 1 ? R.t : 0)) * q.P + R.p0) * q.Da;
  const float* baseB = q.Db ? q.Bs + ((size_t)((int64_t)R.b * q.Tb + (q.Tb > 1 ? R.t : 0)) * q.P + R.p0) * q.Db : baseA;
  const float* baseY = q.Y + ((size_t)((int64_t)R.b * q.Ty + (q.Ty > 1 ? R.t : 0)) * q.P + R.p0) * q.Cy;
#pragma unroll
  for (int c = 0; c < PROBE_CHUNKS; ++c) {
    R.v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (M.row[c] >= 0 && ((R.live >> M.row[c]) & 1ull)) R.v[c] = *reinterpret_cast<const f32x4*>((c < M.nA ? baseA : baseB) + M.goff[c]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    R.y[j] = 0.f;
    if (M.yrow[j] >= 0 && ((R.live >> M.yrow[j]) & 1ull)) R.y[j] = baseY[tid + 256 * j];
  }
}

// VEC: the LDS row stride is a multiple of 4 floats.  centre_y: targets minus their pivot (accumulate) or as they are (evaluate).
template <bool VEC>
__device__ __forceinline__ void probe_commit(const ProbeIn& q, const ProbeMap& M, const ProbeRegs& R, float* vt, int ys, const float* piv,
                                             bool centre_x, bool centre_y, int tid) {
  const int D = q.Da + q.Db;
  if (!q.fast) {
    probe_stage(vt, ys, piv, q.A, q.Ta, q.Da, 0, false, centre_x, q, R.b, R.t, R.p0, R.live, tid);
    if (q.Db) probe_stage(vt, ys, piv, q.Bs, q.Tb, q.Db, q.Da, false, centre_x, q, R.b, R.t, R.p0, R.live, tid);
    probe_stage(vt, ys, piv, q.Y, q.Ty, q.Cy, D, false, centre_y, q, R.b, R.t, R.p0, R.live, tid);
    return;
  }
#pragma unroll
  for (int c = 0; c < PROBE_CHUNKS; ++c) {
    if (M.row[c] >= 0) {
      f32x4 v = R.v[c];
      if (centre_x && ((R.live >> M.row[c]) & 1ull)) {
        const float* pp = piv + (M.loff[c] - M.row[c] * ys);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] -= pp[j];
      }
      if (VEC) *reinterpret_cast<f32x4*>(vt + M.loff[c]) = v;
      else {
#pragma unroll
        for (int j = 0; j < 4; ++j) vt[M.loff[c] + j] = v[j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (M.yrow[j] >= 0) {
      float v = R.y[j];
      if (centre_y && ((R.live >> M.yrow[j]) & 1ull)) v -= piv[M.yloff[j] - M.yrow[j] * ys];
      vt[M.yloff[j]] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the pivot: masked column means of [x | y] of one call.  A tile is staged as it is; wave w adds rows 16 w .. 16 w + 15 of columns
// lane, lane + 64, lane + 128 in double, tile after tile; the waves, then the workgroups, are added in a fixed order
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void probe_pivot_partial_kernel(ProbeIn q, int ys, double* __restrict__ part, long long* __restrict__ cnts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double wsum[4][192];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int C = q.Da + q.Db + q.Cy;
  float* vt = reinterpret_cast<float*>(smem);                                    // [64][ys]
  double s[3] = {0.0, 0.0, 0.0};
  long long cnt = 0;
  ProbeRegs R;
  ProbeMap M;
  probe_map(q, ys, tid, M);
  for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
    probe_fetch(q, M, tile, tid, lane, false, R);
    if (R.live == 0ull) continue;                                                // uniform
    cnt += __popcll(R.rows);
    __syncthreads();
    probe_commit<true>(q, M, R, vt, ys, nullptr, false, false, tid);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int c = lane + 64 * k;
      if (c < C) {
        const float* col = vt + (wave * 16) * ys + c;
#pragma unroll 4
        for (int r = 0; r < 16; ++r) s[k] += (double)col[r * ys];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) wsum[wave][lane + 64 * k] = s[k];
  __syncthreads();
  if (tid < C) part[(size_t)blockIdx.x * C + tid] = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
  if (tid == 0) cnts[blockIdx.x] = cnt;
}

__global__ __launch_bounds__(1024) void probe_pivot_final_kernel(const double* __restrict__ part, const long long* __restrict__ cnts, int G, int C,
                                                                 float* __restrict__ pivot) {
  __shared__ double ps[4][256];
  __shared__ long long pc[1024];
  const int c = threadIdx.x & 255, p = threadIdx.x >> 8;
  double s = 0.0;
  if (c < C) {
#pragma unroll 8
    for (int g = p; g < G; g += 4) s += part[(size_t)g * C + c];
  }
  ps[p][c] = s;
  long long n = 0;
  for (int g = threadIdx.x; g < G; g += 1024) n += cnts[g];
  pc[threadIdx.x] = n;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) pc[threadIdx.x] += pc[threadIdx.x + o];
    __syncthreads();
  }
  if (p == 0 && c < C) pivot[c] = pc[0] > 0 ? (float)((((ps[0][c] + ps[1][c]) + ps[2][c]) + ps[3][c]) / (double)pc[0]) : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// accumulate.  NBM: blocks of the upper triangle per wave.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int NBM>
__global__ __launch_bounds__(256, (NBM <= 4 ? 4 : NBM <= 8 ? 3 : 2)) void probe_acc_kernel(ProbeIn q, int ys, int CB, float* __restrict__ slabs,
                                                                              long long* __restrict__ cnts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lg = lane >> 4;
  const int D = q.Da + q.Db, C = D + q.Cy, nblk = CB * (CB + 1) / 2;
  float* vt = reinterpret_cast<float*>(smem);                                    // [64][ys]
  float* piv = vt + MOMENT_ROWS * ys;                                            // [16 CB]
  for (int d = tid; d < 16 * CB; d += 256) piv[d] = d < C ? q.pivot[d] : 0.f;
  for (int i = tid; i < MOMENT_ROWS * ys; i += 256) vt[i] = 0.f;                 // the padding columns stay zero

  f32x4 acc[NBM];
  int oa[NBM], ob[NBM];
#pragma unroll
  for (int i = 0; i < NBM; ++i) {
    acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    int ib = 0, jb = 0;
    if (wave + 4 * i < nblk) probe_block(wave + 4 * i, CB, ib, jb);
    oa[i] = lg * ys + ib * 16 + lr;
    ob[i] = lg * ys + jb * 16 + lr;
  }
  long long cnt = 0;

  for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
    int b, t, p0;
    moment_tile(tile, q.PT, q.T, b, t, p0);
    const unsigned long long rows = probe_mask_bits(q, b, p0, lane);
    if (rows == 0ull) continue;                                                  // uniform: every wave sees the same 64 mask bytes
    cnt += __popcll(rows);
    __syncthreads();                                                             // the previous tile is consumed (and the prologue is written)
    probe_stage(vt, ys, piv, q.A, q.Ta, q.Da, 0, q.fast, true, q, b, t, p0, rows, tid);
    if (q.Db) probe_stage(vt, ys, piv, q.Bs, q.Tb, q.Db, q.Da, q.fast, true, q, b, t, p0, rows, tid);
    probe_stage(vt, ys, piv, q.Y, q.Ty, q.Cy, D, false, true, q, b, t, p0, rows, tid);
    if (tid < MOMENT_ROWS) vt[tid * ys + C] = (rows >> tid) & 1ull ? 1.f : 0.f;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NBM; ++i) {
      if (wave + 4 * i < nblk) {
        const float* ap = vt + oa[i];
        const float* bp = vt + ob[i];
#pragma unroll 4
        for (int st = 0; st < MOMENT_ROWS / 4; ++st) acc[i] = mfma16(ap[4 * st * ys], bp[4 * st * ys], acc[i]);
      }
    }
  }
  moment_store_slab<NBM>(slabs + (size_t)blockIdx.x * nblk * 256, acc, wave, lane, nblk);
  if (tid == 0) cnts[blockIdx.x] = cnt;
}

// the slabs added in double (moment_slab_sum), 64 elements per workgroup, into S [C1][C1] (both triangles); workgroup 0 adds the count
__global__ __launch_bounds__(256) void probe_acc_reduce_kernel(const float* __restrict__ slabs, const long long* __restrict__ cnts, int G, int CB,
                                                               int C1, double* __restrict__ S, long long* __restrict__ n) {
  __shared__ long long pc[256];
  const int slabF = CB * (CB + 1) / 2 * 256, e = blockIdx.x * 64 + (threadIdx.x & 63);
  if (blockIdx.x == 0) {
    long long c = 0;
    for (int g = threadIdx.x; g < G; g += 256) c += cnts[g];
    pc[threadIdx.x] = c;
  }
  const double sum = moment_slab_sum(slabs, G, slabF, e, true);                  // its barrier covers pc too
  if (threadIdx.x < 64) {
    int blk, row, col, ib, jb;
    moment_frag_decode(e, blk, row, col);
    probe_block(blk, CB, ib, jb);
    const int i = ib * 16 + row, j = jb * 16 + col;
    if (i <= j && j < C1) {
      const double v = S[(size_t)i * C1 + j] + sum;
      S[(size_t)i * C1 + j] = v;
      S[(size_t)j * C1 + i] = v;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    long long c = 0;
    for (int i = 0; i < 256; ++i) c += pc[i];
    *n += c;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// evaluate: pred_c = bc_c + sum_d (x_d - p_d) Wc_dc as a float32 fmaf chain in d order; lane = pixel of the tile, wave w owns the
// targets c = w, w + 4, ..; sums over unmasked observations in double
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void probe_eval_kernel(ProbeIn q, int ys, const float* __restrict__ Wc, const float* __restrict__ bc, double* __restrict__ dsl,
                                                            long long* __restrict__ cnts, float* __restrict__ pred) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int D = q.Da + q.Db, Cy = q.Cy, C = D + Cy;
  float* Wl = reinterpret_cast<float*>(smem);                                    // [D][4 waves][4]: Wc[d][wave + 4 k], one broadcast read per d
  float* vt = Wl + 16 * D;                                                       // [64][ys]: x - p | y, ys odd
  float* piv = vt + MOMENT_ROWS * ys;                                            // [C]
  for (int i = tid; i < 16 * D; i += 256) {
    const int d = i >> 4, c = ((i >> 2) & 3) + 4 * (i & 3);
    Wl[i] = c < Cy ? Wc[d * Cy + c] : 0.f;
  }
  for (int d = tid; d < C; d += 256) piv[d] = q.pivot[d];
  double sse[4], sy[4], sy2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) sse[k] = sy[k] = sy2[k] = 0.0;
  long long cnt = 0;
  const bool all = pred != nullptr;                                              // every pixel is predicted: no tile is skipped

  ProbeRegs R;
  ProbeMap M;
  probe_map(q, ys, tid, M);
  int tile = blockIdx.x;
  if (tile < q.ntiles) probe_fetch(q, M, tile, tid, lane, all, R);
  while (tile < q.ntiles) {
    const int next = tile + gridDim.x;
    if (R.live == 0ull) {                                                        // uniform
      if (next < q.ntiles) probe_fetch(q, M, next, tid, lane, all, R);
      tile = next;
      continue;
    }
    const unsigned long long rows = R.rows;
    const int b = R.b, t = R.t, p0 = R.p0;
    const int valid = moment_tile_rows(q.P, p0);
    cnt += __popcll(rows);
    __syncthreads();                                                             // the previous tile is consumed (and the prologue is written)
    probe_commit<false>(q, M, R, vt, ys, piv, true, false, tid);
    __syncthreads();
    if (next < q.ntiles) probe_fetch(q, M, next, tid, lane, all, R);                // in flight behind the chain below
    tile = next;
    const float* xr = vt + lane * ys;
    float a[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = wave + 4 * k < Cy ? bc[wave + 4 * k] : 0.f;
    const float* wl = Wl + 4 * wave;
#pragma unroll 4
    for (int d = 0; d < D; ++d) {
      const float xv = xr[d];
      const f32x4 w = *reinterpret_cast<const f32x4*>(wl + 16 * d);
#pragma unroll
      for (int k = 0; k < 4; ++k) a[k] = fmaf(xv, w[k], a[k]);                   // columns beyond Cy carry zeros and are never read
    }
    const bool on = (rows >> lane) & 1ull;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = wave + 4 * k;
      if (c < Cy) {
        if (pred && lane < valid) pred[((size_t)((int64_t)b * q.T + t) * q.P + p0 + lane) * Cy + c] = a[k];
        if (on) {
          const float y = xr[D + c];
          const double er = (double)a[k] - (double)y, yq = (double)y - (double)piv[D + c];
          sse[k] += er * er;
          sy[k] += yq;
          sy2[k] += yq * yq;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = wave + 4 * k;
    if (c < Cy) {
      const double s0 = wave_sum_d(sse[k]), s1 = wave_sum_d(sy[k]), s2 = wave_sum_d(sy2[k]);
      if (lane == 0) {
        double* o = dsl + ((size_t)blockIdx.x * Cy + c) * 3;
        o[0] = s0;
        o[1] = s1;
        o[2] = s2;
      }
    }
  }
  if (tid == 0) cnts[blockIdx.x] = cnt;
}

// E [Cy][3] += the slabs, 16 interleaved parts each in slab order, the parts in order; n += the counts
__global__ __launch_bounds__(1024) void probe_eval_reduce_kernel(const double* __restrict__ dsl, const long long* __restrict__ cnts, int G, int Cy,
                                                                 double* __restrict__ E, long long* __restrict__ n) {
  __shared__ double part[16][64];
  __shared__ long long pc[16];
  const int e = threadIdx.x & 63, p = threadIdx.x >> 6, F = Cy * 3;
  double s = 0.0;
  long long c = 0;
  if (e < F) {
#pragma unroll 8
    for (int g = p; g < G; g += 16) s += dsl[(size_t)g * F + e];
  }
  if (e == 63)
    for (int g = p; g < G; g += 16) c += cnts[g];
  part[p][e] = s;
  if (e == 63) pc[p] = c;
  __syncthreads();
  if (p == 0 && e < F) {
    double v = part[0][e];
    for (int i = 1; i < 16; ++i) v += part[i][e];
    E[e] += v;
  }
  if (p == 0 && e == 63) {
    long long v = 0;
    for (int i = 0; i < 16; ++i) v += pc[i];
    *n += v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

int probe_eval_grid(int64_t ntiles, int workgroups) {
  if (workgroups > 0) return workgroups;
  return (int)(ntiles < PROBE_EVAL_WG ? ntiles : PROBE_EVAL_WG);
}

}  // namespace

void probe_launch_eval_reduce(const double* dsl, const long long* cnts, int G, int Cy, double* E, long long* n, hipStream_t stream) {
  FRL_LAUNCH(probe_eval_reduce_kernel, dim3(1), dim3(1024), 0, stream, dsl, cnts, G, Cy, E, n);
}

extern "C" {

// See include/frl_hip.h.
size_t frl_probe_workspace_bytes(int D, int Cy, int workgroups) {
  if (D < 1 || D > PROBE_MAX_D || Cy < 1 || Cy > PROBE_MAX_CY || !frl_wg_in_range(workgroups)) return 0;
  const ProbeDims g = probe_dims(D, Cy);
  const size_t Ga = workgroups > 0 ? workgroups : (g.nblk <= 16 ? 1024 : 512), Ge = workgroups > 0 ? workgroups : PROBE_EVAL_WG;
  const size_t acc = probe_align16(8 * Ga) + sizeof(float) * Ga * g.slabF;
  const size_t ev = probe_align16(8 * Ge) + sizeof(double) * Ge * Cy * 3;
  const size_t pv = probe_align16(8 * PROBE_PIVOT_WG) + sizeof(double) * PROBE_PIVOT_WG * g.C;
  return acc > ev ? (acc > pv ? acc : pv) : (ev > pv ? ev : pv);
}

int frl_probe_pivot(const float* A, int Ta, int Da, const float* Bs, int Tb, int Db, const float* Y, int Ty, int Cy, const unsigned char* mask,
                    int B, int T, int64_t P, float* pivot, void* ws, size_t ws_bytes, hipStream_t stream) {
  ProbeIn q;
  if (int rc = probe_check("probe_pivot", A, Ta, Da, Bs, Tb, Db, Y, Ty, Cy, mask, B, T, P, q)) return rc;
  if (!pivot) return frl_fail(-2, "probe_pivot: null pointer");
  const int C = Da + Db + Cy;
  const size_t need = probe_align16(8 * PROBE_PIVOT_WG) + sizeof(double) * PROBE_PIVOT_WG * (size_t)C;
  if (int rc = frl_check_workspace("probe_pivot", ws, ws_bytes, need)) return rc;
  long long* cnts = (long long*)ws;
  double* part = (double*)((char*)ws + probe_align16(8 * PROBE_PIVOT_WG));
  const ProbeDims g = probe_dims(Da + Db, Cy);
  const int G = q.ntiles < PROBE_PIVOT_WG ? q.ntiles : PROBE_PIVOT_WG;
  FRL_LAUNCH(probe_pivot_partial_kernel, dim3((unsigned)G), dim3(256), sizeof(float) * MOMENT_ROWS * g.ys, stream, q, g.ys, part, cnts);
  FRL_LAUNCH(probe_pivot_final_kernel, dim3(1), dim3(1024), 0, stream, (const double*)part, (const long long*)cnts, G, C, pivot);
  return frl_check_launch("probe_pivot");
}

int frl_probe_accumulate(const float* A, int Ta, int Da, const float* Bs, int Tb, int Db, const float* Y, int Ty, int Cy,
                         const unsigned char* mask, int B, int T, int64_t P, const float* pivot, int workgroups, double* S, int64_t* n, void* ws,
                         size_t ws_bytes, hipStream_t stream) {
  ProbeIn q;
  if (int rc = probe_check("probe_accumulate", A, Ta, Da, Bs, Tb, Db, Y, Ty, Cy, mask, B, T, P, q)) return rc;
  if (int rc = frl_check_workgroups("probe_accumulate", workgroups)) return rc;
  if (!pivot || !S || !n) return frl_fail(-2, "probe_accumulate: null pointer");
  q.pivot = pivot;
  const ProbeDims g = probe_dims(Da + Db, Cy);
  const int G = probe_acc_grid(q.ntiles, g, workgroups);
  const size_t need = probe_align16(8 * (size_t)G) + sizeof(float) * (size_t)G * g.slabF;
  if (int rc = frl_check_workspace("probe_accumulate", ws, ws_bytes, need)) return rc;
  long long* cnts = (long long*)ws;
  float* slabs = (float*)((char*)ws + probe_align16(8 * (size_t)G));
  const int NB = (g.nblk + 3) / 4;
  if (NB <= 4) FRL_LAUNCH(probe_acc_kernel<4>, dim3((unsigned)G), dim3(256), g.lds, stream, q, g.ys, g.CB, slabs, cnts);
  else if (NB <= 8) FRL_LAUNCH(probe_acc_kernel<8>, dim3((unsigned)G), dim3(256), g.lds, stream, q, g.ys, g.CB, slabs, cnts);
  else FRL_LAUNCH(probe_acc_kernel<14>, dim3((unsigned)G), dim3(256), g.lds, stream, q, g.ys, g.CB, slabs, cnts);
  FRL_LAUNCH(probe_acc_reduce_kernel, dim3((unsigned)(g.slabF / 64)), dim3(256), 0, stream, (const float*)slabs, (const long long*)cnts, G, g.CB,
             g.C1, S, (long long*)n);
  return frl_check_launch("probe_accumulate");
}

int frl_probe_evaluate(const float* A, int Ta, int Da, const float* Bs, int Tb, int Db, const float* Y, int Ty, int Cy, const unsigned char* mask,
                       int B, int T, int64_t P, const float* pivot, const float* Wc, const float* bc, int workgroups, double* E, int64_t* n,
                       float* pred, void* ws, size_t ws_bytes, hipStream_t stream) {
  ProbeIn q;
  if (int rc = probe_check("probe_evaluate", A, Ta, Da, Bs, Tb, Db, Y, Ty, Cy, mask, B, T, P, q)) return rc;
  if (int rc = frl_check_workgroups("probe_evaluate", workgroups)) return rc;
  if (!pivot || !Wc || !bc || !E || !n) return frl_fail(-2, "probe_evaluate: null pointer");
  q.pivot = pivot;
  const int C = Da + Db + Cy, ys = C | 1;
  const int G = probe_eval_grid(q.ntiles, workgroups);
  const size_t need = probe_align16(8 * (size_t)G) + sizeof(double) * (size_t)G * Cy * 3;
  if (int rc = frl_check_workspace("probe_evaluate", ws, ws_bytes, need)) return rc;
  long long* cnts = (long long*)ws;
  double* dsl = (double*)((char*)ws + probe_align16(8 * (size_t)G));
  const size_t lds = sizeof(float) * ((size_t)16 * (Da + Db) + (size_t)MOMENT_ROWS * ys + C);
  FRL_LAUNCH(probe_eval_kernel, dim3((unsigned)G), dim3(256), lds, stream, q, ys, Wc, bc, dsl, cnts, pred);
  probe_launch_eval_reduce(dsl, cnts, G, Cy, E, (long long*)n, stream);
  return frl_check_launch("probe_evaluate");
}

}  // extern "C"
