// The "full" design of the reference's fit_phase_linear_probe.py, [z_type | z_phase | z_type (x) z_phase] with a PCA of the interaction
// block: the moments it needs beyond those of frl_probe_accumulate, and its fused evaluation.
//
// Inputs are laid out as in probe.hip: A = z_type rows [B][Ta][P][Dt], Bs = z_phase rows [B][Tb][P][Dp], Y [B][Ty][P][Cy], mask [B][P].
// With x' = x - pivot_x, p' = p - pivot_p, y' = y - pivot_y (float32 subtractions; the whole row is zero where the mask is),
// c = [x' | p' | y' | m] (C + 1 columns, C = Dt + Dp + Cy) and q' = x' (x) p' (Dq = Dt Dp columns, column i Dp + a = x'_i p'_a, one float32
// multiplication), frl_probe_full_accumulate adds
//     Scq [C+1][Dq] += c^T q',     Sqq [Dq][Dq] += q'^T q'   (both triangles)
// in double.  c^T c and the count stay with frl_probe_accumulate.
//
// The scheme is that of frl_moments.hpp: tiles of 64 pixels of one (b, t), staged once in LDS as [c | 0], v_mfma_f32_16x16x4_f32 with
// the accumulators in registers for the whole grid-stride loop, one float32 slab per workgroup in fragment order, a second kernel that
// adds the slabs in double in the order of moment_slab_sum.  The output is too large for one workgroup (1464 blocks of 16 x 16 at
// Dt = 64, Dp = 12, Cy = 7), so it is cut into rectangles of 4 x 4 blocks, one per wave: a wave reads 4 + 4 operands for 16 MFMAs per
// k-step.  The rectangles are the c rows against the q' columns (ceil(CB / 4) x CG of them, CB = ceil((C + 1) / 16), CG = ceil(ceil(Dq / 16)
// / 4)) and then the upper triangle of q' against q' (CG (CG + 1) / 2); grid.y walks them four at a time and every slice stages the same
// tile again, which is nothing beside the arithmetic.  An operand is always the product of two staged values: x'_i p'_a for a column of
// q', c_j m for a column of c (m is 1 on every row that is not zero already), 0 * 0 from a column that is kept zero for the padding.
// A tile whose 64 mask bytes are zero is skipped before it is read.  No float atomics: two runs give the same bits.
//
// frl_probe_full_evaluate: lane = pixel of the tile, wave w owns the targets w, w + 4, ..  For target c the prediction is a float32 fmaf
// chain in this order:
//     h_a = fma(x'_i, Omega_c[i][a], h_a) for i = 0 .. Dt - 1, from h_a = 0              (a < Dp, independent chains)
//     r = beta_c;  r = fma(x'_i, u_c[i], r) for i = 0 .. Dt - 1;  r = fma(p'_a, v_c[a], r) for a = 0 .. Dp - 1;
//     r = fma(h_a, p'_a, r) for a = 0 .. Dp - 1.
// The sums over unmasked observations are those of frl_probe_evaluate, in double per lane, and are reduced by its kernel.
#include "probe_common.hpp"

#define PFULL_MAX_DT 64
#define PFULL_MAX_DP 16
#define PFULL_MAX_DQ 768
#define PFULL_EVAL_WG 1024
#define PFULL_ACC_SLOTS 768

namespace {

struct PFullDims {
  int Dt, Dp, Cy, C, C1, CB, ys, Dq, QB, CG, RGc, nrect, NS, slabF;
  size_t lds;
};

PFullDims pfull_dims(int Dt, int Dp, int Cy) {
  PFullDims g;
  g.Dt = Dt, g.Dp = Dp, g.Cy = Cy;
  g.C = Dt + Dp + Cy;
  g.C1 = g.C + 1;
  g.CB = (g.C1 + 16) / 16;                                                       // at least one padding column, which stays zero: column C1
  g.ys = frl_tile_stride(16 * g.CB);
  g.Dq = Dt * Dp;
  g.QB = (g.Dq + 15) / 16;
  g.CG = (g.QB + 3) / 4;
  g.RGc = ((g.C1 + 15) / 16 + 3) / 4;
  g.nrect = g.RGc * g.CG + g.CG * (g.CG + 1) / 2;
  g.NS = (g.nrect + 3) / 4;
  g.slabF = g.nrect * 4096;
  g.lds = sizeof(float) * ((size_t)MOMENT_ROWS * g.ys + 16 * g.CB);
  return g;
}

// tile groups of the accumulate kernel: every workgroup does the same work, so all slices of all groups are resident at once, three
// workgroups on each of 256 CUs (a grid one third larger runs a second, mostly empty round)
int pfull_acc_groups(const PFullDims& g) { return PFULL_ACC_SLOTS / g.NS > 1 ? PFULL_ACC_SLOTS / g.NS : 1; }
int pfull_acc_grid(int64_t ntiles, const PFullDims& g, int workgroups) {
  if (workgroups > 0) return workgroups;
  const int64_t cap = pfull_acc_groups(g);
  return (int)(ntiles < cap ? ntiles : cap);
}

int pfull_eval_grid(int64_t ntiles, int workgroups) {
  if (workgroups > 0) return workgroups;
  return (int)(ntiles < PFULL_EVAL_WG ? ntiles : PFULL_EVAL_WG);
}

}  // namespace

// rectangle -> (crow: rows are blocks of c, else of q'; rg, cg: group of four row blocks, of four column blocks of q')
__device__ __forceinline__ void pfull_rect(int rect, int RGc, int CG, bool& crow, int& rg, int& cg) {
  crow = rect < RGc * CG;
  if (crow) {
    rg = rect / CG, cg = rect - rg * CG;
    return;
  }
  int b = rect - RGc * CG;
  rg = 0;
  while (b >= CG - rg) {
    b -= CG - rg;
    ++rg;
  }
  cg = rg + b;
}

// the two staged columns whose product is column j of q' (zero beyond Dq)
__device__ __forceinline__ void pfull_qcol(int j, int Dt, int Dp, int Dq, int Z, int& o1, int& o2) {
  o1 = o2 = Z;
  if (j < Dq) {
    o1 = j / Dp;
    o2 = Dt + (j - o1 * Dp);
  }
}

__global__ __launch_bounds__(256, 3) void probe_full_acc_kernel(ProbeIn q, int ys, int CB, int RGc, int CG, int nrect, float* __restrict__ slabs) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lr = lane & 15, lg = lane >> 4;
  const int Dt = q.Da, Dp = q.Db, D = Dt + Dp, C = D + q.Cy, C1 = C + 1, Dq = Dt * Dp, Z = C1;
  float* vt = reinterpret_cast<float*>(smem);                                    // [64][ys]
  float* piv = vt + MOMENT_ROWS * ys;                                            // [16 CB]
  for (int d = tid; d < 16 * CB; d += 256) piv[d] = d < C ? q.pivot[d] : 0.f;
  for (int i = tid; i < MOMENT_ROWS * ys; i += 256) vt[i] = 0.f;                 // the padding columns stay zero

  const int rect = blockIdx.y * 4 + wave;
  const bool live = rect < nrect;                                                // uniform in a wave
  bool crow = false;
  int rg = 0, cg = 0;
  if (live) pfull_rect(rect, RGc, CG, crow, rg, cg);
  int ra1[4], ra2[4], cb1[4], cb2[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int jr = (4 * rg + i) * 16 + lr, jc = (4 * cg + i) * 16 + lr;
    if (crow) {
      ra1[i] = jr < C1 ? jr : Z;
      ra2[i] = jr < C1 ? C : Z;
    } else {
      pfull_qcol(jr, Dt, Dp, Dq, Z, ra1[i], ra2[i]);
    }
    pfull_qcol(jc, Dt, Dp, Dq, Z, cb1[i], cb2[i]);
    ra1[i] += lg * ys, ra2[i] += lg * ys, cb1[i] += lg * ys, cb2[i] += lg * ys;
  }
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
    int b, t, p0;
    moment_tile(tile, q.PT, q.T, b, t, p0);
    const unsigned long long rows = probe_mask_bits(q, b, p0, lane);
    if (rows == 0ull) continue;                                                  // uniform: every wave sees the same 64 mask bytes
    __syncthreads();                                                             // the previous tile is consumed (and the prologue is written)
    probe_stage(vt, ys, piv, q.A, q.Ta, Dt, 0, q.fast, true, q, b, t, p0, rows, tid);
    probe_stage(vt, ys, piv, q.Bs, q.Tb, Dp, Dt, q.fast, true, q, b, t, p0, rows, tid);
    probe_stage(vt, ys, piv, q.Y, q.Ty, q.Cy, D, false, true, q, b, t, p0, rows, tid);
    if (tid < MOMENT_ROWS) vt[tid * ys + C] = (rows >> tid) & 1ull ? 1.f : 0.f;
    __syncthreads();
    if (live) {
#pragma unroll 2
      for (int st = 0; st < MOMENT_ROWS / 4; ++st) {
        const float* v = vt + 4 * st * ys;
        float a[4], bb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a[i] = v[ra1[i]] * v[ra2[i]];
          bb[i] = v[cb1[i]] * v[cb2[i]];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(a[i], bb[j], acc[i][j]);
      }
    }
  }
  if (live) {
    float* slab = slabs + ((size_t)blockIdx.x * nrect + rect) * 4096;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(slab + ((size_t)(i * 4 + j) * 64 + lane) * 4) = acc[i][j];
  }
}

// the slabs added in double (moment_slab_sum), 64 elements per workgroup, into Scq [C1][Dq] and Sqq [Dq][Dq] (both triangles)
__global__ __launch_bounds__(256) void probe_full_acc_reduce_kernel(const float* __restrict__ slabs, int G, int RGc, int CG, int nrect, int C1, int Dq,
                                                                    double* __restrict__ Scq, double* __restrict__ Sqq) {
  const int e = blockIdx.x * 64 + (threadIdx.x & 63);
  int blk, row, col, rg, cg;
  bool crow;
  moment_frag_decode(e, blk, row, col);
  pfull_rect(blk >> 4, RGc, CG, crow, rg, cg);
  const int gi = (4 * rg + ((blk >> 2) & 3)) * 16 + row, gj = (4 * cg + (blk & 3)) * 16 + col;
  const bool live = gj < Dq && (crow ? gi < C1 : gi <= gj);
  const double sum = moment_slab_sum(slabs, G, nrect * 4096, e, live);
  if (threadIdx.x < 64 && live) {
    if (crow) {
      Scq[(size_t)gi * Dq + gj] += sum;
    } else {
      const double v = Sqq[(size_t)gi * Dq + gj] + sum;
      Sqq[(size_t)gi * Dq + gj] = v;
      Sqq[(size_t)gj * Dq + gi] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// evaluate.  DP4 = ceil(Dp / 4): a row of Omega in LDS is 4 DP4 floats, zeros beyond Dp
// ---------------------------------------------------------------------------------------------------------------------------------
template <int DP4>
__global__ __launch_bounds__(256, 2) void probe_full_eval_kernel(ProbeIn q, int ys, const float* __restrict__ beta, const float* __restrict__ U,
                                                                 const float* __restrict__ V, const float* __restrict__ Om, double* __restrict__ dsl,
                                                                 long long* __restrict__ cnts, float* __restrict__ pred) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Dt = q.Da, Dp = q.Db, D = Dt + Dp, Cy = q.Cy, C = D + Cy;
  constexpr int DPP = 4 * DP4;
  float* Ol = reinterpret_cast<float*>(smem);                                    // [Cy][Dt][DPP]
  float* Ul = Ol + (size_t)Cy * Dt * DPP;                                        // [Cy][Dt]
  float* Vl = Ul + Cy * Dt;                                                      // [Cy][Dp]
  float* piv = Vl + Cy * Dp;                                                     // [C]
  float* vt = piv + ((C + 3) & ~3);                                              // [64][ys]: x' | p' | y, ys odd
  for (int i = tid; i < Cy * Dt * DPP; i += 256) {
    const int a = i % DPP, ci = i / DPP;
    Ol[i] = a < Dp ? Om[(size_t)ci * Dp + a] : 0.f;
  }
  for (int i = tid; i < Cy * Dt; i += 256) Ul[i] = U[i];
  for (int i = tid; i < Cy * Dp; i += 256) Vl[i] = V[i];
  for (int d = tid; d < C; d += 256) piv[d] = q.pivot[d];
  double sse[4], sy[4], sy2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) sse[k] = sy[k] = sy2[k] = 0.0;
  long long cnt = 0;
  const bool all = pred != nullptr;                                              // every pixel is predicted: no tile is skipped

  for (int tile = blockIdx.x; tile < q.ntiles; tile += gridDim.x) {
    int b, t, p0;
    moment_tile(tile, q.PT, q.T, b, t, p0);
    const unsigned long long rows = probe_mask_bits(q, b, p0, lane);
    const int valid = moment_tile_rows(q.P, p0);
    const unsigned long long stage = all ? (valid == MOMENT_ROWS ? ~0ull : (1ull << valid) - 1ull) : rows;
    if (stage == 0ull) continue;                                                 // uniform
    cnt += __popcll(rows);
    __syncthreads();                                                             // the previous tile is consumed (and the prologue is written)
    probe_stage(vt, ys, piv, q.A, q.Ta, Dt, 0, false, true, q, b, t, p0, stage, tid);
    probe_stage(vt, ys, piv, q.Bs, q.Tb, Dp, Dt, false, true, q, b, t, p0, stage, tid);
    probe_stage(vt, ys, piv, q.Y, q.Ty, Cy, D, false, false, q, b, t, p0, stage, tid);
    __syncthreads();
    const float* xr = vt + lane * ys;
    const bool on = (rows >> lane) & 1ull;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = wave + 4 * k;
      if (c >= Cy) break;                                                        // uniform in a wave
      const float* ol = Ol + (size_t)c * Dt * DPP;
      const float* ul = Ul + c * Dt;
      const float* vl = Vl + c * Dp;
      float h[DPP];
#pragma unroll
      for (int a = 0; a < DPP; ++a) h[a] = 0.f;
      float r = beta[c];
#pragma unroll 4
      for (int i = 0; i < Dt; ++i) {
        const float xv = xr[i];
        r = fmaf(xv, ul[i], r);
#pragma unroll
        for (int a4 = 0; a4 < DP4; ++a4) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(ol + i * DPP + 4 * a4);
#pragma unroll
          for (int j = 0; j < 4; ++j) h[4 * a4 + j] = fmaf(xv, w[j], h[4 * a4 + j]);
        }
      }
      for (int a = 0; a < Dp; ++a) r = fmaf(xr[Dt + a], vl[a], r);
#pragma unroll
      for (int a = 0; a < DPP; ++a)
        if (a < Dp) r = fmaf(h[a], xr[Dt + a], r);
      if (pred && lane < valid) pred[((size_t)((int64_t)b * q.T + t) * q.P + p0 + lane) * Cy + c] = r;
      if (on) {
        const float y = xr[D + c];
        const double er = (double)r - (double)y, yq = (double)y - (double)piv[D + c];
        sse[k] += er * er;
        sy[k] += yq;
        sy2[k] += yq * yq;
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

// ---------------------------------------------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

bool pfull_dims_ok(int Dt, int Dp, int Cy) {
  return Dt >= 1 && Dt <= PFULL_MAX_DT && Dp >= 1 && Dp <= PFULL_MAX_DP && Dt * Dp <= PFULL_MAX_DQ && Cy >= 1 && Cy <= PROBE_MAX_CY;
}

int pfull_check(const char* what, const float* A, int Ta, int Dt, const float* Bs, int Tb, int Dp, const float* Y, int Ty, int Cy,
                const unsigned char* mask, int B, int T, int64_t P, int workgroups, ProbeIn& q) {
  if (!Bs || !pfull_dims_ok(Dt, Dp, Cy))
    return frl_failf(-2, "%s: needs z_type and z_phase with 1 <= Dt <= 64, 1 <= Dp <= 16, Dt * Dp <= 768, and 1 <= Cy <= 16 targets", what);
  if (int rc = probe_check(what, A, Ta, Dt, Bs, Tb, Dp, Y, Ty, Cy, mask, B, T, P, q)) return rc;
  return frl_check_workgroups(what, workgroups);
}

size_t pfull_eval_lds(int Dt, int Dp, int Cy, int ys) {
  const int C = Dt + Dp + Cy, DPP = (Dp + 3) & ~3;
  return sizeof(float) * ((size_t)Cy * Dt * DPP + (size_t)Cy * (Dt + Dp) + ((C + 3) & ~3) + (size_t)MOMENT_ROWS * ys);
}

}  // namespace

extern "C" {

// See include/frl_hip.h.
size_t frl_probe_full_workspace_bytes(int Dt, int Dp, int Cy, int workgroups) {
  if (!pfull_dims_ok(Dt, Dp, Cy) || !frl_wg_in_range(workgroups)) return 0;
  const PFullDims g = pfull_dims(Dt, Dp, Cy);
  const size_t Ga = workgroups > 0 ? workgroups : pfull_acc_groups(g), Ge = workgroups > 0 ? workgroups : PFULL_EVAL_WG;
  const size_t acc = sizeof(float) * Ga * g.slabF;
  const size_t ev = probe_align16(8 * Ge) + sizeof(double) * Ge * Cy * 3;
  return acc > ev ? acc : ev;
}

int frl_probe_full_accumulate(const float* A, int Ta, int Dt, const float* Bs, int Tb, int Dp, const float* Y, int Ty, int Cy,
                              const unsigned char* mask, int B, int T, int64_t P, const float* pivot, int workgroups, double* Scq, double* Sqq,
                              void* ws, size_t ws_bytes, hipStream_t stream) {
  ProbeIn q;
  if (int rc = pfull_check("probe_full_accumulate", A, Ta, Dt, Bs, Tb, Dp, Y, Ty, Cy, mask, B, T, P, workgroups, q)) return rc;
  if (!pivot || !Scq || !Sqq) return frl_fail(-2, "probe_full_accumulate: null pointer");
  q.pivot = pivot;
  const PFullDims g = pfull_dims(Dt, Dp, Cy);
  const int G = pfull_acc_grid(q.ntiles, g, workgroups);
  if (int rc = frl_check_workspace("probe_full_accumulate", ws, ws_bytes, sizeof(float) * (size_t)G * g.slabF)) return rc;
  float* slabs = (float*)ws;
  FRL_LAUNCH(probe_full_acc_kernel, dim3((unsigned)G, (unsigned)g.NS), dim3(256), g.lds, stream, q, g.ys, g.CB, g.RGc, g.CG, g.nrect, slabs);
  FRL_LAUNCH(probe_full_acc_reduce_kernel, dim3((unsigned)(g.slabF / 64)), dim3(256), 0, stream, (const float*)slabs, G, g.RGc, g.CG, g.nrect, g.C1,
             g.Dq, Scq, Sqq);
  return frl_check_launch("probe_full_accumulate");
}

int frl_probe_full_evaluate(const float* A, int Ta, int Dt, const float* Bs, int Tb, int Dp, const float* Y, int Ty, int Cy,
                            const unsigned char* mask, int B, int T, int64_t P, const float* pivot, const float* beta, const float* u, const float* v,
                            const float* omega, int workgroups, double* E, int64_t* n, float* pred, void* ws, size_t ws_bytes, hipStream_t stream) {
  ProbeIn q;
  if (int rc = pfull_check("probe_full_evaluate", A, Ta, Dt, Bs, Tb, Dp, Y, Ty, Cy, mask, B, T, P, workgroups, q)) return rc;
  if (!pivot || !beta || !u || !v || !omega || !E || !n) return frl_fail(-2, "probe_full_evaluate: null pointer");
  q.pivot = pivot;
  const int ys = (Dt + Dp + Cy) | 1;
  const int G = pfull_eval_grid(q.ntiles, workgroups);
  const size_t need = probe_align16(8 * (size_t)G) + sizeof(double) * (size_t)G * Cy * 3;
  if (int rc = frl_check_workspace("probe_full_evaluate", ws, ws_bytes, need)) return rc;
  long long* cnts = (long long*)ws;
  double* dsl = (double*)((char*)ws + probe_align16(8 * (size_t)G));
  const size_t lds = pfull_eval_lds(Dt, Dp, Cy, ys);
#define PFULL_EVAL(DP4)                                                                                                                              \
  do {                                                                                                                                               \
    auto kern = probe_full_eval_kernel<DP4>;                                                                                                         \
    if (lds > 64 * 1024) FRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                      \
    FRL_LAUNCH_AS("probe_full_eval_kernel", kern, dim3((unsigned)G), dim3(256), lds, stream, q, ys, beta, u, v, omega, dsl, cnts, pred);             \
  } while (0)
  switch ((Dp + 3) / 4) {
    case 1: PFULL_EVAL(1); break;
    case 2: PFULL_EVAL(2); break;
    case 3: PFULL_EVAL(3); break;
    default: PFULL_EVAL(4); break;
  }
#undef PFULL_EVAL
  probe_launch_eval_reduce(dsl, cnts, G, Cy, E, (long long*)n, stream);
  return frl_check_launch("probe_full_evaluate");
}

}  // extern "C"
