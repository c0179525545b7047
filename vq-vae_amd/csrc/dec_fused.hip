// build-flags: -fno-slp-vectorize
// (packed-f32 vector instructions issue slower than the two scalar ones they replace beside MFMAs on gfx950: MI355X_MICROARCH.md, cycle constants)
// Fused decoder + reconstruction loss for the hot configuration (bf16, hidden 128, 64 output features, latent <= 64 ch):
//   xhat = W2 relu(W1 z + b1) + b2 ;  L = mean_valid (xhat - x)^2
// Decoder definition: SURVEY.md 8a row a12 (template Conv2DHead, frl/models/heads.py:128-198; loss frl/losses/reconstruction.py:95-139).
// Forward: one pass over (z, x): the 128-channel hidden tensor and xhat never reach HBM (the modular path writes/reads
// ~0.9 GB for them on the phase path at cfg2); xhat is written only when the caller asks for it.
// Backward: recomputes the chain per pixel in registers, produces dz, and contracts the weight gradients over pixels inside
// the kernel (LDS tiles + ds_read_b64_tr_b16 fragments; every wave owns a block-row of dW2 / dW1), as tcn_fused.hip does.
// One pass (train step): the backward recomputes everything the forward computes, so when the upstream gradient of the loss is known
// before the forward runs (frl_decoder_mse_fwd_bwd) the backward kernel also accumulates the loss and no forward kernel is launched.
#include "frl_common.hpp"
#include "frl_host.hpp"
#include "frl_pack.hpp"
#include "frl_reduce.hpp"

typedef bf16 TT;
typedef bf16x8 frag8;
#define DF_H 128
#define DF_F 64
#define DF_GRID_MAX 1024

__device__ __forceinline__ bf16x8 tr_frag_p(const TT* tile, int pitch, int pix0, int ch0, int r16) {
  const TT* a0 = tile + (pix0 + (r16 >> 2)) * pitch + ch0 + 4 * (r16 & 3);
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(a0));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(a0 + 4 * pitch));
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <int NF>
__device__ __forceinline__ void tile_put(TT* tile, int pitch, int prow, int kc, const LQTile<TT, NF>& t) {
  bf16x8* p = reinterpret_cast<bf16x8*>(tile + prow * pitch + NF * 8 * kc);
#pragma unroll
  for (int s = 0; s < NF; ++s) p[s] = t.f[s];
}

// per-pixel forward chain; returns hidden (32 ch / lane, post-ReLU) and xhat (16 ch / lane)
template <int NFZ>
__device__ __forceinline__ void dec_chain(float (&h)[32], float (&xh)[16], const LQTile<TT, NFZ>& zt, const frag8* __restrict__ w1,
                                          const frag8* __restrict__ w2, const float* __restrict__ b1q, const float* __restrict__ b2q,
                                          LQTile<TT, 4>& ht, int lane, int lane2) {
  f32x4 hacc[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    hacc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NFZ; ++s) hacc[m] = mfma16(w1[(m * NFZ + s) * 64 + lane], zt.f[s], hacc[m]);
  }
#pragma unroll
  for (int j = 0; j < 32; ++j) {
    const float v = hacc[j >> 2][j & 3] + b1q[j];
    h[j] = v > 0.f ? v : 0.f;
    ht.f[j >> 3][j & 7] = (bf16)h[j];
  }
  f32x4 xacc[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    xacc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s) xacc[m] = mfma16(w2[(m * 4 + s) * 64 + lane2], ht.f[s], xacc[m]);
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) xh[j] = xacc[j >> 2][j & 3] + b2q[j];
}

// ------------------------------------------------------------------------------------------------ forward
template <int NFZ>
__global__ __launch_bounds__(256, 4) void dec_mse_fwd_kernel(const TT* __restrict__ Z, const frag8* __restrict__ Wpk, const float* __restrict__ b1,
                                                          const float* __restrict__ b2, const TT* __restrict__ TGT,
                                                          const uint8_t* __restrict__ mask, TT* __restrict__ XHAT, int64_t P, int Cz,
                                                          double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  frag8* w1 = reinterpret_cast<frag8*>(smem);                 // [8][NFZ][64]
  frag8* w2 = w1 + 8 * NFZ * 64;                              // [4][4][64]
  float* tb = reinterpret_cast<float*>(w2 + 16 * 64);         // b1[128] | b2[64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int px = lane & 15, kc = lane >> 4;
  copy_frags_lds<TT>(w1, Wpk, (8 * NFZ + 16) * 64, tid, 256);
  for (int i = tid; i < 192; i += 256) tb[i] = i < 128 ? b1[i] : b2[i - 128];
  __syncthreads();
  const float* b1q = tb + 32 * kc;
  const float* b2q = tb + 128 + 16 * kc;
  const bool fastz = (Cz == 32 * NFZ);
  float sq = 0.f, cnt = 0.f;
  const int64_t ntile = (P + 15) >> 4;
  // the next tile's rows are requested before this tile's chain (a wave is otherwise parked for a full memory latency per tile)
  const int64_t tstep = (int64_t)gridDim.x * 4;
  LQTile<TT, NFZ> zt, zn;
  LQTile<TT, 2> tt, tn;
  {
    const int64_t t0 = (int64_t)blockIdx.x * 4 + wave;
    const int64_t r0 = (t0 < ntile ? t0 : 0) * 16 + px;
    const int64_t rc = r0 < P ? r0 : P - 1;
    lq_load<TT, NFZ>(zt, Z, rc, Cz, kc, fastz);
    lq_load<TT, 2>(tt, TGT, rc, DF_F, kc, true);
  }
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntile; tile += tstep) {
    int64_t row = tile * 16 + px;
    bool valid = row < P;
    if (!valid) row = P - 1;
    if (valid && mask != nullptr) valid = mask[row] != 0;
    {
      const int64_t tnx = tile + tstep < ntile ? tile + tstep : tile;
      const int64_t rn = tnx * 16 + px;
      const int64_t rc = rn < P ? rn : P - 1;
      lq_load<TT, NFZ>(zn, Z, rc, Cz, kc, fastz);
      lq_load<TT, 2>(tn, TGT, rc, DF_F, kc, true);
    }
    float h[32], xh[16];
    LQTile<TT, 4> ht;
    int lw = lane;
    asm volatile("" : "+v"(lw));                                // (opaque per tile: the weight fragments stay in LDS instead of 96 hoisted registers)
    dec_chain<NFZ>(h, xh, zt, w1, w2, b1q, b2q, ht, lw, lw);
    if (valid) {
#pragma unroll
      for (int j = 0; j < 16; ++j) { const float d = xh[j] - (float)tt.f[j >> 3][j & 7]; sq = fmaf(d, d, sq); }
      cnt += 16.f;
    }
    if (XHAT != nullptr && tile * 16 + px < P) {
      bf16x8* xo = reinterpret_cast<bf16x8*>(XHAT + row * DF_F + 16 * kc);
      bf16x8 o0, o1;
#pragma unroll
      for (int j = 0; j < 8; ++j) { o0[j] = (bf16)xh[j]; o1[j] = (bf16)xh[8 + j]; }
      xo[0] = o0;
      xo[1] = o1;
    }
    zt = zn;
    tt = tn;
  }
  double sd = wave_sum_d((double)sq), cd = wave_sum_d((double)cnt);
  __shared__ double red[8];
  if (lane == 0) { red[wave] = sd; red[4 + wave] = cd; }
  __syncthreads();
  if (tid == 0) {
    partial[blockIdx.x * 2 + 0] = red[0] + red[1] + red[2] + red[3];
    partial[blockIdx.x * 2 + 1] = red[4] + red[5] + red[6] + red[7];
  }
}

__global__ __launch_bounds__(256) void dec_mse_finalize_kernel(const double* __restrict__ partial, int n, float* __restrict__ out) {
  __shared__ double rs[256], rc[256];
  double s = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) { s += partial[2 * i]; c += partial[2 * i + 1]; }
  rs[threadIdx.x] = s; rc[threadIdx.x] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) { rs[threadIdx.x] += rs[threadIdx.x + o]; rc[threadIdx.x] += rc[threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = rc[0] > 0.0 ? (float)(rs[0] / rc[0]) : 0.f; out[1] = (float)rc[0]; }
}

// ------------------------------------------------------------------------------------------------ backward
// Barrier of one 4-wave subgroup through a counter in LDS (the scheme of tcn_hot_bwd4.hip): every wave adds 1 and waits until the counter has
// reached 4 x the number of barriers it has passed; all waves of the workgroup are resident and a subgroup's waves run the same rounds.
__device__ __forceinline__ void df_sg_sync(unsigned* bar, unsigned& gen, int lane) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  gen += 4u;
  if (lane == 0) __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  for (;;) {
    const unsigned seen = (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    if ((int)(seen - gen) >= 0) break;
    __builtin_amdgcn_s_sleep(1);
  }
  asm volatile("" ::: "memory");
}
#define DF_SG_SHARE0 19      // subgroup 0's share of a workgroup's rounds in 32nds (the older waves of a SIMD run faster: tcn_hot_bwd4.hip)

// NW waves per workgroup (SG = false) or per SUBGROUP (SG = true: the workgroup is two independent 4-wave subgroups, one wave of each per
// SIMD, each with its own 64-row tiles, rounds, barriers and slab -- the two waves of a SIMD then sit in different phases of the round
// instead of both waiting at the same barrier); tile = 16*NW rows.  slab (floats): dW2 [64][128] | dW1 [128][CZP] | db2 [64] | db1 [128]
//
// LOSS: the kernel also accumulates the masked sum of diff^2 and the valid count (float per lane, double per wave and workgroup, as
// dec_mse_fwd_kernel does) and leaves them in la.partial for dec_mse_finalize_kernel.  (A fold by the last workgroup to arrive, behind a
// release fence and a ticket as in vq_assign_resident_kernel, was measured and dropped: it lengthened the <2,4> kernel by 9 us at 262 k
// rows and the subgroup kernel by 2..7 us at 1.3 M rows, run-to-run noise included; the finalize launch it would replace costs 5.)
// n_valid must be known before the pass: la.nv_host (no mask: P * 64) or la.out[1] (dec_mask_count_kernel).
//
// CB: 16-wide blocks of the latent in the dz GEMM, the dW1 accumulators and the w1t image: 1 for Cz <= 16, else CZP / 16.  (z -> hidden
// stays K = 32, the slab keeps its stride CZP: the columns >= 16 of a CB = 1 slab are never written and DecEpi drops every column >= Cz.)
//
// PAIR (NFZ = 2, NW = 8: latents of more than 32 channels at two waves per SIMD).  The two 4-wave halves of the workgroup take the rounds
// of the 4-wave lockstep workgroup <2, 4> two at a time -- half 0 round blockIdx.x + 2 i gridDim.x, half 1 the one after it -- into one
// 128-row tile set, and all eight waves contract it, each owning half the accumulator tiles of a 4-wave workgroup's wave.  Every
// accumulator tile therefore meets the same rows in the same order as in <2, 4> on the same grid, and every float32 sum (slabs, loss
// partials) is bit for bit that kernel's.  The loss chain of a lane of <2, 4> runs over all rounds, so half 1 hands its masked
// differences to half 0 through the LDS (into the rows of t_h that the receiving wave overwrites next, one more barrier per round pair).
// Two tile sets fit the LDS only beside THREE weight images, so w2t is not kept (WT):
// the dxhat -> dhidden fragments come out of the forward image w2 through transposing reads.  Fragment (m, s) of w2t holds, for lane
// (r, kc) and element e, W2[f = 16 kc + 8 s + e][h = 32 (r >> 2) + 4 m + (r & 3)]; in w2 that element is block mb = 2 s + (e >> 2),
// k-step m >> 1, lane slot (row 4 kc + (e & 3), quarter r >> 2), element 4 (m & 1) + (r & 3).  ds_read_b64_tr_b16 hands lane r of a
// 16-lane group element (r & 3) of the 8 bytes that lane 4 e + (r >> 2) of the group points at, so lane j of group kc points at slot
// (row 4 kc + (j >> 2), quarter j & 3) of block 2 s (e < 4) or 2 s + 1 (e >= 4: 4 KB further), 8 (m & 1) bytes in.  Slots of quarters 2
// and 3 are stored at row ^ 8 (df_w2_slot): the 32 lanes of a half-wave then meet two to a bank instead of four; ds_read_b128 of the
// forward fragments stays conflict-free.  The register ring is one round shallower there.
__device__ __forceinline__ int df_w2_slot(int l) { return l ^ ((l >> 2) & 8); }
__device__ __forceinline__ bf16x8 df_w2t_frag(const char* a) {
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(a));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(a + 4096));
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
template <bool LOSS> struct DecLoss {};
template <> struct DecLoss<true> {
  double* partial;      // [gridDim.x][2]
  const float* out;     // {loss, n_valid} record: only n_valid is read
  float* out_w;         // (host side: the record dec_mse_finalize_kernel writes behind the pass)
  float nv_host;        // n_valid when the host knows it, else < 0: read from out[1]
};

template <int NFZ, int NW, bool SG, bool LOSS, int CB>
__global__ __launch_bounds__(SG ? 512 : 64 * NW) void dec_mse_bwd_kernel(const TT* __restrict__ Z, const frag8* __restrict__ Wpk, const float* __restrict__ b1,
                                                               const float* __restrict__ b2, const TT* __restrict__ TGT,
                                                               const uint8_t* __restrict__ mask, const float* __restrict__ gscale,
                                                               const float* __restrict__ stats, TT* __restrict__ DZ, int64_t P, int Cz,
                                                               float* __restrict__ slab, const DecLoss<LOSS> la) {
  constexpr int CZP = 32 * NFZ, R = 16 * NW, NTH = SG ? 512 : 64 * NW;
  constexpr bool PAIR = !SG && NW == 8 && NFZ == 2, WT = PAIR;
  constexpr int RR = PAIR ? 64 : R;                           // rows of a round
  static_assert(!(SG && NFZ == 2), "latents of more than 32 channels: PAIR");
  static_assert(CB == CZP / 16 || (CB == 1 && NFZ == 1), "latent blocks");
  constexpr int PX = DF_F + 8, PH = DF_H + 8, PZ = CZP + 8;            // LDS tile pitches (16-byte skew)
  static_assert(!SG || NW == 4, "subgroups are four waves");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  frag8* w1 = reinterpret_cast<frag8*>(smem);                 // [8][NFZ][64]     z -> hidden
  frag8* w2 = w1 + 8 * NFZ * 64;                              // [4][4][64]       hidden -> xhat
  frag8* w2t = w2 + 16 * 64;                                  // [8][2][64]       dxhat -> dhidden (WT: not kept)
  frag8* w1t = w2t + (WT ? 0 : 16 * 64);                      // [CB][4][64]      dhidden -> dz
  float* tb = reinterpret_cast<float*>(w1t + CB * 4 * 64);    // b1[128] | b2[64]
  const int tid = threadIdx.x, lane = tid & 63;
  const int sg = SG ? (tid >> 8) : 0;                          // subgroup: waves 0-3 / 4-7
  const int wave = SG ? ((tid >> 6) & 3) : (tid >> 6);         // wave inside the workgroup / subgroup
  constexpr int TILE_ELEMS = R * (PX + 2 * PH + PZ);
  unsigned* bars = reinterpret_cast<unsigned*>(tb + 192);     // (SG) two arrival counters, 64 bytes apart
  TT* t_dx = reinterpret_cast<TT*>(tb + 192 + (SG ? 32 : 0)) + sg * TILE_ELEMS;   // [R][PX]
  TT* t_h = t_dx + R * PX;                                    // [R][PH]
  TT* t_dh = t_h + R * PH;                                    // [R][PH]
  TT* t_z = t_dh + R * PH;                                    // [R][PZ]
  const int px = lane & 15, kc = lane >> 4, r16 = px;
  const int prow = wave * 16 + px;
  const int hf = PAIR ? (wave >> 2) : 0;                       // (PAIR) which round of the pair
  const int rrow = PAIR ? (wave & 3) * 16 + px : prow;         // row inside the round
  if constexpr (WT) {
    copy_frags_lds<TT>(w1, Wpk, 8 * NFZ * 64, tid, NTH);
    for (int i = tid; i < 16 * 64; i += NTH) w2[df_w2_slot(i)] = Wpk[8 * NFZ * 64 + i];
    copy_frags_lds<TT>(w1t, Wpk + (8 * NFZ + 32) * 64, CB * 4 * 64, tid, NTH);
  } else {
    copy_frags_lds<TT>(w1, Wpk, (8 * NFZ + 16 + 16 + CB * 4) * 64, tid, NTH);
  }
  const int lane2 = WT ? df_w2_slot(lane) : lane;              // lane slot in the w2 image
  // (WT) byte address of this lane's 8 bytes of block 0, k-step 0 for the transposing reads
  const char* w2tr = reinterpret_cast<const char*>(w2) + 16 * df_w2_slot((px & 3) * 16 + 4 * kc + (px >> 2));
  (void)w2tr;
  for (int i = tid; i < 192; i += NTH) tb[i] = i < 128 ? b1[i] : b2[i - 128];
  if (SG && tid < 2) bars[16 * tid] = 0u;
  unsigned* bar = bars + 16 * sg;
  unsigned bgen = 0;
  (void)bar; (void)bgen;
  __syncthreads();
  const float* b1q = tb + 32 * kc;
  const float* b2q = tb + 128 + 16 * kc;
  const bool fastz = (Cz == CZP);
  float nv;
  if constexpr (LOSS) nv = la.nv_host >= 0.f ? la.nv_host : la.out[1]; else nv = stats[1];
  float sq = 0.f;
  int nrow = 0;                                                // valid rows of this wave (wave-uniform: a scalar register)
  (void)sq; (void)nrow;
  const float ksc = nv > 0.f ? (gscale ? gscale[0] : 1.f) * 2.f / nv : 0.f;

  // weight-gradient ownership
  constexpr int W2CB = (NW == 8) ? 4 : 8;                     // dW2 column blocks per wave
  const int w2row = (NW == 8) ? (wave & 3) : wave;            // dW2 row block (16 output features)
  const int w2col0 = (NW == 8) ? 4 * (wave >> 2) : 0;
  constexpr int W1RB = (NW == 8) ? 1 : 2;                     // dW1 row blocks per wave
  f32x4 a2[W2CB], a1[W1RB][CB], ab2, ab1[W1RB];
#pragma unroll
  for (int i = 0; i < W2CB; ++i) a2[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < W1RB; ++r) {
    ab1[r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < CB; ++i) a1[r][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  ab2 = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16 one = (bf16)1.f, zero = (bf16)0.f;
  const bf16x8 ones = (r16 == 0) ? bf16x8{one, one, one, one, one, one, one, one} : bf16x8{zero, zero, zero, zero, zero, zero, zero, zero};

  const int64_t nwt = (P + RR - 1) / RR;
  // rounds of this workgroup (SG: of this subgroup; PAIR: of this half, w_end counts for half 0): first, step, end
  int64_t w_first = blockIdx.x + (PAIR ? hf * (int64_t)gridDim.x : 0), w_end = nwt;
  const int64_t w_step = (PAIR ? 2 : 1) * (int64_t)gridDim.x;
  if (SG) {                                                    // the workgroup's rounds blockIdx.x + i gridDim.x, split DF_SG_SHARE0 : the rest between the subgroups
    const int64_t n_wg = (int64_t)blockIdx.x < nwt ? (nwt - 1 - blockIdx.x) / w_step + 1 : 0;
    const int64_t n0 = (n_wg * DF_SG_SHARE0 + 16) >> 5;
    w_first = blockIdx.x + (sg ? n0 : 0) * w_step;
    w_end = blockIdx.x + (sg ? n_wg : n0) * w_step;
    if (w_end > nwt) w_end = nwt;
  }
  // The rows of the next THREE rounds are in flight while a round computes: the workgroup is alone on its CU (LDS) and a round's rows
  // are only ~19 KB, so one round of look-ahead left the kernel bound by memory latency (19 KB per ~3 us per CU = 1.3 TB/s over the chip).
  // (WT: TWO rounds, z1 / t1 stay unused)
  constexpr int AHEAD = WT ? 2 : 3;
  LQTile<TT, NFZ> zt, z1, z2, zn;
  LQTile<TT, 2> tt, t1, t2, tn;
  auto fetch = [&](LQTile<TT, NFZ>& zz, LQTile<TT, 2>& tg, int64_t w) {
    const int64_t wc = w < nwt ? w : (nwt - 1);
    const int64_t r0 = wc * RR + rrow;
    const int64_t rc = r0 < P ? r0 : P - 1;
    lq_load<TT, NFZ>(zz, Z, rc, Cz, kc, fastz);
    lq_load<TT, 2>(tg, TGT, rc, DF_F, kc, true);
  };
  fetch(zt, tt, w_first);
  if constexpr (AHEAD == 3) {
    fetch(z1, t1, w_first + w_step);
    fetch(z2, t2, w_first + 2 * w_step);
  } else {
    fetch(z2, t2, w_first + w_step);
  }
  for (int64_t wt = w_first; wt - (PAIR ? hf * (int64_t)gridDim.x : 0) < w_end; wt += w_step) {
    int64_t row = wt * RR + rrow;
    const bool inb = row < P;
    bool valid = inb;
    if (!inb) row = P - 1;
    if (valid && mask != nullptr) valid = mask[row] != 0;
    fetch(zn, tn, wt + AHEAD * w_step);
    float h[32], xh[16];
    LQTile<TT, 4> ht;
    dec_chain<NFZ>(h, xh, zt, w1, w2, b1q, b2q, ht, lane, lane2);
    LQTile<TT, 2> dxt;
    const float kv = valid ? ksc : 0.f;
    float d[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) d[j] = xh[j] - (float)tt.f[j >> 3][j & 7];
    if constexpr (LOSS) {                                       // no branch: a masked row adds +0, which leaves sq bit for bit what it was
#pragma unroll
      for (int j = 0; j < 16; ++j) { const float dm = valid ? d[j] : 0.f; if (!PAIR || hf == 0) sq = fmaf(dm, dm, sq); }
      if constexpr (PAIR) {
        float* xch = reinterpret_cast<float*>(t_h + (wave & 3) * 16 * PH);
        if (hf) {
#pragma unroll
          for (int j = 0; j < 16; ++j) xch[j * 64 + lane] = valid ? d[j] : 0.f;
        }
        __syncthreads();
        if (!hf) {
#pragma unroll
          for (int j = 0; j < 16; ++j) { const float db = xch[j * 64 + lane]; sq = fmaf(db, db, sq); }
        }
      }
      nrow += __popcll(__ballot(valid));                        // (each lane of a valid row holds 16 of its 64 elements)
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) dxt.f[j >> 3][j & 7] = (bf16)(kv * d[j]);
    f32x4 dhacc[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      dhacc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if constexpr (WT) dhacc[m] = mfma16(df_w2t_frag(w2tr + (8 * s + (m >> 1)) * 1024 + 8 * (m & 1)), dxt.f[s], dhacc[m]);
        else dhacc[m] = mfma16(w2t[(m * 2 + s) * 64 + lane], dxt.f[s], dhacc[m]);
      }
    }
    LQTile<TT, 4> dht;
#pragma unroll
    for (int j = 0; j < 32; ++j) dht.f[j >> 3][j & 7] = (bf16)(h[j] > 0.f ? dhacc[j >> 2][j & 3] : 0.f);
    f32x4 dzacc[CB];
#pragma unroll
    for (int m = 0; m < CB; ++m) {
      dzacc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 4; ++s) dzacc[m] = mfma16(w1t[(m * 4 + s) * 64 + lane], dht.f[s], dzacc[m]);
    }
    if (inb) {
      constexpr int QZ = 4 * CB;                               // latent channels per lane quarter
      TT* dzp = DZ + row * (int64_t)Cz + QZ * kc;
      if (QZ >= 8 && fastz) {
        if constexpr (QZ >= 8) {
#pragma unroll
          for (int j = 0; j < QZ; j += 8) {
            bf16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (bf16)dzacc[(j + e) >> 2][(j + e) & 3];
            *reinterpret_cast<bf16x8*>(dzp + j) = o;
          }
        }
      } else if ((Cz & 3) == 0) {                              // 12-channel latent rows: 8-byte stores
#pragma unroll
        for (int j = 0; j < QZ; j += 4)
          if (QZ * kc + j < Cz)
            *reinterpret_cast<bf16x4*>(dzp + j) = bf16x4{(bf16)dzacc[j >> 2][0], (bf16)dzacc[j >> 2][1], (bf16)dzacc[j >> 2][2], (bf16)dzacc[j >> 2][3]};
      } else {
#pragma unroll
        for (int j = 0; j < QZ; ++j)
          if (QZ * kc + j < Cz) dzp[j] = (bf16)dzacc[j >> 2][j & 3];
      }
    }
    if (!inb) {                                               // rows past the end contribute nothing to the weight gradients
#pragma unroll
      for (int s = 0; s < 4; ++s) dht.f[s] = bf16x8{zero, zero, zero, zero, zero, zero, zero, zero};
    }
    tile_put<2>(t_dx, PX, prow, kc, dxt);
    tile_put<4>(t_h, PH, prow, kc, ht);
    tile_put<4>(t_dh, PH, prow, kc, dht);
    tile_put<NFZ>(t_z, PZ, prow, kc, zt);
    if constexpr (SG) df_sg_sync(bar, bgen, lane); else __syncthreads();
#pragma unroll
    for (int ks = 0; ks < R / 32; ++ks) {
      const int pix0 = ks * 32 + 8 * kc;
      const bf16x8 af = tr_frag_p(t_dx, PX, pix0, w2row * 16, r16);                 // dW2 rows: output features
#pragma unroll
      for (int i = 0; i < W2CB; ++i) a2[i] = mfma16(af, tr_frag_p(t_h, PH, pix0, (w2col0 + i) * 16, r16), a2[i]);
      if (NW == 4 || (wave >> 2) == 0) ab2 = mfma16(af, ones, ab2);
#pragma unroll
      for (int r = 0; r < W1RB; ++r) {
        const int rb = (NW == 8) ? wave : 2 * wave + r;                              // dW1 rows: hidden units
        const bf16x8 ah = tr_frag_p(t_dh, PH, pix0, rb * 16, r16);
#pragma unroll
        for (int i = 0; i < CB; ++i) a1[r][i] = mfma16(ah, tr_frag_p(t_z, PZ, pix0, i * 16, r16), a1[r][i]);
        ab1[r] = mfma16(ah, ones, ab1[r]);
      }
    }
    if constexpr (SG) df_sg_sync(bar, bgen, lane); else __syncthreads();
    if constexpr (AHEAD == 3) {
      zt = z1; z1 = z2; z2 = zn;
      tt = t1; t1 = t2; t2 = tn;
    } else {
      zt = z2; z2 = zn;
      tt = t2; t2 = tn;
    }
  }
  float* my = slab + (int64_t)(SG ? 2 * blockIdx.x + sg : blockIdx.x) * (DF_F * DF_H + DF_H * CZP + DF_F + DF_H);   // (SG: a slab per subgroup)
#pragma unroll
  for (int i = 0; i < W2CB; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) my[(w2row * 16 + kc * 4 + r) * DF_H + (w2col0 + i) * 16 + r16] = a2[i][r];
#pragma unroll
  for (int rr = 0; rr < W1RB; ++rr) {
    const int rb = (NW == 8) ? wave : 2 * wave + rr;
#pragma unroll
    for (int i = 0; i < CB; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) my[DF_F * DF_H + (rb * 16 + kc * 4 + r) * CZP + i * 16 + r16] = a1[rr][i][r];
    if (r16 == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) my[DF_F * DF_H + DF_H * CZP + DF_F + rb * 16 + kc * 4 + r] = ab1[rr][r];
    }
  }
  if (r16 == 0 && (NW == 4 || (wave >> 2) == 0)) {
#pragma unroll
    for (int r = 0; r < 4; ++r) my[DF_F * DF_H + DF_H * CZP + w2row * 16 + kc * 4 + r] = ab2[r];
  }
  if constexpr (LOSS) {
    constexpr int NWV = NTH / 64;
    __shared__ double lred[2 * NWV];
    const double sd = wave_sum_d((double)sq), cd = 16.0 * (double)nrow;
    if (lane == 0) { lred[tid >> 6] = sd; lred[NWV + (tid >> 6)] = cd; }
    __syncthreads();
    if (tid == 0) {
      double s = lred[0], c = lred[NWV];
#pragma unroll
      for (int w = 1; w < NWV; ++w) { s += lred[w]; c += lred[NWV + w]; }              // fixed order
      la.partial[2 * blockIdx.x + 0] = s;
      la.partial[2 * blockIdx.x + 1] = c;
    }
  }
}

// Valid-element count of a masked one-pass call, from the mask bytes alone: out[1] = 64 * (non-zero bytes), the value dec_mse_fwd_kernel's
// count comes to.  Integer atomics (order-independent); the last workgroup writes the record and leaves ctl {ticket, -, count} zero.
__global__ __launch_bounds__(256) void dec_mask_count_kernel(const uint8_t* __restrict__ mask, int64_t P, unsigned* __restrict__ ctl,
                                                             float* __restrict__ out) {
  __shared__ unsigned wg_n;
  const int tid = threadIdx.x;
  if (tid == 0) wg_n = 0u;
  __syncthreads();
  const int64_t gtid = (int64_t)blockIdx.x * 256 + tid, gstep = (int64_t)gridDim.x * 256;
  const int64_t n16 = ((reinterpret_cast<uintptr_t>(mask) & 15) == 0) ? (P >> 4) : 0;
  unsigned n = 0;
  const uint4* m16 = reinterpret_cast<const uint4*>(mask);
  for (int64_t i = gtid; i < n16; i += gstep) {
    const uint4 v = m16[i];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)                                // one bit per non-zero byte
      n += __popc((w[k] | ((w[k] & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u);
  }
  for (int64_t i = n16 * 16 + gtid; i < P; i += gstep) n += mask[i] != 0 ? 1u : 0u;
  if (n) atomicAdd(&wg_n, n);
  __syncthreads();
  if (tid == 0) {
    unsigned long long* total = reinterpret_cast<unsigned long long*>(ctl + 2);
    if (wg_n) __hip_atomic_fetch_add(total, (unsigned long long)wg_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned ticket = __hip_atomic_fetch_add(ctl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket == gridDim.x - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned long long t = __hip_atomic_load(total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      out[1] = (float)((double)t * (double)DF_F);
      __hip_atomic_store(total, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(ctl, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <int NFZ, int CB>
__global__ void dec_pack_kernel(frag8* __restrict__ dst, const float* __restrict__ W1, const float* __restrict__ W2, int Cz, int bwd) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x, nt = gridDim.x * blockDim.x;
  pack_weights_lds<TT, NFZ>(dst, W1, DF_H, Cz, 8, Cz, 1, tid, nt);                       // hidden[o] = sum_i W1[o][i] z[i]
  frag8* p = dst + 8 * NFZ * 64;
  pack_weights_lds<TT, 4>(p, W2, DF_F, DF_H, 4, DF_H, 1, tid, nt);                       // xhat[o] = sum_i W2[o][i] h[i]
  if (!bwd) return;
  p += 16 * 64;
  pack_weights_lds<TT, 2>(p, W2, DF_H, DF_F, 8, 1, DF_H, tid, nt);                       // dh[o=h] = sum_f W2[f][h] dx[f]
  p += 16 * 64;
  pack_weights_lds<TT, 4>(p, W1, Cz, DF_H, CB, 1, Cz, tid, nt);                          // dz[o=c] = sum_h W1[h][c] dh[h]
}

// Packed image of the decoder weights (layout of dec_pack_kernel): from the caller's image cache when one is active, else packed into `ws_pk`.
template <int NFZ, int CB = 2 * NFZ>
static const frag8* dec_packed(const float* w1, const float* w2, int Cz, int bwd, frag8* ws_pk, hipStream_t st) {
  FrlPackJob jobs[4];
  size_t off = 0;
  jobs[0] = frl_pack_job_pw(w1, off, FRL_BF16, NFZ, DF_H, Cz, 8, Cz, 1);
  off += (size_t)8 * NFZ * 64 * sizeof(frag8);
  jobs[1] = frl_pack_job_pw(w2, off, FRL_BF16, 4, DF_F, DF_H, 4, DF_H, 1);
  off += (size_t)16 * 64 * sizeof(frag8);
  int n = 2;
  if (bwd) {
    jobs[2] = frl_pack_job_pw(w2, off, FRL_BF16, 2, DF_H, DF_F, 8, 1, DF_H);
    off += (size_t)16 * 64 * sizeof(frag8);
    jobs[3] = frl_pack_job_pw(w1, off, FRL_BF16, 4, Cz, DF_H, CB, 1, Cz);
    off += (size_t)CB * 4 * 64 * sizeof(frag8);
    n = 4;
  }
  bool hit = false;
  frag8* pk = ws_pk;
  if (void* img = frl_pack_cached(jobs, n, off, &hit)) pk = (frag8*)img;
  if (!hit) FRL_LAUNCH((dec_pack_kernel<NFZ, CB>), dim3(32), dim3(256), 0, st, pk, w1, w2, Cz, bwd);
  return pk;
}


static unsigned df_fwd_grid(int64_t P) { int64_t g = ((P + 15) / 16 + 3) / 4; if (g > DF_GRID_MAX) g = DF_GRID_MAX; return (unsigned)(g < 1 ? 1 : g); }
static unsigned df_bwd_grid(int64_t P, int R) { int64_t g = (P + R - 1) / R; if (g > 256) g = 256; return (unsigned)(g < 1 ? 1 : g); }

// LOSS (one pass): the slabs are left unreduced in `ws` (frl_decoder_mse_reduce), *nslab_out receives their number
template <int NFZ, int NW, bool LOSS = false, int CB = 2 * NFZ>
static int launch_dec_bwd(const void* z, const float* w1, const float* b1, const float* w2, const float* b2, const void* tgt,
                          const uint8_t* mask, const float* gscale, const float* stats, void* dz, float* dw1, float* db1, float* dw2,
                          float* db2, int64_t P, int Cz, char* ws, hipStream_t st, DecLoss<LOSS> la = DecLoss<LOSS>{}, int* nslab_out = nullptr) {
  constexpr int CZP = 32 * NFZ, R = 16 * NW;
  constexpr bool PAIR = NFZ == 2 && NW == 8;                   // the grid (and the slabs) of <2, 4>, no w2t image in the LDS
  const unsigned grid = df_bwd_grid(P, PAIR ? 64 : R);
  const size_t slab_n = (size_t)DF_F * DF_H + DF_H * CZP + DF_F + DF_H;
  const frag8* pk = dec_packed<NFZ, CB>(w1, w2, Cz, 1, reinterpret_cast<frag8*>(ws + ((grid * slab_n * sizeof(float) + 255) / 256) * 256), st);
  const size_t lds = (size_t)(8 * NFZ + 16 + (PAIR ? 0 : 16) + CB * 4) * 64 * sizeof(frag8) + 192 * sizeof(float) +
                     (size_t)R * ((DF_F + 8) + 2 * (DF_H + 8) + (CZP + 8)) * sizeof(TT);
  auto kern = dec_mse_bwd_kernel<NFZ, NW, false, LOSS, CB>;
  FRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  FRL_LAUNCH_AS(LOSS ? "dec_mse_bwd_loss_kernel" : "dec_mse_bwd_kernel", kern, dim3(grid), dim3(64 * NW), lds, st, (const TT*)z, (const frag8*)pk, b1, b2, (const TT*)tgt, mask, gscale, stats, (TT*)dz, P, Cz,
             (float*)ws, la);
  if constexpr (LOSS) {
    FRL_LAUNCH(dec_mse_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)la.partial, (int)grid, la.out_w);
    *nslab_out = (int)grid;
    return frl_check_launch("decoder_mse_fwd_bwd");
  }
  launch_slab_reduce_deferrable<float, DecEpi>((const float*)ws, (int)grid, (int64_t)slab_n, DecEpi{dw2, dw1, db2, db1, Cz, CZP, DF_F, DF_H}, st);
  return frl_check_launch("decoder_mse_bwd");
}

// two independent 4-wave subgroups per workgroup (64-row tiles each), a slab per subgroup
template <int NFZ, bool LOSS = false, int CB = 2 * NFZ>
static int launch_dec_bwd_sg(const void* z, const float* w1, const float* b1, const float* w2, const float* b2, const void* tgt,
                             const uint8_t* mask, const float* gscale, const float* stats, void* dz, float* dw1, float* db1, float* dw2,
                             float* db2, int64_t P, int Cz, char* ws, hipStream_t st, DecLoss<LOSS> la = DecLoss<LOSS>{}, int* nslab_out = nullptr) {
  constexpr int CZP = 32 * NFZ, R = 64;
  constexpr int NIMG = 8 * NFZ + 16 + 16 + CB * 4;
  int64_t g = (P + 2 * R - 1) / (2 * R);
  if (g > 256) g = 256;
  if (g < 1) g = 1;
  const unsigned grid = (unsigned)g, nslab = 2 * grid;
  const size_t slab_n = (size_t)DF_F * DF_H + DF_H * CZP + DF_F + DF_H;
  const frag8* pk = dec_packed<NFZ, CB>(w1, w2, Cz, 1, reinterpret_cast<frag8*>(ws + ((nslab * slab_n * sizeof(float) + 255) / 256) * 256), st);
  const size_t lds = (size_t)NIMG * 64 * sizeof(frag8) + (192 + 32) * sizeof(float) +
                     (size_t)2 * R * ((DF_F + 8) + 2 * (DF_H + 8) + (CZP + 8)) * sizeof(TT);
  auto kern = dec_mse_bwd_kernel<NFZ, 4, true, LOSS, CB>;
  FRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  FRL_LAUNCH_AS(LOSS ? "dec_mse_bwd_sg_loss_kernel" : "dec_mse_bwd_sg_kernel", kern, dim3(grid), dim3(512), lds, st, (const TT*)z, (const frag8*)pk, b1, b2, (const TT*)tgt, mask, gscale, stats, (TT*)dz, P,
                Cz, (float*)ws, la);
  if constexpr (LOSS) {
    FRL_LAUNCH(dec_mse_finalize_kernel, dim3(1), dim3(256), 0, st, (const double*)la.partial, (int)grid, la.out_w);
    *nslab_out = (int)nslab;
    return frl_check_launch("decoder_mse_fwd_bwd");
  }
  launch_slab_reduce_deferrable<float, DecEpi>((const float*)ws, (int)nslab, (int64_t)slab_n, DecEpi{dw2, dw1, db2, db1, Cz, CZP, DF_F, DF_H}, st);
  return frl_check_launch("decoder_mse_bwd");
}

static int g_dec_subgroups = 1;     // A/B hook (frl_decoder_mse_bwd_subgroups): 0 = the lockstep 8-wave / 4-wave workgroups of round 2

extern "C" {

int frl_decoder_mse_bwd_subgroups(int on) { const int was = g_dec_subgroups; g_dec_subgroups = on ? 1 : 0; return was; }

int frl_decoder_mse_fused_supported(int Cz, int hidden, int F, int dtype) {
  return (dtype == FRL_BF16 && hidden == DF_H && F == DF_F && Cz >= 1 && Cz <= 64) ? 1 : 0;
}

size_t frl_decoder_mse_workspace_bytes(int64_t P, int Cz) {
  const size_t czp = Cz <= 32 ? 32 : 64;
  const size_t slab_n = (size_t)DF_F * DF_H + DF_H * czp + DF_F + DF_H;
  const size_t bwd = 512 * slab_n * sizeof(float) + 256 + (size_t)(8 * 2 + 32 + 16) * 64 * 16;     // (a slab per subgroup: two per workgroup)
  const size_t fwd = (size_t)DF_GRID_MAX * 2 * sizeof(double) + 256 + (size_t)(8 * 2 + 16) * 64 * 16;
  (void)P;
  return bwd > fwd ? bwd : fwd;
}

// z [P][Cz], target [P][64] bf16; w1 [128][Cz], w2 [64][128] f32.  out = {mean squared error over valid elements, n_valid};
// xhat (optional, [P][64]) receives the reconstruction.
int frl_decoder_mse_fwd(const void* z, const float* w1, const float* b1, const float* w2, const float* b2, const void* target,
                        const uint8_t* mask, void* xhat, float* out, int64_t P, int Cz, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (P <= 0) return frl_fail(-2, "decoder_mse_fwd: empty input");
  if (Cz < 1 || Cz > 64) return frl_fail(-2, "decoder_mse_fwd: latent width must be 1..64");
  if (ws_bytes < frl_decoder_mse_workspace_bytes(P, Cz)) return frl_fail(-4, "decoder_mse_fwd: workspace too small");
  char* w = (char*)ws;
  double* partial = (double*)w;
  frag8* ws_pk = reinterpret_cast<frag8*>(w + (size_t)DF_GRID_MAX * 2 * sizeof(double) + 256);
  const unsigned grid = df_fwd_grid(P);
  if (Cz <= 32) {
    const frag8* pk = dec_packed<1>(w1, w2, Cz, 0, ws_pk, stream);
    const size_t lds = (size_t)(8 + 16) * 64 * sizeof(frag8) + 192 * sizeof(float);
    FRL_LAUNCH((dec_mse_fwd_kernel<1>), dim3(grid), dim3(256), lds, stream, (const TT*)z, (const frag8*)pk, b1, b2, (const TT*)target, mask,
               (TT*)xhat, P, Cz, partial);
  } else {
    const frag8* pk = dec_packed<2>(w1, w2, Cz, 0, ws_pk, stream);
    const size_t lds = (size_t)(16 + 16) * 64 * sizeof(frag8) + 192 * sizeof(float);
    FRL_LAUNCH((dec_mse_fwd_kernel<2>), dim3(grid), dim3(256), lds, stream, (const TT*)z, (const frag8*)pk, b1, b2, (const TT*)target, mask,
               (TT*)xhat, P, Cz, partial);
  }
  FRL_LAUNCH(dec_mse_finalize_kernel, dim3(1), dim3(256), 0, stream, (const double*)partial, (int)grid, out);
  return frl_check_launch("decoder_mse_fwd");
}

// gradients: dz [P][Cz] bf16; dw1 [128][Cz], db1 [128], dw2 [64][128], db2 [64] f32.  gscale: device scalar (upstream grad of
// the loss) or null; stats = frl_decoder_mse_fwd's out.
int frl_decoder_mse_bwd(const void* z, const float* w1, const float* b1, const float* w2, const float* b2, const void* target,
                        const uint8_t* mask, const float* gscale, const float* stats, void* dz, float* dw1, float* db1, float* dw2,
                        float* db2, int64_t P, int Cz, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (P <= 0) return frl_fail(-2, "decoder_mse_bwd: empty input");
  if (Cz < 1 || Cz > 64) return frl_fail(-2, "decoder_mse_bwd: latent width must be 1..64");
  if (ws_bytes < frl_decoder_mse_workspace_bytes(P, Cz)) return frl_fail(-4, "decoder_mse_bwd: workspace too small");
#define DF_BWD_ARGS z, w1, b1, w2, b2, target, mask, gscale, stats, dz, dw1, db1, dw2, db2, P, Cz, (char*)ws, stream
  if (g_dec_subgroups && P >= 128) {
    if (Cz <= 16) return launch_dec_bwd_sg<1, false, 1>(DF_BWD_ARGS);
    if (Cz <= 32) return launch_dec_bwd_sg<1>(DF_BWD_ARGS);
    return launch_dec_bwd<2, 8>(DF_BWD_ARGS);
  }
  if (Cz <= 16) return launch_dec_bwd<1, 8, false, 1>(DF_BWD_ARGS);
  if (Cz <= 32) return launch_dec_bwd<1, 8>(DF_BWD_ARGS);
  return launch_dec_bwd<2, 4>(DF_BWD_ARGS);
#undef DF_BWD_ARGS
}

// ---- one pass (train step) ----
// buffer of a one-pass call: the layout of the backward workspace (slabs | packed weights) followed by the workgroups' loss partials
static size_t df_onepass_partial_off(int64_t P, int Cz) { return ((frl_decoder_mse_workspace_bytes(P, Cz) + 255) / 256) * 256; }
size_t frl_decoder_mse_onepass_bytes(int64_t P, int Cz) { return df_onepass_partial_off(P, Cz) + (size_t)256 * 2 * sizeof(double); }

// Loss AND gradients from one pass over (z, target): the backward kernels of frl_decoder_mse_bwd with the loss accumulated on the side.
// gscale: device scalar, the gradient the caller promises the loss will receive (null: 1).  out = {loss, n_valid} as frl_decoder_mse_fwd
// writes it; dz as frl_decoder_mse_bwd writes it.  The weight-gradient slabs stay unreduced in `buf` (which the caller keeps untouched until
// frl_decoder_mse_reduce on it has run -- inside frl_defer_begin/flush: until the flush); *nslab receives their number.  ctl: 4 zeroed
// 32-bit words that no concurrent call shares (the mask count's ticket and total; the call leaves them zero).
int frl_decoder_mse_fwd_bwd(const void* z, const float* w1, const float* b1, const float* w2, const float* b2, const void* target,
                            const uint8_t* mask, const float* gscale, float* out, void* dz, void* buf, size_t buf_bytes, void* ctl,
                            int* nslab, int64_t P, int Cz, hipStream_t stream) {
  if (P <= 0) return frl_fail(-2, "decoder_mse_fwd_bwd: empty input");
  if (Cz < 1 || Cz > 64) return frl_fail(-2, "decoder_mse_fwd_bwd: latent width must be 1..64");
  if (buf_bytes < frl_decoder_mse_onepass_bytes(P, Cz)) return frl_fail(-4, "decoder_mse_fwd_bwd: buffer too small");
  if (out == nullptr || dz == nullptr || ctl == nullptr || nslab == nullptr) return frl_fail(-2, "decoder_mse_fwd_bwd: null output");
  unsigned* c = (unsigned*)ctl;
  DecLoss<true> la;
  la.partial = reinterpret_cast<double*>((char*)buf + df_onepass_partial_off(P, Cz));
  la.out = out;
  la.out_w = out;
  la.nv_host = (float)((double)P * (double)DF_F);
  if (mask != nullptr) {
    int64_t g = (P + 256 * 64 - 1) / (256 * 64);
    if (g > 128) g = 128;
    FRL_LAUNCH(dec_mask_count_kernel, dim3((unsigned)g), dim3(256), 0, stream, mask, P, c, out);
    la.nv_host = -1.f;
  }
#define DF_ONE_ARGS z, w1, b1, w2, b2, target, mask, gscale, nullptr, dz, nullptr, nullptr, nullptr, nullptr, P, Cz, (char*)buf, stream, la, nslab
  if (g_dec_subgroups && P >= 128) {
    if (Cz <= 16) return launch_dec_bwd_sg<1, true, 1>(DF_ONE_ARGS);
    if (Cz <= 32) return launch_dec_bwd_sg<1, true>(DF_ONE_ARGS);
    return launch_dec_bwd<2, 8, true>(DF_ONE_ARGS);
  }
  if (Cz <= 16) return launch_dec_bwd<1, 8, true, 1>(DF_ONE_ARGS);
  if (Cz <= 32) return launch_dec_bwd<1, 8, true>(DF_ONE_ARGS);
  return launch_dec_bwd<2, 4, true>(DF_ONE_ARGS);
#undef DF_ONE_ARGS
}

// The slab reduction of a one-pass call: buf / nslab from frl_decoder_mse_fwd_bwd -> dw1 [128][Cz], db1 [128], dw2 [64][128], db2 [64], in the
// summation order of frl_decoder_mse_bwd.  Parked when a deferral is open (it then launches nothing), else a launch on `stream`.
int frl_decoder_mse_reduce(const void* buf, int nslab, float* dw1, float* db1, float* dw2, float* db2, int Cz, hipStream_t stream) {
  if (Cz < 1 || Cz > 64 || nslab < 1 || nslab > 512) return frl_fail(-2, "decoder_mse_reduce: bad latent width or slab count");
  const int czp = Cz <= 32 ? 32 : 64;
  const size_t slab_n = (size_t)DF_F * DF_H + DF_H * czp + DF_F + DF_H;
  launch_slab_reduce_deferrable<float, DecEpi>((const float*)buf, nslab, (int64_t)slab_n, DecEpi{dw2, dw1, db2, db1, Cz, czp, DF_F, DF_H}, stream);
  return frl_check_launch("decoder_mse_reduce");
}

}  // extern "C"
