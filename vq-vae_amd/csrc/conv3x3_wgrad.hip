// Weight gradient of the 3x3 convolutions, bf16 band kernel (gfx950):
//   dW[oc][ic][dy][dx] = sum_{b,y,x} (dY .* act'(Y))[b,y,x,oc] * X[b,y+dy-1,x+dx-1,ic],   db[oc] = sum (dY .* act'(Y))[b,y,x,oc]
// Replaces autograd's conv2d weight gradient for spatial.py:247-263,296-313 (mix backbone, gate net); the generic kernel of
// conv3x3.hip stays for float32, ragged shapes and channel counts that are not multiples of 64.
//
// Work item = (8 x 32-pixel band of one image, 64 input channels); a workgroup (8 waves, one per CU, persistent) walks its items with
// everything one item ahead:
//   * the 10 x 34-pixel halo of X arrives by LDS-DMA (global_load_lds_dwordx4: no registers, 43 KB in flight per workgroup); pixels
//     outside the image are fetched from a page of zeros, so the DMA needs no predication;
//   * dY and Y of the band are prefetched into registers behind the MFMA phase of the current item, multiplied (act') and written to
//     the other dY buffer after it: ONE barrier per item;
//   * both LDS tiles are unpadded 128-byte pixel rows; the 32-byte windows of a row are permuted by a function of the pixel's COLUMN
//     (bits 1 and 3), which makes the row-major 16-byte writes, the DMA and the transposing ds_read_b64_tr_b16 fragment reads of all
//     nine taps conflict-free, and keeps every fragment address = lane constant + compile-time offset;
//   * a k-step of the contraction is one 32-pixel image row: per k-step a wave reads 2 dY^T and 9 X fragments for 18 MFMAs
//     (its 16 input channels x 32 output channels x 9 taps stay in 72 accumulator registers for the whole kernel).
// Output: per-workgroup float32 slabs in the layout of the generic kernel (tap-major), summed in a fixed order by slab_reduce_t.
#include "frl_common.hpp"
#include "frl_host.hpp"
#include <string.h>
#include <type_traits>

#define C3V_TH 8
#define C3V_TW 32
#define C3V_HP 34                           // halo row pitch (pixels)
#define C3V_HPIX (10 * C3V_HP)              // 340 halo pixels
#define C3V_DY_BYTES (C3V_TH * C3V_TW * 128)
#define C3V_NPIECE 43                       // 1 KB DMA pieces per halo (43 x 8 pixels >= 340)
#define C3V_HALO_BYTES (C3V_NPIECE * 1024)
#define C3V_LDS (2 * C3V_DY_BYTES + 2 * C3V_HALO_BYTES)

__device__ uint4 c3v_zero_page[64];         // 1 KB of zeros: source of the halo pixels outside the image

// 32-byte window permutation of a pixel row, from the pixel's column inside its tile / halo row
__device__ __forceinline__ int c3v_f(int col) { return ((col >> 1) & 1) | (((col >> 3) & 1) << 1); }

__device__ __forceinline__ bf16x8 c3v_tr8(const char* smem, int lo, int hi) {
  const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(smem + lo));
  const bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(smem + hi));
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// One launch serves several weight gradients over images of one shape (B, H, W): a table of up to C3V_MAX_ENTRIES entries travels by
// value in the kernel-argument segment (as FrlDeferTable, defer.hip); entry e owns the workgroups [first_wg, first_wg + nwg).
// A UNIT is what one workgroup of the single call owns: `tiles_per_wg` consecutive tiles, accumulated from zero per 64-channel chunk.
//   nunits == 1 (the single call; merged calls whose tiles all fit the grid): workgroup wg owns unit wg, all `ncks` chunks, slab wg.
//   nunits  > 1 (merged call): workgroup wg owns the units wg, wg + unit_stride, ... and ONE chunk (ck_base); each unit is accumulated
//   from zero and then added to slab wg in float32, in unit order: exactly the chain in which the fixed-order slab reduction adds the
//   single call's slabs wg, wg + 64, wg + 128, wg + 192 (frl_reduce.hpp), so the reduced gradients keep the single call's bits.
#define C3V_MAX_JOBS 4
#define C3V_MAX_ENTRIES 8
struct C3vJob {
  const bf16* dY;
  const bf16* Ymask;
  const bf16* X;
  float* slab;
  int mask_act, Cin, Cout, oc_base, first_wg, nwg, tiles_per_wg, nunits, unit_stride, ck_base, ncks, pad_;
};
struct C3vTable {
  int njobs, B, H, W;
  C3vJob job[C3V_MAX_ENTRIES];
};

// the work of workgroup `wg` of one table entry (Cin: all input channels of the convolution = the channel stride of X and of the slab)
__device__ __forceinline__ void c3v_band_body(const bf16* __restrict__ dY, const bf16* __restrict__ Ymask, int mask_act, const bf16* __restrict__ X,
                                              float* __restrict__ slab, int B, int H, int W, int Cin, int Cout, int oc_base, int tiles_per_wg,
                                              int nunits, int unit_stride, int ck_base, int ncks, int wg, char* smem) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kc = lane >> 4;
  const int ib = wave & 3, og = wave >> 2;                       // 16 input channels of the 64-chunk; 32 output channels
  const int tiles_x = W / C3V_TW, tiles_y = H / C3V_TH;
  const int ntiles = B * tiles_x * tiles_y;
  const int t_begin = wg * tiles_per_wg;
  const int t_end = (t_begin + tiles_per_wg) < ntiles ? (t_begin + tiles_per_wg) : ntiles;
  const int ntl = t_end > t_begin ? t_end - t_begin : 0;
  const bool units = nunits > 1;                                 // (uniform) several units, one chunk
  int nitems = ntl * ncks;                                       // one unit: item i = chunk i / ntl, tile t_begin + i % ntl
  if (units) {                                                   // several: item i = unit i / tiles_per_wg, its tile i % tiles_per_wg
    nitems = 0;                                                  // (units are full up to the last busy one, then empty)
    for (int t = 0; t < nunits; ++t) {
      const int left = ntiles - (wg + t * unit_stride) * tiles_per_wg;
      nitems += left < 0 ? 0 : (left < tiles_per_wg ? left : tiles_per_wg);
    }
  }
  const int64_t slab_n = (int64_t)64 * Cin * 9 + 64;
  float* my = slab + (int64_t)wg * slab_n;

  // ---- lane constants of the fragment reads: column (inside a row) of the lane's first pixel, window swizzle, 8-byte half ----
  int aoff[2][2], boff[3][2];                                    // [output block o][lo / hi], [dx][lo / hi]
#pragma unroll
  for (int hi = 0; hi < 2; ++hi) {
    const int col = 8 * kc + (r16 >> 2) + 4 * hi;
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const int c = 2 * (og * 2 + o) + ((r16 & 3) >> 1);
      aoff[o][hi] = col * 128 + ((c ^ (c3v_f(col) << 1)) << 4) + (r16 & 1) * 8;
    }
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int hc = col + dx;
      const int c = 2 * ib + ((r16 & 3) >> 1);
      boff[dx][hi] = hc * 128 + ((c ^ (c3v_f(hc) << 1)) << 4) + (r16 & 1) * 8;
    }
  }

  auto item_geom = [&](int i, int& b, int& y0, int& x0, int& ck) {
    int tile;
    if (units) {
      const int t = i / tiles_per_wg;
      tile = (wg + t * unit_stride) * tiles_per_wg + (i - t * tiles_per_wg);
      ck = ck_base;
    } else {
      tile = t_begin + i % ntl;
      ck = ck_base + ((i / ntl) << 6);
    }
    b = tile / (tiles_x * tiles_y);
    const int tyx = tile % (tiles_x * tiles_y);
    y0 = (tyx / tiles_x) * C3V_TH;
    x0 = (tyx % tiles_x) * C3V_TW;
  };
  // ---- halo of one item by LDS-DMA: piece p (8 halo pixels = 1 KB) is issued by wave p % 8 ----
  auto dma_halo = [&](int i, int dst) {
    int b, y0, x0, ck;
    item_geom(i, b, y0, x0, ck);
    const bf16* xb = X + (((int64_t)b * H) * W) * Cin + ck;
    int lane_ = lane;
    asm volatile("" : "+v"(lane_));                              // (opaque: the per-piece lane constants are rebuilt per item, not kept in 40 registers)
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int piece = j * 8 + wave;
      if (piece < C3V_NPIECE) {                                  // (wave-uniform)
        const int chunk = piece * 64 + lane_;
        const int hp = chunk >> 3, c = chunk & 7;
        const int hr = (hp * 1928) >> 16, hc = hp - hr * C3V_HP;  // hp / 34 for hp < 344
        const int gy = y0 + hr - 1, gx = x0 + hc - 1;
        const bool ok = hp < C3V_HPIX && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const bf16* src = ok ? xb + ((int64_t)gy * W + gx) * Cin + ((c ^ (c3v_f(hc) << 1)) << 3)
                             : reinterpret_cast<const bf16*>(c3v_zero_page) + (lane_ << 3);
        const int ldst = dst + piece * 1024;
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(src), "s"(ldst) : "memory");
      }
    }
  };
  // ---- dY / Y of one item into registers (4 x 16 bytes each per thread), then masked and written to a dY buffer ----
  bf16x8 ra[4], rm[4];
  auto fetch_dy = [&](int i) {
    int b, y0, x0, ck;
    item_geom(i, b, y0, x0, ck);
    int tid_ = tid;
    asm volatile("" : "+v"(tid_));
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int v = tid_ + 512 * u;
      const int px = v >> 3, c = v & 7;
      const int64_t off = (((int64_t)b * H + y0 + (px >> 5)) * W + x0 + (px & 31)) * Cout + oc_base + c * 8;
      ra[u] = *reinterpret_cast<const bf16x8*>(dY + off);
      if (Ymask != nullptr) rm[u] = *reinterpret_cast<const bf16x8*>(Ymask + off);
    }
  };
  auto commit_dy = [&](int dst) {
    int tid_ = tid;
    asm volatile("" : "+v"(tid_));
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int v = tid_ + 512 * u;
      const int px = v >> 3, c = v & 7;
      bf16x8 val = ra[u];
      if (Ymask != nullptr) {
#pragma unroll
        for (int e = 0; e < 8; ++e) val[e] = (bf16)((float)val[e] * act_bwd_from_y((float)rm[u][e], mask_act));
      }
      *reinterpret_cast<bf16x8*>(smem + dst + px * 128 + ((c ^ (c3v_f(px & 31) << 1)) << 4)) = val;
    }
  };

  f32x4 acc[9][2], accb[2];
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    accb[o] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) acc[tap][o] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  auto write_chunk = [&](int ck) {                               // slab part of one input-channel chunk, then clear the accumulators
    int lane_ = lane;
    asm volatile("" : "+v"(lane_));                              // (slab addresses are built here, not carried through the item loop)
    float* mine = my + (int64_t)(og * 32 + (lane_ >> 4) * 4) * Cin + ck + ib * 16 + (lane_ & 15);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int o = 0; o < 2; ++o) {
#pragma unroll
        for (int r = 0; r < 4; ++r) mine[((int64_t)tap * 64 + o * 16 + r) * Cin] = acc[tap][o][r];
        acc[tap][o] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
  };
  // a later unit of the workgroup: slab += accumulators, each lane on the addresses it stored itself (its earlier stores have been waited
  // for; the loads are device-scope, past the CU's vector cache); float32 adds in unit order = the reduction's chain over the single
  // call's slabs
  auto add_chunk = [&](int ck) {
    int lane_ = lane;
    asm volatile("" : "+v"(lane_));
    float* mine = my + (int64_t)(og * 32 + (lane_ >> 4) * 4) * Cin + ck + ib * 16 + (lane_ & 15);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int o = 0; o < 2; ++o) {
        float old[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) old[r] = __hip_atomic_load(mine + ((int64_t)tap * 64 + o * 16 + r) * Cin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int r = 0; r < 4; ++r) mine[((int64_t)tap * 64 + o * 16 + r) * Cin] = old[r] + acc[tap][o][r];
        acc[tap][o] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
  };
  auto write_bias = [&](bool first) {                            // column 0 of the "ones" product holds the row sums
    if (ib == 0 && r16 == 0) {
      float* mb = my + (int64_t)64 * Cin * 9 + og * 32 + kc * 4;
#pragma unroll
      for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = accb[o][r];
          if (!first) v = __hip_atomic_load(mb + o * 16 + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + v;
          mb[o * 16 + r] = v;
        }
    }
#pragma unroll
    for (int o = 0; o < 2; ++o) accb[o] = f32x4{0.f, 0.f, 0.f, 0.f};
  };

  if (nitems > 0) {
    dma_halo(0, 2 * C3V_DY_BYTES);
    fetch_dy(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    commit_dy(0);
  }
  __syncthreads();
  for (int i = 0; i < nitems; ++i) {
    const int cur = i & 1;
    const int dyb = cur * C3V_DY_BYTES, hb = 2 * C3V_DY_BYTES + cur * C3V_HALO_BYTES;
    if (i + 1 < nitems) {                                        // next item: halo by DMA, dY / Y into registers
      dma_halo(i + 1, 2 * C3V_DY_BYTES + (cur ^ 1) * C3V_HALO_BYTES);
      fetch_dy(i + 1);
    }
    // (fully unrolled, the compiler shares the X fragments of a halo row between the taps of three k-steps: 104 instead of 176 LDS
    // reads per item)
    // (two copies of the fully unrolled k loop, so that the bias MFMAs of the (input chunk 0, ib == 0) waves cost the others no branch
    // inside it: a branch per k-step ends the basic block and with it the overlap of one step's LDS reads with the previous MFMAs)
    auto contract = [&](auto with_bias) {
      int r16_ = r16;
      asm volatile("" : "+v"(r16_));
      const bf16 one_ = (r16_ == 0) ? (bf16)1.f : (bf16)0.f;       // B operand that sums the k dimension into output column 0
      const bf16x8 ones = bf16x8{one_, one_, one_, one_, one_, one_, one_, one_};
#pragma unroll
      for (int ks = 0; ks < C3V_TH; ++ks) {
        bf16x8 af[2];
#pragma unroll
        for (int o = 0; o < 2; ++o) af[o] = c3v_tr8(smem, dyb + ks * (C3V_TW * 128) + aoff[o][0], dyb + ks * (C3V_TW * 128) + aoff[o][1]);
        if constexpr (decltype(with_bias)::value) {
#pragma unroll
          for (int o = 0; o < 2; ++o) accb[o] = mfma16(af[o], ones, accb[o]);
        }
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int dy = tap / 3, dx = tap % 3;
          const int ro = hb + (ks + dy) * (C3V_HP * 128);
          const bf16x8 bfr = c3v_tr8(smem, ro + boff[dx][0], ro + boff[dx][1]);
#pragma unroll
          for (int o = 0; o < 2; ++o) acc[tap][o] = mfma16(af[o], bfr, acc[tap][o]);
        }
      }
    };
    if ((units ? ck_base == 0 : i < ntl) && ib == 0) contract(std::true_type{});   // (uniform) the bias gradient rides with input chunk 0
    else contract(std::false_type{});
    if (i + 1 < nitems) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // dY / Y registers and this wave's DMA pieces have landed
      commit_dy((cur ^ 1) * C3V_DY_BYTES);
    }
    if (units) {                                                 // (uniform) last tile of a unit
      if ((i + 1) % tiles_per_wg == 0 || i + 1 == nitems) {
        if (i < tiles_per_wg) write_chunk(ck_base); else add_chunk(ck_base);
        if (ck_base == 0) write_bias(i < tiles_per_wg);
      }
    } else if ((i + 1) % ntl == 0) write_chunk((i / ntl) << 6);  // (uniform) last tile of an input-channel chunk
    __syncthreads();
  }
  if (units) return;
  if (nitems == 0) {                                             // a workgroup without tiles still owns a slab: zeros
    for (int ck = 0; ck < Cin; ck += 64) write_chunk(ck);
  }
  write_bias(true);
}

__global__ __launch_bounds__(512) void conv3x3_wgrad_band_kernel(const C3vTable tab) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int j = 0;
  while (j + 1 < tab.njobs && (int)blockIdx.x >= tab.job[j + 1].first_wg) ++j;     // block-uniform: scalar loads from the argument segment
  const C3vJob& job = tab.job[j];
  const int wg = (int)blockIdx.x - job.first_wg;
  if (wg >= job.nwg) return;
  c3v_band_body(job.dY, job.Ymask, job.mask_act, job.X, job.slab, tab.B, tab.H, tab.W, job.Cin, job.Cout, job.oc_base, job.tiles_per_wg, job.nunits,
                job.unit_stride, job.ck_base, job.ncks, wg, smem);
}

// ---- host side (called from frl_conv3x3_bwd_weight, conv3x3.hip) ----
static int g_c3v_off = 0;

bool c3v_supported(int B, int H, int W, int Cin, int Cout, int dtype) {
  return !g_c3v_off && dtype == FRL_BF16 && B > 0 && (W % C3V_TW) == 0 && (H % C3V_TH) == 0 && (Cin % 64) == 0 && (Cout % 64) == 0;
}
int c3v_workgroups(int B, int H, int W) {
  const int tiles = B * (H / C3V_TH) * (W / C3V_TW);
  return tiles < 256 ? tiles : 256;
}
int c3v_launch(const void* dy, const void* ym, int act, const void* x, float* ws, int B, int H, int W, int Cin, int Cout, int oc_base,
               hipStream_t st) {
  const int nwg = c3v_workgroups(B, H, W);
  const int tiles = B * (H / C3V_TH) * (W / C3V_TW);
  const int tpw = (tiles + nwg - 1) / nwg;
  C3vTable tab;
  memset(&tab, 0, sizeof(tab));
  tab.njobs = 1; tab.B = B; tab.H = H; tab.W = W;
  tab.job[0] = C3vJob{(const bf16*)dy, (const bf16*)ym, (const bf16*)x, ws, act, Cin, Cout, oc_base, 0, nwg, tpw, 1, 0, 0, Cin / 64, 0};
  auto kern = conv3x3_wgrad_band_kernel;
  FRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C3V_LDS));
  FRL_LAUNCH_AS("conv3x3_wgrad_kernel", kern, dim3(nwg), dim3(512), C3V_LDS, st, tab);
  return frl_check_launch("conv3x3_bwd_weight");
}

// ---- several weight gradients over images of one shape in ONE launch (frl_conv3x3_bwd_weight_multi, conv3x3.hip) ----
// The split of the workgroup budget over the jobs, a function of the shapes alone (mirrored by frl_hip/wgrad_split.py), chosen so that
// every reduced gradient keeps the bits of the single call; tiles = B * (H / 8) * (W / 32), budget 256 workgroups:
//   * the jobs' tiles together fit the budget: every workgroup owns one tile and all chunks (nslab_j = tiles), as in the single call;
//   * tiles >= 256 (the single call runs 256 workgroups of tpw = ceil(tiles / 256) tiles and reduces 256 slabs, in chains of four:
//     k, k + 64, k + 128, k + 192): 64 workgroups per (job, 64-channel chunk), workgroup k runs those four units one after the other and
//     adds them up in its slab in that order: nslab_j = 64, a quarter of the slabs, and items per workgroup = 4 * tpw for every job;
//   * anything else (or more than 8 chunks in all) is no case for the merged launch.
static int g_c3v_multi = 1;
#define C3V_BUDGET 256
#define C3V_CHAIN 4                          // slabs per chain of the reduction at 256 slabs (frl_reduce.hpp: k += 64)

bool c3v_multi_supported(int njobs, int B, int H, int W, const int* cin, const int* cout, int dtype) {
  if (!g_c3v_multi || njobs < 1 || njobs > C3V_MAX_JOBS) return false;
  int chunks = 0;
  for (int j = 0; j < njobs; ++j) {
    if (cout[j] != 64 || !c3v_supported(B, H, W, cin[j], cout[j], dtype)) return false;
    chunks += cin[j] / 64;
  }
  const int64_t tiles = (int64_t)B * (H / C3V_TH) * (W / C3V_TW);
  return tiles * njobs <= C3V_BUDGET || (tiles >= C3V_BUDGET && chunks <= C3V_MAX_ENTRIES);
}
// -> grid; nslab / tpw / nunits [njobs] are written (call only where c3v_multi_supported holds)
int c3v_multi_split(int njobs, int B, int H, int W, const int* cin, int* nslab, int* tpw, int* nunits) {
  const int64_t tiles = (int64_t)B * (H / C3V_TH) * (W / C3V_TW);
  int grid = 0;
  for (int j = 0; j < njobs; ++j) {
    if (tiles * njobs <= C3V_BUDGET) {
      nslab[j] = (int)tiles; tpw[j] = 1; nunits[j] = 1;
      grid += nslab[j];
    } else {
      nslab[j] = C3V_BUDGET / C3V_CHAIN; tpw[j] = (int)((tiles + C3V_BUDGET - 1) / C3V_BUDGET); nunits[j] = C3V_CHAIN;
      grid += nslab[j] * (cin[j] / 64);
    }
  }
  return grid;
}
int c3v_launch_multi(int njobs, const void* const* dy, const void* const* ym, const int* act, const void* const* x, float* const* slab, int B,
                     int H, int W, const int* cin, const int* nslab, const int* tpw, const int* nunits, hipStream_t st) {
  C3vTable tab;
  memset(&tab, 0, sizeof(tab));
  tab.B = B; tab.H = H; tab.W = W;
  int e = 0, grid = 0;
  const int64_t tiles = (int64_t)B * (H / C3V_TH) * (W / C3V_TW);
  for (int j = 0; j < njobs; ++j) {
    // every workgroup must own at least one tile: the kernel stores a slab only behind a unit's last tile, and the reduction reads all
    // nslab slabs (tiles >= 256 gives >= 128 busy units for the 64 workgroups of a chained entry; one tile per workgroup otherwise)
    if (nslab[j] < 1 || tpw[j] < 1 || (int64_t)(nslab[j] - 1) * tpw[j] >= tiles) return frl_fail(-2, "conv3x3_bwd_weight_multi: a workgroup without a tile");
    const int parts = nunits[j] > 1 ? cin[j] / 64 : 1;             // several units: one table entry per 64-channel chunk
    for (int q = 0; q < parts; ++q) {
      if (e >= C3V_MAX_ENTRIES) return frl_fail(-2, "conv3x3_bwd_weight_multi: too many chunks for one launch");
      tab.job[e++] = C3vJob{(const bf16*)dy[j], (const bf16*)ym[j], (const bf16*)x[j], slab[j], act[j], cin[j], 64, 0, grid, nslab[j], tpw[j],
                            nunits[j], C3V_BUDGET / C3V_CHAIN, q * 64, nunits[j] > 1 ? 1 : cin[j] / 64, 0};
      grid += nslab[j];
    }
  }
  tab.njobs = e;
  auto kern = conv3x3_wgrad_band_kernel;
  FRL_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C3V_LDS));
  FRL_LAUNCH_AS("conv3x3_wgrad_multi_kernel", kern, dim3(grid), dim3(512), C3V_LDS, st, tab);
  return frl_check_launch("conv3x3_bwd_weight_multi");
}

extern "C" {
// A/B hook: 0 makes frl_conv3x3_bwd_weight_multi run its jobs one after the other through the single-call route (the bits of
// frl_conv3x3_bwd_weight); default 1: one launch.  Returns the previous setting.
int frl_conv3x3_wgrad_multi(int on) {
  const int was = g_c3v_multi;
  g_c3v_multi = on ? 1 : 0;
  return was;
}

// Test / A-B hook: 1 routes every 3x3 weight gradient through the generic kernel of conv3x3.hip; returns the previous setting.
int frl_conv3x3_wgrad_force_generic(int on) {
  const int was = g_c3v_off;
  g_c3v_off = on ? 1 : 0;
  return was;
}
}
