// Streaming form of the pointwise weight gradient (pw_wgrad.hip) for thin outputs: bf16, Cin = 64, Cout in {4, 8, 12, 16}, no mask,
// no time shift, whole 64-row tiles.  The 64 -> 12 phase head is the case it exists for: 200 MB of dh and y3 per step against
// 0.8 GFLOP, a pure streaming pass.
//
// Same partition, same slabs and same bits as pw_wgrad_kernel<bf16, 1, 4>: a workgroup reduces its contiguous row range in increasing
// order, 32 rows per k-step, into ONE accumulator set (four 16-column blocks + the "ones" bias column) held by wave 0; every MFMA sees
// the operands wave 0 of the generic kernel sees, in the same sequence.  What differs is how the rows arrive:
//   * a ring of PWT_D tile buffers in LDS, filled by LDS-DMA (global_load_lds_dwordx4: no registers) by all four waves, PWT_D - 1 tiles
//     ahead of the consuming wave: two resident workgroups keep 2 x 3 x 9.5 KB = 57 KB per CU in flight (the generic kernel: 19 KB);
//   * one raw s_barrier per tile.  Each wave retires its own pieces of tile t with a counted s_waitcnt vmcnt(N) that leaves the younger
//     tiles in flight; the barrier then (a) makes tile t readable and (b) frees the buffer of tile t - 1, which wave 0 has finished
//     reading (lgkmcnt(0) before the barrier), for the DMA of tile t + PWT_D - 1 that every wave issues right after it;
//   * the x tile is written linearly by the DMA (128-byte rows); the 32-byte windows of a row are permuted by bits 1 and 3 of the row
//     through the DMA's per-lane SOURCE address, and the transposing ds_read_b64_tr_b16 fragment reads apply the same XOR (conflict-free,
//     as in conv3x3_wgrad.hip); the dY tile is the flat Cout-pitch run of the generic kernel;
//   * waves 1-3 only feed the ring: no fragment reads, no MFMAs.
// LDS is dynamic only (byte offsets double as M0 values of the DMA).
#include "frl_common.hpp"
#include "frl_host.hpp"

#define PWT_KP 64                              // rows per tile (= WG_KP of pw_wgrad.hip)
#ifndef PWT_D
#define PWT_D 4                                // ring depth (tiles): 3, 4, 6 and 8 measured, 3 and 4 fastest alone (38 us; 6 and 8: 40-41 us)
#endif
#define PWT_XB (PWT_KP * 128)                  // x tile: 64 rows x 64 bf16
#define PWT_YB 2048                            // dY tile slot: 64 rows x Cout bf16 <= 2 KB (the DMA writes whole 1 KB pieces)
#define PWT_SLOT (PWT_XB + PWT_YB)
#define PWT_LDS (PWT_D * PWT_SLOT)

// Every byte is read once, so the loads are non-temporal (nt): they do not displace what the kernels before this one left in the caches.
// Without nt the stream pushes those kernels' dirty lines out while it runs and shares the HBM with their write-back: measured alone
// after a 256 MB fill, 67 us against 35 us (38 / 34 us with nothing dirty); in the train step 53 us against 34.5 us.
__device__ __forceinline__ void pwt_glds16(const void* src, int lds_byte) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(lds_byte) : "memory");
}
template <int N> __device__ __forceinline__ void pwt_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// this wave's DMA of the oldest tile has landed; `rem` (wave-uniform) younger tiles of K instructions each stay in flight
template <int K> __device__ __forceinline__ void pwt_wait(int rem) {
  static_assert(PWT_D >= 3 && PWT_D - 2 <= 6 && 6 * K <= 63, "extend the chain below with the ring");
  if (rem >= 6) pwt_vmcnt<6 * K>();
  else if (rem == 5) pwt_vmcnt<5 * K>();
  else if (rem == 4) pwt_vmcnt<4 * K>();
  else if (rem == 3) pwt_vmcnt<3 * K>();
  else if (rem == 2) pwt_vmcnt<2 * K>();
  else if (rem == 1) pwt_vmcnt<K>();
  else pwt_vmcnt<0>();
}
__device__ __forceinline__ bf16x8 pwt_tr8(const char* smem, int lo, int hi) {
  const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(smem + lo));
  const bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(smem + hi));
  return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

template <int COUT>
__global__ __launch_bounds__(256) void pw_wgrad_thin_kernel(const bf16* __restrict__ dY, const bf16* __restrict__ X, float* __restrict__ slab,
                                                            int64_t P, int64_t rows_per_wg) {
  static_assert(COUT % 4 == 0 && COUT <= 16, "thin outputs only");
  constexpr int NVY = PWT_KP * COUT / 8;                       // 16-byte vectors of a dY tile (32 .. 128)
  constexpr int NPY = (NVY + 63) / 64;                         // 1 KB DMA pieces of a dY tile: waves 0 .. NPY - 1 issue one each
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kc = lane >> 4;

  const int64_t p_begin = (int64_t)blockIdx.x * rows_per_wg;
  int64_t p_end = p_begin + rows_per_wg;
  if (p_end > P) p_end = P;
  const int nt = p_end > p_begin ? (int)((p_end - p_begin) / PWT_KP) : 0;   // whole tiles: P and rows_per_wg are multiples of 64

  // ---- DMA of tile i into ring buffer `slot`: x pieces 2 wave, 2 wave + 1 (8 rows each), dY piece `wave` ----
  const int xr8 = lane >> 3, xc = lane & 7;                    // row inside a piece, 16-byte chunk of the row this lane WRITES
  auto issue = [&](int i, int slot) {
    const int64_t p0 = p_begin + (int64_t)i * PWT_KP;
    const int base = slot * PWT_SLOT;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int piece = 2 * wave + j;                           // rows 8 piece .. 8 piece + 7: bit 3 of the row = piece & 1
      const int f = ((xr8 >> 1) & 1) | ((piece & 1) << 1);
      pwt_glds16(X + (p0 + piece * 8 + xr8) * 64 + ((xc ^ (f << 1)) << 3), base + piece * 1024);
    }
    if (wave < NPY) {                                           // (wave-uniform) lanes past the tile re-read its last vector into the slot's tail
      int v = wave * 64 + lane;
      v = v < NVY ? v : NVY - 1;
      pwt_glds16(dY + p0 * COUT + v * 8, base + PWT_XB + wave * 1024);
    }
  };
  auto wait_oldest = [&](int rem) {
    if (wave < NPY) pwt_wait<3>(rem);
    else pwt_wait<2>(rem);
  };

  // ---- fragment addresses of wave 0 (bytes inside a ring buffer); row = 32 ks + 8 kc + (r16 >> 2) (+ 4 for the high half) ----
  const int fr = ((r16 >> 3) & 1) | ((kc & 1) << 1);           // window permutation of the lane's rows (bits 1 and 3: same for lo and hi, any ks)
  const int xrow = (8 * kc + (r16 >> 2)) * 128 + ((r16 & 3) >> 1) * 16 + (r16 & 1) * 8;
  int xoff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) xoff[i] = xrow + ((i ^ fr) << 5);
  const int yoff = PWT_XB + ((8 * kc + (r16 >> 2)) * COUT + 4 * (r16 & 3)) * 2;
  const bf16 one_ = (r16 == 0) ? (bf16)1.f : (bf16)0.f;         // B operand that sums the k dimension into output column 0
  const bf16x8 ones = bf16x8{one_, one_, one_, one_, one_, one_, one_, one_};

  f32x4 acc[4], accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  int issued = 0, islot = 0, cslot = 0;
  for (; issued < PWT_D - 1 && issued < nt; ++issued) {
    issue(issued, islot);
    ++islot;                                                    // (at most PWT_D - 1 tiles: no wrap yet)
  }
  for (int t = 0; t < nt; ++t) {
    wait_oldest(issued - 1 - t);                                // own pieces of tile t have landed
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");         // wave 0: the fragment reads of tile t - 1 are done
    __builtin_amdgcn_s_barrier();                               // tile t is complete; the buffer of tile t - 1 is free
    asm volatile("" ::: "memory");
    if (issued < nt) {
      issue(issued, islot);
      ++issued;
      islot = islot + 1 == PWT_D ? 0 : islot + 1;
    }
    if (wave == 0) {
      const char* tb = smem + cslot * PWT_SLOT;
#pragma unroll
      for (int ks = 0; ks < PWT_KP / 32; ++ks) {
        const bf16x8 af = pwt_tr8(tb, yoff + ks * (32 * COUT * 2), yoff + ks * (32 * COUT * 2) + 4 * COUT * 2);
        bf16x8 bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bf[i] = pwt_tr8(tb, xoff[i] + ks * (32 * 128), xoff[i] + ks * (32 * 128) + 4 * 128);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = mfma16(af, bf[i], acc[i]);
        accb = mfma16(af, ones, accb);
      }
    }
    cslot = cslot + 1 == PWT_D ? 0 : cslot + 1;
  }

  // ---- private slab of the workgroup: [Cout * 64] weights then [Cout] bias (zeros from a workgroup without rows) ----
  if (wave == 0) {
    float* my = slab + (int64_t)blockIdx.x * (COUT * 64 + COUT);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int oc = kc * 4 + r;
        if (oc < COUT) my[oc * 64 + i * 16 + r16] = acc[i][r];
      }
    if (r16 == 0) {                                             // column 0 of the "ones" product holds the row sums
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int oc = kc * 4 + r;
        if (oc < COUT) my[COUT * 64 + oc] = accb[r];
      }
    }
  }
}

// ---- host side (called from conv_tap_bwd_weight, pw_wgrad.hip) ----
static int g_wgrad_thin = 1;

bool pwt_supported(const void* dy, const void* ymask, const void* x, int64_t P, int Cin, int Cout, int64_t ldy, int T, int toff, int dtype,
                   int flags) {
  return g_wgrad_thin && dtype == FRL_BF16 && Cin == 64 && (Cout % 4) == 0 && Cout >= 4 && Cout <= 16 && ldy == Cout && ymask == nullptr &&
         T == 1 && toff == 0 && P > 0 && (P % PWT_KP) == 0 && (flags & 1) == 0 && ((uintptr_t)dy % 16) == 0 && ((uintptr_t)x % 16) == 0;
}

template <int COUT>
static void pwt_launch_t(const void* dy, const void* x, float* ws, int64_t P, int nwg, int64_t rows, hipStream_t st) {
  if (PWT_LDS > 64 * 1024) (void)hipFuncSetAttribute((const void*)pw_wgrad_thin_kernel<COUT>, hipFuncAttributeMaxDynamicSharedMemorySize, PWT_LDS);
  FRL_LAUNCH_AS("pw_wgrad_thin_kernel", pw_wgrad_thin_kernel<COUT>, dim3(nwg), dim3(256), PWT_LDS, st, (const bf16*)dy, (const bf16*)x, ws, P,
                rows);
}

// nwg workgroups of `rows` rows each (a multiple of 64), as launch_wgrad cuts them; ws holds nwg slabs of Cout * 64 + Cout floats
int pwt_launch(const void* dy, const void* x, float* ws, int64_t P, int Cout, int nwg, int64_t rows, hipStream_t st) {
  switch (Cout) {
    case 4: pwt_launch_t<4>(dy, x, ws, P, nwg, rows, st); break;
    case 8: pwt_launch_t<8>(dy, x, ws, P, nwg, rows, st); break;
    case 12: pwt_launch_t<12>(dy, x, ws, P, nwg, rows, st); break;
    case 16: pwt_launch_t<16>(dy, x, ws, P, nwg, rows, st); break;
    default: return frl_fail(-2, "pw_wgrad_thin: unsupported Cout");
  }
  return frl_check_launch("pw_wgrad_thin");
}

extern "C" {

// A/B hook: 1 (default) = eligible thin-output weight gradients take the streaming kernel, 0 = every call takes pw_wgrad_kernel;
// returns the previous setting.  Both routes give the same bits.
int frl_wgrad_thin(int on) {
  const int was = g_wgrad_thin;
  g_wgrad_thin = on ? 1 : 0;
  return was;
}

}  // extern "C"
