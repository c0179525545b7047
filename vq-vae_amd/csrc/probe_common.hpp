// What probe.hip and probe_full.hip share: the description of a call's inputs, its check, and the staging of a tile of 64 pixels.
#pragma once
#include "frl_common.hpp"
#include "frl_host.hpp"
#include "frl_moments.hpp"

#define PROBE_MAX_D 128
#define PROBE_MAX_CY 16

struct ProbeIn {
  const float* A;
  const float* Bs;
  const float* Y;
  const unsigned char* mask;
  const float* pivot;
  int Ta, Da, Tb, Db, Ty, Cy, B, T, P, PT, ntiles, fast;
};

static inline size_t probe_align16(size_t v) { return (v + 15) & ~(size_t)15; }

// the mask bits of a tile, one per pixel, the same in every wave
__device__ __forceinline__ unsigned long long probe_mask_bits(const ProbeIn& q, int b, int p0, int lane) {
  const unsigned char m = lane < moment_tile_rows(q.P, p0) ? q.mask[(size_t)b * q.P + p0 + lane] : (unsigned char)0;
  return __ballot(m != 0);
}

// stages columns [col0, col0 + Dn) of a tile straight from memory: src row minus pivot where the bit of `rows` is set, zero elsewhere.
// vec: the rows are whole 16-byte aligned float4 and so is the LDS row stride
__device__ __forceinline__ void probe_stage(float* vt, int ys, const float* piv, const float* __restrict__ src, int Ts, int Dn, int col0, bool vec,
                                            bool centre, const ProbeIn& q, int b, int t, int p0, unsigned long long rows, int tid) {
  const float* base = src + ((size_t)((int64_t)b * Ts + (Ts > 1 ? t : 0)) * q.P + p0) * Dn;
  if (vec) {
    const int q4 = Dn >> 2, n4 = MOMENT_ROWS * q4;
    for (int e = tid; e < n4; e += 256) {
      const int row = e / q4, c = (e - row * q4) * 4;
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if ((rows >> row) & 1ull) {
        v = *reinterpret_cast<const f32x4*>(base + (size_t)row * Dn + c);
        if (centre) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] -= piv[col0 + c + j];
        }
      }
      *reinterpret_cast<f32x4*>(vt + row * ys + col0 + c) = v;
    }
    return;
  }
  const int n = MOMENT_ROWS * Dn;
  for (int e = tid; e < n; e += 256) {
    const int row = e / Dn, c = e - row * Dn;
    float v = 0.f;
    if ((rows >> row) & 1ull) {
      v = base[(size_t)row * Dn + c];
      if (centre) v -= piv[col0 + c];
    }
    vt[row * ys + col0 + c] = v;
  }
}

// probe.hip: E [Cy][3] += G slabs of (SSE, sum (y - q), sum (y - q)^2) in the order of probe_eval_reduce_kernel, n += the G counts
void probe_launch_eval_reduce(const double* dsl, const long long* cnts, int G, int Cy, double* E, long long* n, hipStream_t stream);

static inline int probe_check(const char* what, const float* A, int Ta, int Da, const float* Bs, int Tb, int Db, const float* Y, int Ty, int Cy,
                              const unsigned char* mask, int B, int T, int64_t P, ProbeIn& q) {
  const char* why = nullptr;
  if (!A || !Y || !mask) why = "non-null A, Y and mask";
  else if (Da < 1 || Db < 0 || (Db > 0) != (Bs != nullptr)) why = "Da >= 1, and Bs exactly when Db > 0";
  else if (Da + Db > PROBE_MAX_D) why = "Da + Db <= 128 feature columns";
  else if (Cy < 1 || Cy > PROBE_MAX_CY) why = "1 <= Cy <= 16 targets";
  else if (B < 1 || T < 1 || P < 1) why = "B, T, P >= 1";
  else if ((Ta != 1 && Ta != T) || (Db > 0 && Tb != 1 && Tb != T) || (Ty != 1 && Ty != T)) why = "Ta, Tb and Ty each 1 or T";
  else if (!frl_obs_fit(B, T, P)) why = "B * T * P < 2^31 observations";
  if (why) return frl_failf(-2, "%s: needs %s", what, why);
  q.A = A; q.Bs = Bs; q.Y = Y; q.mask = mask; q.pivot = nullptr;
  q.Ta = Ta; q.Da = Da; q.Tb = Db ? Tb : 1; q.Db = Db; q.Ty = Ty; q.Cy = Cy;
  q.B = B; q.T = T; q.P = (int)P;
  q.ntiles = frl_moment_tiles(B, T, P, q.PT);
  // rows of whole float4 on 16-byte boundaries in every feature source: the register-prefetch path
  q.fast = (Da & 3) == 0 && ((uintptr_t)A & 15) == 0 && (Db == 0 || ((Db & 3) == 0 && ((uintptr_t)Bs & 15) == 0));
  return 0;
}
