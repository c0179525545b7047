// Backward of the quantizer (code sums, g_z, g_E), EMA codebook update and dead-code revival.
#pragma once
#include "vq_common.hpp"

// ---------------------------------------------------------------------------------------------
// backward: g_z = g_out + cz * (z - e_idx) ; code sums S_k = sum_{n: idx=k} z_n (LDS f32 accumulation)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void vq_bwd_kernel(const T* __restrict__ gout, const T* __restrict__ Z,
                                                     const float* __restrict__ E, const int32_t* __restrict__ idx,
                                                     const float* __restrict__ gscale, float cz_base, int64_t N, int K, int d,
                                                     int Kc, int64_t rows_per_wg, T* __restrict__ gz,
                                                     float* __restrict__ slab /*[grid][K][d]*/) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* acc = reinterpret_cast<float*>(smem);        // [Kc][d]
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  int64_t r1 = r0 + rows_per_wg;
  if (r1 > N) r1 = N;
  const float cz = cz_base * (gscale ? gscale[0] : 1.f);
  constexpr int VEC = DT<T>::VEC;
  const bool fast = (d % VEC) == 0;
  const int vpr = (d + VEC - 1) / VEC;                // vectors per row
  const int nchunks = (K + Kc - 1) / Kc;
  for (int c = 0; c < nchunks; ++c) {
    const int kbase = c * Kc;
    __syncthreads();
    for (int i = tid; i < Kc * d; i += 256) acc[i] = 0.f;
    __syncthreads();
    const int64_t nvec = (r1 > r0 ? (r1 - r0) : 0) * vpr;
    for (int64_t i = tid; i < nvec; i += 256) {
      const int64_t n = r0 + i / vpr;
      const int c0 = (int)(i % vpr) * VEC;
      const int k = idx[n];
      const bool mine = (k >= kbase && k < kbase + Kc);
      if (c == 0 || mine) {
        float zv[VEC];
        if (fast) Vec<T>::load(Z + n * (int64_t)d + c0, zv);
        else {
#pragma unroll
          for (int e = 0; e < VEC; ++e) zv[e] = (c0 + e < d) ? to_f32(Z[n * (int64_t)d + c0 + e]) : 0.f;
        }
        if (mine) {
#pragma unroll
          for (int e = 0; e < VEC; ++e)
            if (c0 + e < d) atomicAdd(&acc[(k - kbase) * d + c0 + e], zv[e]);
        }
        if (c == 0 && gz != nullptr) {
          float gv[VEC], ov[VEC];
          if (gout != nullptr) {
            if (fast) Vec<T>::load(gout + n * (int64_t)d + c0, gv);
            else {
#pragma unroll
              for (int e = 0; e < VEC; ++e) gv[e] = (c0 + e < d) ? to_f32(gout[n * (int64_t)d + c0 + e]) : 0.f;
            }
          } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) gv[e] = 0.f;
          }
#pragma unroll
          for (int e = 0; e < VEC; ++e) {
            const float ev = (c0 + e < d) ? to_f32(from_f32<T>(E[(int64_t)k * d + c0 + e])) : 0.f;
            ov[e] = gv[e] + cz * (zv[e] - ev);
          }
          if (fast) Vec<T>::store(gz + n * (int64_t)d + c0, ov);
          else {
#pragma unroll
            for (int e = 0; e < VEC; ++e)
              if (c0 + e < d) gz[n * (int64_t)d + c0 + e] = from_f32<T>(ov[e]);
          }
        }
      }
    }
    __syncthreads();
    const int kn = (K - kbase) < Kc ? (K - kbase) : Kc;
    float* dst = slab + ((int64_t)blockIdx.x * K + kbase) * d;
    for (int i = tid; i < kn * d; i += 256) dst[i] = acc[i];
  }
}

// ---------------------------------------------------------------------------------------------
// bf16 backward on the matrix cores: code sums S[k][:] = sum_{n: idx_n = k} z_n as the GEMM  onehot(idx)^T * Z  with K = rows.
// The one-hot A fragments are generated in registers from the staged indices (exact 0/1 in bf16), the z tile is fetched
// k-strided with ds_read_b64_tr_b16, products are exact and accumulated in f32 in a fixed order -> bit-reproducible,
// no LDS float atomics.  g_z = g_out + cz (z - e_idx) is fused on the staged tile.
// Each of the NWV = 8 waves (two per SIMD: LDS and matrix-pipe latencies of one hide behind the other) owns RB row blocks (16 codes
// each) x CB column blocks (16 channels) of the [Kc x d] chunk; chunks of the
// codebook are an outer loop (z is re-read once per chunk; one chunk covers K <= 512 at d <= 64).
// ---------------------------------------------------------------------------------------------
template <int RB, int CB, int NWV>
__global__ __launch_bounds__(64 * NWV) void vq_bwd_mfma_kernel(const bf16* __restrict__ gout, const bf16* __restrict__ Z, const bf16* __restrict__ ZQ,
                                                          const float* __restrict__ E,
                                                          const int32_t* __restrict__ idx, const float* __restrict__ gscale, float cz_base,
                                                          int64_t N, int K, int d, int64_t rows_per_wg, bf16* __restrict__ gz,
                                                          float* __restrict__ slab /*[grid][K][d]*/) {
  constexpr int DP = CB * 16, PITCH = DP + 8, KC = RB * NWV * 16, NTH = 64 * NWV;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* zt = reinterpret_cast<bf16*>(smem);                      // [64][PITCH]
  int* it = reinterpret_cast<int*>(zt + 64 * PITCH);             // [64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r16 = lane & 15, kc = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  int64_t r1 = r0 + rows_per_wg;
  if (r1 > N) r1 = N;
  const float cz = cz_base * (gscale ? gscale[0] : 1.f);
  const bool fast = (d % 8) == 0;
  const int vpr = DP / 8;
  const bf16 one = (bf16)1.f, zero = (bf16)0.f;
  for (int kbase = 0; kbase < K; kbase += KC) {
    f32x4 acc[RB][CB];
#pragma unroll
    for (int a = 0; a < RB; ++a)
#pragma unroll
      for (int b = 0; b < CB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    // register image of the NEXT 64-row tile (16-byte channel vectors): z, and on the first chunk g_out and z_q for the fused
    // g_z = g_out + cz (z - z_q); requested behind the MFMAs of the current tile
    constexpr int NV = (64 * (DP / 8) + NTH - 1) / NTH;
    const bool pre = fast && (ZQ != nullptr || gz == nullptr || kbase != 0);      // prefetch path: no codebook gather needed
    const bool want_gz = (kbase == 0 && gz != nullptr);
    bf16x8 rz[NV], rg[NV], rq[NV];
    auto fetch = [&](int64_t p0) {
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const int i = tid + u * NTH;
        const int row = i / vpr, c0 = (i % vpr) * 8;
        const int64_t n = p0 + row;
        const bool ok = i < 64 * vpr && n < r1 && c0 < d;
        const int64_t off = ok ? n * (int64_t)d + c0 : 0;
        bf16x8 v = *reinterpret_cast<const bf16x8*>(Z + off);
        if (!ok) v = bf16x8{};
        rz[u] = v;
        if (want_gz) {
          rg[u] = gout != nullptr ? *reinterpret_cast<const bf16x8*>(gout + off) : bf16x8{};
          rq[u] = *reinterpret_cast<const bf16x8*>(ZQ + off);
        }
      }
    };
    if (pre && r0 < r1) fetch(r0);
    for (int64_t p0 = r0; p0 < r1; p0 += 64) {
      __syncthreads();
      if (pre) {
#pragma unroll
        for (int u = 0; u < NV; ++u) {
          const int i = tid + u * NTH;
          if (i >= 64 * vpr) continue;
          const int row = i / vpr, c0 = (i % vpr) * 8;
          const int64_t n = p0 + row;
          if (want_gz && n < r1 && c0 < d) {
            float ov[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) ov[e] = (float)rg[u][e] + cz * ((float)rz[u][e] - (float)rq[u][e]);
            Vec<bf16>::store(gz + n * (int64_t)d + c0, ov);
          }
          *reinterpret_cast<bf16x8*>(zt + row * PITCH + c0) = rz[u];
        }
      } else {
      // stage 64 rows of z (zero padded) and their indices; first chunk also writes g_z
      for (int i = tid; i < 64 * vpr; i += NTH) {
        const int row = i / vpr, c0 = (i % vpr) * 8;
        const int64_t n = p0 + row;
        float zv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) zv[e] = 0.f;
        if (n < r1 && c0 < d) {
          if (fast) Vec<bf16>::load(Z + n * (int64_t)d + c0, zv);
          else {
#pragma unroll
            for (int e = 0; e < 8; ++e) if (c0 + e < d) zv[e] = (float)Z[n * (int64_t)d + c0 + e];
          }
          if (kbase == 0 && gz != nullptr) {
            const int k = idx[n];
            float gv[8], ov[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) gv[e] = 0.f;
            if (gout != nullptr) {
              if (fast) Vec<bf16>::load(gout + n * (int64_t)d + c0, gv);
              else {
#pragma unroll
                for (int e = 0; e < 8; ++e) if (c0 + e < d) gv[e] = (float)gout[n * (int64_t)d + c0 + e];
              }
            }
            float qv[8];
            if (ZQ != nullptr && fast) Vec<bf16>::load(ZQ + n * (int64_t)d + c0, qv);     // coalesced z_q instead of a codebook gather
            else {
#pragma unroll
              for (int e = 0; e < 8; ++e) qv[e] = (c0 + e < d) ? (float)(bf16)E[(int64_t)k * d + c0 + e] : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) ov[e] = gv[e] + cz * (zv[e] - qv[e]);
            if (fast) Vec<bf16>::store(gz + n * (int64_t)d + c0, ov);
            else {
#pragma unroll
              for (int e = 0; e < 8; ++e) if (c0 + e < d) gz[n * (int64_t)d + c0 + e] = (bf16)ov[e];
            }
          }
        }
        Vec<bf16>::store(zt + row * PITCH + c0, zv);
      }
      }
      if (tid < 64) it[tid] = (p0 + tid < r1) ? idx[p0 + tid] - kbase : -1;
      __syncthreads();
      if (pre && p0 + 64 < r1) fetch(p0 + 64);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int pix0 = ks * 32 + 8 * kc;
        int id8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) id8[j] = it[pix0 + j];
        bf16x8 bfr[CB];
#pragma unroll
        for (int b = 0; b < CB; ++b) {
          const bf16* a0 = zt + (pix0 + (r16 >> 2)) * PITCH + b * 16 + 4 * (r16 & 3);
          bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(a0));
          bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((bf16x4 __attribute__((address_space(3)))*)(a0 + 4 * PITCH));
          bfr[b] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
#pragma unroll
        for (int a = 0; a < RB; ++a) {
          const int code = (wave * RB + a) * 16 + r16;            // chunk-local code of this lane's A row
          bf16x8 af;
#pragma unroll
          for (int j = 0; j < 8; ++j) af[j] = (id8[j] == code) ? one : zero;
#pragma unroll
          for (int b = 0; b < CB; ++b) acc[a][b] = mfma16(af, bfr[b], acc[a][b]);
        }
      }
    }
    float* dst = slab + (int64_t)blockIdx.x * K * d;
#pragma unroll
    for (int a = 0; a < RB; ++a)
#pragma unroll
      for (int b = 0; b < CB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = kbase + (wave * RB + a) * 16 + kc * 4 + r, c = b * 16 + r16;
          if (k < K && c < d) dst[(int64_t)k * d + c] = acc[a][b][r];
        }
  }
}

// g_E[k][j] = ce * gscale * (n_k * e_k[j] - sum_wg slab[wg][k][j]);  also exports code sums when asked
template <typename T>
__global__ void vq_code_reduce_kernel(const float* __restrict__ slab, int nslab, const float* __restrict__ E,
                                      const int32_t* __restrict__ counts, const float* __restrict__ gscale, float ce_base,
                                      int K, int d, float* __restrict__ gE, float* __restrict__ sums_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)K * d) return;
  float s = 0.f;
  for (int w = 0; w < nslab; ++w) s += slab[(int64_t)w * K * d + i];
  if (sums_out) sums_out[i] = s;
  if (gE) {
    const float ce = ce_base * (gscale ? gscale[1] : 1.f);
    const float ev = to_f32(from_f32<T>(E[i]));
    gE[i] = ce * ((float)counts[i / d] * ev - s);
  }
}

// EMA update (scripts/train_vqvae.py:412-414): N_k, m_k moving averages + Laplace-smoothed codebook
// ok (optional device float): <= 0 leaves the running averages and the codebook untouched (isfinite guard of the train step)
__global__ __launch_bounds__(256) void vq_ema_kernel(const float* __restrict__ sums, const int32_t* __restrict__ counts, int K, int d,
                                                     float decay, float eps, float* __restrict__ ema_count,
                                                     float* __restrict__ ema_sum, float* __restrict__ E, const float* __restrict__ ok) {
  __shared__ double red[256];
  if (ok != nullptr && !(ok[0] > 0.f)) return;
  double s = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) {
    const float nc = decay * ema_count[k] + (1.f - decay) * (float)counts[k];
    ema_count[k] = nc;
    s += (double)nc;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  const float n = (float)red[0];
  for (int i = threadIdx.x; i < K * d; i += 256) {
    const int k = i / d;
    const float ms = decay * ema_sum[i] + (1.f - decay) * sums[i];
    ema_sum[i] = ms;
    const float smoothed = (ema_count[k] + eps) / (n + (float)K * eps) * n;
    E[i] = ms / smoothed;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Dead-code revival (CodebookManager of the legacy trainer, scripts/train_vqvae.py:92,196-198; the manager module itself is not
// in the reference tree -- build definition): a code whose usage count over the manager's window is below `min_count` is re-seeded
// with an encoder output row of the current batch, row index = splitmix64(seed + k) mod N; its AdamW moments are cleared so the
// stale momentum does not drag the new vector back.  One workgroup per code, no host round trip; `revived` counts them.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long vq_splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
template <typename T>
__global__ __launch_bounds__(64) void vq_revive_kernel(float* __restrict__ E, const long long* __restrict__ window_counts, long long min_count,
                                                       const T* __restrict__ z, long long N, int K, int d, unsigned long long seed,
                                                       float* __restrict__ m, float* __restrict__ v, int* __restrict__ revived) {
  const int k = blockIdx.x;
  if (k >= K || window_counts[k] >= min_count) return;
  const unsigned long long r = vq_splitmix64(seed + (unsigned long long)k) % (unsigned long long)N;
  for (int j = threadIdx.x; j < d; j += 64) {
    E[(size_t)k * d + j] = to_f32(z[(size_t)r * d + j]);
    if (m != nullptr) m[(size_t)k * d + j] = 0.f;
    if (v != nullptr) v[(size_t)k * d + j] = 0.f;
  }
  if (threadIdx.x == 0) atomicAdd(revived, 1);
}
