#pragma once
#include "frl_common.hpp"

// The "prepared codebook" image [control block][en: kpad floats][packed fragments] that frl_vq_prepare hands to the caller, who keeps it
// until the codebook changes.  Its two item kinds are device functions so that vq_prepare_kernel and the post-optimizer pack launch
// (pack_cache.hip: a FRL_PACK_VQ job) write the same bits from one piece of code.

// item k of the norms part: ||e_k||^2 of the code rounded to T (3e38 beyond K: such a code never wins); the items also zero the control
// block of the one-launch assignment kernels: {done, namb, ...} (64 ints), then counts_acc[K]
template <typename T>
__device__ __forceinline__ void vq_prepare_norm(const float* __restrict__ E, int K, int d, float* __restrict__ en, int kpad, int* __restrict__ ctl, int k) {
  if (k >= kpad) return;
  if (k < 64) ctl[k] = 0;
  if (k < K) ctl[64 + k] = 0;
  float s = 3.0e38f;
  if (k < K) {
    // one fmaf chain over the channels in order, whatever the width of the loads: the lane is alone with its row, so 16-byte loads,
    // four in flight, are what hides the latency (512 codes of 64 channels: vq_prepare_kernel 10.6 -> 5.8 us; as a job of the pack launch
    // the scalar loop, two items per thread, added 11 us to that launch, this form with one item per thread 0.1 us)
    s = 0.f;
    const float* row = E + (int64_t)k * d;
    if ((d & 3) == 0 && (reinterpret_cast<uintptr_t>(E) & 15) == 0) {
#pragma unroll 4
      for (int j = 0; j < d; j += 4) {
        const f32x4 r = *reinterpret_cast<const f32x4*>(row + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = to_f32(from_f32<T>(r[e]));
          s = fmaf(v, v, s);
        }
      }
    } else {
      for (int j = 0; j < d; ++j) {
        const float v = to_f32(from_f32<T>(row[j]));
        s = fmaf(v, v, s);
      }
    }
  }
  en[k] = s;
}

// item i of the packed part: one lane's MFMA A fragment of -2 e
template <typename T, int NF>
__device__ __forceinline__ void vq_prepare_frag(const float* __restrict__ E, int K, int d, typename DT<T>::frag_t* __restrict__ pk, int i) {
  constexpr int FE = DT<T>::FE;
  constexpr int q = NF * FE;
  const int ln = i & 63, fs = i >> 6;
  const int s = fs % NF, mb = fs / NF;
  const int code = mb * 16 + (ln & 15), kq = ln >> 4;
  if constexpr (FE == 8) {
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int ch = q * kq + 8 * s + e;
      v[e] = (code < K && ch < d) ? (bf16)(-2.f * (float)(bf16)E[(int64_t)code * d + ch]) : (bf16)0.f;
    }
    pk[i] = v;
  } else {
    const int ch = q * kq + s;
    pk[i] = (code < K && ch < d) ? -2.f * E[(int64_t)code * d + ch] : 0.f;
  }
}

// prep + pack in ONE launch (blocks [0, npack) write fragments, the rest the norms)
template <typename T, int NF>
__global__ void vq_prepare_kernel(const float* __restrict__ E, int K, int d, float* __restrict__ en, int kpad,
                                  typename DT<T>::frag_t* __restrict__ pk, int total, int npack_blocks, int* __restrict__ ctl) {
  if ((int)blockIdx.x >= npack_blocks) {
    vq_prepare_norm<T>(E, K, d, en, kpad, ctl, ((int)blockIdx.x - npack_blocks) * blockDim.x + threadIdx.x);
    return;
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) vq_prepare_frag<T, NF>(E, K, d, pk, i);
}
