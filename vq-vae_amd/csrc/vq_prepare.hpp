#pragma once
#include "vq_common.hpp"

// prep + pack in ONE launch (blocks [0, npack) write fragments, the rest the norms): the "prepared codebook" image
// [en: kpad floats][packed fragments] that frl_vq_prepare hands to the caller, who keeps it until the codebook changes
template <typename T, int NF>
__global__ void vq_prepare_kernel(const float* __restrict__ E, int K, int d, float* __restrict__ en, int kpad,
                                  typename DT<T>::frag_t* __restrict__ pk, int total, int npack_blocks, int* __restrict__ ctl) {
  constexpr int FE = DT<T>::FE;
  constexpr int q = NF * FE;
  if ((int)blockIdx.x >= npack_blocks) {
    const int k = ((int)blockIdx.x - npack_blocks) * blockDim.x + threadIdx.x;
    if (k >= kpad) return;
    if (k < 64) ctl[k] = 0;                                  // control block of the resident kernel: {done, namb, ...}, counts_acc[K]
    if (k < K) ctl[64 + k] = 0;
    float s = 3.0e38f;                                     // codes beyond K never win
    if (k < K) {
      s = 0.f;
      for (int j = 0; j < d; ++j) {
        const float v = to_f32(from_f32<T>(E[(int64_t)k * d + j]));
        s = fmaf(v, v, s);
      }
    }
    en[k] = s;
    return;
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
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
