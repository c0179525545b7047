// Device tails shared by the loss kernels (soft_neighborhood.hip, evt_soft_neighborhood.hip, phase_margin.hip, contrastive.hip,
// spectral_negatives.hip).  Every helper states its summation order: the callers rely on it for bit-reproducible losses and gradients.
#pragma once
#include "frl_common.hpp"

// Compensated float32 sum over c = 0 .. W-1, in that order, of (a[c] - b[c])^2: the product's own rounding error comes from the fma, the
// additions' from a two-sum, and the error terms are added to the running sum once, at the end.  A plain running sum over 256 columns
// loses 3e-7 of a distance, which a logit of -d / tau = -45 turns into more than the loss bounds allow.
__device__ __forceinline__ float sumsq_diff(const float* __restrict__ a, const float* __restrict__ b, int W) {
  float s = 0.f, lo = 0.f;
  for (int c = 0; c < W; ++c) {
    const float df = a[c] - b[c];
    const float p = df * df, pe = fmaf(df, df, -p);
    const float n = s + p, bp = n - s;
    lo += ((s - (n - bp)) + (p - bp)) + pe;
    s = n;
  }
  return s + lo;
}

// Sum over an aligned group of 16 lanes; every lane of the group returns it.  Butterfly over the lane offsets 8, 4, 2, 1.
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
  return v;
}

// Sum of K f64 components over a workgroup of WAVES waves: wave_sum_d per component, lane 0 parks the wave's sum in red[wave][k], then
// thread k adds the wave sums to +0.0 in wave order, from wave 0.  The totals are left in red[0][0 .. K-1], behind a barrier.
template <int K, int WAVES>
__device__ __forceinline__ void block_sum_d(const double (&s)[K], double (*red)[K]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double v = wave_sum_d(s[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double v = 0.0;
    for (int w = 0; w < WAVES; ++w) v += red[w][threadIdx.x];
    red[0][threadIdx.x] = v;
  }
  __syncthreads();
}
