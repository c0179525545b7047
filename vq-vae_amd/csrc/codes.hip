// Code-map decoding: out[p][:] = table[idx[p]][:] for a decoded-code table [K][F] (the decoder applied to the K codebook rows once).
// The decoder of the VQ-VAE is a 1x1 MLP of z_q = round_T(E[idx]), so a pixel's reconstruction depends on its code only: decoding P pixels
// is a row gather from a table of at most K * F * sizeof(T) bytes (128 KB at K = 1024, F = 64 bf16), which stays L2 resident, so the
// kernel is a pure stream: 4 B of index in, one output row out.  The copy is dtype agnostic: whole 16-byte chunks when a row is a
// multiple of 16 bytes (F = 64: 8 chunks per bf16 row, 16 per f32 row), one element per lane otherwise.
//
// Index convention of the sparse ops (ops.sanitize_indices): an index in [-K, 0) wraps to idx + K, anything else outside [0, K) is
// clamped into range and ORs 1 into `flag` (the per-device word behind ops.index_errors); flag may be NULL.
#include "frl_common.hpp"
#include "frl_host.hpp"

#define DC_BLOCK 256
#define DC_GRID_MAX 16384

// V: the unit copied per lane (uint4 = 16-byte chunk, uint16_t / uint32_t = one element); I: index arithmetic type (uint32_t whenever
// P * VR fits, which avoids the 64-bit division per lane)
template <typename V, typename I>
__global__ __launch_bounds__(DC_BLOCK) void decode_codes_kernel(const int32_t* __restrict__ idx, const V* __restrict__ table,
                                                                V* __restrict__ out, I total, int K, int VR, int* __restrict__ flag) {
  int bad = 0;
  const I stride = (I)gridDim.x * DC_BLOCK;
  for (I i = (I)blockIdx.x * DC_BLOCK + threadIdx.x; i < total; i += stride) {
    const I row = i / (I)VR;
    const int c = (int)(i - row * (I)VR);
    int v = idx[row];
    if (v < 0) v += K;                                       // [-K, 0) wraps; v + K cannot overflow for v < 0 < K
    if (v < 0 || v >= K) {
      bad = 1;
      v = v < 0 ? 0 : K - 1;
    }
    out[i] = table[(int64_t)v * VR + c];
  }
  if (bad && flag != nullptr) atomicOr(flag, 1);
}

template <typename V>
static void dc_launch(const int32_t* idx, const void* table, void* out, int64_t total, int K, int VR, int* flag, hipStream_t stream) {
  int64_t g = (total + DC_BLOCK - 1) / DC_BLOCK;
  if (g > DC_GRID_MAX) g = DC_GRID_MAX;
  // the loop index may step past `total` by one grid stride before the test: keep that sum representable in 32 bits too
  if (total + (int64_t)DC_GRID_MAX * DC_BLOCK < ((int64_t)1 << 32))
    FRL_LAUNCH((decode_codes_kernel<V, uint32_t>), dim3((unsigned)g), dim3(DC_BLOCK), 0, stream, idx, (const V*)table, (V*)out,
               (uint32_t)total, K, VR, flag);
  else
    FRL_LAUNCH((decode_codes_kernel<V, uint64_t>), dim3((unsigned)g), dim3(DC_BLOCK), 0, stream, idx, (const V*)table, (V*)out,
               (uint64_t)total, K, VR, flag);
}

extern "C" {

int frl_decode_codes(const int32_t* idx, const void* table, void* out, int64_t P, int K, int F, int dtype, int32_t* index_flag,
                     hipStream_t stream) {
  if (P < 0) return frl_fail(-2, "decode_codes: P < 0");
  if (K <= 0) return frl_fail(-2, "decode_codes: K <= 0");
  if (F <= 0) return frl_fail(-2, "decode_codes: F <= 0");
  if (dtype != FRL_F32 && dtype != FRL_BF16) return frl_fail(-2, "decode_codes: dtype must be float32 or bfloat16");
  if (P == 0) return 0;
  if (idx == nullptr || table == nullptr || out == nullptr) return frl_fail(-1, "decode_codes: null pointer");
  const int esize = dtype == FRL_F32 ? 4 : 2;
  const int64_t row_bytes = (int64_t)F * esize;
  int* flag = reinterpret_cast<int*>(index_flag);
  if (row_bytes % 16 == 0 && ((uintptr_t)table & 15) == 0 && ((uintptr_t)out & 15) == 0) {
    const int VR = (int)(row_bytes / 16);
    dc_launch<uint4>(idx, table, out, P * VR, K, VR, flag, stream);
  } else if (esize == 4) {
    dc_launch<uint32_t>(idx, table, out, P * F, K, F, flag, stream);
  } else {
    dc_launch<uint16_t>(idx, table, out, P * F, K, F, flag, stream);
  }
  return frl_check_launch("decode_codes");
}

}  // extern "C"
