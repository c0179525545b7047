// Multi-chunk route of the nearest-code assignment: vq_assign_kernel, then vq_fixup_tile_kernel for the flagged rows and
// vq_finalize_kernel for the statistics.
#pragma once
#include "vq_common.hpp"

// NW = waves per workgroup: 16 (one workgroup per CU, ONE LDS copy of the codebook chunk shared by four waves per SIMD) when the
// batch is large enough, else 4.
// Multi-chunk assignment (codebook image larger than one LDS chunk: K = 8192, d = 128 of BASELINE configs[3]).  The packed image is
// streamed through TWO LDS chunk buffers by LDS-DMA (global_load_lds_dwordx4: the image is contiguous, no registers involved): chunk
// i + 1 arrives while chunk i is scored, one barrier per chunk, the chunk sequence runs on across the workgroup's batches.  Keys are the
// float-ordered ones of the resident kernel (no batch bias, per-row threshold), flagged rows go to a global list with their limits
// (vq_fixup_tile_kernel), the histogram to integer atomics on the zeroed accumulator.
template <typename T, int NF, int NT, int NW>
__global__ __launch_bounds__(NW * 64, (NW == 8 ? 4 : 2)) void vq_assign_kernel(
    const T* __restrict__ Z, const float* __restrict__ E, const float* __restrict__ en_g, int64_t N, int K, int d, int Kc,
    int32_t* __restrict__ idx_out, T* __restrict__ zq_out, float* __restrict__ partial /*[grid*NW]*/, int32_t* __restrict__ counts_acc,
    VqHeader* __restrict__ hdr_w, int32_t* __restrict__ amb_list, float* __restrict__ amb_lim, const typename DT<T>::frag_t* __restrict__ pk) {
  typedef typename DT<T>::frag_t frag_t;
  constexpr int FE = DT<T>::FE;
  constexpr int q = NF * FE;                 // channels per lane quarter
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int chunk_bytes = (Kc / 16) * NF * 64 * (int)sizeof(frag_t);  // a multiple of 1 KB
  const int buf_bytes = chunk_bytes + Kc * 4;                         // fragments | ||e||^2 of the chunk
  float* cbw = reinterpret_cast<float*>(smem + 2 * buf_bytes);         // [NW] scratch of the prologue
  // histogram: small codebooks are hit by many rows per code, so the workgroup counts in LDS and adds each used code once at the end;
  // large ones (K > 2048: few rows per code, 32 KB of LDS) go straight to the global integer atomics
  int* hist = reinterpret_cast<int*>(smem + 2 * buf_bytes + 64);
  const bool lds_hist = K <= 2048;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int vx = lane & 15, kc = lane >> 4;
  const int nchunks = (K + Kc - 1) / Kc;
  const bool fast = (d == 4 * q);
  float enmax;
  {                                                                    // max ||e||^2 over the real codes, by the workgroup itself
    float m = 0.f;
    for (int k = tid; k < K; k += NW * 64) m = fmaxf(m, en_g[k]);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (lane == 0) cbw[wave] = m;
    __syncthreads();
    float mm = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) mm = fmaxf(mm, cbw[w]);
    enmax = mm;
  }
  const VqThr th = vq_thresholds(q, enmax);
  float sq_acc = 0.f;
  if (lds_hist)
    for (int k = tid; k < K; k += NW * 64) hist[k] = 0;            // (visible behind the first chunk barrier)

  // chunk c of the image (fragments, then its norms) into buffer `buf`: 1 KB pieces dealt round-robin to the waves
  const int npiece = chunk_bytes >> 10;
  auto dma_chunk = [&](int c, int buf) {
    const char* src = reinterpret_cast<const char*>(pk) + (size_t)c * chunk_bytes;
    int lane_ = lane;
    asm volatile("" : "+v"(lane_));
    for (int p = wave; p < npiece; p += NW) {                      // (wave-uniform trip count)
      const char* sp = src + p * 1024 + lane_ * 16;
      const int ldst = buf * buf_bytes + p * 1024;
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(sp), "s"(ldst) : "memory");
    }
    for (int p = wave; p < (Kc >> 6); p += NW) {                   // the chunk's norms, 64 floats per piece (en_g holds kpad entries: 3e38 beyond K)
      const float* sp = en_g + c * Kc + p * 64 + lane_;
      const int ldst = buf * buf_bytes + chunk_bytes + p * 256;
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(sp), "s"(ldst) : "memory");
    }
  };

  const int64_t vec_per_batch = NW * NT * 16;
  const int64_t nbatch = (N + vec_per_batch - 1) / vec_per_batch;
  const int64_t my_batches = (int64_t)blockIdx.x < nbatch ? (nbatch - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
  const int64_t total_it = my_batches * nchunks;                  // chunk iterations of this workgroup, across its batches
  int64_t it = 0;
  if (total_it > 0) dma_chunk(0, 0);
  for (int64_t batch = blockIdx.x; batch < nbatch; batch += gridDim.x) {
    const int64_t v0 = (batch * NW + wave) * (NT * 16);
    LQTile<T, NF> zt[NT];
    float thr[NT];
    unsigned g1[NT], g2[NT];
    int gc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      int64_t row = v0 + t * 16 + vx;
      if (row >= N) row = N - 1;
      lq_load<T, NF>(zt[t], Z, row, d, kc, fast);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      thr[t] = vq_row_threshold<T, NF>(zt[t], th);
#pragma unroll
      for (int s = 0; s < NF; ++s) asm volatile("" : "+v"(zt[t].f[s]));   // (else the unpacked floats stay live through the chunk loop)
      g1[t] = 0x7F800000u; g2[t] = 0x7F800000u; gc[t] = 0;         // +inf
    }
    unsigned maskv = ~VQ_IDX_MASK;
    asm volatile("" : "+v"(maskv));                                // (opaque and in a register: (score & mask) | index then selects as ONE v_and_or_b32)
    for (int c = 0; c < nchunks; ++c, ++it) {
      const int buf = (int)(it & 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's pieces of chunk `it` (and its norm loads) have landed
      __syncthreads();                                           // ... everybody's; everybody is done with the other buffer
      if (it + 1 < total_it) dma_chunk((c + 1 == nchunks) ? 0 : c + 1, buf ^ 1);
      const frag_t* wl = reinterpret_cast<const frag_t*>(smem + buf * buf_bytes);
      const float* enl = reinterpret_cast<const float*>(smem + buf * buf_bytes + chunk_bytes);
      const int nmb = Kc / 16;
      for (int g0 = 0; g0 < nmb; g0 += 8) {
        unsigned c1[NT], c2[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) { c1[t] = 0x7F800000u; c2[t] = 0x7F800000u; }
        const int g1e = (g0 + 8) < nmb ? (g0 + 8) : nmb;
        for (int mb = g0; mb < g1e; ++mb) {
          const f32x4 en4 = *reinterpret_cast<const f32x4*>(enl + mb * 16 + 4 * kc);
          frag_t a[NF];
#pragma unroll
          for (int s = 0; s < NF; ++s) a[s] = wl[(mb * NF + s) * 64 + lane];
          const unsigned lidx = (unsigned)((mb - g0) * 4);            // (wave-uniform)
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            f32x4 acc = en4;
#pragma unroll
            for (int s = 0; s < NF; ++s) acc = mfma16(a[s], zt[t].f[s], acc);
#pragma unroll
            for (int r = 0; r < 4; r += 2) {
              // key index = (block in group) * 4 + accumulator row (the lane adds its quarter when it decodes); two keys per update:
              // with c1 <= c2 the second smallest of {c1, c2, k0, k1} is min(c2, median(c1, k0, k1)); 2.5 vector operations per score
              unsigned i0 = lidx + r, i1 = lidx + r + 1;
              asm("" : "+s"(i0), "+s"(i1));                            // (opaque scalars: else the odd index becomes v_and + v_or3)
              const unsigned k0 = (__float_as_uint(acc[r]) & maskv) | i0, k1 = (__float_as_uint(acc[r + 1]) & maskv) | i1;
              unsigned m;
              asm("v_med3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(c1[t]), "v"(k0), "v"(k1));
              asm("v_min_f32 %0, %1, %2" : "=v"(c2[t]) : "v"(c2[t]), "v"(m));
              asm("v_min3_f32 %0, %1, %2, %3" : "=v"(c1[t]) : "v"(c1[t]), "v"(k0), "v"(k1));
            }
          }
        }
        const int gid = c * (Kc / 16) + g0;                     // group base in units of 16 codes
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const float a1 = __uint_as_float(g1[t]), a2 = __uint_as_float(g2[t]), b1 = __uint_as_float(c1[t]), b2 = __uint_as_float(c2[t]);
          const float hi = fmaxf(a1, b1), lo2 = fminf(a2, b2);
          g2[t] = __float_as_uint(fminf(hi, lo2));
          if (b1 < a1) { g1[t] = c1[t]; gc[t] = gid; }
        }
      }
    }
    // ---- min-reduce over the 4 lane groups that share a row; ambiguity test; z_q, squared error, histogram of the settled rows ----
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      int cd1 = (gc[t] + (int)((g1[t] & VQ_IDX_MASK) >> 2)) * 16 + 4 * kc + (int)(g1[t] & 3u);   // the lane's own best code
#pragma unroll
      for (int off = 16; off <= 32; off <<= 1) {
        const unsigned o1 = __shfl_xor(g1[t], off, 64), o2 = __shfl_xor(g2[t], off, 64);
        const int oc = __shfl_xor(cd1, off, 64);
        const float a1 = __uint_as_float(g1[t] & ~VQ_IDX_MASK), a2 = __uint_as_float(g2[t]), b1 = __uint_as_float(o1 & ~VQ_IDX_MASK), b2 = __uint_as_float(o2);
        const float hi = fmaxf(__uint_as_float(g1[t]), __uint_as_float(o1)), lo2 = fminf(a2, b2);
        g2[t] = __float_as_uint(fminf(hi, lo2));
        if (b1 < a1 || (b1 == a1 && oc < cd1)) { g1[t] = o1; cd1 = oc; }
      }
      const int64_t row = v0 + t * 16 + vx;
      const int code = cd1;
      const float s1 = __uint_as_float(g1[t] & ~VQ_IDX_MASK), s2 = __uint_as_float(g2[t] & ~VQ_IDX_MASK);
      const bool amb = !((s2 - s1) > thr[t]) || (unsigned)code >= (unsigned)K;   // also catches NaN / inf rows
      if (row < N) {
        if (kc == 0) {
          idx_out[row] = amb ? 0 : code;
          if (amb) {
            const int pos = atomicAdd(&hdr_w->namb, 1);
            amb_list[pos] = (int32_t)row;
            amb_lim[pos] = s1 + thr[t] + 2.3841858e-7f * fabsf(s1);   // every code whose f32 score is <= this may be the float64 arg-min
          }
        }
        if (!amb) {
          // gather z_q (rounded to T) for this lane's channel quarter, accumulate squared error
          const float* er = E + (int64_t)code * d + q * kc;
          T* zo = zq_out + row * (int64_t)d + q * kc;
          if (fast) {
#pragma unroll
            for (int s = 0; s < NF * FE; s += DT<T>::VEC) {
              float ev[DT<T>::VEC];
#pragma unroll
              for (int e = 0; e < DT<T>::VEC; ++e) ev[e] = to_f32(from_f32<T>(er[s + e]));
              Vec<T>::store(zo + s, ev);
#pragma unroll
              for (int e = 0; e < DT<T>::VEC; ++e) {
                const float df = lq_get<T, NF>(zt[t], (s + e) / FE, (s + e) % FE) - ev[e];
                sq_acc = fmaf(df, df, sq_acc);
              }
            }
          } else {
#pragma unroll
            for (int s = 0; s < NF * FE; ++s) {
              if (q * kc + s < d) {
                const float ev = to_f32(from_f32<T>(er[s]));
                zo[s] = from_f32<T>(ev);
                const float df = lq_get<T, NF>(zt[t], s / FE, s % FE) - ev;
                sq_acc = fmaf(df, df, sq_acc);
              }
            }
          }
          if (kc == 0) atomicAdd(lds_hist ? &hist[code] : &counts_acc[code], 1);   // integer sums: order-independent, bit-reproducible
        }
      }
    }
  }
  // ---- per-workgroup output: wave partials of the squared error; LDS histogram -> one global add per used code ----
  const float ws_ = wave_sum(sq_acc);
  if (lane == 0) partial[blockIdx.x * NW + wave] = ws_;
  if (lds_hist) {
    __syncthreads();
    vq_flush_hist<NW>(hist, counts_acc, K, tid);
  }
}

// ---------------------------------------------------------------------------------------------
// Exact re-evaluation of the flagged rows of the multi-chunk path, 16 rows per workgroup (8 waves, each with its share of the code
// blocks, merged in wave order): the rows are re-scored against the WHOLE packed
// image on the matrix cores (fragments streamed from L2: 2 MB per tile at K = 8192, d = 128, instead of the 4 MB float32 codebook per
// ROW of the former one-wave-per-row kernels -- 17 ms at 1 % flagged rows), codes under the row's limit are evaluated in float64
// in-lane (up to two pending per lane, flushed together), first index wins ties.  Nothing depends on the order of the list, which the
// timing of the appends decides: the histogram uses integer atomics, and the squared error of each row (one float32: the fmaf chain of
// each lane quarter, quarters added 16 and then 32 lanes away) is added EXACTLY, as an integer, to the fixed-point bins of
// VqHeader::sq_bins (LDS first, one global atomic per used bin and workgroup), so that stats are the same bits from call to call.
// ---------------------------------------------------------------------------------------------
#define VQ_FIXT_WAVES 8      // waves per tile of 16 flagged rows: each scores its share of the code blocks
template <typename T, int NF>
__global__ __launch_bounds__(64 * VQ_FIXT_WAVES) void vq_fixup_tile_kernel(const T* __restrict__ Z, const float* __restrict__ E, const float* __restrict__ en_g,
                                                            const typename DT<T>::frag_t* __restrict__ pk, int K, int kpad, int d,
                                                            const int32_t* __restrict__ amb_list, const float* __restrict__ amb_lim,
                                                            VqHeader* __restrict__ hdr, int32_t* __restrict__ idx_out, T* __restrict__ zq_out,
                                                            int32_t* __restrict__ counts_fix) {
  constexpr int FE = DT<T>::FE;
  constexpr int q = NF * FE;
  __shared__ double mrg_d[VQ_FIXT_WAVES][16];
  __shared__ int mrg_k[VQ_FIXT_WAVES][16];
  __shared__ unsigned long long bins[VQ_SQ_BINS];
  __shared__ float row_sq[16];                                       // squared errors of the tile's rows, -1: no row
  if (threadIdx.x < VQ_SQ_BINS) bins[threadIdx.x] = 0ull;            // (visible behind the first barrier of the tile loop)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int vx = lane & 15, kc = lane >> 4;
  const bool fast = (d == 4 * q);
  const int namb = hdr->namb;
  const int ntile = (namb + 15) >> 4, nmb = kpad >> 4;
  const int mb0 = (wave * nmb) / VQ_FIXT_WAVES, mb1 = ((wave + 1) * nmb) / VQ_FIXT_WAVES;
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int li = tile * 16 + vx;
    const bool valid = li < namb;
    const int64_t row = amb_list[valid ? li : tile * 16];
    const float lm = amb_lim[valid ? li : tile * 16];
    LQTile<T, NF> zr;
    lq_load<T, NF>(zr, Z, row, d, kc, fast);
    const VqBest own = vq_resolve_inlane<T, NF>(zr, pk, en_g, mb0, mb1, K, lane, valid, lm, [&](int p0, int p1, double& d0, double& d1) {
      vq_exact_pair<T, 1>(Z, E, row, p0, p1, d, d0, d1);
    });
    double bestd = own.d;
    int bk = own.k;
    // the waves' shares are merged in wave order: smallest distance, then smallest code (= first index over the whole codebook)
    if (kc == 0) { mrg_d[wave][vx] = bestd; mrg_k[wave][vx] = bk; }
    __syncthreads();
    if (wave == 0) {
      bestd = mrg_d[0][vx]; bk = mrg_k[0][vx];
#pragma unroll
      for (int w = 1; w < VQ_FIXT_WAVES; ++w) {
        const double ob = mrg_d[w][vx];
        const int okk = mrg_k[w][vx];
        if (ob < bestd || (ob == bestd && okk < bk)) { bestd = ob; bk = okk; }
      }
      if ((unsigned)bk >= (unsigned)K) bk = 0;                       // no candidate at all (NaN row): argmin of an all-NaN row is 0
      float rs = 0.f;                                                // squared error of the row: this quarter, then all four
      if (valid) vq_write_row<T, NF>(zr, E, zq_out, row, bk, d, kc, rs);
      rs += __shfl_xor(rs, 16, 64);
      rs += __shfl_xor(rs, 32, 64);
      if (valid && kc == 0) { idx_out[row] = bk; atomicAdd(&counts_fix[bk], 1); }
      if (kc == 0) row_sq[vx] = valid ? rs : -1.f;
    }
    __syncthreads();
    // (by another wave, so that the integer arithmetic stays out of the register budget of the resolve; row_sq is rewritten behind
    // the next tile's first barrier)
    if (wave == 1 && lane < 16 && !(row_sq[lane] == -1.f)) vq_sq_bins_add(bins, &hdr->sq_fix, row_sq[lane]);
  }
  __syncthreads();
  if (threadIdx.x < VQ_SQ_BINS && bins[threadIdx.x] != 0ull) atomicAdd(&hdr->sq_bins[threadIdx.x], bins[threadIdx.x]);
}

// stats = {sqerr_sum, perplexity, n_re-evaluated, 0}
__global__ __launch_bounds__(256) void vq_finalize_kernel(const float* __restrict__ partial, int npartial, const VqHeader* __restrict__ hdr,
                                                          const int32_t* __restrict__ counts_acc, int32_t* __restrict__ counts, int K, int64_t N,
                                                          int d, float* __restrict__ stats, float* __restrict__ stats_copy /*[4] or null*/) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < npartial; i += 256) s += (double)partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  const double sq = red[0] + (vq_sq_bins_value(hdr->sq_bins) + hdr->sq_fix);
  __syncthreads();
  double h = 0.0;
  for (int k = threadIdx.x; k < K; k += 256) {
    const int cnt = counts_acc[k];
    counts[k] = cnt;
    const double p = (double)cnt / (double)N;
    h += p * log(p + 1e-10);
  }
  red[threadIdx.x] = h;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) {
    stats[0] = (float)sq;
    stats[1] = (float)exp(-red[0]);
    stats[2] = (float)hdr->namb;
    stats[3] = (float)(sq / ((double)N * (double)d));
    if (stats_copy) {
      for (int i = 0; i < 4; ++i) stats_copy[i] = stats[i];
    }
  }
}
