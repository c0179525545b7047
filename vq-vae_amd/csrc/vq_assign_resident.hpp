#pragma once
#include "vq_common.hpp"

// ---------------------------------------------------------------------------------------------
// Resident-codebook assignment: the whole codebook image fits one LDS chunk (<= 64 KB: K <= 512 at d = 64 bf16), and ONE launch does
// everything, with nothing to zero beforehand:
//   * NO batch bias: score = ||e||^2 - 2 z.e straight from the accumulator; the key (f32 bits & ~127) | index is ordered with the FLOAT
//     v_min_f32 / v_med3_f32, which order positive and negative keys alike (among equal truncated negative scores the larger index
//     wins: irrelevant, equal scores are re-evaluated exactly anyway; NaN keys are ignored and leave the row at +inf = ambiguous);
//     the ambiguity threshold is per row, from the row's own norm;
//   * rows whose two best scores are within the bound are parked in an LDS list in ROW ORDER (ballot ranks + a prefix over the waves:
//     the slot of a row does not depend on timing, so the squared-error sum is bit-reproducible) and resolved by the whole workgroup
//     while the codebook is resident: every wave re-scores the parked rows against its share of the code blocks on the matrix cores and
//     appends the codes under the row's limit to a candidate list; one LANE per candidate evaluates the float64 distance (vq_exact_one:
//     same summation order for every candidate, so duplicate codes tie exactly), LDS integer atomics keep the minimum and then the
//     smallest code among the minima (first index wins);  more than VQ_FAST_ROWS parked rows or more candidates than threads (constructed
//     inputs: every row a tie) take the sequential per-wave path with the same arithmetic;
//   * z_q comes from the LDS image (-0.5 x the packed -2e is exact) on the bf16 fast path;
//   * histogram: integer atomics into the control block of the prepared image; the workgroup that arrives last (ticket behind an
//     agent-scope release / acquire) folds squared-error partials and perplexity, writes stats / counts and ZEROES the control block
//     again for the next call (the first zeroing is vq_prepare_kernel's).  One call in flight per prepared image.
// ---------------------------------------------------------------------------------------------
#define VQ_PZ_CAP 16         // parked rows per batch whose z row is kept in LDS (the usual case: ~0.3-0.7 % of a batch's rows are parked)

template <typename T, int NF, int NT, int NW>
__global__ __launch_bounds__(NW * 64, (NW == 8 ? 4 : 1)) void vq_assign_resident_kernel(
    const T* __restrict__ Z, const float* __restrict__ E, const float* __restrict__ en_g, int64_t N, int K, int d, int Kc,
    int32_t* __restrict__ idx_out, T* __restrict__ zq_out, float* __restrict__ partial /*[grid*NW]*/,
    const typename DT<T>::frag_t* __restrict__ pk, VqCtl* __restrict__ ctl, int32_t* __restrict__ counts_out, float* __restrict__ stats_out,
    float* __restrict__ stats_copy /*[4] or null*/) {
  typedef typename DT<T>::frag_t frag_t;
  constexpr int FE = DT<T>::FE;
  constexpr int q = NF * FE;                 // channels per lane quarter
  constexpr int BATCH = NW * NT * 16;        // rows per workgroup batch = capacity of the parked list
  constexpr int CAND_CAP = NW * 64;          // one candidate per thread
  extern __shared__ __attribute__((aligned(16))) char smem[];
  frag_t* wl = reinterpret_cast<frag_t*>(smem);                                               // [Kc/16][NF][64]
  float* enl = reinterpret_cast<float*>(smem + (size_t)(Kc / 16) * NF * 64 * sizeof(frag_t)); // [Kc] ||e||^2 (3e38 beyond K)
  int* hist = reinterpret_cast<int*>(enl + Kc);                                               // [K]
  unsigned long long* best = reinterpret_cast<unsigned long long*>(hist + ((K + 1) & ~1));    // [VQ_FAST_ROWS] float64 bits of the minimum
  int* bestk = reinterpret_cast<int*>(best + VQ_FAST_ROWS);                                   // [VQ_FAST_ROWS]
  int* park = bestk + VQ_FAST_ROWS;                                                           // [BATCH] x {row - batch base, limit (f32 bits)}
  int* cand = park + 2 * BATCH;                                                               // [CAND_CAP] (slot << 16) | code
  int* misc = cand + CAND_CAP;                                                                // [0..NW) parked per wave, [16] candidates, [17] last flag, [18..18+NW) f32 maxima
  T* park_z = reinterpret_cast<T*>(misc + 32);                                                // [VQ_PZ_CAP][d] rows of the parked vectors (bf16 fast path only)
  int32_t* counts_acc = reinterpret_cast<int32_t*>(ctl + 1);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int vx = lane & 15, kc = lane >> 4;
  const bool fast = (d == 4 * q);
  const int nmb = Kc / 16;
#ifdef VQ_STAMPS
  __shared__ unsigned long long vq_ts[16][8];
  if (tid < 128) (&vq_ts[0][0])[tid] = 0ull;
  unsigned long long t_prev = __builtin_amdgcn_s_memtime();
  const unsigned long long t_begin = t_prev;
  const unsigned long long w_begin = wall_clock64();               // constant 100 MHz counter: calibrates the s_memtime ticks
#endif

  // ---- the first batch's rows are requested before the codebook image so that both latencies overlap ----
  const int64_t nbatch = (N + BATCH - 1) / BATCH;
  LQTile<T, NF> zt[NT];
  auto load_batch = [&](int64_t b, int tid_) {
    const int64_t r0 = b * BATCH + (int64_t)(tid_ >> 6) * (NT * 16);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      int64_t row = r0 + t * 16 + (tid_ & 15);
      if (row >= N) row = N - 1;
      lq_load<T, NF>(zt[t], Z, row, d, (tid_ >> 4) & 3, fast);
    }
  };
  if ((int64_t)blockIdx.x < nbatch) load_batch(blockIdx.x, tid);
  // ---- once per workgroup: codebook image, norms, their maximum, cleared histogram / lists ----
  copy_frags_lds<T>(wl, pk, nmb * NF * 64, tid, NW * 64);
  float enmax;
  {
    float m = 0.f;
    for (int i = tid; i < Kc; i += NW * 64) {
      const float v = i < K ? en_g[i] : 3.0e38f;
      enl[i] = v;
      if (i < K) m = fmaxf(m, v);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if (lane == 0) misc[18 + wave] = __float_as_int(m);
  }
  for (int k = tid; k < K; k += NW * 64) hist[k] = 0;
  if (tid < VQ_FAST_ROWS) { best[tid] = ~0ull; bestk[tid] = 0x7fffffff; }
  if (tid == 0) misc[16] = 0;
  __syncthreads();
  {
    float m = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) m = fmaxf(m, __int_as_float(misc[18 + w]));
    enmax = m;
  }
  const float err_rel = (float)(4 * q + 8) * 1.1920929e-7f;            // (d_pad+8) * 2^-23: f32 accumulation of exact products
  const float thr_rel = (3.0517578125e-5f + 2.f * err_rel) * 1.001953125f;   // 2^-15: key truncation of both scores, + 2*err, + margin
  const float enroot = sqrtf(enmax);
  float sq_acc = 0.f;
  int n_resolved = 0;
  VQ_ST(2);

  for (int64_t batch = blockIdx.x; batch < nbatch; batch += gridDim.x) {
    const int64_t base = batch * BATCH;
    const int64_t v0 = base + (int64_t)wave * (NT * 16);
    if (batch != (int64_t)blockIdx.x) {                            // (the first batch is already in flight)
      int tidl = tid;
      asm volatile("" : "+v"(tidl));                               // (no row addresses carried around the loop)
      load_batch(batch, tidl);
    }
    float thr[NT];
    unsigned g1[NT], g2[NT];
    int gc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      float zn = 0.f;
#pragma unroll
      for (int s = 0; s < NF; ++s)
#pragma unroll
        for (int e = 0; e < FE; ++e) { const float v = lq_get<T, NF>(zt[t], s, e); zn = fmaf(v, v, zn); }
      zn += __shfl_xor(zn, 16, 64);
      zn += __shfl_xor(zn, 32, 64);
      const float sroot = sqrtf(zn) + enroot;                      // |score| and every partial sum <= (||z|| + ||e||max)^2
      thr[t] = sroot * sroot * thr_rel + 1e-37f;
#pragma unroll
      for (int s = 0; s < NF; ++s) asm volatile("" : "+v"(zt[t].f[s]));   // (else the unpacked floats stay live through the main loop)
      g1[t] = 0x7F800000u; g2[t] = 0x7F800000u; gc[t] = 0;         // +inf
    }
    VQ_ST(0);                                                      // z loads + norms (includes the load latency)
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
        const unsigned lidx = (unsigned)((mb - g0) * 16 + 4 * kc);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          f32x4 acc = en4;
#pragma unroll
          for (int s = 0; s < NF; ++s) acc = mfma16(a[s], zt[t].f[s], acc);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const unsigned key = (__float_as_uint(acc[r]) & ~VQ_IDX_MASK) | (lidx + r);
            asm("v_med3_f32 %0, %1, %2, %3" : "=v"(c2[t]) : "v"(c1[t]), "v"(c2[t]), "v"(key));   // runner-up (c1 <= c2)
            asm("v_min_f32 %0, %1, %2" : "=v"(c1[t]) : "v"(c1[t]), "v"(key));
          }
        }
      }
#pragma unroll
      for (int t = 0; t < NT; ++t) {                               // fold the group of 128 codes into the running (best, runner-up, group)
        const float a1 = __uint_as_float(g1[t]), a2 = __uint_as_float(g2[t]), b1 = __uint_as_float(c1[t]), b2 = __uint_as_float(c2[t]);
        const float hi = fmaxf(a1, b1), lo2 = fminf(a2, b2);
        g2[t] = __float_as_uint(fminf(hi, lo2));
        if (b1 < a1) { g1[t] = c1[t]; gc[t] = g0; }
      }
    }
    VQ_ST(3);                                                      // MFMA + key / min / med3 main loop
    // ---- min-reduce over the 4 lane groups that share a row; ambiguity test; z_q, squared error, histogram of the settled rows ----
    // (opaque copies of the lane coordinates: keeps the epilogue's address arithmetic out of the main loop's register budget)
    int tide = tid;
    asm volatile("" : "+v"(tide));
    const int vxe = tide & 15, kce = (tide >> 4) & 3;
    const int64_t v0e = base + (int64_t)(tide >> 6) * (NT * 16);
    float lim[NT];
    unsigned ambm = 0u;                                            // bit t: row (t, vxe) is parked (valid in the kce == 0 lanes)
    int nparked = 0, rank[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int off = 16; off <= 32; off <<= 1) {
        const unsigned o1 = __shfl_xor(g1[t], off, 64), o2 = __shfl_xor(g2[t], off, 64);
        const int oc = __shfl_xor(gc[t], off, 64);
        const float a1 = __uint_as_float(g1[t]), a2 = __uint_as_float(g2[t]), b1 = __uint_as_float(o1), b2 = __uint_as_float(o2);
        const float hi = fmaxf(a1, b1), lo2 = fminf(a2, b2);
        g2[t] = __float_as_uint(fminf(hi, lo2));
        if (b1 < a1 || (b1 == a1 && (oc < gc[t] || (oc == gc[t] && o1 < g1[t])))) { g1[t] = o1; gc[t] = oc; }
      }
      const int64_t row = v0e + t * 16 + vxe;
      const int code = gc[t] * 16 + (int)(g1[t] & VQ_IDX_MASK);
      const float s1 = __uint_as_float(g1[t] & ~VQ_IDX_MASK), s2 = __uint_as_float(g2[t] & ~VQ_IDX_MASK);
      const bool amb = !((s2 - s1) > thr[t]) || (unsigned)code >= (unsigned)K;   // also catches NaN / inf rows
      lim[t] = s1 + thr[t] + 2.3841858e-7f * fabsf(s1);
      const unsigned long long pm = __builtin_amdgcn_ballot_w64(amb && kce == 0 && row < N);
      rank[t] = nparked + __builtin_popcountll(pm & ((1ull << vxe) - 1ull));
      nparked += __builtin_popcountll(pm);
      if (amb) ambm |= 1u << t;
      if (row < N && !amb) {
        T* zo = zq_out + row * (int64_t)d + q * kce;
        if (fast) {
          if constexpr (FE == 8) {                                 // e (rounded to bf16) = -0.5 * the packed -2e: exact
#pragma unroll
            for (int s = 0; s < NF; ++s) {
              const bf16x8 pv = wl[((code >> 4) * NF + s) * 64 + (code & 15) + 16 * kce];
              bf16x8 ev;
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                const float f = -0.5f * (float)pv[e];
                ev[e] = (bf16)f;
                const float df = (float)zt[t].f[s][e] - f;
                sq_acc = fmaf(df, df, sq_acc);
              }
              *reinterpret_cast<bf16x8*>(zo + 8 * s) = ev;
            }
          } else {
            const float* er = E + (int64_t)code * d + q * kce;
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
          }
        } else {
          const float* er = E + (int64_t)code * d + q * kce;
#pragma unroll
          for (int s = 0; s < NF * FE; ++s) {
            if (q * kce + s < d) {
              const float ev = to_f32(from_f32<T>(er[s]));
              zo[s] = from_f32<T>(ev);
              const float df = lq_get<T, NF>(zt[t], s / FE, s % FE) - ev;
              sq_acc = fmaf(df, df, sq_acc);
            }
          }
        }
        if (kce == 0) { idx_out[row] = code; atomicAdd(&hist[code], 1); }
      }
    }
    VQ_ST(4);                                                      // reduce, ambiguity test, z_q, histogram
    // ---- park the ambiguous rows in row order: slot = (rows parked by the waves before this one) + rank inside the wave ----
    if ((tide & 63) == 0) misc[tide >> 6] = nparked;
    VQ_LDS_BARRIER();
    int pbase = 0, n = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { const int c = misc[w]; if (w < (tide >> 6)) pbase += c; n += c; }
    if (n == 0) { VQ_LDS_BARRIER(); continue; }                     // (uniform) nothing to resolve in this batch
    if (kce == 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (((ambm >> t) & 1u) && v0e + t * 16 + vxe < N) {
          park[2 * (pbase + rank[t])] = (tide >> 6) * (NT * 16) + t * 16 + vxe;
          park[2 * (pbase + rank[t]) + 1] = __float_as_int(lim[t]);
        }
    }
    // bf16 rows, few of them parked (the usual case): their vectors go to LDS as well, straight from the registers of the four lanes
    // that hold them; the screen, the float64 distances and the outputs below then touch no global memory but the final stores (the
    // global-memory form of this pass was a chain of dependent L2 / HBM latencies behind barriers: ~9 us per batch)
    bool zlds = false;
    if constexpr (FE == 8) {
      zlds = fast && n <= VQ_PZ_CAP;
      if (zlds) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
          if (((ambm >> t) & 1u) && v0e + t * 16 + vxe < N) {
#pragma unroll
            for (int s = 0; s < NF; ++s) *reinterpret_cast<bf16x8*>(park_z + (pbase + rank[t]) * d + q * kce + 8 * s) = zt[t].f[s];
          }
      }
    }
    VQ_LDS_BARRIER();
    bool all_waves = n <= VQ_FAST_ROWS;
    int tidr = tid;
    asm volatile("" : "+v"(tidr));
    if (all_waves) {
      // ---- screen: wave w re-scores every tile of 16 parked rows against its share of the code blocks ----
      const int waver = tidr >> 6, laner = tidr & 63, vxr = tidr & 15, kcr = (tidr >> 4) & 3;
      const int mb0 = (waver * nmb) / NW, mb1 = ((waver + 1) * nmb) / NW;
      for (int t0 = 0; t0 < n; t0 += 16) {
        const int li = t0 + vxr;
        const bool valid = li < n;
        const int64_t row = base + park[2 * (valid ? li : t0)];
        const float lm = __int_as_float(park[2 * (valid ? li : t0) + 1]);
        LQTile<T, NF> zr;
        bool from_lds = false;
        if constexpr (FE == 8) {
          if (zlds) {
            from_lds = true;
#pragma unroll
            for (int s = 0; s < NF; ++s) zr.f[s] = *reinterpret_cast<const bf16x8*>(park_z + (valid ? li : t0) * d + q * kcr + 8 * s);
          }
        }
        if (!from_lds) lq_load<T, NF>(zr, Z, row, d, kcr, fast);
        for (int mb = mb0; mb < mb1; ++mb) {
          f32x4 acc = *reinterpret_cast<const f32x4*>(enl + mb * 16 + 4 * kcr);
#pragma unroll
          for (int s = 0; s < NF; ++s) acc = mfma16(wl[(mb * NF + s) * 64 + laner], zr.f[s], acc);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int code = mb * 16 + 4 * kcr + r;
            if (valid && acc[r] <= lm && code < K) {
              const int pos = atomicAdd(&misc[16], 1);
              if (pos < CAND_CAP) cand[pos] = (li << 16) | code;
            }
          }
        }
      }
      VQ_LDS_BARRIER();
      const int ncand = misc[16];
      all_waves = ncand <= CAND_CAP;                               // (uniform)
      if (all_waves) {
        // ---- one lane per candidate: float64 distance; minimum per row, then the smallest code among the minima ----
        const int c = laner * NW + waver;                            // spread the few candidates over the waves
        int li = 0, code = 0;
        unsigned long long bits = ~0ull;
        if (c < ncand) {
          const int cv = cand[c];
          li = cv >> 16; code = cv & 0xffff;
          double dist;
          bool done_ = false;
          if constexpr (FE == 8) {
            if (zlds) { dist = vq_exact_lds<NF>(reinterpret_cast<const bf16*>(park_z) + li * d, reinterpret_cast<const bf16x8*>(wl), code, d); done_ = true; }
          }
          if (!done_) dist = vq_exact_one<T>(Z, E, base + park[2 * li], code, d);
          bits = (unsigned long long)__double_as_longlong(dist);
          __hip_atomic_fetch_min(&best[li], bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        VQ_LDS_BARRIER();
        if (c < ncand && bits == best[li]) __hip_atomic_fetch_min(&bestk[li], code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        VQ_LDS_BARRIER();
        // ---- outputs of the resolved rows: 16 lanes per row ----
        const int j = tidr & 15;
        for (int li2 = tidr >> 4; li2 < n; li2 += NW * 4) {
          int bk = bestk[li2];
          if ((unsigned)bk >= (unsigned)K) bk = 0;                 // no candidate at all (NaN row): argmin of an all-NaN row is 0
          const int64_t row = base + park[2 * li2];
          for (int ch = j; ch < d; ch += 16) {
            float ev, zv;
            bool done_ = false;
            if constexpr (FE == 8) {
              if (zlds) {
                ev = -0.5f * (float)reinterpret_cast<const bf16x8*>(wl)[((bk >> 4) * NF + ((ch % q) >> 3)) * 64 + (bk & 15) + 16 * (ch / q)][ch & 7];
                zv = (float)reinterpret_cast<const bf16*>(park_z)[li2 * d + ch];
                done_ = true;
              }
            }
            if (!done_) {
              ev = to_f32(from_f32<T>(E[(int64_t)bk * d + ch]));
              zv = to_f32(Z[row * (int64_t)d + ch]);
            }
            zq_out[row * (int64_t)d + ch] = from_f32<T>(ev);
            const float df = zv - ev;
            sq_acc = fmaf(df, df, sq_acc);
          }
          if (j == 0) { idx_out[row] = bk; atomicAdd(&hist[bk], 1); }
        }
        VQ_LDS_BARRIER();
        if (tidr < VQ_FAST_ROWS && tidr < n) {
          int m1 = -1;
          asm volatile("" : "+v"(m1));                              // (materialised here, not carried through the batch loop)
          best[tidr] = ((unsigned long long)(unsigned)m1 << 32) | (unsigned)m1;
          bestk[tidr] = 0x7fffffff;
        }
      }
    }
    if (!all_waves) {
      // ---- many parked rows / candidates (constructed inputs): one wave per tile of 16 parked rows, candidates evaluated in-lane
      // (up to two pending per lane, flushed together); same float64 arithmetic as above ----
      for (int t0 = wave * 16; t0 < n; t0 += NW * 16) {
        const int li = t0 + vx;
        const bool valid = li < n;
        const int64_t row = base + park[2 * (valid ? li : t0)];
        const float lm = __int_as_float(park[2 * (valid ? li : t0) + 1]);
        LQTile<T, NF> zr;
        lq_load<T, NF>(zr, Z, row, d, kc, fast);
        int bk = vq_resolve_inlane<T, NF>(zr, wl, enl, 0, nmb, K, lane, valid, lm, [&](int p0, int p1, double& d0, double& d1) {
          vq_exact_pair<T, 1>(Z, E, row, p0, p1, d, d0, d1);
        }).k;
        if ((unsigned)bk >= (unsigned)K) bk = 0;                   // no candidate at all (NaN row): argmin of an all-NaN row is 0
        if (valid) {
          vq_write_row<T, NF>(zr, E, zq_out, row, bk, d, kc, sq_acc);
          if (kc == 0) { idx_out[row] = bk; atomicAdd(&hist[bk], 1); }
        }
      }
    }
    n_resolved += n;
    VQ_LDS_BARRIER();
    if (tid == 0) misc[16] = 0;
    VQ_ST(5);                                                      // exact re-evaluation of the parked rows
  }
  // ---- per-workgroup outputs: wave partials of the squared error; histogram by integer atomics (order-independent) ----
  int tidt = tid;                                                   // (opaque: the tail's addresses are computed here, not kept in registers / scratch from the prologue on)
  asm volatile("" : "+v"(tidt));
  const float ws_ = wave_sum(sq_acc);
  if ((tidt & 63) == 0) partial[blockIdx.x * NW + (tidt >> 6)] = ws_;
  __syncthreads();
  vq_flush_hist<NW>(hist, counts_acc, K, tidt);
  if (tidt == 0 && n_resolved) atomicAdd(&ctl->namb, n_resolved);
  // publish (partials by plain stores, counts by atomics), then take a ticket; the last workgroup folds everything
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tidt == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int ticket = __hip_atomic_fetch_add(&ctl->done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    misc[17] = (ticket == (int)gridDim.x - 1) ? 1 : 0;
    if (ticket == (int)gridDim.x - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  const bool last = misc[17] != 0;
  __syncthreads();                                                  // (red below may overlap misc when the image is tiny)
  // (smem: the codebook fragments are no longer needed)
  if (last) vq_fold_stats<NW>(reinterpret_cast<double*>(smem), tidt, tidt & 63, tidt >> 6, partial, (int)gridDim.x * NW, ctl, K, N, d, counts_out, stats_out, stats_copy);
#ifdef VQ_STAMPS
  VQ_ST(6);                                                        // partials, histogram atomics, ticket, (last workgroup) statistics
  __syncthreads();
  if (tid < 128) vq_dbg[(size_t)blockIdx.x * 128 + tid] = (&vq_ts[0][0])[tid];
  if (tid == 0) { vq_dbg[(size_t)gridDim.x * 128 + 2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - t_begin; vq_dbg[(size_t)gridDim.x * 128 + 2 * blockIdx.x + 1] = wall_clock64() - w_begin; }
#endif
}
