// Type-local spectral baseline of the cross-patch phase block (frl/training/representation/step.py:920-928):
//   sim = Z_k Z_k^T with the diagonal at -inf, topk(k) per row, S_mean = mean_t spec, S_hat = mean over the k neighbours of S_mean,
//   out = spec - S_hat.  The reference writes the [N, N] similarity matrix (133 MB at 5760 anchors) for topk to read once.
// Here: a time-mean pass [N][T][C] -> [N][C], then one kernel that selects and demeans with the layout of knn_kernel / phase_pairs_kernel
// (one wave per anchor, four per workgroup, candidate rows staged once per workgroup in 64-row tiles) but WITHOUT their score rows in
// LDS, which cap N near 9900: a lane scores one candidate per tile, a ballot marks those that beat the wave's k-th best so far, and the
// marked ones are inserted one at a time, lowest lane first, into a sorted list held one rank per lane (k <= 64).  Candidates arrive in
// ascending index and a strict comparison keeps an earlier equal ahead of a later one: the order is (similarity descending, index
// ascending); torch.topk leaves equal values unordered.  After the first tiles almost no tile carries an insertion (about k ln(N / k)
// per anchor).  Nothing N x N and nothing N x k x C is written, there are no float atomics, and results are bit-identical run to run.
// A NaN similarity ranks as -inf.
#include "frl_common.hpp"
#include "frl_host.hpp"

#define TB_WAVES 4
#define TB_MAX_K 64        // width of a projected row: a tile is [TB_MAX_K][64] floats in LDS
#define TB_MAX_C 256
#define TB_NONE 0x7fffffff // index of a list entry that holds no candidate yet

// s_mean[n][c] = (sum_t spec[n][t][c]) / T, summed in order of t; adjacent threads read adjacent c
__global__ __launch_bounds__(256) void type_baseline_mean_kernel(const float* __restrict__ spec, int N, int T, int C, float* __restrict__ s_mean) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)N * C) return;
  const size_t n = e / C;
  const float* p = spec + n * (size_t)T * C + (e - n * C);
  float s = 0.f;
#pragma unroll 4
  for (int t = 0; t < T; ++t) s += p[(size_t)t * C];
  s_mean[e] = s / (float)T;
}

// LDS: tile [K][64] (a 64-row tile of z, transposed: lane l reads its candidate's column at stride 1) | q [TB_WAVES][K] | shat [TB_WAVES][C].
// A tile of z [N][K] is the contiguous run of 64 K floats from row 64 tix: 16 K float4 pieces, at most four per thread, fetched into
// registers one tile ahead (vecz: z is 16-byte aligned; the partial last tile ends element by element).
__global__ __launch_bounds__(64 * TB_WAVES) void type_baseline_select_kernel(const float* __restrict__ z, const float* __restrict__ spec,
                                                                             const float* __restrict__ s_mean, int N, int K, int T, int C,
                                                                             int k, int vecz, int vecs, float* __restrict__ out,
                                                                             float* __restrict__ s_hat, long long* __restrict__ idx) {
  __shared__ __attribute__((aligned(16))) float tile[TB_MAX_K * 64];
  __shared__ float qall[TB_WAVES][TB_MAX_K];
  __shared__ __attribute__((aligned(16))) float shat[TB_WAVES][TB_MAX_C];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int iq = blockIdx.x * TB_WAVES + wave;
  const bool live = iq < N;
  const int i = live ? iq : N - 1;                                               // surplus waves shadow the last anchor (no stores)
  const float* q = qall[wave];
  if (lane < K) qall[wave][lane] = z[(size_t)i * K + lane];
  const int ntiles = (N + 63) >> 6, npieces = 16 * K;
  const float ninf = -__builtin_inff();
  f32x4 pre[4];
  auto fetch = [&](int tix) {
    const size_t base = (size_t)tix * 64 * K;
    const int rows = N - tix * 64 < 64 ? N - tix * 64 : 64, nv = rows * K;      // floats of the tile that exist
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int f0 = 4 * (tid + 256 * u);
      if (f0 >= 4 * npieces) continue;
      if (vecz && f0 + 4 <= nv) pre[u] = *reinterpret_cast<const f32x4*>(z + base + f0);
      else {
#pragma unroll
        for (int e = 0; e < 4; ++e) pre[u][e] = f0 + e < nv ? z[base + f0 + e] : 0.f;
      }
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int f0 = 4 * (tid + 256 * u);
      if (f0 >= 4 * npieces) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = (f0 + e) / K, col = (f0 + e) - row * K;
        tile[col * 64 + row] = pre[u][e];
      }
    }
  };
  // the list: lane r holds rank r, sorted by (similarity descending, index ascending); entries without a candidate sort last
  float lv = ninf;
  int li = TB_NONE;
  fetch(0);
  for (int tix = 0; tix < ntiles; ++tix) {
    __syncthreads();                                                             // everyone is done with the previous tile (and q is written)
    commit();
    __syncthreads();
    if (tix + 1 < ntiles) fetch(tix + 1);
    const int j = tix * 64 + lane;
    float s = 0.f;
    for (int c = 0; c < K; ++c) s = fmaf(q[c], tile[c * 64 + lane], s);
    if (!(s == s)) s = ninf;
    const bool cand = j < N && j != i;                                           // never itself
    float thr = __shfl(lv, k - 1, 64);
    int thri = __shfl(li, k - 1, 64);
    unsigned long long m = __ballot(cand && (thri == TB_NONE || s > thr));       // wave-uniform from here on
    while (m) {
      const int src = __builtin_ctzll(m);
      const float cs = __shfl(s, src, 64);
      const int cj = tix * 64 + src;
      // entries that stay ahead of the candidate form a prefix of the lanes; the rest move down one lane and the candidate takes the gap
      const bool ahead = li != TB_NONE && lv >= cs;
      const float pv = __shfl_up(lv, 1, 64);
      const int pi = __shfl_up(li, 1, 64);
      const int pahead = __shfl_up((int)ahead, 1, 64);
      if (!ahead) {
        const bool gap = lane == 0 || pahead;
        lv = gap ? cs : pv;
        li = gap ? cj : pi;
      }
      thr = __shfl(lv, k - 1, 64);
      thri = __shfl(li, k - 1, 64);
      m &= m - 1;
      m &= __ballot(cand && (thri == TB_NONE || s > thr));                       // the bar has risen: drop the marks it now excludes
    }
  }
  // ---- S_hat: lanes stride over c, the k neighbours' S_mean rows summed in rank order (k <= N - 1 candidates exist: the list is full)
  for (int c0 = 0; c0 < C; c0 += 64) {
    const int c = c0 + lane;
    float acc = 0.f;
    for (int r = 0; r < k; ++r) {
      int j = __shfl(li, r, 64);
      if ((unsigned)j >= (unsigned)N) j = i;                                     // never leave the rows
      if (c < C) acc += s_mean[(size_t)j * C + c];
    }
    if (c < C) {
      const float v = acc / (float)k;
      shat[wave][c] = v;
      if (live) s_hat[(size_t)i * C + c] = v;
    }
  }
  if (!live) return;                                                             // (no workgroup barrier below)
  if (lane < k) idx[(size_t)i * k + lane] = li;
  __builtin_amdgcn_wave_barrier();
  // ---- the T demeaned rows of the anchor: T C contiguous floats
  const size_t rb = (size_t)i * T * C;
  const int total = T * C;
  if (vecs) {                                                                    // C % 4 == 0, spec and out 16-byte aligned
    for (int e = 4 * lane; e < total; e += 256) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(spec + rb + e);
      const f32x4 b = *reinterpret_cast<const f32x4*>(&shat[wave][e % C]);
      *reinterpret_cast<f32x4*>(out + rb + e) = v - b;
    }
  } else {
    for (int e = lane; e < total; e += 64) out[rb + e] = spec[rb + e] - shat[wave][e % C];
  }
}

extern "C" {

// the time means S_mean [N][C]
size_t frl_type_baseline_workspace_bytes(int N, int C) {
  if (N < 1 || C < 1) return 0;
  return (size_t)N * C * sizeof(float);
}

// See include/frl_hip.h.
int frl_type_baseline(const float* z_k, const float* spec, int N, int K, int T, int C, int k, float* out, float* s_hat, int64_t* idx, void* ws,
                      size_t ws_bytes, hipStream_t stream) {
  if (N < 2) return frl_fail(-2, "type_baseline: needs N >= 2 anchors (an anchor is never its own neighbour)");
  if (K < 1 || K > TB_MAX_K) return frl_fail(-2, "type_baseline: the projected width K must be in 1..64");
  if (k < 1 || k > 64 || k > N - 1) return frl_fail(-2, "type_baseline: k must be in 1..min(64, N - 1) (one lane per neighbour)");
  if (C < 1 || C > TB_MAX_C) return frl_fail(-2, "type_baseline: 1 <= C <= 256 spectral channels");
  if (T < 1 || (int64_t)T * C > 0x7fffffff) return frl_fail(-2, "type_baseline: T must be positive and T * C below 2^31");
  if (!z_k || !spec || !out || !s_hat || !idx) return frl_fail(-2, "type_baseline: null pointer");
  if (ws == nullptr || ws_bytes < frl_type_baseline_workspace_bytes(N, C)) return frl_fail(-4, "type_baseline: workspace too small");
  if (((uintptr_t)z_k | (uintptr_t)spec | (uintptr_t)out | (uintptr_t)s_hat | (uintptr_t)ws) & 3)
    return frl_fail(-2, "type_baseline: float pointers must be 4-byte aligned");
  float* s_mean = (float*)ws;
  const size_t nc = (size_t)N * C;
  if ((nc + 255) / 256 > 0x7fffffffull) return frl_fail(-2, "type_baseline: N * C too large for one launch");
  FRL_LAUNCH(type_baseline_mean_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, stream, spec, N, T, C, s_mean);
  const int vecz = ((uintptr_t)z_k & 15) == 0;
  const int vecs = (C & 3) == 0 && (((uintptr_t)spec | (uintptr_t)out) & 15) == 0;
  FRL_LAUNCH(type_baseline_select_kernel, dim3((unsigned)((N + TB_WAVES - 1) / TB_WAVES)), dim3(64 * TB_WAVES), 0, stream, z_k, spec,
             (const float*)s_mean, N, K, T, C, k, vecz, vecs, out, s_hat, (long long*)idx);
  return frl_check_launch("type_baseline");
}

}  // extern "C"
