// Host-side helpers shared by the C-ABI entry points (error string, launch checks).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>

int frl_fail(int code, const char* msg);           // records thread-local message, returns code
int frl_check_launch(const char* what);            // hipGetLastError() -> 0 or negative code

// Kernel launch with per-launch error capture.  hipGetLastError() is sticky per thread and may hold a stale error from
// runtime initialisation done elsewhere in the process (e.g. by PyTorch), so the state is cleared before every launch
// and the first failure of a call is parked in g_frl_pending until frl_check_launch() reports it.
extern thread_local hipError_t g_frl_pending;
// Optional per-kernel timing (frl_kernel_timing_enable): a HIP event pair recorded on the launch stream immediately around every
// kernel the library launches, keyed by the kernel expression -- the live counterpart of a rocprofv3 kernel trace (bench.py).
extern int g_frl_timing;
void frl_timing_begin(const char* kernel, hipStream_t st);
void frl_timing_end(hipStream_t st);
#define FRL_ARG1_(a, ...) a
#define FRL_ARG5_(a, b, c, d, e, ...) e
#define FRL_STR2_(...) #__VA_ARGS__
#define FRL_STR_(...) FRL_STR2_(__VA_ARGS__)
#define FRL_LAUNCH(...)                                                     \
  do {                                                                      \
    (void)hipGetLastError();                                                \
    if (g_frl_timing) frl_timing_begin(FRL_STR_(FRL_ARG1_(__VA_ARGS__)), FRL_ARG5_(__VA_ARGS__)); \
    hipLaunchKernelGGL(__VA_ARGS__);                                        \
    if (g_frl_timing) frl_timing_end(FRL_ARG5_(__VA_ARGS__));               \
    hipError_t _le = hipGetLastError();                                     \
    if (_le != hipSuccess && g_frl_pending == hipSuccess) g_frl_pending = _le; \
  } while (0)

// same with an explicit timing name (for launches through a function-pointer variable)
#define FRL_LAUNCH_AS(name, ...)                                            \
  do {                                                                      \
    (void)hipGetLastError();                                                \
    if (g_frl_timing) frl_timing_begin(name, FRL_ARG5_(__VA_ARGS__));       \
    hipLaunchKernelGGL(__VA_ARGS__);                                        \
    if (g_frl_timing) frl_timing_end(FRL_ARG5_(__VA_ARGS__));               \
    hipError_t _le = hipGetLastError();                                     \
    if (_le != hipSuccess && g_frl_pending == hipSuccess) g_frl_pending = _le; \
  } while (0)

#define FRL_HIP(expr)                                            \
  do {                                                           \
    hipError_t _e = (expr);                                      \
    if (_e != hipSuccess) return frl_fail(-100 - (int)_e, hipGetErrorString(_e)); \
  } while (0)

// grid of a grid-stride kernel: ceil(work / per_block) workgroups, at least 1 and at most cap
static inline unsigned frl_grid(int64_t work, int per_block, int cap) {
  int64_t g = (work + per_block - 1) / per_block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (unsigned)g;
}

static inline int frl_failf(int code, const char* fmt, const char* a, const char* b = "") {   // frl_fail(code, fmt % (a, b))
  char msg[200];
  snprintf(msg, sizeof(msg), fmt, a, b);
  return frl_fail(code, msg);
}
// gmm.hip, probe.hip, strata.hip: `workgroups` (0: the library's choice) slabs in a workspace of the caller's: the limit and the two refusals
#define FRL_MAX_WG 4096
static inline bool frl_wg_in_range(int wg) { return wg >= 0 && wg <= FRL_MAX_WG; }
static inline int frl_check_workgroups(const char* what, int wg) { return frl_wg_in_range(wg) ? 0 : frl_failf(-2, "%s: workgroups must be in 0..4096 (0: the library's choice)", what); }
static inline int frl_check_workspace(const char* what, const void* ws, size_t ws_bytes, size_t need) {
  return ws && !((uintptr_t)ws & 15) && ws_bytes >= need ? 0 : frl_failf(-4, "%s: workspace too small or not 16-byte aligned", what);
}

// moment kernels that give each workgroup a contiguous range of rows, staged rows_per_tile at a time (vicreg.hip, leakage.hip): the
// number of workgroups (= slabs), and the rows of one workgroup, a whole number of tiles
static inline int frl_moment_wgs(int64_t N, int rows_per_tile, int max_wgs) { return (int)frl_grid(N, rows_per_tile, max_wgs); }
static inline int64_t frl_moment_rows_per_wg(int64_t N, int rows_per_tile, int max_wgs) {
  const int nwg = frl_moment_wgs(N, rows_per_tile, max_wgs);
  return ((N + nwg - 1) / nwg + rows_per_tile - 1) / rows_per_tile * rows_per_tile;
}

// Runs the statement(s) once with T naming the element type of a FRL_F32 / FRL_BF16 dtype that the caller has validated, so the argument
// list of a launch templated on the type is written once:  FRL_BY_DTYPE(dtype, T, rc = launch<T, true>(x, n, stream));
#define FRL_BY_DTYPE(dtype, T, ...)                       \
  do {                                                    \
    if ((dtype) == FRL_F32) { using T = float; __VA_ARGS__; } \
    else { using T = bf16; __VA_ARGS__; }                 \
  } while (0)

// internal cross-file dispatchers
int frl_pw_dispatch(const void* x, const void* xmask, int mask_act, const float* w, int64_t so, int64_t si,
                    const float* bias, void* y, int64_t P, int Cin, int Cout, int act, int dtype, void* ws, size_t ws_bytes,
                    hipStream_t st, const void* yadd = nullptr);
