// The keying of an observation (b, t, p) by its EVT code, shared by strata.hip and quantile.hip: codes [B][P] (int32 or float32) looked up
// in vocab [G] (int32, strictly increasing), which a workgroup keeps in LDS and searches by bisection.  A code is valid when it is finite
// and > 0 (the reference's np.isfinite(evt_grid) & (evt_grid > 0)); a valid float code is truncated as astype(np.int32) does.
#pragma once
#include "frl_common.hpp"
#include "frl_host.hpp"
#include "frl_moments.hpp"

#define STRATA_MAX_G 4095

struct StrataKeys {
  const void* codes;
  const unsigned char* mask;
  const int* vocab;
  int codes_float, Tm, G, B, T, P;
};

// index of `code` in the increasing vl [G], or -1
__device__ __forceinline__ int strata_find(const int* vl, int G, int code) {
  int lo = 0, hi = G;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (vl[mid] < code) lo = mid + 1;
    else hi = mid;
  }
  return lo < G && vl[lo] == code ? lo : -1;
}

// the code of pixel i of codes [B P]: false where it is not finite or not > 0; a float is truncated (2^31 and above: INT_MAX)
__device__ __forceinline__ bool strata_code(const StrataKeys& q, size_t i, int& code) {
  if (q.codes_float) {
    const float f = reinterpret_cast<const float*>(q.codes)[i];
    if (!(f > 0.f) || f == __builtin_inff()) return false;
    code = f >= 2147483648.f ? 0x7fffffff : (int)f;
    return true;
  }
  code = reinterpret_cast<const int*>(q.codes)[i];
  return code > 0;
}

static inline int strata_check_keys(const char* what, const void* codes, int codes_float, const unsigned char* mask, int Tm, const int32_t* vocab, int G,
                                    int B, int T, int64_t P, int workgroups, StrataKeys& k) {
  const char* why = nullptr;
  if (!codes || !vocab) why = "non-null codes and vocab";
  else if (codes_float != 0 && codes_float != 1) why = "codes_float 0 (int32) or 1 (float32)";
  else if (G < 1 || G > STRATA_MAX_G) why = "1 <= G <= 4095 codes in the vocabulary";
  else if (B < 1 || T < 1 || P < 1) why = "B, T, P >= 1";
  else if (mask && Tm != 1 && Tm != T) why = "Tm 1 or T";
  else if (!frl_obs_fit(B, T, P)) why = "B * T * P < 2^31 observations";
  else if (!frl_wg_in_range(workgroups)) why = "workgroups in 0..4096 (0: the library's choice)";
  if (why) return frl_failf(-2, "%s: needs %s", what, why);
  k.codes = codes; k.mask = mask; k.vocab = vocab;
  k.codes_float = codes_float; k.Tm = mask ? Tm : 1; k.G = G; k.B = B; k.T = T; k.P = (int)P;
  return 0;
}
