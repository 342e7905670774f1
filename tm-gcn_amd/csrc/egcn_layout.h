// What the narrow (evolvegcn.hip) and the wide (evolvegcn_wide.hip) EvolveGCN-H kernels share: the packed parameter
// layout, the total order of the top-k, the fp64 helpers of the GRU and the entry points' argument checks.
#pragma once
#include "common.h"

#include <math.h>

namespace tmgcn {
namespace {

__host__ __device__ constexpr int64_t eg_params(int F, int k) { return F + 3LL * (2LL * F * F + (int64_t)F * k); }

// packed P (the reference's draw order, ef:37-46): p [F] | W_Z U_Z [F][F] B_Z [F][k] | W_R U_R B_R | W_H U_H B_H
struct EgOff {
  int W[3], U[3], B[3];
  __host__ __device__ EgOff(int F, int k) {
    for (int g = 0; g < 3; ++g) {
      W[g] = F + g * (2 * F * F + F * k);
      U[g] = W[g] + F * F;
      B[g] = U[g] + F * F;
    }
  }
};

__device__ __forceinline__ bool eg_better(double s, int i, double s2, int i2) { return s > s2 || (s == s2 && i < i2); }

__device__ __forceinline__ double eg_norm(const double* __restrict__ p, int F) {
  double s = 0.0;
  for (int f = 0; f < F; ++f) s = fma(p[f], p[f], s);
  return sqrt(s);
}

__device__ __forceinline__ double eg_sigmoid(double x) { return 1.0 / (1.0 + exp(-x)); }

// The argument checks of tmgcn_egcn_fwd / _bwd and their wide twins, in the order the C-ABI reports them.  `supported`:
// the entry's width predicate; `max` / `without`: its domain as the message words it, 1..max each and, where `without` is
// not 0, minus the narrow kernels' 1..without each; `always` / `slices`: the pointers every call needs / those read only
// when T_run > 0 are all there.
inline int eg_check(const char* who, bool supported, int max, int without, int64_t N, int32_t T_run, int32_t F, int32_t k,
                    bool always, bool slices) {
  TMGCN_REQUIRE(supported || without, "%s: F=%d, k=%d outside 1..%d x 1..%d", who, F, k, max, max);
  TMGCN_REQUIRE(supported, "%s: F=%d, k=%d outside 1..%d x 1..%d without 1..%d x 1..%d (tmgcn_egcn_*)", who, F, k, max, max,
                without, without);
  TMGCN_REQUIRE(T_run >= 0 && T_run <= 65535, "%s: T_run=%d outside 0..65535", who, T_run);
  TMGCN_REQUIRE(N >= 0 && N < (int64_t)0x7fffffff, "%s: N=%lld outside 0..2^31-2", who, (long long)N);
  TMGCN_REQUIRE(T_run == 0 || N >= k, "%s: top-k needs N >= k (N=%lld, k=%d) (ef:82)", who, (long long)N, k);
  TMGCN_REQUIRE((int64_t)T_run * N * F < (int64_t)1 << 62, "%s: T_run x N x F too large", who);
  TMGCN_REQUIRE(always, "%s: null pointer", who);
  TMGCN_REQUIRE(T_run == 0 || slices, "%s: null pointer", who);
  return TMGCN_OK;
}

// the forward's layer-2 operands (rowptr given: the selected rows are formed again in fp64 from Â, X_prev and W_prev)
inline int eg_check_rows(const char* who, bool has_rowptr, bool operands, int32_t F_prev, int64_t N, int32_t T_run) {
  TMGCN_REQUIRE(!has_rowptr || (operands && F_prev >= 1),
                "%s: the fp64 rows of layer 2 need X_prev, W_prev and F_prev >= 1 (F_prev=%d)", who, F_prev);
  TMGCN_REQUIRE(!has_rowptr || (int64_t)T_run * N * F_prev < (int64_t)1 << 62, "%s: T_run x N x F_prev too large", who);
  return TMGCN_OK;
}

// what the backward does before its launches: the workspace (needed only when T_run > 0) and dH = 0 when asked for
inline int eg_bwd_prepare(const char* who, const void* workspace, int64_t workspace_bytes, int64_t need, float* dH, int64_t N,
                          int32_t T_run, int32_t F, hipStream_t st) {
  if (T_run > 0)
    if (int rc = check_workspace(who, workspace, workspace_bytes, need)) return rc;
  if (dH && T_run > 0 && hipMemsetAsync(dH, 0, (size_t)T_run * N * F * sizeof(float), st) != hipSuccess) {
    set_error("%s: hipMemsetAsync failed", who);
    return TMGCN_ERR_LAUNCH;
  }
  return TMGCN_OK;
}

}  // namespace
}  // namespace tmgcn
