// What the narrow (evolvegcn.hip) and the wide (evolvegcn_wide.hip) EvolveGCN-H kernels share: the packed parameter
// layout, the total order of the top-k and the fp64 helpers of the GRU.
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

}  // namespace
}  // namespace tmgcn
