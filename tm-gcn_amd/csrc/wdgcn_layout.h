// What the narrow (wdgcn.hip) and the wide (wdgcn_wide.hip) WD-GCN kernels share: the packed parameter count and the
// sigmoid.  WdOff states the layout for both; the narrow kernels index through it, the wide kernels write the same
// offsets out (see wdgcn_wide.hip).
#pragma once
#include "common.h"

namespace tmgcn {
namespace {

__host__ __device__ constexpr int64_t wd_params(int F0, int H) { return (int64_t)F0 * H + 8LL * H * H + 4LL * H; }

// Packed parameters P (the order of wgf:36-51): W [F0][H] | Wf Wj Wc Wo [H][H] | Uf Uj Uc Uo [H][H] | bf bj bc bo [H]
struct WdOff {
  int w, wg, ug, b;
  __host__ __device__ __forceinline__ WdOff(int F0, int H)
      : w(0), wg(F0 * H), ug(F0 * H + 4 * H * H), b(F0 * H + 8 * H * H) {}
};

__device__ __forceinline__ float wd_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

}  // namespace
}  // namespace tmgcn
