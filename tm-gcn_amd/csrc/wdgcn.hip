// WD-GCN (TensorGCN-master/wd_gcn_functions.py, "wgf"): the GCN input map fused into the LSTM recurrence over the T
// slices, and its backpropagation through time.
//
//   forward   Y = relu(AX·W) (wgf:70), then for t = 0..T_run-1 (wgf:86-98)
//               f = σ(Y_t Wf + h Uf + bf)   j = σ(Y_t Wj + h Uj + bj)   o = σ(Y_t Wo + h Uo + bo)
//               ct = σ(Y_t Wc + h Uc + bc)  (a sigmoid on the candidate, as in the reference)
//               c = j·ct + f·c   h = o·tanh(c)   Z_t = h
//   backward  dZ -> dW, dWf..dWo, dUf..dUo, dbf..dbo; the gates are recomputed from the stored cell state and Z.
//
// Mapping: one lane per (node, hidden unit) in lane groups of G = 1, 2, 4 or 8 lanes (the power of two >= H), so a wave
// holds 64/G nodes.  A lane keeps its unit's columns of W and of the eight gate matrices in registers (the backward
// also the unit's rows) and works out its own y_t[u]; y_t and h_{t-1} are exchanged inside the lane group every step
// (__shfl within G lanes).  Nothing but Z (and the cell state when a gradient is wanted) is written.
//
// What bounds it: the chain of dependent instructions of one step (exchange, gate sums, four sigmoids, tanh), T_run
// times over: the work is only nodes x units wide (N·H lanes: 7 301 x 8 = 913 waves at the chess shape, fewer than the
// 1 024 SIMDs), so it is latency-bound.  The inputs of later steps do not depend on the recurrence: every lane keeps
// the loads of the next kWdPF steps in flight (a register ring), so no step waits on memory.
//
// The backward walks t downwards carrying dh and dc per lane.  Parameter gradients are summed in registers over a
// wave's nodes and steps (node groups are dealt to the waves statically: blockIdx.x, blockIdx.x + gridDim.x, ...),
// reduced across the wave's node groups with xor shuffles and written as one row of a per-wave slab; a second launch
// sums the rows in row order in fp64.  No atomics: two runs give the same bits.
#include "common.h"
#include "wdgcn_layout.h"   // wd_params, WdOff, wd_sigmoid

namespace tmgcn {
namespace {

constexpr int kWdMaxH = 8;          // hidden units (lane group of at most 8)
constexpr int kWdMaxF = 8;          // input features F0
constexpr int kWdPF = 8;            // steps whose inputs are in flight ahead of the one being computed
constexpr int kWdMaxRows = 1024;    // waves (= slab rows) of the backward

__host__ __device__ constexpr int wd_group(int H) { return H <= 1 ? 1 : H <= 2 ? 2 : H <= 4 ? 4 : 8; }
inline int64_t wd_rows(int64_t N, int H) {
  const int64_t groups = (N + 64 / wd_group(H) - 1) / (64 / wd_group(H));
  return groups < kWdMaxRows ? groups : kWdMaxRows;
}

// this lane's unit u: its column of W (w[i] = W[i][u]), of every gate matrix (wg[g][k] = Wg[k][u], ug[g][k] = Ug[k][u])
// and its biases; zero for the padding lanes u >= H
template <int H>
__device__ __forceinline__ void wd_load_columns(const float* __restrict__ P, int F0, int u, float (&w)[kWdMaxF],
                                                float (&wg)[4][H], float (&ug)[4][H], float (&b)[4]) {
  const WdOff o(F0, H);
  const bool ok = u < H;
#pragma unroll
  for (int i = 0; i < kWdMaxF; ++i) w[i] = (ok && i < F0) ? P[o.w + i * H + u] : 0.f;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int k = 0; k < H; ++k) {
      wg[g][k] = ok ? P[o.wg + g * H * H + k * H + u] : 0.f;
      ug[g][k] = ok ? P[o.ug + g * H * H + k * H + u] : 0.f;
    }
    b[g] = ok ? P[o.b + g * H + u] : 0.f;
  }
}

// one step's gates in lane u: z_g = (Σ_k y_k Wg[k][u] + Σ_k h_k Ug[k][u]) + bg[u]; y and h of the whole node come
// through the lane group (ys / hs keep them for the backward's parameter gradients)
template <int H, int G>
__device__ __forceinline__ void wd_gates(float y, float h, const float (&wg)[4][H], const float (&ug)[4][H],
                                         const float (&b)[4], float (&gate)[4], float (&ys)[H], float (&hs)[H]) {
  float sy[4] = {0.f, 0.f, 0.f, 0.f}, sh[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < H; ++k) {
    ys[k] = G > 1 ? __shfl(y, k, G) : y;
    hs[k] = G > 1 ? __shfl(h, k, G) : h;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      sy[g] = fmaf(ys[k], wg[g][k], sy[g]);
      sh[g] = fmaf(hs[k], ug[g][k], sh[g]);
    }
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) gate[g] = wd_sigmoid((sy[g] + sh[g]) + b[g]);
}

template <int H>
__global__ __launch_bounds__(64) void wdgcn_fwd_kernel(const float* __restrict__ AX, const float* __restrict__ P,
                                                       const float* __restrict__ h0, const float* __restrict__ c0,
                                                       float* __restrict__ Z, float* __restrict__ Cst, int64_t N,
                                                       int T_run, int F0) {
  constexpr int G = wd_group(H);
  const int lane = threadIdx.x;
  const int u = lane & (G - 1);
  const int64_t n = (int64_t)blockIdx.x * (64 / G) + lane / G;
  const bool node_ok = n < N, store = node_ok && u < H;
  float w[kWdMaxF], wg[4][H], ug[4][H], b[4];
  wd_load_columns<H>(P, F0, u, w, wg, ug, b);
  float h = u < H ? h0[u] : 0.f, c = u < H ? c0[u] : 0.f;      // wgf:87-88 (the same start for every node)

  const float* ax = AX + (node_ok ? n : 0) * F0;
  const int64_t step = N * F0;
  float pre[kWdPF][kWdMaxF];
#pragma unroll
  for (int s = 0; s < kWdPF; ++s)
#pragma unroll
    for (int i = 0; i < kWdMaxF; ++i) pre[s][i] = (node_ok && i < F0 && s < T_run) ? ax[s * step + i] : 0.f;

  for (int t0 = 0; t0 < T_run; t0 += kWdPF) {
#pragma unroll
    for (int s = 0; s < kWdPF; ++s) {
      const int t = t0 + s;
      if (t >= T_run) break;                                     // uniform: every lane leaves together
      float p = 0.f;
#pragma unroll
      for (int i = 0; i < kWdMaxF; ++i) p = fmaf(pre[s][i], w[i], p);
      const int tn = t + kWdPF;
#pragma unroll
      for (int i = 0; i < kWdMaxF; ++i) pre[s][i] = (node_ok && i < F0 && tn < T_run) ? ax[tn * step + i] : 0.f;
      const float y = fmaxf(p, 0.f);                             // wgf:70
      float gate[4], ys[H], hs[H];
      wd_gates<H, G>(y, h, wg, ug, b, gate, ys, hs);             // f j c o: wgf:90-93
      c = gate[1] * gate[2] + gate[0] * c;                       // wgf:94
      h = gate[3] * tanhf(c);                                    // wgf:95
      if (store) {
        const int64_t idx = ((int64_t)t * N + n) * H + u;
        Z[idx] = h;                                              // wgf:96
        if (Cst) Cst[idx] = c;
      }
    }
  }
}

template <int H>
__global__ __launch_bounds__(64) void wdgcn_bwd_kernel(const float* __restrict__ AX, const float* __restrict__ P,
                                                       const float* __restrict__ h0, const float* __restrict__ c0,
                                                       const float* __restrict__ Z, const float* __restrict__ Cst,
                                                       const float* __restrict__ dZ, float* __restrict__ slab,
                                                       int64_t N, int T_run, int F0) {
  constexpr int G = wd_group(H);
  const int lane = threadIdx.x;
  const int u = lane & (G - 1);
  const bool unit_ok = u < H;
  float w[kWdMaxF], wg[4][H], ug[4][H], b[4];
  wd_load_columns<H>(P, F0, u, w, wg, ug, b);
  // this lane's unit's ROWS of the gate matrices: dy_t[u] and dh_{t-1}[u] sum the gate gradients of all units
  const WdOff o(F0, H);
  float wr[4][H], ur[4][H];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int k = 0; k < H; ++k) {
      wr[g][k] = unit_ok ? P[o.wg + g * H * H + u * H + k] : 0.f;
      ur[g][k] = unit_ok ? P[o.ug + g * H * H + u * H + k] : 0.f;
    }
  const float hi = unit_ok ? h0[u] : 0.f, ci = unit_ok ? c0[u] : 0.f;

  float dw[kWdMaxF], dwg[4][H], dug[4][H], db[4];
#pragma unroll
  for (int i = 0; i < kWdMaxF; ++i) dw[i] = 0.f;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    db[g] = 0.f;
#pragma unroll
    for (int k = 0; k < H; ++k) dwg[g][k] = dug[g][k] = 0.f;
  }

  const int64_t n_groups = (N + 64 / G - 1) / (64 / G);
  const int64_t stepA = N * F0, stepZ = N * H;
  for (int64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const int64_t n = grp * (64 / G) + lane / G;
    const bool node_ok = n < N, ld = node_ok && unit_ok;
    const float* ax = AX + (node_ok ? n : 0) * F0;
    const int64_t zoff = (node_ok ? n : 0) * H + (unit_ok ? u : 0);
    // the ring holds, for step t: AX[t], dZ[t], and c_{t-1}, h_{t-1} (c0 / h0 at t = 0)
    float pa[kWdPF][kWdMaxF], pdz[kWdPF], pc[kWdPF], ph[kWdPF];
#pragma unroll
    for (int s = 0; s < kWdPF; ++s) {
      const int t = T_run - 1 - s;
#pragma unroll
      for (int i = 0; i < kWdMaxF; ++i) pa[s][i] = (node_ok && i < F0 && t >= 0) ? ax[t * stepA + i] : 0.f;
      pdz[s] = (ld && t >= 0) ? dZ[t * stepZ + zoff] : 0.f;
      pc[s] = (ld && t >= 1) ? Cst[(t - 1) * stepZ + zoff] : ci;
      ph[s] = (ld && t >= 1) ? Z[(t - 1) * stepZ + zoff] : hi;
    }
    float ct_ = ld ? Cst[(T_run - 1) * stepZ + zoff] : 0.f;        // c_t of the step being walked
    float dh = 0.f, dc = 0.f;
    for (int r0 = 0; r0 < T_run; r0 += kWdPF) {
#pragma unroll
      for (int s = 0; s < kWdPF; ++s) {
        const int t = T_run - 1 - (r0 + s);
        if (t < 0) break;                                          // uniform
        float a[kWdMaxF];
#pragma unroll
        for (int i = 0; i < kWdMaxF; ++i) a[i] = pa[s][i];
        const float dz = pdz[s], cp = pc[s], hp = ph[s];
        const int tn = t - kWdPF;
#pragma unroll
        for (int i = 0; i < kWdMaxF; ++i) pa[s][i] = (node_ok && i < F0 && tn >= 0) ? ax[tn * stepA + i] : 0.f;
        pdz[s] = (ld && tn >= 0) ? dZ[tn * stepZ + zoff] : 0.f;
        pc[s] = (ld && tn >= 1) ? Cst[(tn - 1) * stepZ + zoff] : ci;
        ph[s] = (ld && tn >= 1) ? Z[(tn - 1) * stepZ + zoff] : hi;

        // the step's forward again: y_t, the gates
        float p = 0.f;
#pragma unroll
        for (int i = 0; i < kWdMaxF; ++i) p = fmaf(a[i], w[i], p);
        float gate[4], ys[H], hs[H];
        wd_gates<H, G>(fmaxf(p, 0.f), hp, wg, ug, b, gate, ys, hs);
        const float f = gate[0], j = gate[1], cc = gate[2], og = gate[3];
        const float tc = tanhf(ct_);
        // h = o·tanh(c), c = j·ct + f·c_{t-1}
        const float dht = dz + dh;
        const float dct = dc + (dht * og) * (1.f - tc * tc);
        float dzg[4];
        dzg[0] = (dct * cp) * ((1.f - f) * f);
        dzg[1] = (dct * cc) * ((1.f - j) * j);
        dzg[2] = (dct * j) * ((1.f - cc) * cc);
        dzg[3] = (dht * tc) * ((1.f - og) * og);
        dc = dct * f;
        ct_ = cp;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          db[g] += dzg[g];
#pragma unroll
          for (int k = 0; k < H; ++k) {
            dwg[g][k] = fmaf(ys[k], dzg[g], dwg[g][k]);
            dug[g][k] = fmaf(hs[k], dzg[g], dug[g][k]);
          }
        }
        // dy_t[u] = Σ_g Σ_v dz_g[v] Wg[u][v],  dh_{t-1}[u] = Σ_g Σ_v dz_g[v] Ug[u][v]
        float dy = 0.f, dhn = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int v = 0; v < H; ++v) {
            const float q = G > 1 ? __shfl(dzg[g], v, G) : dzg[g];
            dy = fmaf(q, wr[g][v], dy);
            dhn = fmaf(q, ur[g][v], dhn);
          }
        dh = dhn;
        const float dp = p > 0.f ? dy : 0.f;                       // relu'
#pragma unroll
        for (int i = 0; i < kWdMaxF; ++i) dw[i] = fmaf(a[i], dp, dw[i]);
      }
    }
  }

  // the wave's node groups -> lanes 0..G-1 (fixed xor tree), then one slab row per wave
#pragma unroll
  for (int off = G; off < 64; off <<= 1) {
#pragma unroll
    for (int i = 0; i < kWdMaxF; ++i) dw[i] += __shfl_xor(dw[i], off, 64);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      db[g] += __shfl_xor(db[g], off, 64);
#pragma unroll
      for (int k = 0; k < H; ++k) {
        dwg[g][k] += __shfl_xor(dwg[g][k], off, 64);
        dug[g][k] += __shfl_xor(dug[g][k], off, 64);
      }
    }
  }
  if (lane < G && unit_ok) {
    float* row = slab + (int64_t)blockIdx.x * wd_params(F0, H);
#pragma unroll
    for (int i = 0; i < kWdMaxF; ++i)
      if (i < F0) row[o.w + i * H + u] = dw[i];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int k = 0; k < H; ++k) {
        row[o.wg + g * H * H + k * H + u] = dwg[g][k];
        row[o.ug + g * H * H + k * H + u] = dug[g][k];
      }
      row[o.b + g * H + u] = db[g];
    }
  }
}

// dP[j] = Σ_r slab[r][j], r ascending per thread then a fixed LDS tree (fp64): one block per parameter
__global__ __launch_bounds__(256) void wdgcn_slab_sum_kernel(const float* __restrict__ slab, float* __restrict__ dP,
                                                             int rows, int np) {
  __shared__ double part[256];
  const int j = blockIdx.x;
  double s = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) s += (double)slab[(int64_t)r * np + j];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) dP[j] = (float)part[0];
}

template <int H>
int wd_fwd(const float* AX, const float* P, const float* h0, const float* c0, float* Z, float* C, int64_t N, int T_run,
           int F0, hipStream_t st) {
  constexpr int G = wd_group(H);
  const int64_t blocks = (N + 64 / G - 1) / (64 / G);
  hipLaunchKernelGGL(wdgcn_fwd_kernel<H>, dim3((unsigned)blocks), dim3(64), 0, st, AX, P, h0, c0, Z, C, N, T_run, F0);
  return check_launch("wdgcn_fwd");
}

template <int H>
int wd_bwd(const float* AX, const float* P, const float* h0, const float* c0, const float* Z, const float* C,
           const float* dZ, float* dP, int64_t N, int T_run, int F0, float* slab, hipStream_t st) {
  const int rows = (int)wd_rows(N, H);
  hipLaunchKernelGGL(wdgcn_bwd_kernel<H>, dim3(rows), dim3(64), 0, st, AX, P, h0, c0, Z, C, dZ, slab, N, T_run, F0);
  int rc = check_launch("wdgcn_bwd");
  if (rc) return rc;
  const int np = (int)wd_params(F0, H);
  hipLaunchKernelGGL(wdgcn_slab_sum_kernel, dim3(np), dim3(256), 0, st, slab, dP, rows, np);
  return check_launch("wdgcn_bwd slab sum");
}

// f(std::integral_constant<int, H>) for the run-time H of 1..kWdMaxH: the kernels are instantiated per width
template <typename F>
int wd_dispatch(int H, F f) {
  switch (H) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

}  // namespace
}  // namespace tmgcn

using namespace tmgcn;

extern "C" int tmgcn_wdgcn_supported(int32_t F0, int32_t H) {
  return F0 >= 1 && F0 <= kWdMaxF && H >= 1 && H <= kWdMaxH;
}

extern "C" int64_t tmgcn_wdgcn_param_count(int32_t F0, int32_t H) {
  return tmgcn_wdgcn_supported(F0, H) ? wd_params(F0, H) : -1;
}

extern "C" int64_t tmgcn_wdgcn_bwd_workspace_bytes(int64_t N, int32_t F0, int32_t H) {
  if (!tmgcn_wdgcn_supported(F0, H) || N < 0) return -1;
  return N == 0 ? 0 : wd_rows(N, H) * wd_params(F0, H) * (int64_t)sizeof(float);
}

static int wd_check(const char* who, int64_t N, int32_t T_run, int32_t F0, int32_t H) {
  TMGCN_REQUIRE(tmgcn_wdgcn_supported(F0, H), "%s: F0=%d, H=%d outside 1..%d x 1..%d", who, F0, H, kWdMaxF, kWdMaxH);
  TMGCN_REQUIRE(N >= 0 && T_run >= 0, "%s: negative size (N=%lld, T_run=%d)", who, (long long)N, T_run);
  TMGCN_REQUIRE(N < (int64_t)1 << 31 && (int64_t)T_run * N * (H > F0 ? H : F0) < (int64_t)1 << 62,
                "%s: N=%lld too large", who, (long long)N);
  return TMGCN_OK;
}

extern "C" int tmgcn_wdgcn_fwd_f32(const float* AX, const float* P, const float* h0, const float* c0, float* Z, float* C,
                                   int64_t N, int32_t T_run, int32_t F0, int32_t H, void* stream) {
  if (int rc = wd_check("wdgcn_fwd", N, T_run, F0, H)) return rc;
  if (N == 0 || T_run == 0) return TMGCN_OK;
  TMGCN_REQUIRE(AX && P && h0 && c0 && Z, "wdgcn_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  return wd_dispatch(H, [&](auto h) { return wd_fwd<decltype(h)::value>(AX, P, h0, c0, Z, C, N, T_run, F0, st); });
}

extern "C" int tmgcn_wdgcn_bwd_f32(const float* AX, const float* P, const float* h0, const float* c0, const float* Z,
                                   const float* C, const float* dZ, float* dP, int64_t N, int32_t T_run, int32_t F0,
                                   int32_t H, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = wd_check("wdgcn_bwd", N, T_run, F0, H)) return rc;
  TMGCN_REQUIRE(dP, "wdgcn_bwd: null dP");
  hipStream_t st = (hipStream_t)stream;
  if (N == 0 || T_run == 0) {                                      // nothing ran: every gradient is zero
    if (hipMemsetAsync(dP, 0, wd_params(F0, H) * sizeof(float), st) != hipSuccess) {
      set_error("wdgcn_bwd: hipMemsetAsync failed");
      return TMGCN_ERR_LAUNCH;
    }
    return TMGCN_OK;
  }
  TMGCN_REQUIRE(AX && P && h0 && c0 && Z && C && dZ, "wdgcn_bwd: null pointer");
  if (int rc = check_workspace("wdgcn_bwd", workspace, workspace_bytes, tmgcn_wdgcn_bwd_workspace_bytes(N, F0, H))) return rc;
  float* slab = static_cast<float*>(workspace);
  return wd_dispatch(H, [&](auto h) {
    return wd_bwd<decltype(h)::value>(AX, P, h0, c0, Z, C, dZ, dP, N, T_run, F0, slab, st);
  });
}
