// EvolveGCN-H at widths up to 64 x 64 (the statements and tensors of evolvegcn.hip; F = the layer's input width, k = its
// output width, every pair of 1..64 x 1..64 that is not 1..8 x 1..8).  Everything the reference has in fp64 stays fp64,
// on the vector FMAs.
//
// Selection.  Scores, top-k and X_g depend on the layer input and on p only: all T_run slices at once.  A block takes
// kEgwSort = 1024 nodes of one slice, writes (score, node) pairs to LDS — NaN as the sentinel (-inf, 2^31-1) that ranks
// below every node — and sorts them with a bitonic network under the total order of evolvegcn.hip (higher score first,
// equal scores by the lower node index); its best 64 are the block's candidates.  One block per slice then folds the
// candidates in, 960 at a time next to the best 64 so far, with the same sort.  The order is total, so the selected set
// and its order depend neither on the block count nor on the order of the folds.  A third launch, one wave per selected
// row, forms the row (for layer 2 again in fp64 from Â, X_prev and W_prev[t+1]), its score, H_sel and X_g.
//
// Chain.  Every product of the matrix GRU is a left multiplication and the rest is elementwise: column j of W_t depends
// on column j of X_t, of W_{t-1} and of the biases only.  One wave per column walks t with lane f holding entry (f, j);
// the blocks never synchronise.  The input-side products W_g·X_t do not depend on the chain and come from a launch of
// their own, over (t, g); the chain keeps U_Z, U_R, U_H in LDS (F padded to a multiple of 8; 3·64·64 doubles = 96 KiB at
// F = 64, transposed so that lanes read consecutive words) and the loads of the next kEgwPF steps in flight.
//
// Backward.  The BPTT chain runs the same way, t downwards, carrying dW and writing daz, dar, dah (pre-activation);
// dX_t = W_Zᵀ·daz + W_Rᵀ·dar + W_Hᵀ·dah follows for all t at once; the six F x F parameter gradients are sums over
// (t, j) of outer products, one 16 x 16 tile per block walking t and j upwards; the biases sum over t; the summary's
// backward is that of evolvegcn.hip.  No atomics, every sum in a fixed order: two runs give the same bits.
// Launches: 5 forward, 5 backward (+ one memset when dH is asked for), whatever T_run is.
#include "common.h"
#include "egcn_layout.h"

#include <math.h>

namespace tmgcn {
namespace {

constexpr int kEgwMax = 64;          // F and k
constexpr int kEgNarrowMax = 8;      // both at most this: the narrow kernels' domain
constexpr int kEgwL = 64;            // candidates a block keeps (>= k)
constexpr int kEgwThreads = 256;
constexpr int kEgwSort = 1024;       // entries of the LDS sort = nodes a selection block covers
constexpr int kEgwFold = kEgwSort - kEgwL;
constexpr int kEgwPF = 4;            // chain steps whose inputs are in flight ahead of the one being computed
constexpr int kEgwNone = 0x7fffffff; // ranks below every node, -inf scores included
constexpr int kEgwTile = 16;         // the parameter-gradient tile

__host__ __device__ constexpr int egw_pad(int F) { return (F + 7) & ~7; }   // the chain's LDS stride
// EgOff's W[g] / U[g] for a gate index that is not a compile-time constant (indexing the struct's arrays with one would
// put them in scratch)
__device__ __forceinline__ int egw_off_w(int F, int k, int g) { return F + g * (2 * F * F + F * k); }
__device__ __forceinline__ int egw_off_u(int F, int k, int g) { return egw_off_w(F, k, g) + F * F; }
inline int64_t egw_blocks(int64_t N) { return (N + kEgwSort - 1) / kEgwSort; }

// the kEgwSort pairs of (s, ix) -> descending.  All threads of the block; the pairs must be visible (a barrier after the
// last write), and a barrier follows the last stage.
__device__ __forceinline__ void egw_sort(double* s, int* ix) {
  for (int w = 2; w <= kEgwSort; w <<= 1)
    for (int d = w >> 1; d > 0; d >>= 1) {
      for (int i = threadIdx.x; i < kEgwSort / 2; i += kEgwThreads) {
        const int lo = ((i & ~(d - 1)) << 1) | (i & (d - 1)), hi = lo + d;
        const double sa = s[lo], sb = s[hi];
        const int ia = ix[lo], ib = ix[hi];
        const bool sw = (lo & w) == 0 ? eg_better(sb, ib, sa, ia) : eg_better(sa, ia, sb, ib);
        if (sw) {
          s[lo] = sb;
          ix[lo] = ib;
          s[hi] = sa;
          ix[hi] = ia;
        }
      }
      __syncthreads();
    }
}

// grid (blocks per slice, T_run): the best kEgwL of the block's nodes -> cs / ci [T_run][nblk][kEgwL]
__global__ __launch_bounds__(kEgwThreads) void egw_topk_kernel(const float* __restrict__ H, const double* __restrict__ P,
                                                               int64_t N, int F, int vec4, double* __restrict__ cs,
                                                               int* __restrict__ ci) {
  __shared__ double ls[kEgwSort];
  __shared__ int li[kEgwSort];
  __shared__ double pl[kEgwMax];
  const int t = blockIdx.y, nblk = gridDim.x, tid = threadIdx.x;
  if (tid < kEgwMax) pl[tid] = tid < F ? P[tid] : 0.0;
  __syncthreads();
  const double nrm = eg_norm(pl, F);
#pragma unroll
  for (int r = 0; r < kEgwSort / kEgwThreads; ++r) {
    const int slot = r * kEgwThreads + tid;
    const int64_t n = (int64_t)blockIdx.x * kEgwSort + slot;
    double sc = -INFINITY;
    int id = kEgwNone;
    if (n < N) {
      const float* h = H + ((int64_t)t * N + n) * F;
      double d = 0.0;
      if (vec4) {
        for (int f = 0; f < F; f += 4) {
          const float4 v = *reinterpret_cast<const float4*>(h + f);
          d = fma((double)v.x, pl[f], d);
          d = fma((double)v.y, pl[f + 1], d);
          d = fma((double)v.z, pl[f + 2], d);
          d = fma((double)v.w, pl[f + 3], d);
        }
      } else {
        for (int f = 0; f < F; ++f) d = fma((double)h[f], pl[f], d);
      }
      const double y = d / nrm;                                  // ef:81
      if (!isnan(y)) {                                           // NaN keeps the sentinel: never selected
        sc = y;
        id = (int)n;
      }
    }
    ls[slot] = sc;
    li[slot] = id;
  }
  __syncthreads();
  egw_sort(ls, li);
  if (tid < kEgwL) {
    const int64_t o = ((int64_t)t * nblk + blockIdx.x) * kEgwL + tid;
    cs[o] = ls[tid];
    ci[o] = li[tid];
  }
}

// one block per slice: fold the slice's nblk·kEgwL candidates into the best kEgwL; idx [T_run][k] (-1: none) and the
// fp32-ranked score y_sel [T_run][k]
__global__ __launch_bounds__(kEgwThreads) void egw_select_kernel(const double* __restrict__ cs, const int* __restrict__ ci,
                                                                 int nblk, int k, int* __restrict__ idx,
                                                                 double* __restrict__ ysel) {
  __shared__ double ls[kEgwSort];
  __shared__ int li[kEgwSort];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int64_t nc = (int64_t)nblk * kEgwL;
  const double* cst = cs + (int64_t)t * nc;
  const int* cit = ci + (int64_t)t * nc;
  if (tid < kEgwL) {
    ls[tid] = -INFINITY;
    li[tid] = kEgwNone;
  }
  for (int64_t c0 = 0; c0 < nc; c0 += kEgwFold) {
    for (int slot = kEgwL + tid; slot < kEgwSort; slot += kEgwThreads) {
      const int64_t c = c0 + (slot - kEgwL);
      ls[slot] = c < nc ? cst[c] : -INFINITY;
      li[slot] = c < nc ? cit[c] : kEgwNone;
    }
    __syncthreads();
    egw_sort(ls, li);
  }
  if (tid < k) {
    const int n = li[tid];
    idx[(int64_t)t * k + tid] = n != kEgwNone ? n : -1;
    ysel[(int64_t)t * k + tid] = n != kEgwNone ? ls[tid] : 0.0;
  }
}

// grid (k, T_run), one wave per selected row: H_sel [T_run][k][F], X_g [T_run][F][k], and with rowptr (layer 2:
// H = relu(Â_t·X_t·W_t) of the layer below, stored in fp32 for the GCONV) the row and its score formed again in fp64 from
// Â (CSR), X_prev and the fp64 W_prev[t+1] — the ranking stays the fp32 one.  Any F_prev: 64 columns of Â·X at a time.
__global__ __launch_bounds__(64) void egw_rows_kernel(const float* __restrict__ H, const double* __restrict__ P, int64_t N,
                                                      int F, int k, const int64_t* __restrict__ rowptr,
                                                      const int* __restrict__ col, const float* __restrict__ val,
                                                      const float* __restrict__ Xp, const double* __restrict__ Wp, int Fp,
                                                      const int* __restrict__ idx, double* __restrict__ ysel,
                                                      double* __restrict__ Hsel, double* __restrict__ Xg) {
  __shared__ double ax[64], hh[kEgwMax];
  const int j = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
  const int64_t q = (int64_t)t * k + j;
  const int n = idx[q];
  const bool act = lane < F;
  double h = 0.0, y = 0.0;
  if (n >= 0 && rowptr) {
    const double* w = Wp + (int64_t)(t + 1) * Fp * F;
    const int64_t r = (int64_t)t * N + n, e0 = rowptr[r], e1 = rowptr[r + 1];
    double a = 0.0;
    for (int q0 = 0; q0 < Fp; q0 += 64) {                        // uniform
      const int qq = q0 + lane;
      double s = 0.0;
      if (qq < Fp)
        for (int64_t e = e0; e < e1; ++e) s = fma((double)val[e], (double)Xp[((int64_t)t * N + col[e]) * Fp + qq], s);
      ax[lane] = s;
      __syncthreads();
      const int qn = Fp - q0 < 64 ? Fp - q0 : 64;
      if (act)
        for (int m = 0; m < qn; ++m) a = fma(ax[m], w[(int64_t)(q0 + m) * F + lane], a);
      __syncthreads();
    }
    h = a > 0.0 ? a : 0.0;                                       // relu (ef:168)
    hh[lane] = act ? h : 0.0;
    __syncthreads();
    double d = 0.0;
    for (int f = 0; f < F; ++f) d = fma(hh[f], P[f], d);
    y = d / eg_norm(P, F);                                       // ef:185
  } else if (n >= 0) {
    if (act) h = (double)H[((int64_t)t * N + n) * F + lane];
    y = ysel[q];
  }
  if (rowptr && lane == 0) ysel[q] = y;
  if (act) {
    Hsel[q * F + lane] = h;
    Xg[((int64_t)t * F + lane) * k + j] = h * y;                 // ef:83
  }
}

// grid (T_run, 3): pre[j][t][g][f] = (W_g·X_t)[f][j] — the part of the gates that does not depend on the chain, stored by
// column so that the chain's lanes read consecutive words
__global__ __launch_bounds__(kEgwThreads) void egw_hoist_kernel(const double* __restrict__ P, const double* __restrict__ Xg,
                                                                int T_run, int F, int k, double* __restrict__ pre) {
  const int t = blockIdx.x, g = blockIdx.y;
  const EgOff o(F, k);
  const double* W = P + o.W[g];
  const double* X = Xg + (int64_t)t * F * k;
  for (int e = threadIdx.x; e < F * k; e += kEgwThreads) {
    const int f = e / k, j = e - f * k;
    double s = 0.0;
    for (int m = 0; m < F; ++m) s = fma(W[f * F + m], X[m * k + j], s);
    pre[(((int64_t)j * T_run + t) * 3 + g) * F + f] = s;
  }
}

// grid (k): one wave per column j, lane f = entry (f, j).  W_seq[0] = W0, W_seq[t+1] = g(X_g[t], W_seq[t]) (ef:86-91);
// W32[t] = (float)W_seq[t+1]; gates (when not null) keep Z, R, Ĥ of every step for the backward.
// LDS: Ut [3][FP][FP] (Ut[g][m][f] = U_g[f][m]; FP = F rounded up to 8, zero beyond F, so that the products run in
// groups of 8 whose LDS reads are issued together) | hs [64] | rs [64]
__global__ __launch_bounds__(64) void egw_chain_fwd_kernel(const double* __restrict__ P, const double* __restrict__ W0,
                                                           const double* __restrict__ pre, int T_run, int F, int k,
                                                           double* __restrict__ Wseq, float* __restrict__ W32,
                                                           double* __restrict__ gates) {
  extern __shared__ double egw_lds[];
  const int FP = egw_pad(F), FF = FP * FP, Fk = F * k, lane = threadIdx.x, j = blockIdx.x;
  double* Ut = egw_lds;
  double* hs = Ut + 3 * FF;
  double* rs = hs + 64;
  const EgOff o(F, k);
  for (int i = lane; i < 3 * FF; i += 64) {
    const int g = i / FF, r = i - g * FF, m = r / FP, f = r - m * FP;
    Ut[i] = (m < F && f < F) ? P[egw_off_u(F, k, g) + f * F + m] : 0.0;
  }
  const bool act = lane < F;
  const int f = act ? lane : 0, e = f * k + j;
  const double bz = P[o.B[0] + e], br = P[o.B[1] + e], bh = P[o.B[2] + e];
  double h = W0[e];
  if (act) Wseq[e] = h;
  const double* uz = Ut + f;
  const double* ur = Ut + FF + f;
  const double* uh = Ut + 2 * FF + f;
  const double* pj = pre + (int64_t)j * T_run * 3 * F + f;

  double pz[kEgwPF], pr[kEgwPF], ph[kEgwPF];                      // (W_g·X_t)[f][j] of the steps in flight
#pragma unroll
  for (int s = 0; s < kEgwPF; ++s) {
    const bool ld = s < T_run;
    pz[s] = ld ? pj[(int64_t)s * 3 * F] : 0.0;
    pr[s] = ld ? pj[(int64_t)s * 3 * F + F] : 0.0;
    ph[s] = ld ? pj[(int64_t)s * 3 * F + 2 * F] : 0.0;
  }
  __syncthreads();
  for (int t0 = 0; t0 < T_run; t0 += kEgwPF) {
#pragma unroll
    for (int s = 0; s < kEgwPF; ++s) {
      const int t = t0 + s;
      if (t >= T_run) break;                                     // uniform
      const double ax = pz[s], ar = pr[s], ah = ph[s];
      const int tn = t + kEgwPF;
      const bool ld = tn < T_run;
      pz[s] = ld ? pj[(int64_t)tn * 3 * F] : 0.0;
      pr[s] = ld ? pj[(int64_t)tn * 3 * F + F] : 0.0;
      ph[s] = ld ? pj[(int64_t)tn * 3 * F + 2 * F] : 0.0;
      hs[lane] = act ? h : 0.0;
      __syncthreads();
      double az0 = 0.0, az1 = 0.0, ar0 = 0.0, ar1 = 0.0;         // even and odd m: two chains per product
      for (int m = 0; m < FP; m += 8) {
        double hv[8], a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          hv[u] = hs[m + u];
          a[u] = uz[(m + u) * FP];
          b[u] = ur[(m + u) * FP];
        }
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
          az0 = fma(a[u], hv[u], az0);
          ar0 = fma(b[u], hv[u], ar0);
          az1 = fma(a[u + 1], hv[u + 1], az1);
          ar1 = fma(b[u + 1], hv[u + 1], ar1);
        }
      }
      const double Z = eg_sigmoid((ax + (az0 + az1)) + bz);      // ef:87
      const double R = eg_sigmoid((ar + (ar0 + ar1)) + br);      // ef:88
      rs[lane] = act ? R * h : 0.0;
      __syncthreads();
      double ah0 = 0.0, ah1 = 0.0;
      for (int m = 0; m < FP; m += 8) {
        double rv[8], a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          rv[u] = rs[m + u];
          a[u] = uh[(m + u) * FP];
        }
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
          ah0 = fma(a[u], rv[u], ah0);
          ah1 = fma(a[u + 1], rv[u + 1], ah1);
        }
      }
      const double Ht = tanh((ah + (ah0 + ah1)) + bh);           // ef:89
      const double hn = (1.0 - Z) * h + Z * Ht;                  // ef:90
      if (act) {
        Wseq[(int64_t)(t + 1) * Fk + e] = hn;
        W32[(int64_t)t * Fk + e] = (float)hn;
        if (gates) {
          double* gt = gates + (int64_t)t * 3 * Fk + e;
          gt[0] = Z;
          gt[Fk] = R;
          gt[2 * Fk] = Ht;
        }
      }
      h = hn;
    }
  }
}

// grid (k): one wave per column j, t = T_run-1..0: with G = dL/dW_t (carried + dW32[t] + dWseq[t+1]) the step's
// pre-activation gradients daz, dar, dah -> dA [T_run][4][F·k] (slot 3, dX, is egw_dx_kernel's); dW0 = the carried
// gradient after t = 0 (+ dWseq[0]).  LDS: U [3][FP][FP] (U[g][m][f] = U_g[m][f], zero beyond F) | e1 e2 e3 [64]: dah,
// daz, dar of the column
__global__ __launch_bounds__(64) void egw_chain_bwd_kernel(const double* __restrict__ P, const double* __restrict__ Wseq,
                                                           const double* __restrict__ gates,
                                                           const float* __restrict__ dW32,
                                                           const double* __restrict__ dWseq, int T_run, int F, int k,
                                                           double* __restrict__ dA, double* __restrict__ dW0) {
  extern __shared__ double egw_lds[];
  const int FP = egw_pad(F), FF = FP * FP, Fk = F * k, lane = threadIdx.x, j = blockIdx.x;
  double* U = egw_lds;
  double* e1 = U + 3 * FF;
  double* e2 = e1 + 64;
  double* e3 = e2 + 64;
  const EgOff o(F, k);
  for (int i = lane; i < 3 * FF; i += 64) {
    const int g = i / FF, r = i - g * FF, m = r / FP, f = r - m * FP;
    U[i] = (m < F && f < F) ? P[egw_off_u(F, k, g) + m * F + f] : 0.0;
  }
  const bool act = lane < F;
  const int f = act ? lane : 0, e = f * k + j;
  const double* cuz = U + f;                                     // column f: U_g[m][f]
  const double* cur = U + FF + f;
  const double* cuh = U + 2 * FF + f;
  // the ring, for step t: W_t (the step's input), Z R Ĥ, and the injected gradient of the step's output
  double ph[kEgwPF], pz[kEgwPF], pr[kEgwPF], pt[kEgwPF], pg[kEgwPF];
#pragma unroll
  for (int s = 0; s < kEgwPF; ++s) {
    const int t = T_run - 1 - s;
    const bool ld = t >= 0;
    ph[s] = ld ? Wseq[(int64_t)t * Fk + e] : 0.0;
    pz[s] = ld ? gates[(int64_t)t * 3 * Fk + e] : 0.0;
    pr[s] = ld ? gates[(int64_t)t * 3 * Fk + Fk + e] : 0.0;
    pt[s] = ld ? gates[(int64_t)t * 3 * Fk + 2 * Fk + e] : 0.0;
    pg[s] = (ld && dW32 ? (double)dW32[(int64_t)t * Fk + e] : 0.0) + (ld && dWseq ? dWseq[(int64_t)(t + 1) * Fk + e] : 0.0);
  }
  __syncthreads();
  double Gc = 0.0;
  for (int r0 = 0; r0 < T_run; r0 += kEgwPF) {
#pragma unroll
    for (int s = 0; s < kEgwPF; ++s) {
      const int t = T_run - 1 - (r0 + s);
      if (t < 0) break;                                          // uniform
      const double h = ph[s], Z = pz[s], R = pr[s], Ht = pt[s], G = Gc + pg[s];
      const int tn = t - kEgwPF;
      const bool ld = tn >= 0;
      ph[s] = ld ? Wseq[(int64_t)tn * Fk + e] : 0.0;
      pz[s] = ld ? gates[(int64_t)tn * 3 * Fk + e] : 0.0;
      pr[s] = ld ? gates[(int64_t)tn * 3 * Fk + Fk + e] : 0.0;
      pt[s] = ld ? gates[(int64_t)tn * 3 * Fk + 2 * Fk + e] : 0.0;
      pg[s] = (ld && dW32 ? (double)dW32[(int64_t)tn * Fk + e] : 0.0) +
              (ld && dWseq ? dWseq[(int64_t)(tn + 1) * Fk + e] : 0.0);

      // W_t = (1−Z)∘H + Z∘Ĥ
      const double daz = (G * (Ht - h)) * (Z * (1.0 - Z));
      const double dah = (G * Z) * (1.0 - Ht * Ht);
      e1[lane] = act ? dah : 0.0;
      e2[lane] = act ? daz : 0.0;
      __syncthreads();
      double d0 = 0.0, d1 = 0.0;                                 // (U_Hᵀ dah)[f][j]
      for (int m = 0; m < FP; m += 8) {
        double ev[8], a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          ev[u] = e1[m + u];
          a[u] = cuh[(m + u) * FP];
        }
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
          d0 = fma(a[u], ev[u], d0);
          d1 = fma(a[u + 1], ev[u + 1], d1);
        }
      }
      const double dRH = d0 + d1;
      const double dar = (dRH * h) * (R * (1.0 - R));
      e3[lane] = act ? dar : 0.0;
      __syncthreads();
      double z0 = 0.0, r1 = 0.0;                                 // (U_Zᵀ daz)[f][j], (U_Rᵀ dar)[f][j]
      for (int m = 0; m < FP; m += 8) {
        double zv[8], rv[8], a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          zv[u] = e2[m + u];
          rv[u] = e3[m + u];
          a[u] = cuz[(m + u) * FP];
          b[u] = cur[(m + u) * FP];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          z0 = fma(a[u], zv[u], z0);
          r1 = fma(b[u], rv[u], r1);
        }
      }
      if (act) {
        double* d = dA + (int64_t)t * 4 * Fk + e;
        d[0] = daz;
        d[Fk] = dar;
        d[2 * Fk] = dah;
      }
      Gc = (G * (1.0 - Z) + dRH * R) + (z0 + r1);
    }
  }
  if (act) dW0[e] = Gc + (dWseq ? dWseq[e] : 0.0);
}

// grid (blocks over F·k, T_run): dX_t[m][j] = Σ_f W_Z[f][m]·daz[f][j] + W_R[f][m]·dar[f][j] + W_H[f][m]·dah[f][j]
__global__ __launch_bounds__(kEgwThreads) void egw_dx_kernel(const double* __restrict__ P, int F, int k,
                                                             double* __restrict__ dA) {
  const int Fk = F * k, t = blockIdx.y, e = blockIdx.x * kEgwThreads + threadIdx.x;
  if (e >= Fk) return;
  const int m = e / k, j = e - m * k;
  const EgOff o(F, k);
  const double* wz = P + o.W[0] + m;
  const double* wr = P + o.W[1] + m;
  const double* wh = P + o.W[2] + m;
  double* d = dA + (int64_t)t * 4 * Fk;
  double dx = 0.0;
  for (int f = 0; f < F; ++f) {
    dx = fma(wz[f * F], d[f * k + j], dx);
    dx = fma(wr[f * F], d[Fk + f * k + j], dx);
    dx = fma(wh[f * F], d[2 * Fk + f * k + j], dx);
  }
  d[3 * Fk + e] = dx;
}

// grid (T_run), one wave: dy[t][j] = dZs_j·H[idx_j] (dZs[j][m] = dX[m][j]) and, when asked for,
// dH[idx_j] = y_j·dZs_j + dy_j·p/‖p‖ (the indices of one slice are distinct)
__global__ __launch_bounds__(64) void egw_dy_kernel(const double* __restrict__ Hsel, const double* __restrict__ P,
                                                    const double* __restrict__ dA, const int* __restrict__ idx,
                                                    const double* __restrict__ ysel, int64_t N, int F, int k,
                                                    double* __restrict__ dy, float* __restrict__ dH) {
  const int t = blockIdx.x, j = threadIdx.x, Fk = F * k;
  if (j >= k) return;
  const int64_t q = (int64_t)t * k + j;
  const double* dX = dA + (int64_t)t * 4 * Fk + 3 * Fk;
  const double* h = Hsel + q * F;
  double d = 0.0;
  for (int m = 0; m < F; ++m) d = fma(dX[m * k + j], h[m], d);
  const int n = idx[q];
  dy[q] = n >= 0 ? d : 0.0;
  if (dH && n >= 0) {
    const double nrm = eg_norm(P, F), y = ysel[q];
    float* g = dH + ((int64_t)t * N + n) * F;
    for (int m = 0; m < F; ++m) g[m] = (float)(y * dX[m * k + j] + d * (P[m] / nrm));
  }
}

// grid (tiles over m, tiles over f, 6 = gate x {W, U}): dM[f][m] = Σ_t Σ_j d_g[t][f][j]·In[t][m][j] with In = X_g (W_g),
// W_{t-1} (U_Z, U_R) or R∘W_{t-1} (U_H); t and j upwards.  The next slice's tiles are in registers while this one's are
// multiplied out of LDS.
__global__ __launch_bounds__(kEgwThreads) void egw_mat_grad_kernel(const double* __restrict__ Xg,
                                                                   const double* __restrict__ Wseq,
                                                                   const double* __restrict__ gates,
                                                                   const double* __restrict__ dA, int T_run, int F, int k,
                                                                   double* __restrict__ dP) {
  constexpr int LD = kEgwMax + 1, PER = kEgwTile * kEgwMax / kEgwThreads;
  __shared__ double Ds[kEgwTile * LD], Is[kEgwTile * LD];
  const int tid = threadIdx.x, tf = tid / kEgwTile, tm = tid - tf * kEgwTile;
  const int f0 = blockIdx.y * kEgwTile, m0 = blockIdx.x * kEgwTile, g = blockIdx.z >> 1, isU = blockIdx.z & 1;
  const int Fk = F * k, ne = kEgwTile * k;
  double rd[PER], ri[PER];
  auto fetch = [&](int t) {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = q * kEgwThreads + tid, r = e / k, j = e - r * k;
      double vd = 0.0, vi = 0.0;
      if (e < ne) {
        if (f0 + r < F) vd = dA[(int64_t)t * 4 * Fk + g * Fk + (f0 + r) * k + j];
        if (m0 + r < F) {
          const int64_t a = (int64_t)t * Fk + (m0 + r) * k + j;
          if (!isU) vi = Xg[a];
          else vi = g == 2 ? gates[(int64_t)t * 3 * Fk + Fk + (m0 + r) * k + j] * Wseq[a] : Wseq[a];
        }
      }
      rd[q] = vd;
      ri[q] = vi;
    }
  };
  double s = 0.0;
  if (T_run > 0) fetch(0);
  for (int t = 0; t < T_run; ++t) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int e = q * kEgwThreads + tid, r = e / k, j = e - r * k;
      if (e < ne) {
        Ds[r * LD + j] = rd[q];
        Is[r * LD + j] = ri[q];
      }
    }
    __syncthreads();
    if (t + 1 < T_run) fetch(t + 1);
    for (int j = 0; j < k; ++j) s = fma(Ds[tf * LD + j], Is[tm * LD + j], s);
  }
  if (f0 + tf < F && m0 + tm < F) dP[(isU ? egw_off_u(F, k, g) : egw_off_w(F, k, g)) + (f0 + tf) * F + (m0 + tm)] = s;
}

// blocks 0..F-1, one wave each: dp[e] = Σ_t Σ_j dy_j·(H[idx_j][e]/‖p‖ − y_j·p[e]/‖p‖²), lane l taking the pairs l, l + 64,
// ... upwards and a fixed xor tree over the lanes; the blocks after them: dB_g[f][j] = Σ_t d_g[t][f][j], 64 entries each
__global__ __launch_bounds__(64) void egw_small_grad_kernel(const double* __restrict__ Hsel, const double* __restrict__ P,
                                                            const double* __restrict__ dA, const double* __restrict__ dy,
                                                            const int* __restrict__ idx, const double* __restrict__ ysel,
                                                            int T_run, int F, int k, double* __restrict__ dP) {
  const int lane = threadIdx.x, Fk = F * k, b = blockIdx.x;
  if (b < F) {
    const double nrm = eg_norm(P, F);
    const int64_t pairs = (int64_t)T_run * k;
    double s = 0.0;
    for (int64_t q = lane; q < pairs; q += 64) {
      if (idx[q] < 0) continue;
      s = fma(dy[q], Hsel[q * F + b] / nrm - ysel[q] * P[b] / (nrm * nrm), s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) dP[b] = s;
    return;
  }
  const int i = (b - F) * 64 + lane;
  if (i >= 3 * Fk) return;
  const int g = i / Fk, r = i - g * Fk;
  double s = 0.0;
  for (int t = 0; t < T_run; ++t) s += dA[(int64_t)t * 4 * Fk + g * Fk + r];
  const EgOff o(F, k);
  dP[o.B[g] + r] = s;
}

inline int64_t egw_cand_count(int64_t N, int T_run) { return (int64_t)T_run * egw_blocks(N) * kEgwL; }

}  // namespace
}  // namespace tmgcn

using namespace tmgcn;

extern "C" int tmgcn_egcn_wide_supported(int32_t F, int32_t k) {
  return F >= 1 && F <= kEgwMax && k >= 1 && k <= kEgwMax && !(F <= kEgNarrowMax && k <= kEgNarrowMax);
}

// candidates (score fp64, node int32) | pre [k][T_run][3][F] fp64; the doubles first
extern "C" int64_t tmgcn_egcn_wide_fwd_workspace_bytes(int64_t N, int32_t T_run, int32_t F, int32_t k) {
  if (!tmgcn_egcn_wide_supported(F, k) || N < 0 || T_run < 0) return -1;
  return egw_cand_count(N, T_run) * (int64_t)(sizeof(double) + sizeof(int)) + (int64_t)T_run * 3LL * F * k * (int64_t)sizeof(double);
}

// dA [T_run][4][F·k] | dy [T_run][k]
extern "C" int64_t tmgcn_egcn_wide_bwd_workspace_bytes(int32_t T_run, int32_t F, int32_t k) {
  if (!tmgcn_egcn_wide_supported(F, k) || T_run < 0) return -1;
  return (int64_t)T_run * (4LL * F * k + k) * (int64_t)sizeof(double);
}

extern "C" int tmgcn_egcn_wide_fwd(const float* H, const double* P, const double* W0, const int64_t* rowptr,
                                   const int32_t* col, const float* val, const float* X_prev, const double* W_prev,
                                   int32_t F_prev, int32_t* idx, double* ysel, double* Hsel, double* Xg, double* Wseq,
                                   float* W32, double* gates, int64_t N, int32_t T_run, int32_t F, int32_t k,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = eg_check("egcn_wide_fwd", tmgcn_egcn_wide_supported(F, k), kEgwMax, kEgNarrowMax, N, T_run, F, k,
                        P && W0 && Wseq, H && idx && ysel && Hsel && Xg && W32))
    return rc;
  if (int rc = eg_check_rows("egcn_wide_fwd", rowptr, X_prev && W_prev, F_prev, N, T_run)) return rc;
  hipStream_t st = (hipStream_t)stream;
  double* pre = nullptr;
  if (T_run > 0) {
    if (int rc = check_workspace("egcn_wide_fwd", workspace, workspace_bytes,
                                 tmgcn_egcn_wide_fwd_workspace_bytes(N, T_run, F, k)))
      return rc;
    const int64_t nblk = egw_blocks(N);
    double* cs = static_cast<double*>(workspace);
    pre = cs + egw_cand_count(N, T_run);
    int* ci = reinterpret_cast<int*>(pre + (int64_t)T_run * 3 * F * k);
    const int vec4 = F % 4 == 0 && (reinterpret_cast<uintptr_t>(H) & 15) == 0;
    hipLaunchKernelGGL(egw_topk_kernel, dim3((unsigned)nblk, (unsigned)T_run), dim3(kEgwThreads), 0, st, H, P, N, (int)F, vec4,
                       cs, ci);
    if (int rc = check_launch("egcn_wide_fwd topk")) return rc;
    hipLaunchKernelGGL(egw_select_kernel, dim3((unsigned)T_run), dim3(kEgwThreads), 0, st, cs, ci, (int)nblk, (int)k, idx, ysel);
    if (int rc = check_launch("egcn_wide_fwd select")) return rc;
    hipLaunchKernelGGL(egw_rows_kernel, dim3((unsigned)k, (unsigned)T_run), dim3(64), 0, st, H, P, N, (int)F, (int)k, rowptr, col,
                       val, X_prev, W_prev, (int)F_prev, idx, ysel, Hsel, Xg);
    if (int rc = check_launch("egcn_wide_fwd rows")) return rc;
    hipLaunchKernelGGL(egw_hoist_kernel, dim3((unsigned)T_run, 3), dim3(kEgwThreads), 0, st, P, Xg, (int)T_run, (int)F, (int)k,
                       pre);
    if (int rc = check_launch("egcn_wide_fwd hoist")) return rc;
  }
  const size_t lds = (size_t)(3 * egw_pad(F) * egw_pad(F) + 128) * sizeof(double);
  if (int rc = allow_large_lds(egw_chain_fwd_kernel, lds, "egcn_wide_fwd")) return rc;
  hipLaunchKernelGGL(egw_chain_fwd_kernel, dim3((unsigned)k), dim3(64), lds, st, P, W0, pre, (int)T_run, (int)F, (int)k, Wseq,
                     W32, gates);
  return check_launch("egcn_wide_fwd chain");
}

extern "C" int tmgcn_egcn_wide_bwd(const double* P, const double* Xg, const int32_t* idx, const double* ysel,
                                   const double* Hsel, const double* Wseq, const double* gates, const float* dW32,
                                   const double* dWseq, double* dP, double* dW0, float* dH, int64_t N, int32_t T_run,
                                   int32_t F, int32_t k, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = eg_check("egcn_wide_bwd", tmgcn_egcn_wide_supported(F, k), kEgwMax, kEgNarrowMax, N, T_run, F, k,
                        P && Wseq && dP && dW0, Xg && idx && ysel && Hsel && gates))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = eg_bwd_prepare("egcn_wide_bwd", workspace, workspace_bytes, tmgcn_egcn_wide_bwd_workspace_bytes(T_run, F, k), dH,
                              N, T_run, F, st))
    return rc;
  const int Fk = F * k;
  double* dA = static_cast<double*>(workspace);
  double* dy = dA + (int64_t)T_run * 4 * Fk;
  const size_t lds = (size_t)(3 * egw_pad(F) * egw_pad(F) + 192) * sizeof(double);
  if (int rc = allow_large_lds(egw_chain_bwd_kernel, lds, "egcn_wide_bwd")) return rc;
  hipLaunchKernelGGL(egw_chain_bwd_kernel, dim3((unsigned)k), dim3(64), lds, st, P, Wseq, gates, dW32, dWseq, (int)T_run, (int)F,
                     (int)k, dA, dW0);
  if (int rc = check_launch("egcn_wide_bwd chain")) return rc;
  if (T_run > 0) {
    hipLaunchKernelGGL(egw_dx_kernel, dim3((unsigned)((Fk + kEgwThreads - 1) / kEgwThreads), (unsigned)T_run), dim3(kEgwThreads), 0,
                       st, P, (int)F, (int)k, dA);
    if (int rc = check_launch("egcn_wide_bwd dX")) return rc;
    hipLaunchKernelGGL(egw_dy_kernel, dim3((unsigned)T_run), dim3(64), 0, st, Hsel, P, dA, idx, ysel, N, (int)F, (int)k, dy, dH);
    if (int rc = check_launch("egcn_wide_bwd dy")) return rc;
  }
  const unsigned tiles = (unsigned)((F + kEgwTile - 1) / kEgwTile);
  hipLaunchKernelGGL(egw_mat_grad_kernel, dim3(tiles, tiles, 6), dim3(kEgwThreads), 0, st, Xg, Wseq, gates, dA, (int)T_run, (int)F,
                     (int)k, dP);
  if (int rc = check_launch("egcn_wide_bwd matrices")) return rc;
  hipLaunchKernelGGL(egw_small_grad_kernel, dim3((unsigned)(F + (3 * Fk + 63) / 64)), dim3(64), 0, st, Hsel, P, dA, dy, idx, ysel,
                     (int)T_run, (int)F, (int)k, dP);
  return check_launch("egcn_wide_bwd sums");
}
