// EvolveGCN-H (TensorGCN-master/evolvegcn_functions.py, "ef"): the weight evolution of one layer over the T slices —
// the top-k summary of every slice and the matrix GRU that turns W_{t-1} into W_t — and its backpropagation.
//
//   summary   y = H_t·p/‖p‖, idx = topk(y, k), Zs = H_t[idx]·y[idx] (row j scaled by its score)         ef:80-84
//   chain     X = Zsᵀ [F,k], H = W_{t-1} [F,k]:                                                          ef:86-91
//               Z = σ(W_Z X + U_Z H + B_Z)  R = σ(W_R X + U_R H + B_R)  Ĥ = tanh(W_H X + U_H (R∘H) + B_H)
//               W_t = (1−Z)∘H + Z∘Ĥ
//   The GCONV (A_t·H_t)·W_t is not here: it is the batched per-slice GEMM / SpMM+GEMM of the other files.
//
// What is sequential: the summaries depend on the layer input H and on p only, so all T_run of them run in one launch
// (grid = blocks per slice x slices) and a second launch merges each slice's candidates.  Only the chain is a
// recurrence, on matrices of at most 8x8: one wave walks t = 0..T_run-1, one lane per entry (f, j) of W, everything in
// fp64 as in the reference.  Its inputs X_t do not depend on the chain: every lane keeps the loads of the next kEgPF
// steps in flight.  Per step the lanes exchange H and R∘H through LDS (two barriers of one wave).
//
// Top-k order: a higher score ranks first; equal scores rank by the lower node index; NaN is never selected (a slice
// with fewer than k numbers leaves idx = -1 and a zero column).  Every thread sorts its 8 nodes with a bitonic network
// and keeps them as its best kEgL = 8 (>= k); an LDS tree merges the lists two at a time (a half-cleaner and three
// network stages per merge); the merge launch merges the blocks' lists the same way.  The order is total, so the set
// and its order do not depend on the merge order: the result is the same on every run and for every block count.
//
// The backward: one wave walks t downwards carrying dW, adds the injected gradients of W_t (the GEMMs' per-slice dW and
// that of the returned fp64 W_seq) and writes the step's gate gradients (pre-activation) and dX_t.  A second launch,
// one wave per parameter entry, forms the parameter gradients — Σ_t of small outer products in a fixed order — and the
// summary's backward:
//   dy_j = dZs_j·H[idx_j],  dH[idx_j] = y_j·dZs_j + dy_j·p/‖p‖,  dp = Σ_t Σ_j dy_j·(H[idx_j]/‖p‖ − y_j·p/‖p‖²)
// with the fp64 rows H_sel the forward kept (it reads no H).
// No atomics: the indices of one slice are distinct and every sum has a fixed order, two runs give the same bits.
#include "common.h"
#include "egcn_layout.h"   // eg_params, EgOff, eg_better, eg_norm, eg_sigmoid; eg_check, eg_check_rows, eg_bwd_prepare

#include <math.h>

namespace tmgcn {
namespace {

constexpr int kEgMax = 8;            // F and k
constexpr int kEgL = 8;              // candidates a thread keeps (the top 8 hold the top k)
constexpr int kEgThreads = 256;
constexpr int kEgNodesPerThread = 8;
constexpr int kEgNodesPerBlock = kEgThreads * kEgNodesPerThread;
constexpr int kEgPF = 4;             // chain steps whose inputs are in flight ahead of the one being computed

inline int64_t eg_blocks(int64_t N) { return (N + kEgNodesPerBlock - 1) / kEgNodesPerBlock; }

// insert (cs, ci) into the descending list (s, ix): a fixed chain of compare-exchanges, static register indices only
__device__ __forceinline__ void eg_insert(double (&s)[kEgL], int (&ix)[kEgL], double cs, int ci) {
#pragma unroll
  for (int q = 0; q < kEgL; ++q) {
    const bool b = eg_better(cs, ci, s[q], ix[q]);
    const double ts = s[q];
    const int ti = ix[q];
    s[q] = b ? cs : ts;
    ix[q] = b ? ci : ti;
    cs = b ? ts : cs;
    ci = b ? ti : ci;
  }
}

__device__ __forceinline__ void eg_empty(double (&s)[kEgL], int (&ix)[kEgL]) {
#pragma unroll
  for (int q = 0; q < kEgL; ++q) {
    s[q] = -INFINITY;
    ix[q] = 0x7fffffff;              // ranks below every node, -inf scores included
  }
}

// compare-exchange: afterwards (sa, ia) ranks before (sb, ib)
__device__ __forceinline__ void eg_cx(double& sa, int& ia, double& sb, int& ib) {
  const bool sw = eg_better(sb, ib, sa, ia);
  const double ts = sa;
  const int ti = ia;
  sa = sw ? sb : sa;
  ia = sw ? ib : ia;
  sb = sw ? ts : sb;
  ib = sw ? ti : ib;
}

// 8 entries in any order -> descending: a bitonic sorting network (6 stages of 4 independent compare-exchanges)
__device__ __forceinline__ void eg_sort8(double (&s)[kEgL], int (&ix)[kEgL]) {
#pragma unroll
  for (int w = 2; w <= kEgL; w <<= 1)
#pragma unroll
    for (int d = w >> 1; d > 0; d >>= 1)
#pragma unroll
      for (int q = 0; q < kEgL; ++q) {
        const int l = q ^ d;
        if (l > q) {
          if ((q & w) == 0) eg_cx(s[q], ix[q], s[l], ix[l]);
          else eg_cx(s[l], ix[l], s[q], ix[q]);
        }
      }
}

// (s, ix) := the best 8 of two descending lists.  The better of s[q] and o[7-q] for every q is the best 8 as a bitonic
// sequence (the half-cleaner of a bitonic merge); three stages of 4 independent compare-exchanges sort it.
__device__ __forceinline__ void eg_merge(double (&s)[kEgL], int (&ix)[kEgL], const double (&os)[kEgL],
                                         const int (&oi)[kEgL]) {
#pragma unroll
  for (int q = 0; q < kEgL; ++q) {
    const bool b = eg_better(os[kEgL - 1 - q], oi[kEgL - 1 - q], s[q], ix[q]);
    s[q] = b ? os[kEgL - 1 - q] : s[q];
    ix[q] = b ? oi[kEgL - 1 - q] : ix[q];
  }
#pragma unroll
  for (int d = kEgL / 2; d > 0; d >>= 1)
#pragma unroll
    for (int q = 0; q < kEgL; ++q)
      if ((q & d) == 0) eg_cx(s[q], ix[q], s[q + d], ix[q + d]);
}

// the block's lists (each descending) -> thread 0's (and LDS slot 0): a tree over the threads, each level merging slot
// tid + w into tid
__device__ __forceinline__ void eg_block_merge(double (&s)[kEgL], int (&ix)[kEgL], double* ls, int* li) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < kEgL; ++q) {
    ls[q * kEgThreads + tid] = s[q];
    li[q * kEgThreads + tid] = ix[q];
  }
  __syncthreads();
  for (int w = kEgThreads / 2; w > 0; w >>= 1) {
    if (tid < w) {
      double os[kEgL];
      int oi[kEgL];
#pragma unroll
      for (int q = 0; q < kEgL; ++q) {
        os[q] = ls[q * kEgThreads + tid + w];
        oi[q] = li[q * kEgThreads + tid + w];
      }
      eg_merge(s, ix, os, oi);
#pragma unroll
      for (int q = 0; q < kEgL; ++q) {
        ls[q * kEgThreads + tid] = s[q];
        li[q * kEgThreads + tid] = ix[q];
      }
    }
    __syncthreads();
  }
}

// grid (blocks per slice, T_run): the best kEgL of the block's nodes -> cs / ci [T_run][nblk][kEgL]
__global__ __launch_bounds__(kEgThreads) void egcn_topk_kernel(const float* __restrict__ H, const double* __restrict__ P,
                                                               int64_t N, int F, double* __restrict__ cs,
                                                               int* __restrict__ ci) {
  __shared__ double ls[kEgL * kEgThreads];
  __shared__ int li[kEgL * kEgThreads];
  const int t = blockIdx.y, nblk = gridDim.x;
  double p[kEgMax];
#pragma unroll
  for (int f = 0; f < kEgMax; ++f) p[f] = f < F ? P[f] : 0.0;
  const double nrm = eg_norm(P, F);
  static_assert(kEgNodesPerThread == kEgL, "a thread sorts its nodes with the 8-entry network");
  double s[kEgL];
  int ix[kEgL];
  eg_empty(s, ix);
  const int64_t base = (int64_t)blockIdx.x * kEgNodesPerBlock + threadIdx.x;
#pragma unroll
  for (int r = 0; r < kEgNodesPerThread; ++r) {
    const int64_t n = base + (int64_t)r * kEgThreads;
    if (n < N) {
      const float* h = H + ((int64_t)t * N + n) * F;
      double d = 0.0;
#pragma unroll
      for (int f = 0; f < kEgMax; ++f)
        if (f < F) d = fma((double)h[f], p[f], d);
      const double y = d / nrm;                                  // ef:81
      if (!isnan(y)) {                                           // NaN keeps the slot's sentinel: never selected
        s[r] = y;
        ix[r] = (int)n;
      }
    }
  }
  eg_sort8(s, ix);
  eg_block_merge(s, ix, ls, li);
  if (threadIdx.x < kEgL) {
    const int64_t o = ((int64_t)t * nblk + blockIdx.x) * kEgL + threadIdx.x;
    cs[o] = ls[threadIdx.x * kEgThreads];
    ci[o] = li[threadIdx.x * kEgThreads];
  }
}

// one block per slice: merge the slice's nblk·kEgL candidates, write idx / y_sel [T_run][k], the selected rows
// H_sel [T_run][k][F] and X_g [T_run][F][k], all fp64.  With rowptr (layer 2: H = relu(Â_t·X_t·W_t) of the layer
// below, stored in fp32 for the GCONV) the selected rows are formed again in fp64 from Â (CSR), X_prev and the fp64
// W_prev[t+1] — the ranking stays the fp32 one, the values, scores and gradients get the reference's precision.
__global__ __launch_bounds__(kEgThreads) void egcn_select_kernel(
    const float* __restrict__ H, const double* __restrict__ P, const double* __restrict__ cs, const int* __restrict__ ci,
    int nblk, int64_t N, int F, int k, const int64_t* __restrict__ rowptr, const int* __restrict__ col,
    const float* __restrict__ val, const float* __restrict__ Xp, const double* __restrict__ Wp, int Fp,
    int* __restrict__ idx, double* __restrict__ ysel, double* __restrict__ Hsel, double* __restrict__ Xg) {
  __shared__ double ls[kEgL * kEgThreads];
  __shared__ int li[kEgL * kEgThreads];
  const int t = blockIdx.x;
  double s[kEgL];
  int ix[kEgL];
  eg_empty(s, ix);
  const int64_t nc = (int64_t)nblk * kEgL;
  const double* cst = cs + (int64_t)t * nc;
  const int* cit = ci + (int64_t)t * nc;
  for (int64_t c = threadIdx.x; c < nc; c += kEgThreads)
    if (cit[c] != 0x7fffffff) eg_insert(s, ix, cst[c], cit[c]);
  eg_block_merge(s, ix, ls, li);
  const int j = threadIdx.x;
  if (j < k) {
    const int n = li[j * kEgThreads];
    const bool ok = n != 0x7fffffff;
    double h[kEgMax];
#pragma unroll
    for (int f = 0; f < kEgMax; ++f) h[f] = 0.0;
    double y = 0.0;
    if (ok && rowptr) {
      // h = relu(Σ_e val_e·X_prev[col_e]·W_prev[t+1]) for any width F_prev (ef:168 in fp64); col / val are read only
      // for the row's entries
      double a[kEgMax];
#pragma unroll
      for (int f = 0; f < kEgMax; ++f) a[f] = 0.0;
      const double* w = Wp + (int64_t)(t + 1) * Fp * F;
      const int64_t r = (int64_t)t * N + n;
      for (int64_t e = rowptr[r]; e < rowptr[r + 1]; ++e) {
        const float* x = Xp + ((int64_t)t * N + col[e]) * Fp;
        const double v = (double)val[e];
        for (int q = 0; q < Fp; ++q) {
          const double xv = v * (double)x[q];
#pragma unroll
          for (int f = 0; f < kEgMax; ++f)
            if (f < F) a[f] = fma(xv, w[q * F + f], a[f]);
        }
      }
      double d = 0.0;
#pragma unroll
      for (int f = 0; f < kEgMax; ++f) {
        h[f] = (f < F && a[f] > 0.0) ? a[f] : 0.0;               // relu (ef:168)
        if (f < F) d = fma(h[f], P[f], d);
      }
      y = d / eg_norm(P, F);                                     // ef:185
    } else if (ok) {
#pragma unroll
      for (int f = 0; f < kEgMax; ++f)
        if (f < F) h[f] = (double)H[((int64_t)t * N + n) * F + f];
      y = ls[j * kEgThreads];
    }
    idx[(int64_t)t * k + j] = ok ? n : -1;
    ysel[(int64_t)t * k + j] = y;
#pragma unroll
    for (int f = 0; f < kEgMax; ++f)
      if (f < F) {
        Hsel[((int64_t)t * k + j) * F + f] = h[f];
        Xg[((int64_t)t * F + f) * k + j] = h[f] * y;             // ef:83
      }
  }
}

// one wave: W_seq[0] = W0, W_seq[t+1] = g(X_g[t], W_seq[t]) (ef:86-91); W32[t] = (float)W_seq[t+1]; gates (when
// not null) keep Z, R, Ĥ of every step for the backward
__global__ __launch_bounds__(64) void egcn_chain_fwd_kernel(const double* __restrict__ P, const double* __restrict__ W0,
                                                            const double* __restrict__ Xg, int T_run, int F, int k,
                                                            double* __restrict__ Wseq, float* __restrict__ W32,
                                                            double* __restrict__ gates) {
  __shared__ double hx[kEgMax * kEgMax], rx[kEgMax * kEgMax];   // [j][m]: column j of H, of R∘H
  const int lane = threadIdx.x, Fk = F * k;
  const bool act = lane < Fk;
  const int f = act ? lane / k : 0, j = act ? lane - f * k : 0;
  const EgOff o(F, k);
  double wz[kEgMax], uz[kEgMax], wr[kEgMax], ur[kEgMax], wh[kEgMax], uh[kEgMax];   // row f
#pragma unroll
  for (int m = 0; m < kEgMax; ++m) {
    const bool ok = act && m < F;
    wz[m] = ok ? P[o.W[0] + f * F + m] : 0.0;
    uz[m] = ok ? P[o.U[0] + f * F + m] : 0.0;
    wr[m] = ok ? P[o.W[1] + f * F + m] : 0.0;
    ur[m] = ok ? P[o.U[1] + f * F + m] : 0.0;
    wh[m] = ok ? P[o.W[2] + f * F + m] : 0.0;
    uh[m] = ok ? P[o.U[2] + f * F + m] : 0.0;
  }
  const double bz = act ? P[o.B[0] + f * k + j] : 0.0, br = act ? P[o.B[1] + f * k + j] : 0.0,
               bh = act ? P[o.B[2] + f * k + j] : 0.0;
  double h = act ? W0[lane] : 0.0;
  if (act) Wseq[lane] = h;

  double pre[kEgPF][kEgMax];                                     // X_g[t][m][j], m < F
#pragma unroll
  for (int s = 0; s < kEgPF; ++s)
#pragma unroll
    for (int m = 0; m < kEgMax; ++m) pre[s][m] = (act && m < F && s < T_run) ? Xg[((int64_t)s * F + m) * k + j] : 0.0;

  for (int t0 = 0; t0 < T_run; t0 += kEgPF) {
#pragma unroll
    for (int s = 0; s < kEgPF; ++s) {
      const int t = t0 + s;
      if (t >= T_run) break;                                     // uniform
      double x[kEgMax];
#pragma unroll
      for (int m = 0; m < kEgMax; ++m) x[m] = pre[s][m];
      const int tn = t + kEgPF;
#pragma unroll
      for (int m = 0; m < kEgMax; ++m)
        pre[s][m] = (act && m < F && tn < T_run) ? Xg[((int64_t)tn * F + m) * k + j] : 0.0;
      double ax = 0.0, ar = 0.0, ah = 0.0;                       // W_g·X: off the chain
#pragma unroll
      for (int m = 0; m < kEgMax; ++m) {
        ax = fma(wz[m], x[m], ax);
        ar = fma(wr[m], x[m], ar);
        ah = fma(wh[m], x[m], ah);
      }
      if (act) hx[j * kEgMax + f] = h;
      __syncthreads();
      double az = 0.0, arr = 0.0;
#pragma unroll
      for (int m = 0; m < kEgMax; ++m) {
        const double hm = m < F ? hx[j * kEgMax + m] : 0.0;
        az = fma(uz[m], hm, az);
        arr = fma(ur[m], hm, arr);
      }
      const double Z = eg_sigmoid((ax + az) + bz);               // ef:87
      const double R = eg_sigmoid((ar + arr) + br);              // ef:88
      if (act) rx[j * kEgMax + f] = R * h;
      __syncthreads();
      double ahh = 0.0;
#pragma unroll
      for (int m = 0; m < kEgMax; ++m) ahh = fma(uh[m], m < F ? rx[j * kEgMax + m] : 0.0, ahh);
      const double Ht = tanh((ah + ahh) + bh);                   // ef:89
      const double hn = (1.0 - Z) * h + Z * Ht;                  // ef:90
      if (act) {
        Wseq[(int64_t)(t + 1) * Fk + lane] = hn;
        W32[(int64_t)t * Fk + lane] = (float)hn;
        if (gates) {
          double* gt = gates + (int64_t)t * 3 * Fk + lane;
          gt[0] = Z;
          gt[Fk] = R;
          gt[2 * Fk] = Ht;
        }
      }
      h = hn;
    }
  }
}

// one wave, t = T_run-1..0: with G = dL/dW_t (carried + dW32[t] + dWseq[t+1]) the step's pre-activation gradients
// daz, dar, dah and dX_t -> dA [T_run][4][F·k]; dW0 = the carried gradient after t = 0 (+ dWseq[0])
__global__ __launch_bounds__(64) void egcn_chain_bwd_kernel(const double* __restrict__ P, const double* __restrict__ Wseq,
                                                            const double* __restrict__ gates,
                                                            const float* __restrict__ dW32,
                                                            const double* __restrict__ dWseq, int T_run, int F, int k,
                                                            double* __restrict__ dA, double* __restrict__ dW0) {
  __shared__ double e1[kEgMax * kEgMax], e2[kEgMax * kEgMax], e3[kEgMax * kEgMax];   // [j][m]: dah, daz, dar
  const int lane = threadIdx.x, Fk = F * k;
  const bool act = lane < Fk;
  const int f = act ? lane / k : 0, j = act ? lane - f * k : 0;
  const EgOff o(F, k);
  double cwz[kEgMax], cuz[kEgMax], cwr[kEgMax], cur[kEgMax], cwh[kEgMax], cuh[kEgMax];   // column f: M[m][f]
#pragma unroll
  for (int m = 0; m < kEgMax; ++m) {
    const bool ok = act && m < F;
    cwz[m] = ok ? P[o.W[0] + m * F + f] : 0.0;
    cuz[m] = ok ? P[o.U[0] + m * F + f] : 0.0;
    cwr[m] = ok ? P[o.W[1] + m * F + f] : 0.0;
    cur[m] = ok ? P[o.U[1] + m * F + f] : 0.0;
    cwh[m] = ok ? P[o.W[2] + m * F + f] : 0.0;
    cuh[m] = ok ? P[o.U[2] + m * F + f] : 0.0;
  }
  // the ring, for step t: W_{t} (the step's input), Z R Ĥ, and the injected gradient of the step's output
  double ph[kEgPF], pz[kEgPF], pr[kEgPF], pt[kEgPF], pg[kEgPF];
#pragma unroll
  for (int s = 0; s < kEgPF; ++s) {
    const int t = T_run - 1 - s;
    const bool ld = act && t >= 0;
    ph[s] = ld ? Wseq[(int64_t)t * Fk + lane] : 0.0;
    pz[s] = ld ? gates[(int64_t)t * 3 * Fk + lane] : 0.0;
    pr[s] = ld ? gates[(int64_t)t * 3 * Fk + Fk + lane] : 0.0;
    pt[s] = ld ? gates[(int64_t)t * 3 * Fk + 2 * Fk + lane] : 0.0;
    pg[s] = (ld && dW32 ? (double)dW32[(int64_t)t * Fk + lane] : 0.0) + (ld && dWseq ? dWseq[(int64_t)(t + 1) * Fk + lane] : 0.0);
  }
  double Gc = 0.0;
  for (int r0 = 0; r0 < T_run; r0 += kEgPF) {
#pragma unroll
    for (int s = 0; s < kEgPF; ++s) {
      const int t = T_run - 1 - (r0 + s);
      if (t < 0) break;                                          // uniform
      const double h = ph[s], Z = pz[s], R = pr[s], Ht = pt[s], G = Gc + pg[s];
      const int tn = t - kEgPF;
      const bool ld = act && tn >= 0;
      ph[s] = ld ? Wseq[(int64_t)tn * Fk + lane] : 0.0;
      pz[s] = ld ? gates[(int64_t)tn * 3 * Fk + lane] : 0.0;
      pr[s] = ld ? gates[(int64_t)tn * 3 * Fk + Fk + lane] : 0.0;
      pt[s] = ld ? gates[(int64_t)tn * 3 * Fk + 2 * Fk + lane] : 0.0;
      pg[s] = (ld && dW32 ? (double)dW32[(int64_t)tn * Fk + lane] : 0.0) +
              (ld && dWseq ? dWseq[(int64_t)(tn + 1) * Fk + lane] : 0.0);

      // W_t = (1−Z)∘H + Z∘Ĥ
      const double daz = (G * (Ht - h)) * (Z * (1.0 - Z));
      const double dah = (G * Z) * (1.0 - Ht * Ht);
      if (act) e1[j * kEgMax + f] = dah;
      __syncthreads();
      double a1[kEgMax];
#pragma unroll
      for (int m = 0; m < kEgMax; ++m) a1[m] = m < F ? e1[j * kEgMax + m] : 0.0;
      double dRH = 0.0;                                          // (U_Hᵀ dah)[f][j]
#pragma unroll
      for (int m = 0; m < kEgMax; ++m) dRH = fma(cuh[m], a1[m], dRH);
      const double dar = (dRH * h) * (R * (1.0 - R));
      if (act) {
        e2[j * kEgMax + f] = daz;
        e3[j * kEgMax + f] = dar;
      }
      __syncthreads();
      double dh = G * (1.0 - Z) + dRH * R, dx = 0.0;
#pragma unroll
      for (int m = 0; m < kEgMax; ++m) {
        const double z2 = m < F ? e2[j * kEgMax + m] : 0.0, r3 = m < F ? e3[j * kEgMax + m] : 0.0;
        dh = fma(cuz[m], z2, dh);
        dh = fma(cur[m], r3, dh);
        dx = fma(cwz[m], z2, dx);
        dx = fma(cwr[m], r3, dx);
        dx = fma(cwh[m], a1[m], dx);
      }
      if (act) {
        double* d = dA + (int64_t)t * 4 * Fk + lane;
        d[0] = daz;
        d[Fk] = dar;
        d[2 * Fk] = dah;
        d[3 * Fk] = dx;
      }
      Gc = dh;
    }
  }
  if (act) dW0[lane] = Gc + (dWseq ? dWseq[lane] : 0.0);
}

// one wave per parameter entry (blocks 0..np-1) and one for the summary's dH rows (block np): lane l takes the (t, j)
// pairs l, l + 64, ... in ascending order, a fixed xor tree sums the 64 partials — the same bits on every run.
// dy_j = dZs_j·H[idx_j] (dZs[j][m] = dX[m][j]) is formed again where it is needed.
__device__ __forceinline__ double eg_dy(const double* __restrict__ dA, const double* __restrict__ Hsel, int64_t t, int j,
                                        int F, int k) {
  const double* dX = dA + t * 4 * F * k + 3 * F * k;
  const double* h = Hsel + (t * k + j) * F;
  double d = 0.0;
  for (int m = 0; m < F; ++m) d = fma(dX[m * k + j], h[m], d);
  return d;
}

__global__ __launch_bounds__(64) void egcn_grad_kernel(
    const double* __restrict__ Hsel, const double* __restrict__ P, const double* __restrict__ Xg,
    const double* __restrict__ Wseq, const double* __restrict__ gates, const double* __restrict__ dA,
    const int* __restrict__ idx, const double* __restrict__ ysel, int64_t N, int T_run, int F, int k,
    double* __restrict__ dP, float* __restrict__ dH) {
  const int lane = threadIdx.x, Fk = F * k, e = blockIdx.x;
  const int np = (int)eg_params(F, k);
  const double nrm = eg_norm(P, F);
  const int64_t pairs = (int64_t)T_run * k;
  if (e == np) {                                                 // dH[idx_j] = y_j·dZs_j + dy_j·p/‖p‖
    if (!dH) return;
    for (int64_t q = lane; q < pairs; q += 64) {
      const int64_t t = q / k;
      const int j = (int)(q - t * k);
      const int n = idx[q];
      if (n < 0) continue;
      const double d = eg_dy(dA, Hsel, t, j, F, k), y = ysel[q];
      const double* dX = dA + t * 4 * Fk + 3 * Fk;
      float* g = dH + (t * N + n) * F;
      for (int m = 0; m < F; ++m) g[m] = (float)(y * dX[m * k + j] + d * (P[m] / nrm));
    }
    return;
  }
  const EgOff o(F, k);
  const int g = e < F ? -1 : (e - F) / (2 * F * F + F * k);
  const int r = g < 0 ? 0 : e - o.W[g];
  double s = 0.0;
  for (int64_t q = lane; q < pairs; q += 64) {
    const int64_t t = q / k;
    const int j = (int)(q - t * k);
    if (g < 0) {                                                 // dp
      if (idx[q] < 0) continue;
      const double y = ysel[q];
      s = fma(eg_dy(dA, Hsel, t, j, F, k), Hsel[q * F + e] / nrm - y * P[e] / (nrm * nrm), s);
    } else {
      const double* d = dA + t * 4 * Fk + g * Fk;
      if (r < F * F) {                                           // W_g[f][m] += d_g[f][j]·X[m][j]
        const int f = r / F, m = r - f * F;
        s = fma(d[f * k + j], Xg[t * Fk + m * k + j], s);
      } else if (r < 2 * F * F) {                                // U_g[f][m] += d_g[f][j]·In_g[m][j]
        const int f = (r - F * F) / F, m = (r - F * F) - f * F;
        const double w = Wseq[t * Fk + m * k + j];
        s = fma(d[f * k + j], g == 2 ? gates[t * 3 * Fk + Fk + m * k + j] * w : w, s);
      } else {                                                   // B_g[f][j] += d_g[f][j]
        const int fj = r - 2 * F * F;
        if (fj % k == j) s += d[fj];
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) dP[e] = s;
}

}  // namespace
}  // namespace tmgcn

using namespace tmgcn;

extern "C" int tmgcn_egcn_supported(int32_t F, int32_t k) { return F >= 1 && F <= kEgMax && k >= 1 && k <= kEgMax; }

extern "C" int64_t tmgcn_egcn_param_count(int32_t F, int32_t k) { return tmgcn_egcn_supported(F, k) ? eg_params(F, k) : -1; }

extern "C" int64_t tmgcn_egcn_fwd_workspace_bytes(int64_t N, int32_t T_run, int32_t F, int32_t k) {
  if (!tmgcn_egcn_supported(F, k) || N < 0 || T_run < 0) return -1;
  return (int64_t)T_run * eg_blocks(N) * kEgL * (int64_t)(sizeof(double) + sizeof(int));
}

extern "C" int64_t tmgcn_egcn_bwd_workspace_bytes(int32_t T_run, int32_t F, int32_t k) {
  if (!tmgcn_egcn_supported(F, k) || T_run < 0) return -1;
  return (int64_t)T_run * 4LL * F * k * (int64_t)sizeof(double);
}

extern "C" int tmgcn_egcn_fwd(const float* H, const double* P, const double* W0, const int64_t* rowptr,
                              const int32_t* col, const float* val, const float* X_prev, const double* W_prev,
                              int32_t F_prev, int32_t* idx, double* ysel, double* Hsel, double* Xg, double* Wseq,
                              float* W32, double* gates, int64_t N, int32_t T_run, int32_t F, int32_t k,
                              void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = eg_check("egcn_fwd", tmgcn_egcn_supported(F, k), kEgMax, 0, N, T_run, F, k, P && W0 && Wseq,
                        H && idx && ysel && Hsel && Xg && W32))
    return rc;
  if (int rc = eg_check_rows("egcn_fwd", rowptr, X_prev && W_prev, F_prev, N, T_run)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (T_run > 0) {
    if (int rc = check_workspace("egcn_fwd", workspace, workspace_bytes, tmgcn_egcn_fwd_workspace_bytes(N, T_run, F, k)))
      return rc;
    const int64_t nblk = eg_blocks(N);
    TMGCN_REQUIRE(nblk < (int64_t)1 << 31, "egcn_fwd: N=%lld too large", (long long)N);
    double* cs = static_cast<double*>(workspace);
    int* ci = reinterpret_cast<int*>(cs + (int64_t)T_run * nblk * kEgL);
    hipLaunchKernelGGL(egcn_topk_kernel, dim3((unsigned)nblk, (unsigned)T_run), dim3(kEgThreads), 0, st, H, P, N, F, cs, ci);
    if (int rc = check_launch("egcn_fwd topk")) return rc;
    hipLaunchKernelGGL(egcn_select_kernel, dim3((unsigned)T_run), dim3(kEgThreads), 0, st, H, P, cs, ci, (int)nblk, N, F, k,
                       rowptr, col, val, X_prev, W_prev, (int)F_prev, idx, ysel, Hsel, Xg);
    if (int rc = check_launch("egcn_fwd select")) return rc;
  }
  hipLaunchKernelGGL(egcn_chain_fwd_kernel, dim3(1), dim3(64), 0, st, P, W0, Xg, (int)T_run, (int)F, (int)k, Wseq, W32, gates);
  return check_launch("egcn_fwd chain");
}

extern "C" int tmgcn_egcn_bwd(const double* P, const double* Xg, const int32_t* idx, const double* ysel,
                              const double* Hsel, const double* Wseq, const double* gates, const float* dW32,
                              const double* dWseq, double* dP, double* dW0, float* dH, int64_t N, int32_t T_run,
                              int32_t F, int32_t k, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = eg_check("egcn_bwd", tmgcn_egcn_supported(F, k), kEgMax, 0, N, T_run, F, k, P && Wseq && dP && dW0,
                        Xg && idx && ysel && Hsel && gates))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = eg_bwd_prepare("egcn_bwd", workspace, workspace_bytes, tmgcn_egcn_bwd_workspace_bytes(T_run, F, k), dH, N,
                              T_run, F, st))
    return rc;
  double* dA = static_cast<double*>(workspace);
  hipLaunchKernelGGL(egcn_chain_bwd_kernel, dim3(1), dim3(64), 0, st, P, Wseq, gates, dW32, dWseq, (int)T_run, (int)F,
                     (int)k, dA, dW0);
  if (int rc = check_launch("egcn_bwd chain")) return rc;
  hipLaunchKernelGGL(egcn_grad_kernel, dim3((unsigned)eg_params(F, k) + 1), dim3(64), 0, st, Hsel, P, Xg, Wseq, gates, dA,
                     idx, ysel, N, (int)T_run, (int)F, (int)k, dP, dH);
  return check_launch("egcn_bwd grad");
}
