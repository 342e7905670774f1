// WD-GCN at widths beyond the lane-group kernels of wdgcn.hip: 1 <= F0 <= 64, 1 <= H <= 64 and not (F0 <= 8 and H <= 8).
// The same statements (wgf:70, 86-98; see wdgcn.hip), with the products on the exact-f32 matrix cores.
//
// Mapping.  Everything is computed TRANSPOSED: gatesᵀ [unit][node] = [W_g; U_g]ᵀ · [y | h]ᵀ on v_mfma_f32_16x16x4_f32,
// the weights as the A operand (output unit on lane & 15), the activations as the B operand (node on lane & 15).  The
// result tile then has the node on the lane and the units 4q .. 4q+3 (q = lane >> 4) in its four registers, and that
// is exactly a B operand of the next product when the k index inside a 16-unit tile is taken in the order
// k = 4q + s for k-step s: register s of a result tile IS the B fragment of k-step s.  So y_t feeds the gate product
// and h_t feeds step t + 1 with no lane movement, no LDS round trip and no barrier; the weights are staged once per
// block in LDS in that permuted order ([tile][gate][k-step][lane]: every fragment read is 64 consecutive dwords) and
// stay there for all steps.  Widths that are no multiple of 16 are zero-padded in that LDS image.
//
//   forward     a wave owns 16 nodes for the whole recurrence (a block 64), h and c of its nodes live in registers;
//               the AX rows of the next kWwPF steps are in flight in a register ring.  Per step and wave
//               NT·(4·nj) + 4·NT·8·NT MFMAs (NT = ⌈H/16⌉, nj = ⌈F0/16⌉): 512 + 64 at 64 x 64.  Writes Z and, when a
//               gradient is wanted, y, c and the four gate activations of every step (`saved`).
//   backward 1  the recurrence, t downwards, the same ownership: dz_g pointwise from the saved activations, then
//               dh_{t-1} = Σ_g U_g dz_g and dy_t = Σ_g W_g dz_g on the MFMA from a transposed LDS image of the weights;
//               stores dG = dz_f | dz_j | dz_c | dz_o and dy ⊙ relu' per step.
//   backward 2  the parameter gradients are products over the T_run·N rows: dW_g = Yᵀ dz_g, dU_g = H_{t-1}ᵀ dz_g,
//               db_g = Σ dz_g, dW = AXᵀ (dy ⊙ relu').  Block b takes a fixed run of rows, wave g the gate g (and the
//               16 features g of dW); the block's sums go to row b of a slab in the packed layout of P.
//   backward 3  the slab rows are added in row order in fp64.  No atomics: two runs give the same bits.
//
// What bounds it: the MFMA issue of the gate product (32 cycles each per SIMD) plus the pointwise part of the step (four
// sigmoids and a tanh per node and unit), which a wave runs after its products; at the chess shape there are fewer
// waves than SIMDs, so no other wave fills the gap.  At H = 64 the 128 KB weight image admits one block per CU.
// Measured: DESIGN.md §4 "WD-GCN, wide", profiles/wdgcn_wide_epoch.json.
#include "common.h"
#include "wdgcn_layout.h"   // wd_params, wd_sigmoid

namespace tmgcn {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWwMaxF = 64, kWwMaxH = 64;
constexpr int kWwNodes = 64;        // nodes of a block (16 per wave)
constexpr int kWwPF = 4;            // steps whose AX rows are in flight
constexpr int kWwMaxSlabs = 512;    // blocks (= slab rows) of the parameter-gradient kernel
constexpr int kWwSlabRows = 256;    // rows a parameter-gradient block takes at least

inline int ww_tiles(int H) { return (H + 15) / 16; }
inline int ww_slabs(int64_t R) {
  const int64_t b = (R + kWwSlabRows - 1) / kWwSlabRows;
  return (int)(b < kWwMaxSlabs ? b : kWwMaxSlabs);
}
inline size_t ww_fwd_lds(int F0, int H) {
  const int NT = ww_tiles(H), nj = (F0 + 15) / 16;
  return (size_t)((NT * 4 * 8 * NT + NT * 4 * nj) * 64 + 4 * 16 * NT) * sizeof(float);
}
inline size_t ww_bwd_lds(int NT) {
  return (size_t)(2 * NT * 4 * 4 * NT) * 64 * sizeof(float);
}

__device__ __forceinline__ f32x4 ww_mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// four consecutive units u0 .. u0+3 of one row ([..][H], p at the row's start); zero past H or when !ok
__device__ __forceinline__ f32x4 ww_load4(const float* __restrict__ p, int u0, int H, bool ok, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (ok && u0 < H) {
    if (vec) {
      v = *reinterpret_cast<const f32x4*>(p + u0);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (u0 + e < H) v[e] = p[u0 + e];
    }
  }
  return v;
}
__device__ __forceinline__ void ww_store4(float* __restrict__ p, int u0, int H, bool ok, bool vec, f32x4 v) {
  if (ok && u0 < H) {
    if (vec) {
      *reinterpret_cast<f32x4*>(p + u0) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (u0 + e < H) p[u0 + e] = v[e];
    }
  }
}

// the AX row of one node and step as B fragments: pre[4j + s] = AX[f = 16j + 4q + s]
__device__ __forceinline__ void ww_load_ax(const float* __restrict__ row, int F0, int nj, int q, bool ok, bool vec,
                                           float (&pre)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int f = 16 * j + 4 * q;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (j < nj) v = ww_load4(row, f, F0, ok, vec);
#pragma unroll
    for (int s = 0; s < 4; ++s) pre[4 * j + s] = v[s];
  }
}

// saved: y | c | f | j | ct | o, each [T_run][N][H]
constexpr int kWwSaved = 6;

template <int NT>
__global__ __launch_bounds__(256) void wdgcn_wide_fwd_kernel(const float* __restrict__ AX, const float* __restrict__ P,
                                                             const float* __restrict__ h0, const float* __restrict__ c0,
                                                             float* __restrict__ Z, float* __restrict__ saved, int64_t N,
                                                             int T_run, int F0, int H, int vec_ax, int vec_h) {
  extern __shared__ float ww_lds[];
  constexpr int KS = 8 * NT;                      // k-steps of a gate product: 4·NT over y, then 4·NT over h
  const int nj = (F0 + 15) / 16;
  float* Gs = ww_lds;                             // [NT][4][KS][64]: gate g, output tile mt
  float* Ws = Gs + NT * 4 * KS * 64;              // [NT][4·nj][64]
  float* Bs = Ws + NT * 4 * nj * 64;              // [4][16·NT]: the biases, zero past H
  // WdOff's offsets (wdgcn_layout.h), written out here and in the two kernels below: through the struct these kernels
  // compile to different code
  const int off_wg = F0 * H, off_ug = off_wg + 4 * H * H, off_b = off_ug + 4 * H * H;
  for (int i = threadIdx.x; i < NT * 4 * KS * 64; i += 256) {
    const int l = i & 63, ks = (i >> 6) % KS, g = ((i >> 6) / KS) & 3, mt = (i >> 6) / (KS * 4);
    const bool is_u = ks >= 4 * NT;
    const int kk = is_u ? ks - 4 * NT : ks;
    const int k = 16 * (kk >> 2) + 4 * (l >> 4) + (kk & 3), u = 16 * mt + (l & 15);
    Gs[i] = (k < H && u < H) ? P[(is_u ? off_ug : off_wg) + g * H * H + k * H + u] : 0.f;
  }
  for (int i = threadIdx.x; i < NT * 4 * nj * 64; i += 256) {
    const int l = i & 63, ks = (i >> 6) % (4 * nj), mt = (i >> 6) / (4 * nj);
    const int f = 16 * (ks >> 2) + 4 * (l >> 4) + (ks & 3), u = 16 * mt + (l & 15);
    Ws[i] = (f < F0 && u < H) ? P[f * H + u] : 0.f;
  }
  for (int i = threadIdx.x; i < 4 * 16 * NT; i += 256) {
    const int g = i / (16 * NT), u = i % (16 * NT);
    Bs[i] = u < H ? P[off_b + g * H + u] : 0.f;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int64_t n = (int64_t)blockIdx.x * kWwNodes + wave * 16 + r;
  const bool node_ok = n < N;
  const bool vax = vec_ax != 0, vh = vec_h != 0;

  f32x4 h[NT], c[NT];
#pragma unroll
  for (int mt = 0; mt < NT; ++mt) {
    const int u0 = 16 * mt + 4 * q;
    h[mt] = ww_load4(h0, u0, H, true, false);      // wgf:87-88 (the same start for every node)
    c[mt] = ww_load4(c0, u0, H, true, false);
  }

  const float* ax = AX + (node_ok ? n : 0) * F0;
  const int64_t stepA = N * F0, stepZ = N * H, plane = (int64_t)T_run * stepZ;
  float pre[kWwPF][16];
#pragma unroll
  for (int s = 0; s < kWwPF; ++s) ww_load_ax(ax + s * stepA, F0, nj, q, node_ok && s < T_run, vax, pre[s]);

  for (int t0 = 0; t0 < T_run; t0 += kWwPF) {
#pragma unroll
    for (int ps = 0; ps < kWwPF; ++ps) {
      const int t = t0 + ps;
      if (t >= T_run) break;                                       // uniform
      // y_t = relu(AX_t · W), transposed                            wgf:70
      f32x4 y[NT];
#pragma unroll
      for (int mt = 0; mt < NT; ++mt) y[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < nj) {                                                // uniform
          float a[4][NT];                                            // the fragments first, then the products: no
#pragma unroll                                                       // product waits for its own LDS read
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int mt = 0; mt < NT; ++mt) a[s][mt] = Ws[(mt * 4 * nj + 4 * j + s) * 64 + lane];
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int mt = 0; mt < NT; ++mt) y[mt] = ww_mfma(a[s][mt], pre[ps][4 * j + s], y[mt]);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      const int tn = t + kWwPF;
      ww_load_ax(ax + tn * stepA, F0, nj, q, node_ok && tn < T_run, vax, pre[ps]);
#pragma unroll
      for (int mt = 0; mt < NT; ++mt)
#pragma unroll
        for (int e = 0; e < 4; ++e) y[mt][e] = fmaxf(y[mt][e], 0.f);

      // the four gates' pre-activations: [W_g; U_g]ᵀ · [y | h]ᵀ + b_g      wgf:90-93
      f32x4 acc[4][NT];
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int mt = 0; mt < NT; ++mt) acc[g][mt] = *reinterpret_cast<const f32x4*>(Bs + g * 16 * NT + 16 * mt + 4 * q);
      // the 4·NT weight fragments of k-step ks + 1 are read while the products of k-step ks issue (the fences keep the
      // compiler from sinking every read next to its product, where each product would wait out the LDS latency)
      float af[2][4 * NT];
#pragma unroll
      for (int i = 0; i < 4 * NT; ++i) af[0][i] = Gs[(i * KS + 0) * 64 + lane];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if (ks + 1 < KS) {
#pragma unroll
          for (int i = 0; i < 4 * NT; ++i) af[(ks + 1) & 1][i] = Gs[(i * KS + ks + 1) * 64 + lane];
        }
        __builtin_amdgcn_sched_barrier(0);
        const int kk = ks < 4 * NT ? ks : ks - 4 * NT;
        const float b = ks < 4 * NT ? y[kk >> 2][kk & 3] : h[kk >> 2][kk & 3];
#pragma unroll
        for (int mt = 0; mt < NT; ++mt)
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g][mt] = ww_mfma(af[ks & 1][mt * 4 + g], b, acc[g][mt]);
        __builtin_amdgcn_sched_barrier(0);
      }

      const int64_t row = ((int64_t)t * N + (node_ok ? n : 0)) * H;
#pragma unroll
      for (int mt = 0; mt < NT; ++mt) {
        const int u0 = 16 * mt + 4 * q;
        f32x4 gf, gj, gc, go;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          gf[e] = wd_sigmoid(acc[0][mt][e]);
          gj[e] = wd_sigmoid(acc[1][mt][e]);
          gc[e] = wd_sigmoid(acc[2][mt][e]);
          go[e] = wd_sigmoid(acc[3][mt][e]);
          const float cn = gj[e] * gc[e] + gf[e] * c[mt][e];       // wgf:94
          c[mt][e] = cn;
          h[mt][e] = u0 + e < H ? go[e] * tanhf(cn) : 0.f;         // wgf:95; padding units stay zero
        }
        ww_store4(Z + row, u0, H, node_ok, vh, h[mt]);             // wgf:96
        if (saved) {
          ww_store4(saved + 0 * plane + row, u0, H, node_ok, vh, y[mt]);
          ww_store4(saved + 1 * plane + row, u0, H, node_ok, vh, c[mt]);
          ww_store4(saved + 2 * plane + row, u0, H, node_ok, vh, gf);
          ww_store4(saved + 3 * plane + row, u0, H, node_ok, vh, gj);
          ww_store4(saved + 4 * plane + row, u0, H, node_ok, vh, gc);
          ww_store4(saved + 5 * plane + row, u0, H, node_ok, vh, go);
        }
      }
    }
  }
}

// The recurrence of the backward.  dG [4][T_run·N][H], dYr [T_run·N][H].
template <int NT>
__global__ __launch_bounds__(256) void wdgcn_wide_bwd_kernel(const float* __restrict__ P, const float* __restrict__ c0,
                                                             const float* __restrict__ saved, const float* __restrict__ dZ,
                                                             float* __restrict__ dG, float* __restrict__ dYr, int64_t N,
                                                             int T_run, int F0, int H, int vec_h) {
  extern __shared__ float ww_lds[];
  constexpr int KS = 4 * NT;                      // k-steps over the units of one gate
  float* Ts = ww_lds;                             // [2: U, W][NT][4][KS][64]: M_g[k = 16mt + r][u = 16(ks>>2) + 4q + (ks&3)]
  const int off_wg = F0 * H, off_ug = off_wg + 4 * H * H;
  for (int i = threadIdx.x; i < 2 * NT * 4 * KS * 64; i += 256) {
    const int l = i & 63, ks = (i >> 6) % KS, g = ((i >> 6) / KS) & 3, mt = ((i >> 6) / (KS * 4)) % NT;
    const int wh = (i >> 6) / (KS * 4 * NT);
    const int k = 16 * mt + (l & 15), u = 16 * (ks >> 2) + 4 * (l >> 4) + (ks & 3);
    Ts[i] = (k < H && u < H) ? P[(wh ? off_wg : off_ug) + g * H * H + k * H + u] : 0.f;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int64_t n = (int64_t)blockIdx.x * kWwNodes + wave * 16 + r;
  const bool node_ok = n < N, vh = vec_h != 0;
  const int64_t stepZ = N * H, plane = (int64_t)T_run * stepZ;
  const int64_t noff = (node_ok ? n : 0) * H;
  const float *Ys = saved, *Cs = saved + plane, *Fs = saved + 2 * plane, *Js = saved + 3 * plane, *Ks = saved + 4 * plane,
              *Os = saved + 5 * plane;

  f32x4 ci[NT], ct_[NT], dh[NT], dc[NT];
#pragma unroll
  for (int mt = 0; mt < NT; ++mt) {
    const int u0 = 16 * mt + 4 * q;
    ci[mt] = ww_load4(c0, u0, H, node_ok, false);
    ct_[mt] = ww_load4(Cs + (int64_t)(T_run - 1) * stepZ + noff, u0, H, node_ok, vh);     // c_t of the step being walked
    dh[mt] = dc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // what a step reads: dZ_t, y_t, the gates of t, c_{t-1}
  f32x4 in[7][NT];
  auto load_step = [&](int t, f32x4 (&d)[7][NT], f32x4 (&yy)[NT]) {
    const int64_t row = (int64_t)t * stepZ + noff;
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) {
      const int u0 = 16 * mt + 4 * q;
      d[0][mt] = ww_load4(dZ + row, u0, H, node_ok, vh);
      yy[mt] = ww_load4(Ys + row, u0, H, node_ok, vh);
      d[2][mt] = ww_load4(Fs + row, u0, H, node_ok, vh);
      d[3][mt] = ww_load4(Js + row, u0, H, node_ok, vh);
      d[4][mt] = ww_load4(Ks + row, u0, H, node_ok, vh);
      d[5][mt] = ww_load4(Os + row, u0, H, node_ok, vh);
      d[6][mt] = t >= 1 ? ww_load4(Cs + row - stepZ, u0, H, node_ok, vh) : ci[mt];
    }
  };
  load_step(T_run - 1, in, in[1]);

  for (int t = T_run - 1; t >= 0; --t) {
    const int64_t row = (int64_t)t * stepZ + noff;
    f32x4 dzg[4][NT];
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) {
      const int u0 = 16 * mt + 4 * q;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float f = in[2][mt][e], j = in[3][mt][e], cc = in[4][mt][e], og = in[5][mt][e], cp = in[6][mt][e];
        const float tc = tanhf(ct_[mt][e]);
        // h = o·tanh(c), c = j·ct + f·c_{t-1}
        const float dht = in[0][mt][e] + dh[mt][e];
        const float dct = dc[mt][e] + (dht * og) * (1.f - tc * tc);
        dzg[0][mt][e] = (dct * cp) * ((1.f - f) * f);
        dzg[1][mt][e] = (dct * cc) * ((1.f - j) * j);
        dzg[2][mt][e] = (dct * j) * ((1.f - cc) * cc);
        dzg[3][mt][e] = (dht * tc) * ((1.f - og) * og);
        dc[mt][e] = dct * f;
        ct_[mt][e] = cp;
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) ww_store4(dG + g * plane + row, u0, H, node_ok, vh, dzg[g][mt]);
    }
    // the next step's inputs go into the registers this one has finished with: in flight under the products below
    f32x4 y_next[NT];
    if (t >= 1) load_step(t - 1, in, y_next);
    // dh_{t-1}[k] = Σ_g Σ_u U_g[k][u] dz_g[u],  dy_t[k] = Σ_g Σ_u W_g[k][u] dz_g[u]
    f32x4 dy[NT];
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) dh[mt] = dy[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // fragment reads one (gate, k-step) ahead of the products, as in the forward
    float af[2][2 * NT];
    auto frags = [&](int i, float (&a)[2 * NT]) {                   // i = g·KS + ks
#pragma unroll
      for (int m = 0; m < 2 * NT; ++m) a[m] = Ts[(m * 4 * KS + i) * 64 + lane];          // m = wh·NT + mt
    };
    frags(0, af[0]);
#pragma unroll
    for (int i = 0; i < 4 * KS; ++i) {
      if (i + 1 < 4 * KS) frags(i + 1, af[(i + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
      const int g = i / KS, ks = i % KS;
      const float b = dzg[g][ks >> 2][ks & 3];
#pragma unroll
      for (int mt = 0; mt < NT; ++mt) {
        dh[mt] = ww_mfma(af[i & 1][mt], b, dh[mt]);
        dy[mt] = ww_mfma(af[i & 1][NT + mt], b, dy[mt]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) {
#pragma unroll
      for (int e = 0; e < 4; ++e) dy[mt][e] = in[1][mt][e] > 0.f ? dy[mt][e] : 0.f;      // relu'
      ww_store4(dYr + row, 16 * mt + 4 * q, H, node_ok, vh, dy[mt]);
      if (t >= 1) in[1][mt] = y_next[mt];
    }
  }
}

// The parameter gradients of rows [lo, hi) of the T_run·N rows -> row blockIdx.x of the slab (packed like P).
// Wave g: dW_g, dU_g, db_g and the features 16g .. 16g+15 of dW.  A operand: the row's y / h_{t-1} / AX values
// (output row k on lane & 15), B operand: dz_g / dy⊙relu' (output column u on lane & 15), four rows per MFMA.
template <int NT>
__global__ __launch_bounds__(256) void wdgcn_wide_dparam_kernel(const float* __restrict__ AX, const float* __restrict__ h0,
                                                                const float* __restrict__ Z, const float* __restrict__ saved,
                                                                const float* __restrict__ dG, const float* __restrict__ dYr,
                                                                float* __restrict__ slab, int64_t N, int T_run, int F0,
                                                                int H) {
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int64_t R = (int64_t)T_run * N;
  const int64_t chunk = ((R + gridDim.x - 1) / gridDim.x + 3) / 4 * 4;
  const int64_t lo = blockIdx.x * chunk, hi = lo + chunk < R ? lo + chunk : R;
  const float* Ys = saved;
  const float* Gg = dG + g * R * H;
  const bool ax_wave = 16 * g < F0;
  const int fx = 16 * g + r;

  f32x4 aw[NT][NT], au[NT][NT], adw[NT];
  float db[NT];
#pragma unroll
  for (int mu = 0; mu < NT; ++mu) {
    adw[mu] = f32x4{0.f, 0.f, 0.f, 0.f};
    db[mu] = 0.f;
#pragma unroll
    for (int mk = 0; mk < NT; ++mk) aw[mk][mu] = au[mk][mu] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll 2
  for (int64_t r0 = lo; r0 < hi; r0 += 4) {
    const int64_t row = r0 + q;
    const bool ok = row < hi;
    const int64_t rr = ok ? row : lo;
    float bG[NT], bD[NT], aY[NT], aH[NT];
#pragma unroll
    for (int m = 0; m < NT; ++m) {
      const int u = 16 * m + r;
      const bool uo = ok && u < H;
      bG[m] = uo ? Gg[rr * H + u] : 0.f;
      aY[m] = uo ? Ys[rr * H + u] : 0.f;
      aH[m] = uo ? (rr < N ? h0[u] : Z[(rr - N) * H + u]) : 0.f;
      bD[m] = (uo && ax_wave) ? dYr[rr * H + u] : 0.f;
    }
    const float aX = (ok && ax_wave && fx < F0) ? AX[rr * F0 + fx] : 0.f;
#pragma unroll
    for (int mu = 0; mu < NT; ++mu) {
      db[mu] += bG[mu];
#pragma unroll
      for (int mk = 0; mk < NT; ++mk) {
        aw[mk][mu] = ww_mfma(aY[mk], bG[mu], aw[mk][mu]);
        au[mk][mu] = ww_mfma(aH[mk], bG[mu], au[mk][mu]);
      }
      if (ax_wave) adw[mu] = ww_mfma(aX, bD[mu], adw[mu]);
    }
  }

  float* out = slab + (int64_t)blockIdx.x * wd_params(F0, H);
  const int off_wg = F0 * H, off_ug = off_wg + 4 * H * H, off_b = off_ug + 4 * H * H;
#pragma unroll
  for (int mu = 0; mu < NT; ++mu) {
    const int u = 16 * mu + r;
    float s = db[mu];                                               // rows q = 0..3 of every step -> lane q = 0
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    if (u < H) {
      if (q == 0) out[off_b + g * H + u] = s;
#pragma unroll
      for (int mk = 0; mk < NT; ++mk)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = 16 * mk + 4 * q + e;
          if (k < H) {
            out[off_wg + g * H * H + k * H + u] = aw[mk][mu][e];
            out[off_ug + g * H * H + k * H + u] = au[mk][mu][e];
          }
        }
      if (ax_wave)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int f = 16 * g + 4 * q + e;
          if (f < F0) out[f * H + u] = adw[mu][e];
        }
    }
  }
}

// dP[j] = Σ_r slab[r][j] in row order (fp64), one thread per parameter, eight loads in flight
__global__ __launch_bounds__(256) void wdgcn_wide_slab_sum_kernel(const float* __restrict__ slab, float* __restrict__ dP,
                                                                  int rows, int np) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= np) return;
  double s = 0.0;
  for (int r0 = 0; r0 < rows; r0 += 8) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = r0 + i < rows ? slab[(int64_t)(r0 + i) * np + j] : 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += (double)v[i];
  }
  dP[j] = (float)s;
}

inline bool ww_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int NT>
int ww_fwd(const float* AX, const float* P, const float* h0, const float* c0, float* Z, float* saved, int64_t N, int T_run,
           int F0, int H, hipStream_t st) {
  const size_t lds = ww_fwd_lds(F0, H);
  int rc = allow_large_lds(wdgcn_wide_fwd_kernel<NT>, lds, "wdgcn_wide_fwd");
  if (rc) return rc;
  const int vec_ax = F0 % 4 == 0 && ww_aligned16(AX);
  const int vec_h = H % 4 == 0 && ww_aligned16(Z) && ww_aligned16(saved);
  const int64_t blocks = (N + kWwNodes - 1) / kWwNodes;
  hipLaunchKernelGGL(wdgcn_wide_fwd_kernel<NT>, dim3((unsigned)blocks), dim3(256), lds, st, AX, P, h0, c0, Z, saved, N, T_run,
                     F0, H, vec_ax, vec_h);
  return check_launch("wdgcn_wide_fwd");
}

template <int NT>
int ww_bwd(const float* AX, const float* P, const float* h0, const float* c0, const float* Z, const float* saved,
           const float* dZ, float* dP, int64_t N, int T_run, int F0, int H, float* ws, hipStream_t st) {
  // three unit tiles (H = 33..48) run the recurrence of four: with three the compiler spills registers to scratch, and
  // the padding tile only multiplies zeros
  constexpr int NB = NT == 3 ? 4 : NT;
  const size_t lds = ww_bwd_lds(NB);
  int rc = allow_large_lds(wdgcn_wide_bwd_kernel<NB>, lds, "wdgcn_wide_bwd");
  if (rc) return rc;
  const int64_t R = (int64_t)T_run * N;
  float* dG = ws;
  float* dYr = dG + 4 * R * H;
  float* slab = dYr + R * H;
  const int vec_h = H % 4 == 0 && ww_aligned16(saved) && ww_aligned16(dZ) && ww_aligned16(ws);
  const int64_t blocks = (N + kWwNodes - 1) / kWwNodes;
  hipLaunchKernelGGL(wdgcn_wide_bwd_kernel<NB>, dim3((unsigned)blocks), dim3(256), lds, st, P, c0, saved, dZ, dG, dYr, N, T_run,
                     F0, H, vec_h);
  rc = check_launch("wdgcn_wide_bwd");
  if (rc) return rc;
  const int rows = ww_slabs(R);
  hipLaunchKernelGGL(wdgcn_wide_dparam_kernel<NT>, dim3(rows), dim3(256), 0, st, AX, h0, Z, saved, dG, dYr, slab, N, T_run, F0,
                     H);
  rc = check_launch("wdgcn_wide_bwd parameter gradients");
  if (rc) return rc;
  const int np = (int)wd_params(F0, H);
  hipLaunchKernelGGL(wdgcn_wide_slab_sum_kernel, dim3((np + 255) / 256), dim3(256), 0, st, slab, dP, rows, np);
  return check_launch("wdgcn_wide_bwd slab sum");
}

// f(std::integral_constant<int, NT>) for the NT = ww_tiles(H) of 1..4 unit tiles: the kernels are instantiated per NT
template <typename F>
int ww_dispatch(int H, F f) {
  switch (ww_tiles(H)) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

}  // namespace
}  // namespace tmgcn

using namespace tmgcn;

extern "C" int tmgcn_wdgcn_wide_supported(int32_t F0, int32_t H) {
  return F0 >= 1 && F0 <= kWwMaxF && H >= 1 && H <= kWwMaxH && !tmgcn_wdgcn_supported(F0, H);
}

extern "C" int64_t tmgcn_wdgcn_wide_saved_bytes(int64_t N, int32_t T_run, int32_t F0, int32_t H) {
  if (!tmgcn_wdgcn_wide_supported(F0, H) || N < 0 || T_run < 0) return -1;
  return (int64_t)kWwSaved * T_run * N * H * (int64_t)sizeof(float);
}

extern "C" int64_t tmgcn_wdgcn_wide_bwd_workspace_bytes(int64_t N, int32_t T_run, int32_t F0, int32_t H) {
  if (!tmgcn_wdgcn_wide_supported(F0, H) || N < 0 || T_run < 0) return -1;
  const int64_t R = (int64_t)T_run * N;
  if (R == 0) return 0;
  return (5 * R * H + ww_slabs(R) * wd_params(F0, H)) * (int64_t)sizeof(float);
}

static int ww_check(const char* who, int64_t N, int32_t T_run, int32_t F0, int32_t H) {
  TMGCN_REQUIRE(tmgcn_wdgcn_wide_supported(F0, H), "%s: F0=%d, H=%d outside the wide kernels' widths (1..%d x 1..%d, "
                "beyond the narrow kernels' 1..8 x 1..8)", who, F0, H, kWwMaxF, kWwMaxH);
  TMGCN_REQUIRE(N >= 0 && T_run >= 0, "%s: negative size (N=%lld, T_run=%d)", who, (long long)N, T_run);
  TMGCN_REQUIRE(N < (int64_t)1 << 31 && (int64_t)T_run * N < (int64_t)1 << 48, "%s: N=%lld too large", who, (long long)N);
  return TMGCN_OK;
}

extern "C" int tmgcn_wdgcn_wide_fwd_f32(const float* AX, const float* P, const float* h0, const float* c0, float* Z,
                                        void* saved, int64_t N, int32_t T_run, int32_t F0, int32_t H, void* stream) {
  if (int rc = ww_check("wdgcn_wide_fwd", N, T_run, F0, H)) return rc;
  if (N == 0 || T_run == 0) return TMGCN_OK;
  TMGCN_REQUIRE(AX && P && h0 && c0 && Z, "wdgcn_wide_fwd: null pointer");
  hipStream_t st = (hipStream_t)stream;
  float* sv = static_cast<float*>(saved);
  return ww_dispatch(H, [&](auto nt) { return ww_fwd<decltype(nt)::value>(AX, P, h0, c0, Z, sv, N, T_run, F0, H, st); });
}

extern "C" int tmgcn_wdgcn_wide_bwd_f32(const float* AX, const float* P, const float* h0, const float* c0, const float* Z,
                                        const void* saved, const float* dZ, float* dP, int64_t N, int32_t T_run, int32_t F0,
                                        int32_t H, void* workspace, int64_t workspace_bytes, void* stream) {
  if (int rc = ww_check("wdgcn_wide_bwd", N, T_run, F0, H)) return rc;
  TMGCN_REQUIRE(dP, "wdgcn_wide_bwd: null dP");
  hipStream_t st = (hipStream_t)stream;
  if (N == 0 || T_run == 0) {                                      // nothing ran: every gradient is zero
    if (hipMemsetAsync(dP, 0, wd_params(F0, H) * sizeof(float), st) != hipSuccess) {
      set_error("wdgcn_wide_bwd: hipMemsetAsync failed");
      return TMGCN_ERR_LAUNCH;
    }
    return TMGCN_OK;
  }
  TMGCN_REQUIRE(AX && P && h0 && c0 && Z && dZ, "wdgcn_wide_bwd: null pointer");
  TMGCN_REQUIRE(saved, "wdgcn_wide_bwd: null saved (the forward must run with a saved buffer)");
  if (int rc = check_workspace("wdgcn_wide_bwd", workspace, workspace_bytes,
                               tmgcn_wdgcn_wide_bwd_workspace_bytes(N, T_run, F0, H)))
    return rc;
  const float* sv = static_cast<const float*>(saved);
  float* ws = static_cast<float*>(workspace);
  return ww_dispatch(H, [&](auto nt) {
    return ww_bwd<decltype(nt)::value>(AX, P, h0, c0, Z, sv, dZ, dP, N, T_run, F0, H, ws, st);
  });
}
