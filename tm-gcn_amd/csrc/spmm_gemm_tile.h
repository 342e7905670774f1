// The product phase of the GEMM-fused SpMM kernels (gfx950): the 64-row LDS tile of row sums times a wave's 32-column strip
// of Wop on the exact-f32 matrix cores, and the activation epilogue.  Shared by spmm_gemm.hip (fp32 X) and
// spmm_gemm_bf16.hip (bf16-stored X): the two differ in phase 1, the gather, only.  `Args` is the launch's argument
// struct (W, K, Nf, trans_w, rows_per_batch, w_batch_stride, Y, pre, act); one whose Y is not a float* also carries
// `y_bf16` and has its Y stored as fp32 or, rounded to nearest even once from the post-activation fp32 value, as bf16.
#pragma once
#include "common.h"
#include "spmm_row.h"

namespace tmgcn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// Numeric tunables: each feeds a template argument or a constant and guards no alternative code.  The defaults are the
// measured best; tools/ab_variants.sh builds other values.  (The alternatives that were measured and rejected are patches
// under profiles/r6/not_kept/, not switches in this file.)
#ifndef TMGCN_FUSED_OCC
#define TMGCN_FUSED_OCC 4   // min waves per SIMD asked of the register allocator (A/B: 4 beats 3 by 4.5 %)
#endif
#ifndef TMGCN_FUSED_U
#define TMGCN_FUSED_U 4     // gathers in flight per lane (F = 64 / 128 variants)
#endif
#ifndef TMGCN_FUSED_MFMA_PRIO
#define TMGCN_FUSED_MFMA_PRIO 3  // issue priority of the product phase (both kernels)
#endif

constexpr int FBM = 64;         // rows per tile
constexpr int FKC = 128;        // max K (feature width of X)
constexpr int FLDA = FKC + 4;   // LDS row stride in floats

// one element of Y: fp32 as it is, bf16 rounded to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ void store_y(float* p, float v) { store_f1(p, v); }
__device__ __forceinline__ void store_y(uint16_t* p, float v) {
  __builtin_nontemporal_store(__builtin_bit_cast(uint16_t, (__bf16)v), p);
}

// W fragments of a wave's 32-column strip (n0 .. n0+31): B operand of v_mfma_f32_32x32x2_f32, k = 8j + s + 4·lh
template <int NJ, class Args>
__device__ __forceinline__ void fused_load_w(const Args& a, int64_t batch, int n0, int li, int lh, float (&wreg)[NJ][4]) {
  const float* Wb = a.W + (a.rows_per_batch ? batch * a.w_batch_stride : 0);
  const int n = n0 + li;
  const int nc = n < a.Nf ? n : 0;  // clamp: out-of-range columns load column 0, zeroed below
  const float* Wl = a.trans_w ? Wb + (int64_t)nc * a.K + 4 * lh : Wb + (int64_t)(4 * lh) * a.Nf + nc;
  const int64_t sk = a.trans_w ? 1 : a.Nf;  // stride of k
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float w = Wl[(int64_t)(8 * j + s) * sk];
      wreg[j][s] = n < a.Nf ? w : 0.f;
    }
}

// The 16 accumulators of a lane after a 32-row half: accumulator i is row k(i) + 4·lh of the half, k(i) = (i & 3) + 8·(i >> 2).
template <bool GUARD, bool PRE, bool ACT, class YT>
__device__ __forceinline__ void fused_store_half(const f32x16& acc, const ActApply& act, YT* __restrict__ Yb, float* __restrict__ Pb,
                                                 int Nf, int lane_off, int rows_left) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int k = (i & 3) + 8 * (i >> 2);
    const float s = acc[i];
    if (GUARD && k >= rows_left) continue;
    if (PRE) store_f1(&Pb[k * Nf + lane_off], s);
    store_y(&Yb[k * Nf + lane_off], ACT ? act(s) : s);
  }
}
template <bool GUARD, class YT>
__device__ __forceinline__ void fused_store_half(const f32x16& acc, int act_id, YT* __restrict__ Yb, float* __restrict__ Pb, int Nf,
                                                 int lane_off, int rows_left) {
  const ActApply act(act_id);             // decoded once (the same bits as act_apply); no activation: the raw sums, no select chain
  if (act_id == TMGCN_ACT_NONE) {
    if (Pb) fused_store_half<GUARD, true, false>(acc, act, Yb, Pb, Nf, lane_off, rows_left);
    else fused_store_half<GUARD, false, false>(acc, act, Yb, Pb, Nf, lane_off, rows_left);
  } else {
    if (Pb) fused_store_half<GUARD, true, true>(acc, act, Yb, Pb, Nf, lane_off, rows_left);
    else fused_store_half<GUARD, false, true>(acc, act, Yb, Pb, Nf, lane_off, rows_left);
  }
}
// Phase 2: tile · Wop on the matrix cores, the wave's 32 output columns [n0, n0 + 32).
// One 32-row half of the tile at a time: its 16 accumulators are stored before the other half's products
// start, so only ONE accumulator set is live next to the 64 W-fragment registers (both halves live — the
// round 1-3 form — cost 15 spilled VGPRs at 4 waves per SIMD; profiles/archive/r4*_ab_fused_spill.txt).
// A fragments are fetched one k-group ahead of the MFMAs that use them; the sched_barrier keeps hipcc
// from hoisting all the ds_read_b128 to the top.
template <int NJ, class Args>
__device__ __forceinline__ void fused_mfma_tile(const Args& a, const float* As, const float (&wreg)[NJ][4], int64_t row0,
                                                int64_t row_end, int n0, int li, int lh) {
  if (n0 >= a.Nf) return;
  const float* Arow = &As[li * FLDA + 4 * lh];
  const int n = n0 + li;
#pragma unroll
  for (int mb = 0; mb < FBM / 32; ++mb) {
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    float4 av_next = *reinterpret_cast<const float4*>(Arow + mb * 32 * FLDA);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const float4 av = av_next;
      if (j + 1 < NJ) av_next = *reinterpret_cast<const float4*>(Arow + mb * 32 * FLDA + 8 * (j + 1));
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, wreg[j][0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, wreg[j][1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, wreg[j][2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, wreg[j][3], acc, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (n < a.Nf) {
      // Epilogue: accumulator i of the lane is row rbase + k(i) + 4·lh, column n.  Everything but (4·lh)·Nf + n is uniform: the
      // stores take a scalar base + a 32-bit lane offset, the activation is decoded once (ActApply: the same bits as
      // act_apply; none at all for TMGCN_ACT_NONE), and a half tile that lies inside the slice skips the row guard.  (Round 6:
      // a 64-bit address, a row compare and an activation switch per ELEMENT had made the epilogues a third of the product
      // phase: 6.7 us per tile on an otherwise idle CU where the MFMAs need 3.6.)
      const int64_t rbase = row0 + mb * 32;
      if constexpr (std::is_same<decltype(a.Y), float*>::value) {
        float* __restrict__ Yb = a.Y + rbase * a.Nf;
        float* __restrict__ Pb = a.pre ? a.pre + rbase * a.Nf : nullptr;
        const int lane_off = (4 * lh) * a.Nf + n;
        if (rbase + 32 <= row_end) fused_store_half<false>(acc, a.act, Yb, Pb, a.Nf, lane_off, 32);      // uniform: inside the slice
        else fused_store_half<true>(acc, a.act, Yb, Pb, a.Nf, lane_off, (int)(row_end - rbase) - 4 * lh);  // rows k < rows_left exist
      } else {                                             // Y fp32 or bf16 by the launch's flag (uniform)
        float* __restrict__ Pb = a.pre ? a.pre + rbase * a.Nf : nullptr;
        const int lane_off = (4 * lh) * a.Nf + n;
        const int rows_left = rbase + 32 <= row_end ? 32 : (int)(row_end - rbase) - 4 * lh;
        if (a.y_bf16) fused_store_half<true>(acc, a.act, static_cast<uint16_t*>(a.Y) + rbase * a.Nf, Pb, a.Nf, lane_off, rows_left);
        else fused_store_half<true>(acc, a.act, static_cast<float*>(a.Y) + rbase * a.Nf, Pb, a.Nf, lane_off, rows_left);
      }
    }
  }
}

}  // namespace tmgcn
