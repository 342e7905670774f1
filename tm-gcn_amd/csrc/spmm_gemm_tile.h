// What the GEMM-fused SpMM tile kernels share (gfx950) — spmm_gemm.hip (fp32 X) and spmm_gemm_bf16.hip (bf16-stored X), which
// differ in the piece a lane gathers (spmm_row.h) and in the parts of the schedule they have, named by a policy:
//   * the product phase: the 64-row LDS tile of row sums times a wave's 32-column strip of Wop on the exact-f32 matrix
//     cores, and the activation epilogue;
//   * phase 1, the gather of one tile (fused_gather_tile), and the persistent loop around both (fused_tile_loop);
//   * the host side both entry points start with (fused_check_args, fused_plan_tiles).
// `Args` is the launch's argument struct (FusedArgs / FusedBf16Args); one whose Y is not a float* also carries `y_bf16` and
// has its Y stored as fp32 or, rounded to nearest even once from the post-activation fp32 value, as bf16.
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

// ---- phase 1 and the persistent loop, shared by spmm_gemm_kernel (fp32 X) and spmm_gemm_bf16_kernel (bf16-stored X) ----------
// A kernel names its gather with a small policy: the piece a lane gathers (spmm_row.h) and which parts of the fp32 kernel's
// schedule it has — the entry-major walk of short tiles, the giant-row plan (`Args::giant`).
struct FusedF32 {
  using Piece = PieceF32;
  static constexpr bool kShortTiles = true, kGiantPlan = true;
};
struct FusedBf16 {
  using Piece = PieceBf16;
  static constexpr bool kShortTiles = false, kGiantPlan = false;
};

// Development build only (-DTMGCN_FUSED_TRACE, tools/fused_trace.py): thread 0 of every block sums the 100 MHz wall-clock time
// it spends in each phase of its tiles — separately for short tiles (entry-major walk) and the others — and leaves the
// sums in the device array the kernel hands to fused_tile_loop (spmm_gemm.hip: read back through tmgcn_debug_fused_trace).
// Not part of the library.
#ifdef TMGCN_FUSED_TRACE
#define FT_NOW() wall_clock64()
#define FT_WAIT() asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory")
#define FT_STAMP(name) const unsigned long long name = FT_NOW()
#else
#define FT_STAMP(name) do { } while (0)
#define FT_WAIT() do { } while (0)
#endif

// Phase 1: the row sums of one tile into the LDS tile `As` ([64][FLDA] fp32) and, when asked for, to AX; all four waves.
// A tile of few entries entry-major, several rows per wave at once (spmm_row.h "Short tiles"; a policy without them: every
// row takes the one-wave walk); otherwise 16 rows per wave, long rows afterwards on all four waves.
template <class Pol, int LPR, int U, int US, bool OFF32, class Args>
__device__ __forceinline__ void fused_gather_tile(const Args& a, float* As, typename Pol::Piece::Sum* s_part, const TileRows& rows,
                                                  int64_t row0, int64_t row_end, int lane, int wave, unsigned int* s_row) {
  using P = typename Pol::Piece;
  using Sum = typename P::Sum;
  constexpr int Q = P::kFloats / 4;                // float4 per piece
  const int F = a.K / P::kFloats;                  // pieces per feature row
  // piece fl of the sum of tile row rr (row r of the launch)
  auto flush = [&](int rr, int64_t r, const Sum& acc, int fl, bool to_ax) __attribute__((always_inline)) {
    float4* d = reinterpret_cast<float4*>(&As[rr * FLDA + P::kFloats * fl]);
#pragma unroll
    for (int j = 0; j < Q; ++j) d[j] = P::quad(acc, j);
    if (to_ax) {
      float4* ax = &reinterpret_cast<float4*>(a.AX)[r * (Q * F) + Q * fl];
#pragma unroll
      for (int j = 0; j < Q; ++j) store_f4(ax + j, P::quad(acc, j));
    }
  };
  if constexpr (Pol::kShortTiles) {
    const int n_tile_rows = row_end - row0 < FBM ? (int)(row_end - row0) : FBM;
    const int64_t slice0 = row0 / a.N;
    const bool is_short = short_tile(rows, row0 + n_tile_rows <= (slice0 + 1) * a.N);
    if (is_short) {
      gather_short_tile<LPR, US>(a.col, a.val, a.X + slice0 * (int64_t)a.N * F, rows, n_tile_rows, F, lane, wave, F,
                                 [&](int rr, const float4& acc, int fl) {    // (float4 pieces only: spmm_row.h)
                                   if (fl < F) {
                                     *reinterpret_cast<float4*>(&As[rr * FLDA + 4 * fl]) = acc;
                                     if (a.AX) store_f4(&reinterpret_cast<float4*>(a.AX)[(row0 + rr) * F + fl], acc);
                                   }
                                 });
      return;
    }
  }
  // The rows of the tile are DRAWN by the four waves (an LDS counter, 4 at the start of a tile; the draw is issued in front of
  // the row it follows, so its latency hides under that row's gather): with a fixed deal — rows w, w + 4, … — the waves of a
  // skewed tile met 10.9 us apart at the barrier behind this loop (power-law graph, traced; equal rows: 1.5).  A row is summed
  // by whichever wave draws it, in the same order: the same bits.  Worth 0.3-0.5 % on the power-law graph (the launch is
  // bandwidth-bound: the CU's other blocks fill the wait), nothing on equal rows (profiles/r6/r6_35_*).
  for (int rr = wave; rr < FBM;) {
    unsigned int nxt = 0;
    if (lane == 0) nxt = atomicAdd(s_row, 1u);
    const int64_t r = row0 + rr;
    const bool lng = (rows.long_mask >> rr) & 1;
    Sum acc = P::zero();
    if (r < row_end && !lng) {
      const int64_t slice = r / a.N;
      acc = gather_row<LPR, U, P, OFF32>(a.col, a.val, a.X + slice * (int64_t)a.N * F, readlane64(rows.beg, rr),
                                         readlane64(rows.end, rr), F, lane);
    }
    if (!lng && lane < LPR && lane < F) flush(rr, r, acc, lane, a.AX && r < row_end);   // (rows past the tile's last: zeros for the products)
    rr = (int)__builtin_amdgcn_readfirstlane(nxt);
  }
  for (uint64_t m = rows.long_mask; m; m &= m - 1) {
    const int rr = __builtin_ctzll(m);
    const int64_t r = row0 + rr;
    const int64_t slice = r / a.N;
    const int64_t beg = readlane64(rows.beg, rr), end = readlane64(rows.end, rr);
    Sum acc;
    int gi = -1;
    if constexpr (Pol::kGiantPlan) gi = (a.giant.rows && end - beg > kGiantRow) ? giant_find(a.giant, r) : -1;   // uniform over the four waves
    if (gi >= 0) {
      if (wave != (rr & 3)) continue;
      if constexpr (Pol::kGiantPlan) acc = giant_row_sum(a.giant, gi, F, lane, 0, F);
    } else {
      acc = gather_long_row<LPR, U, P, OFF32>(a.col, a.val, a.X + slice * (int64_t)a.N * F, beg, end, F, lane, wave, s_part);
    }
    if (wave == (rr & 3) && lane < LPR && lane < F) flush(rr, r, acc, lane, a.AX != nullptr);
  }
}

// The persistent loop of a 256-thread block: draw a tile (the heavy ones first), gather it (phase 1), multiply it (phase 2).
// As: the LDS tile [FBM][FLDA]; s_part: [4 * LPR] partial sums of a long row, one per wave (spmm_row.h); s_tile, s_row: one
// LDS word each.  NJ = K / 8.  trace_words: TMGCN_FUSED_TRACE builds only.  The arguments come by value: hipcc then allocates
// the fp32 kernels' registers as it did with this loop written out in the kernel (by reference: 6-15 more spilled SGPRs).
template <class Pol, int LPR, int U, int NJ, int US, bool OFF32, class Args>
__device__ __forceinline__ void fused_tile_loop(const Args a, float* As, typename Pol::Piece::Sum* s_part, unsigned int* s_tile,
                                                unsigned int* s_row, unsigned long long* trace_words = nullptr) {
  const int lane0 = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n0 = wave * 32;
  const TileMap tm = a.tiles;

  float wreg[NJ][4];
  int64_t cur_batch = -1;
  if (threadIdx.x == 0) *s_row = 4;       // (the first use is behind the barrier of the first tile draw)
  HeavyScan heavy;
  heavy.init(a.rowptr, tm);

#ifdef TMGCN_FUSED_TRACE
  unsigned long long ft[16] = {0};        // [8·short + phase]: 0 draw, 1 row pointers, 2 gather (wave 0), 3 barrier, 4 products, 5 barrier, 6 tiles
#endif
  for (;;) {
    // The lane index is laundered through an empty asm once per tile and once more in front of the product phase: what the
    // two phases derive from it (feature lane, stream, LDS and output addresses) is then recomputed where it is used — a few
    // VALU instructions — instead of being hoisted out of this loop and held in registers across the OTHER phase, where the
    // 64 W fragments and the gather's loads in flight need them (round 6: two W fragments lived in scratch and were
    // re-read inside the MFMA chain, four exposed loads per tile).
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    FT_STAMP(ft_a);
    // next tile: first the heavy tiles (spmm_row.h: windows drawn from counter[1]), then from the device counter
    // (counter[0]; ascending, so resident blocks stay inside one slice)
    int64_t tile = -1;
    if (heavy.scanning) tile = heavy.next(a.rowptr, tm, a.tile_counter + 1, s_tile, lane);
    const bool scanning = heavy.scanning;
    if (!scanning) {
      if (threadIdx.x == 0) *s_tile = atomicAdd(a.tile_counter, 1u);
      __syncthreads();
      tile = *s_tile;
      if (tile >= a.n_tiles) break;
    }
    int64_t unit, row0, row_end;
    tile_extent(tm, tile, unit, row0, row_end);
    const int64_t batch = a.rows_per_batch ? row0 / a.rows_per_batch : 0;
    FT_STAMP(ft_b);
    TileRows rows;
    rows.load(a.rowptr, row0, row_end, lane);
    if (!scanning && rows.entries > heavy.thr) {   // done in somebody's pass 1
      __syncthreads();                             // (s_tile is rewritten at the top)
      continue;
    }
    FT_WAIT();
    FT_STAMP(ft_c);
    if (batch != cur_batch) {
      fused_load_w<NJ>(a, batch, n0, lane & 31, lane >> 5, wreg);
      cur_batch = batch;
    }
    fused_gather_tile<Pol, LPR, U, US, OFF32>(a, As, s_part, rows, row0, row_end, lane, wave, s_row);
    FT_WAIT();
    FT_STAMP(ft_d);
    __syncthreads();
    if (threadIdx.x == 0) *s_row = 4;       // for the next tile's row draws (two barriers away)
    FT_STAMP(ft_e);
    // the product phase at raised issue priority: its waves hold the block's LDS tile and share the SIMD with three other
    // blocks' waves that are waiting for gathered rows anyway (round 6: -4.5 % on the chess operand at bench size, -6 % at
    // 4 random entries per row, S4 unchanged; profiles/r6/r6_08_*)
    __builtin_amdgcn_s_setprio(TMGCN_FUSED_MFMA_PRIO);
    {
      int lane_p = lane0;
      asm volatile("" : "+v"(lane_p));
      fused_mfma_tile<NJ>(a, As, wreg, row0, row_end, n0, lane_p & 31, lane_p >> 5);
    }
    __builtin_amdgcn_s_setprio(0);
    FT_STAMP(ft_f);
    __syncthreads();  // tile consumed before the next phase 1 overwrites it
#ifdef TMGCN_FUSED_TRACE
    {
      const int n_tile_rows = row_end - row0 < FBM ? (int)(row_end - row0) : FBM;
      const int k = Pol::kShortTiles && short_tile(rows, row0 + n_tile_rows <= (row0 / a.N + 1) * a.N) ? 8 : 0;
      const unsigned long long ft_g = FT_NOW();
      ft[k + 0] += ft_b - ft_a;
      ft[k + 1] += ft_c - ft_b;
      ft[k + 2] += ft_d - ft_c;
      ft[k + 3] += ft_e - ft_d;
      ft[k + 4] += ft_f - ft_e;
      ft[k + 5] += ft_g - ft_f;
      ft[k + 6] += 1;
    }
#endif
  }
#ifdef TMGCN_FUSED_TRACE
  if (trace_words && threadIdx.x == 0 && blockIdx.x < 4096)
    for (int i = 0; i < 16; ++i) trace_words[blockIdx.x * 16 + i] = ft[i];
#endif
}

// ---- host: what the entry points of the two kernels share ---------------------------------------------------------------------
// The argument checks both make first, in their order.  `widths_ok` / `widths_need`: the entry point's own domain and the
// tail of its message; y_bf16: 0 for an entry point whose Y is always fp32.
inline int fused_check_args(const char* who, int32_t grid_reserve, int64_t n_rows, int32_t N, int32_t K, int32_t Nf, bool widths_ok,
                            const char* widths_need, int32_t act, int32_t y_bf16, int64_t rows_per_batch) {
  TMGCN_REQUIRE(grid_reserve >= 0 && grid_reserve <= 4096, "%s: grid_reserve %d out of range [0, 4096]", who, grid_reserve);
  TMGCN_REQUIRE(n_rows >= 0 && N > 0, "%s: bad shape n_rows=%lld N=%d", who, (long long)n_rows, N);
  TMGCN_REQUIRE(widths_ok, "%s: unsupported widths K=%d Nf=%d %s", who, K, Nf, widths_need);
  TMGCN_REQUIRE(act >= TMGCN_ACT_NONE && act <= TMGCN_ACT_SELU, "%s: unknown activation %d", who, act);
  TMGCN_REQUIRE(y_bf16 == 0 || y_bf16 == 1, "%s: y_bf16=%d is neither 0 (fp32 Y) nor 1 (bf16 Y)", who, y_bf16);
  TMGCN_REQUIRE(rows_per_batch >= 0, "%s: negative rows_per_batch", who);
  return TMGCN_OK;
}

// The launch's tiles and its two device counters ([0] the main loop's tiles, [1] the heavy-tile scan windows).
template <class Args>
inline int fused_plan_tiles(const char* who, Args& a, hipStream_t st) {
  // a unit of tiles = a slice, unless the caller's weight batches do not end on slice boundaries (no layer does that)
  a.tiles = make_tile_map(a.n_rows, (a.rows_per_batch == 0 || a.rows_per_batch % a.N == 0) ? (int64_t)a.N : a.rows_per_batch);
  a.n_tiles = a.tiles.n_tiles;
  TMGCN_REQUIRE(a.n_tiles < (int64_t)0x7fffffff, "%s: too many row tiles", who);
  a.tile_counter = acquire_tile_counters(st, 2);
  TMGCN_REQUIRE(a.tile_counter, "%s: no tile counter: %s", who, pool_error());
  return TMGCN_OK;
}

}  // namespace tmgcn
