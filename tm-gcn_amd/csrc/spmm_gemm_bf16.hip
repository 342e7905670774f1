// P2+P3 fused with the gathered operand STORED IN bf16 — Y = act((Â ⋆ X) · Wop), X as bf16 bit patterns   (gfx950 / CDNA4)
//
// The same contraction as spmm_gemm.hip (the pair  t.sparse.mm(At[k], Xt[k]) ; t.matmul(AtXt, W),
// embedding_help_functions.py:206-207 + 222, 303-304 + 349, 471-472 + 486-489, and with the transposed CSR and Wᵀ its
// backward pair).  That launch is bound by HBM traffic, and 512 of the 535.6 B it moves per stored non-zero at F = 128 are
// the gathered fp32 row of X: here the row is 2·K bytes instead of 4·K.
//   phase 1  (this file) a row of K bf16 values is K/8 sixteen-byte pieces: K/8 lanes cover a row, each with 8 fp32
//            accumulators; the other lanes of the wave split the row's entries into streams (as gather_row, spmm_row.h).
//            Every gathered piece is widened to fp32 — exact: a bf16 is the upper half of an fp32 — and accumulated with
//            fmaf against the fp32 val, in entry order within a stream; the streams are combined by a fixed butterfly.
//            No atomics: the same bits from launch to launch.
//   phase 2  (spmm_gemm_tile.h, shared with the fp32 kernel) the fp32 row sums in the LDS tile [64][K+4] times the wave's
//            strip of W on v_mfma_f32_32x32x2_f32, activation epilogue.  AX and pre_act leave in fp32 (dW is formed from
//            them and keeps its accuracy); Y in fp32 or, rounded to nearest even ONCE from the post-activation fp32
//            value, in bf16.
// Rows of any length are summed correctly; of the fp32 kernel's schedule this one keeps
//   * the persistent grid, the device tile counter and grid_reserve,
//   * the heavy tiles first (HeavyScan) and the rows of a tile drawn by its four waves,
//   * rows of more than kLongRow entries on all four waves (partial sums added in wave order through LDS),
// and leaves out the entry-major walk of short tiles (every row takes the one-wave walk) and the giant-row plan (a row
// beyond TMGCN_GIANT_ROW is walked whole by the four waves).  Domain: K a multiple of 8 in [16, 128], Nf <= 128.
#include "common.h"
#include "spmm_row.h"
#include "spmm_gemm_tile.h"

namespace tmgcn {

struct FusedBf16Args {
  const int64_t* rowptr;
  const int32_t* col;
  const float* val;
  const uint4* X;   // [n_rows][K] bf16: K/8 pieces of 8 values per row
  int64_t n_rows;
  int32_t N;
  int32_t K;        // feature width of X (multiple of 8, 16 .. 128)
  const float* W;
  int32_t Nf;       // output width (<= 128)
  int32_t trans_w;
  int64_t rows_per_batch;  // 0: one shared W; N: one W per slice
  int64_t w_batch_stride;
  void* Y;          // fp32, or bf16 when y_bf16
  int32_t y_bf16;
  float* AX;        // optional: the SpMM result itself ([n_rows][K] fp32), for dW
  float* pre;       // optional: pre-activation (fp32)
  int32_t act;
  TileMap tiles;               // tiles restart at every slice (spmm_row.h)
  int64_t n_tiles;
  unsigned int* tile_counter;  // [0] tiles, [1] scan windows (spmm_row.h)
};

struct Sum8 {       // the 8 fp32 sums of a lane: columns 8·fl .. 8·fl + 7 of the row
  float4 lo, hi;
};
__device__ __forceinline__ Sum8 sum8_zero() { return Sum8{make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)}; }
__device__ __forceinline__ void sum8_add(Sum8& s, const Sum8& t) {
  s.lo.x += t.lo.x;  s.lo.y += t.lo.y;  s.lo.z += t.lo.z;  s.lo.w += t.lo.w;
  s.hi.x += t.hi.x;  s.hi.y += t.hi.y;  s.hi.z += t.hi.z;  s.hi.w += t.hi.w;
}
// acc += v · widen(x): dword d of the piece holds value 2d in its low half and 2d + 1 in its high half
__device__ __forceinline__ void sum8_fma(Sum8& s, float v, const uint4& x) {
  s.lo.x = fmaf(v, __uint_as_float(x.x << 16), s.lo.x);
  s.lo.y = fmaf(v, __uint_as_float(x.x & 0xffff0000u), s.lo.y);
  s.lo.z = fmaf(v, __uint_as_float(x.y << 16), s.lo.z);
  s.lo.w = fmaf(v, __uint_as_float(x.y & 0xffff0000u), s.lo.w);
  s.hi.x = fmaf(v, __uint_as_float(x.z << 16), s.hi.x);
  s.hi.y = fmaf(v, __uint_as_float(x.z & 0xffff0000u), s.hi.y);
  s.hi.z = fmaf(v, __uint_as_float(x.w << 16), s.hi.z);
  s.hi.w = fmaf(v, __uint_as_float(x.w & 0xffff0000u), s.hi.w);
}

// One wave sums one CSR row over [beg, end): gather_row (spmm_row.h) on 16-byte pieces of 8 bf16 values.  LPR lanes cover
// the F8 pieces of a feature row, S = 64/LPR streams split the entries, U gathers in flight per lane.  On return every
// lane of stream 0 holds the full sum of its piece (fixed butterfly order).
// OFF32: the slice of X is smaller than 4 GiB, so a piece's address is the slice's (scalar) base + a 32-bit byte offset —
// one address register per gather in flight instead of two, which at K >= 112, next to the 56-64 W fragments, is the
// difference between three gathers in flight and two (see the launcher).
template <int LPR, int U, bool OFF32>
__device__ __forceinline__ Sum8 gather_row_bf16(const int32_t* __restrict__ col, const float* __restrict__ val,
                                                const uint4* __restrict__ Xs, int64_t beg, int64_t end, int F8, int lane) {
  constexpr int S = kWave / LPR;
  const int sub = lane / LPR;
  const int fl = lane % LPR;
  const bool f_ok = fl < F8;
  Sum8 acc = sum8_zero();
  for (int64_t base = beg; base < end; base += kWave) {
    const int n = (int)((end - base) < kWave ? (end - base) : kWave);
    int c = 0;
    float v = 0.f;
    if (lane < n) {
      c = col[base + lane];
      v = val[base + lane];
    }
    for (int p = 0; p < n; p += S * U) {
      uint4 x[U];
      float vv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int idx = p + u * S + sub;
        const int cc = __shfl(c, idx & 63);
        vv[u] = __shfl(v, idx & 63);
        x[u] = make_uint4(0u, 0u, 0u, 0u);
        if (idx < n && f_ok) {
          if (OFF32) x[u] = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(Xs) + (uint32_t)(cc * F8 + fl) * 16u);
          else x[u] = Xs[(int64_t)cc * F8 + fl];
        }
        if (idx >= n) vv[u] = 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) sum8_fma(acc, vv[u], x[u]);
    }
  }
#pragma unroll
  for (int o = LPR; o < kWave; o <<= 1) {
    Sum8 t;
    t.lo.x = __shfl_xor(acc.lo.x, o);  t.lo.y = __shfl_xor(acc.lo.y, o);  t.lo.z = __shfl_xor(acc.lo.z, o);  t.lo.w = __shfl_xor(acc.lo.w, o);
    t.hi.x = __shfl_xor(acc.hi.x, o);  t.hi.y = __shfl_xor(acc.hi.y, o);  t.hi.z = __shfl_xor(acc.hi.z, o);  t.hi.w = __shfl_xor(acc.hi.w, o);
    sum8_add(acc, t);
  }
  return acc;
}

// A long row on four waves (as gather_long_row, spmm_row.h): wave w gathers quarter w — a multiple of 64 entries —, the
// partial sums meet in `part` ([4][LPR][2] float4 of LDS) and lanes < LPR of EVERY wave return ((p0 + p1) + p2) + p3.
// Called by all 256 threads; two block barriers.
template <int LPR, int U, bool OFF32>
__device__ __forceinline__ Sum8 gather_long_row_bf16(const int32_t* __restrict__ col, const float* __restrict__ val,
                                                     const uint4* __restrict__ Xs, int64_t beg, int64_t end, int F8, int lane,
                                                     int wave, float4* part) {
  const int64_t q = (((end - beg + 3) >> 2) + (kWave - 1)) & ~(int64_t)(kWave - 1);
  int64_t b = beg + wave * q, e = b + q;
  if (b > end) b = end;
  if (e > end) e = end;
  const Sum8 p = gather_row_bf16<LPR, U, OFF32>(col, val, Xs, b, e, F8, lane);
  if (lane < LPR) {
    part[(wave * LPR + lane) * 2] = p.lo;
    part[(wave * LPR + lane) * 2 + 1] = p.hi;
  }
  __syncthreads();
  Sum8 s = sum8_zero();
  if (lane < LPR) {
    s = Sum8{part[lane * 2], part[lane * 2 + 1]};
#pragma unroll
    for (int w = 1; w < 4; ++w) sum8_add(s, Sum8{part[(w * LPR + lane) * 2], part[(w * LPR + lane) * 2 + 1]});
  }
  __syncthreads();
  return s;
}

// Phase 1: the row sums of one tile into the LDS tile `As` ([64][FLDA] fp32) and, when asked for, to AX; all four waves.
// The rows are drawn by the four waves from an LDS counter (see fused_gather_tile, spmm_gemm.hip); long rows afterwards
// on all four waves.
template <int LPR, int U, bool OFF32>
__device__ __forceinline__ void fused_gather_tile_bf16(const FusedBf16Args& a, float* As, float4* s_part, const TileRows& rows,
                                                       int64_t row0, int64_t row_end, int lane, int wave, unsigned int* s_row) {
  const int F8 = a.K / 8;
  auto flush = [&](int rr, int64_t r, const Sum8& acc, bool to_ax) __attribute__((always_inline)) {
    float4* d = reinterpret_cast<float4*>(&As[rr * FLDA + 8 * lane]);
    d[0] = acc.lo;
    d[1] = acc.hi;
    if (to_ax) {
      float4* ax = &reinterpret_cast<float4*>(a.AX)[r * (2 * F8) + 2 * lane];
      store_f4(ax, acc.lo);
      store_f4(ax + 1, acc.hi);
    }
  };
  for (int rr = wave; rr < FBM;) {
    unsigned int nxt = 0;
    if (lane == 0) nxt = atomicAdd(s_row, 1u);
    const int64_t r = row0 + rr;
    const bool lng = (rows.long_mask >> rr) & 1;
    Sum8 acc = sum8_zero();
    if (r < row_end && !lng) {
      const int64_t slice = r / a.N;
      acc = gather_row_bf16<LPR, U, OFF32>(a.col, a.val, a.X + slice * (int64_t)a.N * F8, readlane64(rows.beg, rr), readlane64(rows.end, rr),
                                    F8, lane);
    }
    if (!lng && lane < LPR && lane < F8) flush(rr, r, acc, a.AX && r < row_end);   // (rows past the tile's last: zeros for the products)
    rr = (int)__builtin_amdgcn_readfirstlane(nxt);
  }
  for (uint64_t m = rows.long_mask; m; m &= m - 1) {
    const int rr = __builtin_ctzll(m);
    const int64_t r = row0 + rr;
    const int64_t slice = r / a.N;
    const Sum8 acc = gather_long_row_bf16<LPR, U, OFF32>(a.col, a.val, a.X + slice * (int64_t)a.N * F8, readlane64(rows.beg, rr),
                                                  readlane64(rows.end, rr), F8, lane, wave, s_part);
    if (wave == (rr & 3) && lane < LPR && lane < F8) flush(rr, r, acc, a.AX != nullptr);
  }
}

template <int LPR, int U, int NJ, bool OFF32>  // NJ = K / 8
__global__ __launch_bounds__(256, TMGCN_FUSED_OCC) void spmm_gemm_bf16_kernel(FusedBf16Args a) {
  __shared__ __attribute__((aligned(16))) float As[FBM * FLDA];
  __shared__ float4 s_part[4 * LPR * 2];  // partial sums of a long row, one per wave
  const int lane0 = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n0 = wave * 32;
  const TileMap tm = a.tiles;

  float wreg[NJ][4];
  int64_t cur_batch = -1;
  __shared__ unsigned int s_tile, s_row;
  if (threadIdx.x == 0) s_row = 4;        // (the first use is behind the barrier of the first tile draw)
  HeavyScan heavy;
  heavy.init(a.rowptr, tm);

  for (;;) {
    // the lane index is laundered once per tile and once more in front of the product phase, so that what either phase
    // derives from it is not held in registers across the other (see spmm_gemm_kernel)
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    // next tile: first the heavy tiles (windows drawn from counter[1]), then from the device counter (counter[0])
    int64_t tile = -1;
    if (heavy.scanning) tile = heavy.next(a.rowptr, tm, a.tile_counter + 1, &s_tile, lane);
    const bool scanning = heavy.scanning;
    if (!scanning) {
      if (threadIdx.x == 0) s_tile = atomicAdd(a.tile_counter, 1u);
      __syncthreads();
      tile = s_tile;
      if (tile >= a.n_tiles) break;
    }
    int64_t unit, row0, row_end;
    tile_extent(tm, tile, unit, row0, row_end);
    const int64_t batch = a.rows_per_batch ? row0 / a.rows_per_batch : 0;
    TileRows rows;
    rows.load(a.rowptr, row0, row_end, lane);
    if (!scanning && rows.entries > heavy.thr) {   // done in somebody's pass 1
      __syncthreads();                             // (s_tile is rewritten at the top)
      continue;
    }
    if (batch != cur_batch) {
      fused_load_w<NJ>(a, batch, n0, lane & 31, lane >> 5, wreg);
      cur_batch = batch;
    }
    fused_gather_tile_bf16<LPR, U, OFF32>(a, As, s_part, rows, row0, row_end, lane, wave, &s_row);
    __syncthreads();
    if (threadIdx.x == 0) s_row = 4;        // for the next tile's row draws (two barriers away)
    __builtin_amdgcn_s_setprio(TMGCN_FUSED_MFMA_PRIO);
    {
      int lane_p = lane0;
      asm volatile("" : "+v"(lane_p));
      fused_mfma_tile<NJ>(a, As, wreg, row0, row_end, n0, lane_p & 31, lane_p >> 5);
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();  // tile consumed before the next phase 1 overwrites it
  }
}

}  // namespace tmgcn

using namespace tmgcn;

extern "C" int tmgcn_spmm_gemm_bf16_supported(int32_t K, int32_t Nf) {
  return (K % 8 == 0 && K >= 16 && K <= FKC && Nf >= 1 && Nf <= 128) ? 1 : 0;
}

extern "C" int tmgcn_spmm_gemm_bf16(const int64_t* rowptr, const int32_t* col, const float* val, const uint16_t* X_bf16,
                                    int64_t n_rows, int32_t N, int32_t K, const float* W, int32_t Nf, int32_t trans_w,
                                    int64_t rows_per_batch, int64_t w_batch_stride, int32_t act, void* Y, int32_t y_bf16,
                                    float* AX, float* pre_act, int32_t grid_reserve, float avg_nnz_per_row, void* stream) {
  (void)avg_nnz_per_row;   // every row length takes the same walk (no low-degree variant): the hint steers nothing
  TMGCN_REQUIRE(grid_reserve >= 0 && grid_reserve <= 4096, "spmm_gemm_bf16: grid_reserve %d out of range [0, 4096]", grid_reserve);
  TMGCN_REQUIRE(n_rows >= 0 && N > 0, "spmm_gemm_bf16: bad shape n_rows=%lld N=%d", (long long)n_rows, N);
  TMGCN_REQUIRE(tmgcn_spmm_gemm_bf16_supported(K, Nf),
                "spmm_gemm_bf16: unsupported widths K=%d Nf=%d (need K a multiple of 8 in [16,128] with Nf <= 128)", K, Nf);
  TMGCN_REQUIRE(act >= TMGCN_ACT_NONE && act <= TMGCN_ACT_SELU, "spmm_gemm_bf16: unknown activation %d", act);
  TMGCN_REQUIRE(y_bf16 == 0 || y_bf16 == 1, "spmm_gemm_bf16: y_bf16=%d is neither 0 (fp32 Y) nor 1 (bf16 Y)", y_bf16);
  TMGCN_REQUIRE(rows_per_batch >= 0, "spmm_gemm_bf16: negative rows_per_batch");
  TMGCN_REQUIRE(rowptr && X_bf16 && W && Y, "spmm_gemm_bf16: null pointer");
  TMGCN_REQUIRE(reinterpret_cast<uintptr_t>(X_bf16) % 16 == 0 && reinterpret_cast<uintptr_t>(Y) % 16 == 0 &&
                    (!AX || reinterpret_cast<uintptr_t>(AX) % 16 == 0),
                "spmm_gemm_bf16: X / AX / Y must be 16-byte aligned");
  TMGCN_REQUIRE(n_rows % N == 0, "spmm_gemm_bf16: n_rows=%lld is not a multiple of N=%d", (long long)n_rows, N);
  if (n_rows == 0) return TMGCN_OK;
  FusedBf16Args a{rowptr, col, val, reinterpret_cast<const uint4*>(X_bf16), n_rows, N, K, W, Nf, trans_w, rows_per_batch,
                  w_batch_stride, Y, y_bf16, AX, pre_act, act, TileMap{0, 0, 0, 0}, 0, nullptr};
  // a unit of tiles = a slice, unless the caller's weight batches do not end on slice boundaries (no layer does that)
  a.tiles = make_tile_map(n_rows, (rows_per_batch == 0 || rows_per_batch % N == 0) ? (int64_t)N : rows_per_batch);
  a.n_tiles = a.tiles.n_tiles;
  TMGCN_REQUIRE(a.n_tiles < (int64_t)0x7fffffff, "spmm_gemm_bf16: too many row tiles");
  a.tile_counter = acquire_tile_counters((hipStream_t)stream, 2);      // [0] the main loop's tiles, [1] the heavy-tile scan windows
  TMGCN_REQUIRE(a.tile_counter, "spmm_gemm_bf16: no tile counter: %s", pool_error());
  hipStream_t st = (hipStream_t)stream;
  // persistent blocks, up to 4 per CU (LDS 34-35 KB each), tiles drawn in ascending order: as the fp32 launcher.
  // Gathers in flight per lane: as many as leave the W fragments in registers at 4 waves per SIMD (a spilled fragment is
  // re-read inside the MFMA chain).  Up to K = 104 that is the fp32 kernel's figure; from K = 112 on, three with 32-bit
  // piece offsets — a slice of X below 4 GiB — and two with 64-bit ones.
  const bool off32 = (int64_t)N * K * 2 <= (int64_t)0xffffffff;
#define TMGCN_FUSED_BF16_LAUNCH(KK, L, UU, O)                                                                 \
  {                                                                                                           \
    int64_t gx = persistent_grid_reserved(spmm_gemm_bf16_kernel<L, UU, KK / 8, O>, 256, grid_reserve);        \
    if (gx > a.n_tiles) gx = a.n_tiles;                                                                       \
    hipLaunchKernelGGL((spmm_gemm_bf16_kernel<L, UU, KK / 8, O>), dim3((unsigned)gx), dim3(256), 0, st, a);   \
  }
#define TMGCN_FUSED_BF16_CASE(KK, L, UU) \
  case KK: TMGCN_FUSED_BF16_LAUNCH(KK, L, UU, false) break;
#define TMGCN_FUSED_BF16_CASE_WIDE(KK)                   \
  case KK:                                               \
    if (off32) TMGCN_FUSED_BF16_LAUNCH(KK, 16, 3, true)  \
    else TMGCN_FUSED_BF16_LAUNCH(KK, 16, 2, false)       \
    break;
  switch (K) {  // every multiple of 8 in [16, 128]; lanes per feature row = next power of two >= K/8
    TMGCN_FUSED_BF16_CASE(16, 2, 2)
    TMGCN_FUSED_BF16_CASE(24, 4, 2)
    TMGCN_FUSED_BF16_CASE(32, 4, 2)
    TMGCN_FUSED_BF16_CASE(40, 8, TMGCN_FUSED_U)
    TMGCN_FUSED_BF16_CASE(48, 8, TMGCN_FUSED_U)
    TMGCN_FUSED_BF16_CASE(56, 8, TMGCN_FUSED_U)
    TMGCN_FUSED_BF16_CASE(64, 8, TMGCN_FUSED_U)
    TMGCN_FUSED_BF16_CASE(72, 16, TMGCN_FUSED_U)
    TMGCN_FUSED_BF16_CASE(80, 16, TMGCN_FUSED_U)
    TMGCN_FUSED_BF16_CASE(88, 16, TMGCN_FUSED_U)
    TMGCN_FUSED_BF16_CASE(96, 16, TMGCN_FUSED_U)
    TMGCN_FUSED_BF16_CASE(104, 16, TMGCN_FUSED_U)
    TMGCN_FUSED_BF16_CASE_WIDE(112)
    TMGCN_FUSED_BF16_CASE_WIDE(120)
    TMGCN_FUSED_BF16_CASE_WIDE(128)
  }
#undef TMGCN_FUSED_BF16_CASE_WIDE
#undef TMGCN_FUSED_BF16_LAUNCH
#undef TMGCN_FUSED_BF16_CASE
  return check_launch("spmm_gemm_bf16");
}
