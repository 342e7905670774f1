// P2+P3 fused with the gathered operand STORED IN bf16 — Y = act((Â ⋆ X) · Wop), X as bf16 bit patterns   (gfx950 / CDNA4)
//
// The same contraction as spmm_gemm.hip (the pair  t.sparse.mm(At[k], Xt[k]) ; t.matmul(AtXt, W),
// embedding_help_functions.py:206-207 + 222, 303-304 + 349, 471-472 + 486-489, and with the transposed CSR and Wᵀ its
// backward pair).  That launch is bound by HBM traffic, and 512 of the 535.6 B it moves per stored non-zero at F = 128 are
// the gathered fp32 row of X: here the row is 2·K bytes instead of 4·K.
//   phase 1  (gather_row on PieceBf16, spmm_row.h; the tile's rows: fused_gather_tile, spmm_gemm_tile.h) a row of K bf16
//            values is K/8 sixteen-byte pieces: K/8 lanes cover a row, each with 8 fp32 accumulators; the other lanes of
//            the wave split the row's entries into streams.
//            Every gathered piece is widened to fp32 — exact: a bf16 is the upper half of an fp32 — and accumulated with
//            fmaf against the fp32 val, in entry order within a stream; the streams are combined by a fixed butterfly.
//            No atomics: the same bits from launch to launch.
//   phase 2  (spmm_gemm_tile.h) the fp32 row sums in the LDS tile [64][K+4] times the wave's
//            strip of W on v_mfma_f32_32x32x2_f32, activation epilogue.  AX and pre_act leave in fp32 (dW is formed from
//            them and keeps its accuracy); Y in fp32 or, rounded to nearest even ONCE from the post-activation fp32
//            value, in bf16.
// Gather, tile loop and product phase are the fp32 kernel's own code (one persistent loop, fused_tile_loop, under the policy
// FusedBf16); this file holds the argument struct, the kernel that names the policy, and the entry point.
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

template <int LPR, int U, int NJ, bool OFF32>  // NJ = K / 8
__global__ __launch_bounds__(256, TMGCN_FUSED_OCC) void spmm_gemm_bf16_kernel(FusedBf16Args a) {
  __shared__ __attribute__((aligned(16))) float As[FBM * FLDA];
  __shared__ Sum8 s_part[4 * LPR];        // partial sums of a long row, one per wave (spmm_row.h)
  __shared__ unsigned int s_tile, s_row;
  fused_tile_loop<FusedBf16, LPR, U, NJ, U, OFF32>(a, As, s_part, &s_tile, &s_row);
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
  const int bad = fused_check_args("spmm_gemm_bf16", grid_reserve, n_rows, N, K, Nf, tmgcn_spmm_gemm_bf16_supported(K, Nf),
                                   "(need K a multiple of 8 in [16,128] with Nf <= 128)", act, y_bf16, rows_per_batch);
  if (bad) return bad;
  TMGCN_REQUIRE(rowptr && X_bf16 && W && Y, "spmm_gemm_bf16: null pointer");
  TMGCN_REQUIRE(reinterpret_cast<uintptr_t>(X_bf16) % 16 == 0 && reinterpret_cast<uintptr_t>(Y) % 16 == 0 &&
                    (!AX || reinterpret_cast<uintptr_t>(AX) % 16 == 0),
                "spmm_gemm_bf16: X / AX / Y must be 16-byte aligned");
  TMGCN_REQUIRE(n_rows % N == 0, "spmm_gemm_bf16: n_rows=%lld is not a multiple of N=%d", (long long)n_rows, N);
  if (n_rows == 0) return TMGCN_OK;
  FusedBf16Args a{rowptr, col, val, reinterpret_cast<const uint4*>(X_bf16), n_rows, N, K, W, Nf, trans_w, rows_per_batch,
                  w_batch_stride, Y, y_bf16, AX, pre_act, act, TileMap{0, 0, 0, 0}, 0, nullptr};
  hipStream_t st = (hipStream_t)stream;
  const int no_tiles = fused_plan_tiles("spmm_gemm_bf16", a, st);
  if (no_tiles) return no_tiles;
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
