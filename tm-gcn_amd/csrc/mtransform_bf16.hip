// P1 on bf16-stored activations — the band M-transform with X and / or Y stored in bf16   (gfx950 / CDNA4)
//
// EmbeddingGCN2(act_dtype=torch.bfloat16) gathers the M-transform of the layer-1 output in bf16
// (embedding_help_functions.py:204, 308, 346 in front of the sparse.mm loop), and autograd's Mᵀ product receives that
// gather's gradient in bf16.  With the fp32 kernel either side costs a cast launch more: 4 + 4 B per element for the
// transform and 4 + 2 B for the cast, 14 B, where the operand itself is 6 B (read fp32 / write bf16 forward, read bf16 /
// write fp32 backward).  These kernels are the fp32 band kernel (mtransform_band.h: the same register ring, LDS tap
// table and three phases; one read of X, one write of Y) with the cast folded into the load or the store:
//   X bf16   widened as it is loaded (exact: a bf16 is the upper half of an fp32); the window holds fp32, so the widening
//            costs one VALU operation per element LOADED, not one per tap
//   Y bf16   the fp32 accumulator rounded to nearest even once as it is stored (the rounding of the cast launch)
// Every output element is the fp32 kernel's value — the same taps in the same order through fmaf — so each form equals
// the composition it replaces bit for bit: round_bf16(mtransform(widen(X))).  No atomics; the same bits on every run.
//
// A lane owns four columns, as in the fp32 kernel: the register ring of the 20-row window is then the fp32 kernel's
// (no spill), an fp32 side moves 16 B per lane and a bf16 side 8 B — a wave's lanes cover 1 024 / 512 consecutive bytes.
// The scalar form (one column per lane) takes a C that is no multiple of 4 and bases that are not 16-byte (fp32) /
// 8-byte (bf16) aligned.  Operators wider than 20 diagonals (Minv, dense M) have no kernel here: they keep the fp32
// kernels of mtransform.hip and the casts.  Not carried over from the fp32 entry: group-interleaved rows and the
// column-window form (only the sharded layer uses them, and it exchanges fp32 activations).
#include "common.h"
#include "mtransform_band.h"

namespace tmgcn {

template <int WIDTH, int PF, int VEC, class XT, class YT>
__global__ __launch_bounds__(256) void mtransform_band_bf16_kernel(MtArgsT<XT, YT> a) {
  extern __shared__ float coef[];  // [n_out][WIDTH] taps of this chunk, zero outside the band
  band_kernel_body<WIDTH, PF, VEC, false>(a, coef);
}

template <int VEC, class XT, class YT>
static void launch_cols(const MtArgsT<XT, YT>& a, hipStream_t st) {
  launch_band_width<VEC>(a, [st](auto w, dim3 grid, const MtArgsT<XT, YT>& b) {
    constexpr int WIDTH = decltype(w)::value;
    const size_t smem = (size_t)b.rows_per_chunk * WIDTH * sizeof(float);
    hipLaunchKernelGGL((mtransform_band_bf16_kernel<WIDTH, kBandPrefetch, VEC, XT, YT>), grid, dim3(256), smem, st, b);
  });
}

template <class XT, class YT>
static int launch_bf16(const MtArgsT<XT, YT>& a, hipStream_t st) {
  // four columns per lane: C a multiple of 4 and each base aligned to four of its elements
  const bool vec = (a.C % 4 == 0) && (reinterpret_cast<uintptr_t>(a.X) % (4 * sizeof(XT)) == 0) &&
                   (reinterpret_cast<uintptr_t>(a.Y) % (4 * sizeof(YT)) == 0);
  if (vec)
    launch_cols<4>(a, st);
  else
    launch_cols<1>(a, st);
  return check_launch("mtransform_band_bf16");
}

}  // namespace tmgcn

using namespace tmgcn;

extern "C" int tmgcn_mtransform_bf16_supported(int32_t band_lo, int32_t band_hi) {
  return band_lo >= 0 && band_hi >= 0 && (int64_t)band_lo + band_hi + 1 <= kBandMaxWidth;
}

extern "C" int tmgcn_mtransform_bf16(const float* M, int32_t Tm, int32_t ldm, int32_t transpose, int32_t row_off,
                                      int32_t col_off, int32_t T_out, int32_t T_in, int32_t band_lo, int32_t band_hi,
                                      const void* X, int32_t x_bf16, void* Y, int32_t y_bf16, int64_t C, void* stream) {
  TMGCN_REQUIRE(Tm > 0 && ldm >= Tm, "mtransform_bf16: bad operator shape Tm=%d ldm=%d", Tm, ldm);
  TMGCN_REQUIRE(T_out >= 0 && T_in >= 0 && C >= 0, "mtransform_bf16: negative extent");
  TMGCN_REQUIRE(row_off >= 0 && col_off >= 0 && row_off + T_out <= Tm && col_off + T_in <= Tm,
                "mtransform_bf16: window [%d+%d) x [%d+%d) exceeds the %dx%d operator", row_off, T_out, col_off, T_in, Tm, Tm);
  TMGCN_REQUIRE(band_lo >= 0 && band_hi >= 0, "mtransform_bf16: negative band");
  TMGCN_REQUIRE((x_bf16 == 0 || x_bf16 == 1) && (y_bf16 == 0 || y_bf16 == 1), "mtransform_bf16: x_bf16=%d, y_bf16=%d must be 0 or 1",
                x_bf16, y_bf16);
  TMGCN_REQUIRE(x_bf16 || y_bf16, "mtransform_bf16: X and Y are both fp32: that is tmgcn_mtransform_f32");
  TMGCN_REQUIRE(tmgcn_mtransform_bf16_supported(band_lo, band_hi),
                "mtransform_bf16: a band of %lld diagonals (band_lo=%d, band_hi=%d) is outside the band kernel (at most %d): use "
                "tmgcn_mtransform_f32 and the casts",
                (long long)band_lo + band_hi + 1, band_lo, band_hi, kBandMaxWidth);
  if (T_out == 0 || C == 0) return TMGCN_OK;
  TMGCN_REQUIRE(M && X && Y, "mtransform_bf16: null pointer");
  TMGCN_REQUIRE(X != Y, "mtransform_bf16: in-place transform is not supported");
  TMGCN_REQUIRE(T_in > 0, "mtransform_bf16: X has no rows");
  TMGCN_REQUIRE(reinterpret_cast<uintptr_t>(X) % (x_bf16 ? 2 : 4) == 0, "mtransform_bf16: X is not %d-byte aligned", x_bf16 ? 2 : 4);
  TMGCN_REQUIRE(reinterpret_cast<uintptr_t>(Y) % (y_bf16 ? 2 : 4) == 0, "mtransform_bf16: Y is not %d-byte aligned", y_bf16 ? 2 : 4);
  const hipStream_t st = (hipStream_t)stream;
  if (!x_bf16)
    return launch_bf16(MtArgsT<float, bf16_t>{M, ldm, transpose, row_off, col_off, T_out, T_in, band_lo, band_hi, (const float*)X,
                                               (bf16_t*)Y, C, T_out, 0, 0, nullptr, C, C}, st);
  if (!y_bf16)
    return launch_bf16(MtArgsT<bf16_t, float>{M, ldm, transpose, row_off, col_off, T_out, T_in, band_lo, band_hi, (const bf16_t*)X,
                                               (float*)Y, C, T_out, 0, 0, nullptr, C, C}, st);
  return launch_bf16(MtArgsT<bf16_t, bf16_t>{M, ldm, transpose, row_off, col_off, T_out, T_in, band_lo, band_hi, (const bf16_t*)X,
                                              (bf16_t*)Y, C, T_out, 0, 0, nullptr, C, C}, st);
}
