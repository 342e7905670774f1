// What the band M-transform kernels share (gfx950) — mtransform.hip (fp32 X and Y) and mtransform_bf16.hip (X and / or Y
// stored in bf16), which differ only in how a lane's columns are loaded and stored:
//   * the launch's argument struct MtArgsT<XT, YT> (MtArgs = the fp32 one), row_pos and mop;
//   * Cols<VEC>, a lane's VEC columns as fp32 registers, and ColIo<E, VEC>, their storage form E in memory
//     (float: as they are; bf16_t: bf16 bit patterns, widened on load — exact — and rounded to nearest even once on store,
//     bf16_rne_bits of common.h);
//   * the sliding-window body (BandBody, band_kernel_body) and the launcher that picks the window width and the row chunks
//     (launch_band_width).
// The arithmetic of an output element is the same for every storage form: the same taps in the same order through fmaf on
// fp32 registers.  A bf16 output is that fp32 value rounded once, so the bf16 forms are bit for bit the fp32 kernel
// between the two casts they replace.
#pragma once
#include <type_traits>
#include "common.h"

namespace tmgcn {

template <class XT, class YT>
struct MtArgsT {
  const float* M;
  int32_t ldm;
  int32_t transpose;
  int32_t row_off, col_off;
  int32_t T_out, T_in;
  int32_t band_lo, band_hi;
  const XT* X;
  YT* Y;
  int64_t C;  // columns (elements)
  int32_t rows_per_chunk;
  int32_t x_tl, y_tl;  // group-interleaved row storage (0 = plain row order), see tmgcn.h
  unsigned int* tile_counter;  // dense MFMA kernel: dynamic column-tile scheduling (common.h)
  int64_t ldx, ldy;            // row strides of X and Y in elements (>= C): a column window of a wider tensor
};
using MtArgs = MtArgsT<float, float>;

// storage position of logical row k of a tensor with T rows stored in groups of tl rows:
// (k % tl) * (T / tl) + k / tl — the send/receive layout of the slice<->node all-to-all.
__device__ __forceinline__ int64_t row_pos(int k, int T, int tl) {
  return tl ? (int64_t)(k % tl) * (T / tl) + k / tl : k;
}

template <class Args>
__device__ __forceinline__ float mop(const Args& a, int k, int j) {
  const int64_t r = a.row_off + k, c = a.col_off + j;
  return a.transpose ? a.M[c * a.ldm + r] : a.M[r * a.ldm + c];
}

// VEC-wide column access helpers (VEC = 4: float4, VEC = 1: scalar tail / unaligned)
template <int VEC>
struct Cols;
template <>
struct Cols<4> {
  using T = float4;
  static __device__ __forceinline__ T zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ T load(const float* p) {
    return *reinterpret_cast<const float4*>(p);
  }
  static __device__ __forceinline__ void store(float* p, const T& v) {
    *reinterpret_cast<float4*>(p) = v;
  }
  static __device__ __forceinline__ void fma(T& acc, float m, const T& x) {
    acc.x = fmaf(m, x.x, acc.x);
    acc.y = fmaf(m, x.y, acc.y);
    acc.z = fmaf(m, x.z, acc.z);
    acc.w = fmaf(m, x.w, acc.w);
  }
  static __device__ __forceinline__ void mask(T& v, unsigned bits) {
    v.x = __uint_as_float(__float_as_uint(v.x) & bits);
    v.y = __uint_as_float(__float_as_uint(v.y) & bits);
    v.z = __uint_as_float(__float_as_uint(v.z) & bits);
    v.w = __uint_as_float(__float_as_uint(v.w) & bits);
  }
};
template <>
struct Cols<1> {
  using T = float;
  static __device__ __forceinline__ T zero() { return 0.f; }
  static __device__ __forceinline__ T load(const float* p) { return *p; }
  static __device__ __forceinline__ void store(float* p, const T& v) { *p = v; }
  static __device__ __forceinline__ void fma(T& acc, float m, const T& x) { acc = fmaf(m, x, acc); }
  static __device__ __forceinline__ void mask(T& v, unsigned bits) {
    v = __uint_as_float(__float_as_uint(v) & bits);
  }
};

// A lane's VEC columns in memory, stored as E.  float: Cols<VEC>'s own accesses.  bf16_t: VEC = 4 is one 8-byte access
// (the lanes of a wave cover 512 consecutive bytes), VEC = 1 a 2-byte one; the window and the accumulator stay fp32.
template <class E, int VEC>
struct ColIo;
template <int VEC>
struct ColIo<float, VEC> {
  using V = typename Cols<VEC>::T;
  static __device__ __forceinline__ V load(const float* p) { return Cols<VEC>::load(p); }
  static __device__ __forceinline__ void store(float* p, const V& v) { Cols<VEC>::store(p, v); }
};
template <>
struct ColIo<bf16_t, 4> {
  static __device__ __forceinline__ float4 load(const bf16_t* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float4& v) {
    *reinterpret_cast<uint2*>(p) =
        make_uint2(bf16_rne_bits(v.x) | (bf16_rne_bits(v.y) << 16), bf16_rne_bits(v.z) | (bf16_rne_bits(v.w) << 16));
  }
};
template <>
struct ColIo<bf16_t, 1> {
  static __device__ __forceinline__ float load(const bf16_t* p) { return __uint_as_float((unsigned)*p << 16); }
  static __device__ __forceinline__ void store(bf16_t* p, const float& v) { *p = (bf16_t)bf16_rne_bits(v); }
};

// Sliding-window band kernel.  Each lane owns VEC columns and keeps a ring of W = WIDTH + PF
// input rows in registers: WIDTH rows feed the current output row while the next PF rows are
// already in flight, so X is read once, Y written once, and every lane keeps PF vector loads
// outstanding.  Rows are numbered locally, u = 0.. (u = 0 is the oldest row the chunk's first
// output needs); row u lives in ring slot u mod W.  Three phases keep the steady state free of
// control flow (conditional loads would force s_waitcnt vmcnt(0) and serialise the stream):
//   fill    rows 0..WIDTH-2 and the first PF look-ahead rows: loads only, fully unrolled
//   steady  groups of W output rows, fully unrolled, unconditional loads (row index clamped
//           into the tensor, out-of-range rows selected to zero), one store per row
//   tail    the last < W rows, same body under wave-uniform branches
template <int WIDTH, int PF, int VEC, bool PERM, class XT, class YT>
struct BandBody {
  static constexpr int W = WIDTH + PF;
  using CT = Cols<VEC>;
  using V = typename CT::T;
  using Args = MtArgsT<XT, YT>;

  // input row of local index u
  static __device__ __forceinline__ V fetch(const Args& a, const XT* __restrict__ X, int q0,
                                            int u, int u_max, int64_t c) {
    const int uc = u < u_max ? u : u_max;  // never run past the rows this chunk needs
    const int q = q0 + uc;
    const int qc = q < 0 ? 0 : (q >= a.T_in ? a.T_in - 1 : q);
    const int64_t pos = PERM ? row_pos(qc, a.T_in, a.x_tl) : (int64_t)qc;
    V v = ColIo<XT, VEC>::load(X + pos * a.ldx + c);
    CT::mask(v, q == qc ? 0xFFFFFFFFu : 0u);  // rows outside the tensor are zero (bit mask: no branch)
    return v;
  }

  // output row o of the chunk, completed by the row in ring slot i; taps from the LDS table
  static __device__ __forceinline__ void emit(const Args& a, YT* __restrict__ Y, const V (&win)[W],
                                              const float* coef, int i, int o, int k, int64_t c, bool live) {
    V acc = CT::zero();
    float m[WIDTH];
#pragma unroll
    for (int d = 0; d < WIDTH; ++d) m[d] = coef[o * WIDTH + d];  // wave-uniform: LDS broadcast
#pragma unroll
    for (int d = 0; d < WIDTH; ++d) CT::fma(acc, m[d], win[(i - d + 2 * W) % W]);
    const int64_t pos = PERM ? row_pos(k, a.T_out, a.y_tl) : (int64_t)k;
    if (live) ColIo<YT, VEC>::store(Y + pos * a.ldy + c, acc);
  }
};

constexpr int kBandMaxChunkRows = 512;  // LDS tap table: 512 x 20 x 4 B = 40 KB

// The whole kernel, for a block of 256 threads; `coef` is the block's dynamic LDS: [n_out][WIDTH] taps of this chunk.
template <int WIDTH, int PF, int VEC, bool PERM, class XT, class YT>
__device__ __forceinline__ void band_kernel_body(const MtArgsT<XT, YT>& a, float* coef) {
  using B = BandBody<WIDTH, PF, VEC, PERM, XT, YT>;
  using V = typename Cols<VEC>::T;
  constexpr int W = B::W;
  const int k_begin = blockIdx.y * a.rows_per_chunk;
  int k_end = k_begin + a.rows_per_chunk;
  if (k_end > a.T_out) k_end = a.T_out;
  const int n_out = k_end - k_begin;
  if (n_out <= 0) return;  // whole block
  int64_t c = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
  const bool live = c < a.C;
  if (!live) c = 0;  // idle lanes of the last block shadow column 0 and never store
  const XT* __restrict__ X = a.X;
  YT* __restrict__ Y = a.Y;

  // output row k reads input rows [k + d_lo, k + d_hi]; tap d of row k is input row k + d_hi - d
  const int d_lo = (a.row_off - a.col_off) - a.band_lo;
  const int d_hi = (a.row_off - a.col_off) + a.band_hi;
  for (int t = threadIdx.x; t < n_out * WIDTH; t += blockDim.x) {
    const int o = t / WIDTH, d = t % WIDTH;
    const int k = k_begin + o, j = k + d_hi - d;
    coef[t] = (j >= k + d_lo && j >= 0 && j < a.T_in) ? mop(a, k, j) : 0.f;
  }
  __syncthreads();

  const int q0 = k_begin + d_hi - (WIDTH - 1);  // input row of local index 0
  const int u_max = n_out + WIDTH - 2;          // newest local row any output needs

  V win[W];
  // ---- fill: local rows 0 .. WIDTH-2+PF go to slots 0 .. W-2
#pragma unroll
  for (int u = 0; u < WIDTH - 1 + PF; ++u) win[u] = B::fetch(a, X, q0, u, u_max, c);

  // ---- steady: output o is completed by local row u = WIDTH-1+o in slot (WIDTH-1+o) % W.
  //      Row u + PF is fetched first, into slot (u + PF) % W = (u - WIDTH) % W: the row that
  //      lived there is older than anything output o (or any later one) reads.
  int o = 0;
  for (; o + W <= n_out; o += W) {
#pragma unroll
    for (int i = 0; i < W; ++i) {
      const int u = WIDTH - 1 + o + i;
      win[(WIDTH - 1 + i + PF) % W] = B::fetch(a, X, q0, u + PF, u_max, c);
      B::emit(a, Y, win, coef, (WIDTH - 1 + i) % W, o + i, k_begin + o + i, c, live);
    }
  }
  // ---- tail: fewer than W outputs left (wave-uniform branches)
#pragma unroll
  for (int i = 0; i < W - 1; ++i) {
    if (o + i < n_out) {
      const int u = WIDTH - 1 + o + i;
      if (u + PF <= u_max) win[(WIDTH - 1 + i + PF) % W] = B::fetch(a, X, q0, u + PF, u_max, c);
      B::emit(a, Y, win, coef, (WIDTH - 1 + i) % W, o + i, k_begin + o + i, c, live);
    }
  }
}

// The band kernels' launch: the output rows are cut into chunks only when the column grid alone cannot fill 256 CUs (and
// always into chunks of at most kBandMaxChunkRows rows, the tap table); the window is the narrowest of 1, 2, 4, 8, 12, 16,
// 20 rows that holds the band.  `launch(width tag, grid, a)` enqueues the caller's kernel of that width.  An output
// element's taps and their order depend on the width alone, never on the chunks.
template <int VEC, class XT, class YT, class Launch>
static void launch_band_width(MtArgsT<XT, YT> a, Launch launch) {
  const int64_t cvec = (a.C + VEC - 1) / VEC;
  const int64_t width = (int64_t)a.band_lo + a.band_hi + 1;
  const unsigned col_blocks = (unsigned)((cvec + 255) / 256);
  int chunks = 1;
  if (col_blocks < 2048) {
    chunks = (int)((2048 + col_blocks - 1) / col_blocks);
    const int max_chunks = (a.T_out + 7) / 8;
    if (chunks > max_chunks) chunks = max_chunks;
    if (chunks < 1) chunks = 1;
  }
  const int min_chunks = (a.T_out + kBandMaxChunkRows - 1) / kBandMaxChunkRows;
  if (chunks < min_chunks) chunks = min_chunks;
  a.rows_per_chunk = (a.T_out + chunks - 1) / chunks;
  chunks = (a.T_out + a.rows_per_chunk - 1) / a.rows_per_chunk;
  const dim3 grid(col_blocks, chunks);
  using std::integral_constant;
  if (width <= 1) launch(integral_constant<int, 1>{}, grid, a);
  else if (width <= 2) launch(integral_constant<int, 2>{}, grid, a);
  else if (width <= 4) launch(integral_constant<int, 4>{}, grid, a);
  else if (width <= 8) launch(integral_constant<int, 8>{}, grid, a);
  else if (width <= 12) launch(integral_constant<int, 12>{}, grid, a);
  else if (width <= 16) launch(integral_constant<int, 16>{}, grid, a);
  else launch(integral_constant<int, 20>{}, grid, a);
}

constexpr int kBandPrefetch = 4;  // rows in flight per lane
constexpr int kBandMaxWidth = 20;  // wider windows do not fit the register file unrolled

}  // namespace tmgcn
