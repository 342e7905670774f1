"""GPU: the bf16-stored fused SpMM+GEMM (csrc/spmm_gemm_bf16.hip) over its whole dispatch table and schedule.

tests/test_gpu_spmm_gemm_bf16.py runs six widths on graphs of at most one tile per block.  This file runs what that leaves
out: every K of the launcher's switch and the Nf edges (1, a partial last strip), row lengths on the gather's own
boundaries (the 64-entry fetch, kLongRow = 256), the persistent loop with several tiles per block across slices with a
per-slice W and a heavy tile, exact arithmetic (bit equality on integer operands, round-to-nearest-even ties of a bf16 Y),
the 32-bit piece offsets at their limit with the three 64-bit-offset kernels, and the autograd routes test_autograd does
not take (the fp32 fallback of the backward, per-slice W, leaky / selu, gradients of one input only).

Reference and bounds are the project's own and nothing here is fitted to a run: the C oracle (tests/_util.load_c_oracle:
fp64 accumulation) or fp64 torch on the CPU, fed the exactly widened X.float(); REL_TOL = 1e-5 on fp32 outputs,
tests/_bf16_bound.py on bf16 outputs, torch.equal where the arithmetic is exact.  Every test prints the worst error it
met as a fraction of its bound.
"""
import functools

import pytest
import torch

import test_gpu_spmm_gemm_bf16 as base      # helpers only: importing the module object collects none of its tests here
from _bf16_bound import bf16_excess
from _util import REL_TOL, max_rel_err
from tmgcn_amd import ops

pytestmark = pytest.mark.gpu
DEV = base.DEV
BF16 = torch.bfloat16
ALL_K = list(range(16, 129, 8))              # the 15 cases of the launcher's switch
TILE = 64                                    # rows per tile (csrc/spmm_row.h: kTileRows)
HEAVY_MIN = 8192                             # kHeavyMin: a tile of more entries (and of more than 8x the mean) is heavy


class Worst:
    """The largest error / bound a test has met, printed when it ends: fp32 outputs against 1e-5, bf16 outputs against
    tests/_bf16_bound.py (there one rounding alone reaches the bound at the bottom of a binade, so that figure sits near 1)."""

    def __init__(self, group):
        self.group, self.used32, self.used16 = group, 0.0, 0.0

    def f32(self, got, ref, what):
        assert got.dtype == torch.float32, f"{what}: expected fp32, got {got.dtype}"
        err = max_rel_err(got, ref)
        self.used32 = max(self.used32, err / REL_TOL)
        assert err <= REL_TOL, f"{what}: max|Δ|/max|ref| = {err:.3e} > {REL_TOL:.1e}"

    def bf16(self, got, ref, what):
        assert got.dtype == BF16, f"{what}: expected bf16, got {got.dtype}"
        ex = bf16_excess(got, ref)
        self.used16 = max(self.used16, ex)
        assert ex <= 1.0, f"{what}: |got - ref| reaches {ex:.3f} x (2^-8 |ref| + (1 + 2^-8) 1e-5 max|ref|)"

    def y(self, got, ref, out_dtype, what):
        (self.bf16 if out_dtype is BF16 else self.f32)(got, ref, what)

    def report(self):
        print(f"[worst error / bound] {self.group}: fp32 outputs {self.used32:.3f}, bf16 outputs {self.used16:.3f}")


def launch(A, X, W, **kw):
    return ops.kernels.spmm_gemm_bf16(A, X, W, **kw)


# ------------------------------------------------------------------------------------- 1. every K, the Nf edges
@pytest.mark.parametrize("K", ALL_K)
def test_every_k_of_the_dispatch_table(K):
    """Nf = 1 (one column of one strip), 33 (a second strip of one column), 128 (all four strips), 97 for three K (the last
    strip one column wide); W and Wᵀ; shared W, per-slice W at Nf = 33; Y in fp32 and bf16; AX and pre stored."""
    csr = base.mixed_csr()
    T = csr.T
    Xb, _ = base.operands(T, csr.N, K)
    AXr = base.ref_ax(K)
    A, Xd = csr.to(DEV), Xb.to(DEV)
    worst = Worst(f"dispatch table, K={K}")
    for Nf in (1, 33, 128) + ((97,) if K in (40, 104, 112) else ()):
        for trans_w in (False, True):
            for per_slice in ((False, True) if Nf == 33 else (False,)):
                W = base.weight(K, Nf, trans_w, per_slice, T)
                pre_r = base.ref_gemm(AXr, W, trans_w, per_slice)
                Yr = torch.selu(pre_r)
                Wd = W.to(DEV)
                for out_dtype in (None, BF16):
                    what = f"K={K} Nf={Nf} trans_w={trans_w} per_slice={per_slice} out={out_dtype}"
                    Y, AX, pre = launch(A, Xd, Wd, trans_w=trans_w, act="selu", want_ax=True, want_pre=True, out_dtype=out_dtype)
                    assert Y.shape == (T, csr.N, Nf) and AX.shape == (T, csr.N, K) and pre.shape == (T, csr.N, Nf)
                    worst.y(Y, Yr, out_dtype, "Y " + what)
                    worst.f32(AX, AXr, "AX " + what)
                    worst.f32(pre, pre_r, "pre " + what)
    worst.report()


# ------------------------------------------------------------------------------------- 2. row lengths on the boundaries
WAVE_EDGES = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200]
LONG_EDGES = WAVE_EDGES + [255, 256, 257, 258, 300]


@functools.lru_cache(maxsize=None)
def edge_csrs():
    """Two CSRs of two slices each whose row i holds L[(i + 5·slice) % len(L)] entries.  N = 200 with the lengths round the
    wave's 64-entry fetch (and the row of all N columns); N = 300 with those and 255 .. 258 and 300 as well: 256 is the last
    row one wave walks, 257 the first that four waves share — quarters of 128, so waves 2 and 3 get 1 and 0 entries."""
    out = []
    for N, L, seed in ((200, WAVE_EDGES, 31), (300, LONG_EDGES, 32)):
        cnt = torch.tensor([L[(i + 5 * k) % len(L)] for k in range(2) for i in range(N)], dtype=torch.int64)
        assert int(cnt.max()) == N and set(cnt.tolist()) == set(L)
        out.append(base.csr_from_lengths(2, N, cnt, seed=seed))
    return tuple(out)


@pytest.mark.parametrize("K", [16, 40, 64, 104, 128])       # one K of every (lanes per row, gathers in flight) class
def test_row_lengths_on_the_gather_boundaries(K):
    Nf = 24
    worst = Worst(f"row-length edges, K={K}")
    for csr in edge_csrs():
        Xb, Xw = base.operands(csr.T, csr.N, K, seed=33)
        W = base.weight(K, Nf, False, False, csr.T)
        AXr = base.ref_spmm(csr, Xw)
        Yr = base.ref_gemm(AXr, W)
        A, Xd, Wd = csr.to(DEV), Xb.to(DEV), W.to(DEV)
        Y1, AX1, _ = launch(A, Xd, Wd, want_ax=True)
        Y2, AX2, _ = launch(A, Xd, Wd, want_ax=True)
        worst.f32(AX1, AXr, f"AX N={csr.N}")
        worst.f32(Y1, Yr, f"Y N={csr.N}")
        # per row as well: a short row that lost an entry is invisible next to the 300-entry row's magnitude
        lens = (csr.rowptr[1:] - csr.rowptr[:-1]).view(csr.T, csr.N)
        for L in sorted(set(lens.flatten().tolist())):
            m = lens == L
            if L == 0:
                assert not AX1.cpu()[m].any() and not Y1.cpu()[m].any(), f"rows of no entries, N={csr.N}"
            else:
                worst.f32(AX1.cpu()[m], AXr[m], f"AX of the rows of {L} entries, N={csr.N}")
        assert torch.equal(Y1, Y2) and torch.equal(AX1, AX2), f"two launches differ, N={csr.N}"
    worst.report()


# ------------------------------------------------------------------------------------- 3. several tiles per block
@functools.lru_cache(maxsize=None)
def loop_csr():
    """T = 3, N = 4 200: 66 tiles per slice, the last of 40 rows; 0 .. 12 entries per row, rows of 256, 257 and 300 entries
    in every slice (one of them the slice's last row, in the ragged tile) and, in slice 1, three rows of all 4 200 columns
    inside tile 30."""
    T, N = 3, 4200
    g = torch.Generator().manual_seed(21)
    cnt = torch.randint(0, 13, (T * N,), generator=g)
    for k in range(T):
        for j, r in enumerate((5, 700 + 64 * k, 1501, 2222 + k, 3000, N - 1)):
            cnt[k * N + r] = (256, 257, 300)[(j + k) % 3]
    for r in (3, 20, 41):
        cnt[N + 30 * TILE + r] = N
    return base.csr_from_lengths(T, N, cnt.long(), seed=22)


def tile_entries(csr):
    """Stored entries of every tile of the launch, tiles restarting at every slice (csrc/spmm_row.h: TileMap)."""
    out = []
    for k in range(csr.T):
        for r0 in range(k * csr.N, (k + 1) * csr.N, TILE):
            out.append(int(csr.rowptr[min(r0 + TILE, (k + 1) * csr.N)] - csr.rowptr[r0]))
    return out


def test_loop_csr_has_a_heavy_tile_and_three_tiles_per_block():
    """The premises of the next test, from rowptr alone: 198 tiles for the 64 blocks that grid_reserve = 4096 leaves, and
    exactly one tile beyond the kernel's own threshold max(8192, 8 x the mean) (HeavyScan::init)."""
    csr = loop_csr()
    ent = tile_entries(csr)
    assert len(ent) == 198 and len(ent) >= 3 * 64 and csr.N % TILE == 40
    thr = max(HEAVY_MIN, 8 * (csr.nnz // len(ent)))
    assert [t for t, e in enumerate(ent) if e > thr] == [66 + 30] and ent[66 + 30] >= 12600
    lens = csr.rowptr[1:] - csr.rowptr[:-1]
    for k in range(csr.T):
        assert {256, 257, 300} <= set(lens[k * csr.N:(k + 1) * csr.N].tolist())


@functools.lru_cache(maxsize=None)
def loop_ref_ax(K):
    csr = loop_csr()
    return base.ref_spmm(csr, base.operands(csr.T, csr.N, K, seed=23)[1])


@pytest.mark.parametrize("K", [16, 40, 104, 112, 128])
def test_persistent_loop_with_several_tiles_per_block(K):
    """grid_reserve = 4096 leaves the floor of 64 blocks for 198 tiles: every block walks tile after tile, across slice
    boundaries with a W of its own per slice, behind a heavy-tile pass that found one tile.  Against the oracle, and bit
    for bit against the launch of one block per tile: which block sums a row must not change a bit."""
    csr = loop_csr()
    T = csr.T
    Xb, _ = base.operands(T, csr.N, K, seed=23)
    AXr = loop_ref_ax(K)
    A, Xd = csr.to(DEV), Xb.to(DEV)
    worst = Worst(f"persistent loop, K={K}")
    for Nf in (33, 128):
        W = base.weight(K, Nf, False, True, T)
        pre_r = base.ref_gemm(AXr, W, False, True)
        Yr = torch.relu(pre_r)
        Wd = W.to(DEV)
        for out_dtype in (None, BF16):
            what = f"K={K} Nf={Nf} out={out_dtype}"
            few = launch(A, Xd, Wd, act="relu", want_ax=True, want_pre=True, out_dtype=out_dtype, grid_reserve=4096)
            many = launch(A, Xd, Wd, act="relu", want_ax=True, want_pre=True, out_dtype=out_dtype, grid_reserve=0)
            worst.y(few[0], Yr, out_dtype, "Y " + what)
            worst.f32(few[1], AXr, "AX " + what)
            worst.f32(few[2], pre_r, "pre " + what)
            for name, a, b in zip(("Y", "AX", "pre"), few, many):
                assert torch.equal(a, b), f"{name} differs between 64 blocks and one block per tile, {what}"
    worst.report()


# ------------------------------------------------------------------------------------- 4. exact arithmetic
@pytest.mark.parametrize("K", [24, 128])
def test_integer_operands_give_the_reference_bits(K):
    """X integers in [-8, 8], val in {0.5, 1, 2}, W integers in [-4, 4]: every partial sum, in any order, is a multiple of
    0.5 of magnitude below 2^23 (asserted below for the worst element), hence exact in fp32 — AX, pre and Y must equal the
    fp64 reference bit for bit, and the bf16 Y its one rounding to nearest even."""
    Nf = 40
    src = base.mixed_csr()
    g = torch.Generator().manual_seed(41)
    val = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (src.nnz,), generator=g)]
    csr = base.BatchedCSR(src.rowptr, src.col, val, src.T, src.N)
    Xw = torch.randint(-8, 9, (csr.T, csr.N, K), generator=g).float()
    Xb = Xw.bfloat16()
    assert torch.equal(Xb.float(), Xw)
    W = torch.randint(-4, 5, (K, Nf), generator=g).float()
    sum_abs = base.ref_spmm(csr, Xw.abs()).double().reshape(-1, K) @ W.abs().double()      # Σ|terms| of every output element
    assert float(sum_abs.max()) < 2 ** 23, float(sum_abs.max())
    AXr = base.ref_spmm(csr, Xw)
    pre_r = base.ref_gemm(AXr, W)
    assert torch.equal(pre_r.double().reshape(-1, Nf), AXr.double().reshape(-1, K) @ W.double())   # the oracle's fp32 store was exact
    A, Xd, Wd = csr.to(DEV), Xb.to(DEV), W.to(DEV)
    for act in (None, "relu"):
        Yr = base.ACTS[act](pre_r)
        Y, AX, pre = launch(A, Xd, Wd, act=act, want_ax=True, want_pre=True)
        assert torch.equal(AX.cpu(), AXr), f"AX, act={act}"
        assert torch.equal(Y.cpu(), Yr), f"Y, act={act}"
        if act is not None:
            assert torch.equal(pre.cpu(), pre_r), "pre"
        Yb, _, _ = launch(A, Xd, Wd, act=act, out_dtype=BF16)
        assert Yb.dtype == BF16 and torch.equal(Yb.cpu().view(torch.int16), Yr.bfloat16().view(torch.int16)), f"bf16 Y, act={act}"
    print("[worst error / bound] integer operands: 0 (bit equality)")


def test_bf16_y_rounds_ties_to_even():
    """pre[r, n] = (-1)^n (256 + n) exactly (one entry (col 0, val 1) per row, X[0] = e_0, W[0, n] that value): bf16 numbers
    in [256, 512) are 2 apart, so every odd n is a tie, resolved down and up in turn by round-to-nearest-even.  The
    expected bits differ from truncation and from round-half-away in 32 columns each (asserted: not vacuous)."""
    N, K, Nf = 64, 16, 128
    csr = base.BatchedCSR(torch.arange(N + 1, dtype=torch.int64), torch.zeros(N, dtype=torch.int32), torch.ones(N), 1, N)
    X = torch.zeros(1, N, K)
    X[0, 0, 0] = 1.0
    W = torch.zeros(K, Nf)
    n = torch.arange(Nf)
    W[0] = torch.where(n % 2 == 0, 1.0, -1.0) * (256 + n)
    want = W[0].bfloat16().view(torch.int16)                             # torch's CPU cast rounds to nearest even
    bits = W[0].view(torch.int32)
    truncated = (bits >> 16).to(torch.int16)
    half_away = ((bits + 0x8000) >> 16).to(torch.int16)
    assert int((want != truncated).sum()) >= 32 and int((want != half_away).sum()) >= 32
    assert torch.equal(want.view(BF16).float()[0::2], W[0, 0::2])        # the even columns are bf16 numbers: no rounding there
    Y, _, _ = launch(csr.to(DEV), X.bfloat16().to(DEV), W.to(DEV), out_dtype=BF16)
    assert Y.dtype == BF16 and Y.shape == (1, N, Nf)
    got = Y.cpu().view(torch.int16)[0]
    assert torch.equal(got, want.expand(N, Nf)), "the bf16 Y is not the fp32 value rounded to nearest even"
    print("[worst error / bound] rounding ties: 0 (bit equality)")


# ------------------------------------------------------------------------------------- 6. autograd routes
def grad_refs(csr, Xw, W, act, dY_seen, pre_dev, round_for_dx):
    """Oracle gradients of Y = act((Â ⋆ X)·W), W shared [K, Nf] or per slice [T, K, Nf], for the upstream gradient as the
    backward sees it (dY_seen, fp32: a bf16 upstream widened).  d = dY · act'(pre) is formed as the backward forms it — one
    IEEE fp32 multiply by 1, 0 or the kernel's leaky slope, the mask taken from the DEVICE's own pre (itself held to the
    oracle by the caller) — so the dX reference is fed exactly the tensor the backward gather reads: d rounded to bf16 once
    on the kernel route (round_for_dx), d itself on the fp32 fallback.  dW: fp64 product of the oracle's AX and d."""
    per_slice = W.dim() == 3
    AXr = base.ref_spmm(csr, Xw)
    if act is None:
        d = dY_seen
    elif act == "relu":
        d = dY_seen * (pre_dev > 0).float()
    elif act == "leaky":
        d = dY_seen * torch.where(pre_dev > 0, torch.tensor(1.0), torch.tensor(0.01))
    else:
        raise AssertionError(act)
    d_dx = d.bfloat16().float() if round_for_dx else d
    dXr = base.ref_spmm(csr.transpose(), base.ref_gemm(d_dx, W, trans_w=True, per_slice=per_slice))
    dWr = torch.einsum("tnk,tnf->tkf" if per_slice else "tnk,tnf->kf", AXr.double(), d.double())
    return dXr, dWr


def run_layer(csr, Xb, W, act, out_dtype, dY, x_grad=True, w_grad=True):
    """Forward + backward of ops.spmm_feature_gemm on a fresh device copy of the CSR; returns (Y, dX, dW, A)."""
    A = csr.to(DEV)
    Xd, Wd = Xb.to(DEV).requires_grad_(x_grad), W.to(DEV).requires_grad_(w_grad)
    Y = ops.spmm_feature_gemm(A, Xd, Wd, act=act, out_dtype=out_dtype)
    Y.backward(dY.to(DEV).to(Y.dtype))
    return Y.detach(), Xd.grad, Wd.grad, A


def device_pre(csr, Xb, W, act, Xw, worst):
    """The pre-activation of the device's own forward launch, held to the oracle."""
    if act is None:
        return None
    _, _, pre = launch(csr.to(DEV), Xb.to(DEV), W.to(DEV), act=act, want_pre=True)
    worst.f32(pre, base.ref_gemm(base.ref_spmm(csr, Xw), W, False, W.dim() == 3), "pre of the forward")
    return pre.cpu()


def check_layer(K, Nf, act, out_dtype, per_slice, kernel_route, worst):
    csr = base.mixed_csr()
    Xb, Xw = base.operands(csr.T, csr.N, K)
    W = base.weight(K, Nf, False, per_slice, csr.T)
    dY = torch.randn(csr.T, csr.N, Nf, generator=torch.Generator().manual_seed(12))
    dY_seen = dY.bfloat16().float() if out_dtype is BF16 else dY
    # the route the backward takes is a function of the transposed widths alone (SpmmFeatureGemmBf16Fn::backward)
    assert ops.spmm_gemm_bf16_supported(Nf, K) is kernel_route
    pre_dev = device_pre(csr, Xb, W, act, Xw, worst)
    dXr, dWr = grad_refs(csr, Xw, W, act, dY_seen, pre_dev, round_for_dx=kernel_route)
    Y, dX, dW, _ = run_layer(csr, Xb, W, act, out_dtype, dY)
    what = f"K={K} Nf={Nf} act={act} out={out_dtype} per_slice={per_slice}"
    worst.y(Y, base.ACTS[act](base.ref_gemm(base.ref_spmm(csr, Xw), W, False, per_slice)), out_dtype, "Y " + what)
    assert dX.dtype == BF16 and dX.shape == Xb.shape and dW.dtype == torch.float32 and dW.shape == W.shape
    worst.f32(dW, dWr, "dW " + what)
    worst.bf16(dX, dXr, "dX " + what)


@pytest.mark.parametrize("out_dtype", [None, BF16], ids=["y_f32", "y_bf16"])
@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("K,Nf", [(64, 8), (16, 8), (64, 6), (64, 100)])
def test_autograd_fp32_fallback_of_the_backward(K, Nf, act, out_dtype):
    """Nf outside the kernel's K-domain: the backward gathers the fp32 d — the fp32 fused kernel where it has the transposed
    widths ((16, 8): K = 8 with Nf <= 16), the unfused pair elsewhere — and rounds dX once."""
    assert ops.kernels.spmm_gemm_supported(Nf, K) is ((K, Nf) == (16, 8))
    worst = Worst(f"autograd, fp32 fallback, K={K} Nf={Nf} act={act}")
    check_layer(K, Nf, act, out_dtype, per_slice=False, kernel_route=False, worst=worst)
    worst.report()


@pytest.mark.parametrize("out_dtype", [None, BF16], ids=["y_f32", "y_bf16"])
@pytest.mark.parametrize("K,Nf", [(64, 64), (24, 40)])
def test_autograd_per_slice_w(K, Nf, out_dtype):
    """W [T, K, Nf]: dW per slice, dX through the transposed per-slice W."""
    worst = Worst(f"autograd, per-slice W, K={K} Nf={Nf}")
    check_layer(K, Nf, "relu", out_dtype, per_slice=True, kernel_route=True, worst=worst)
    worst.report()


@pytest.mark.parametrize("out_dtype", [None, BF16], ids=["y_f32", "y_bf16"])
@pytest.mark.parametrize("K,Nf", [(64, 64), (24, 40)])
def test_autograd_leaky(K, Nf, out_dtype):
    worst = Worst(f"autograd, leaky, K={K} Nf={Nf}")
    check_layer(K, Nf, "leaky", out_dtype, per_slice=False, kernel_route=True, worst=worst)
    worst.report()


@pytest.mark.parametrize("K,Nf", [(64, 64), (24, 40)])
def test_autograd_selu(K, Nf):
    """selu's derivative holds an exponential, which is not bit-reproducible between the device and the CPU, and one
    flipped bf16 rounding of d moves dX by more than 1e-5: dW alone is held to the fp32 bar (d formed in fp64 from the
    device's pre), of dX the dtype and the shape."""
    csr = base.mixed_csr()
    Xb, Xw = base.operands(csr.T, csr.N, K)
    W = base.weight(K, Nf, False, False, csr.T)
    dY = torch.randn(csr.T, csr.N, Nf, generator=torch.Generator().manual_seed(12))
    worst = Worst(f"autograd, selu, K={K} Nf={Nf}")
    _, _, pre = launch(csr.to(DEV), Xb.to(DEV), W.to(DEV), act="selu", want_pre=True)
    AXr = base.ref_spmm(csr, Xw)
    worst.f32(pre, base.ref_gemm(AXr, W), "pre of the forward")
    p = pre.cpu().double()
    scale, alpha = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717
    d = dY.double() * torch.where(p > 0, torch.tensor(scale, dtype=torch.float64), scale * alpha * torch.exp(p.clamp(max=0)))
    Y, dX, dW, _ = run_layer(csr, Xb, W, "selu", None, dY)
    worst.f32(Y, torch.selu(base.ref_gemm(AXr, W)), "Y")
    worst.f32(dW, torch.einsum("tnk,tnf->kf", AXr.double(), d), "dW")
    assert dX.dtype == BF16 and dX.shape == Xb.shape
    worst.report()


@pytest.mark.parametrize("K,Nf", [(64, 64), (64, 8)], ids=["kernel_route", "fp32_fallback"])
def test_autograd_of_one_input_only(K, Nf):
    """Only W requires a gradient: no transposed CSR is built or passed, AX is stored; only X: AX is not stored.  Each
    gradient equals the one of the run in which both inputs require theirs, bit for bit."""
    csr = base.mixed_csr()
    Xb, _ = base.operands(csr.T, csr.N, K)
    W = base.weight(K, Nf, False, False, csr.T)
    dY = torch.randn(csr.T, csr.N, Nf, generator=torch.Generator().manual_seed(12))
    Y, dX, dW, A = run_layer(csr, Xb, W, "relu", None, dY)
    assert A._t is not None                                           # (csr.py caches the transpose it built for dX)
    Yw, dXw, dWw, Aw = run_layer(csr, Xb, W, "relu", None, dY, x_grad=False)
    assert dXw is None and Aw._t is None, "a transposed CSR was built although X needs no gradient"
    assert torch.equal(Yw, Y) and torch.equal(dWw, dW)
    Yx, dXx, dWx, _ = run_layer(csr, Xb, W, "relu", None, dY, w_grad=False)
    assert dWx is None
    assert torch.equal(Yx, Y) and torch.equal(dXx, dX)


# ------------------------------------------------------------------------------------- 5. piece offsets: 32 bits at their limit, 64 bits
ROW_LENGTHS = (1, 7, 64, 65, 256, 257, 1000)
OFF32_LIMIT_N = 2 ** 24 - 1                  # K = 128: N·K·2 = 2^32 - 256, the largest slice with 32-bit piece offsets


def off32_limit(K):
    """The largest N whose slice of X the launcher addresses with 32-bit byte offsets: N·K·2 <= 0xffffffff."""
    return 0xffffffff // (2 * K)


@pytest.fixture(scope="module")
def big_x():
    """One flat buffer of N(0,1) values rounded to bf16, filled on the device in chunks from a seeded generator and shared
    by the launches below (each views a prefix of it as its [T, N, K]): 8 GiB, the size of the largest of them."""
    if torch.cuda.get_device_properties(0).total_memory < 32e9:
        pytest.skip("needs 32 GB of device memory")
    n = 2 * OFF32_LIMIT_N * 128
    assert all(n >= (off32_limit(K) + 4097) * K for K in (112, 120, 128))
    flat = torch.empty(n, dtype=BF16, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(51)
    step = 2 ** 28
    for i in range(0, n, step):
        flat[i:min(i + step, n)].normal_(generator=g)
    assert bool(torch.isfinite(flat[:step].float()).all())
    yield flat
    del flat
    torch.cuda.empty_cache()


def sparse_big_csr(T, N, K, slice_with_rows, with_c32, seed):
    """CPU CSR of T·N rows, all empty but the rows of three tiles of one slice — the first, the middle one and the last
    (ragged unless 64 divides N) — whose lengths cycle through ROW_LENGTHS.  Every such row holds, at random places, the
    columns where an offset computation goes wrong — 0, N - 1, c31 - 1 .. c31 + 1 (byte offset 2^31: a signed 32-bit
    offset wraps) and, with_c32, c32 - 1 .. c32 + 1 (byte offset 2^32: a truncated offset lands on columns 0 and 1) — as
    many of them as it has entries, starting at a different one from row to row, so the rows of 1 and 7 entries cover all
    of them between them; the rest of its columns are random.  Returns (csr, global rows, row id / col / val of every entry)."""
    g = torch.Generator().manual_seed(seed)
    c31, c32 = -(-2 ** 31 // (2 * K)), -(-2 ** 32 // (2 * K))
    special = [0, N - 1, c31 - 1, c31, c31 + 1] + ([c32 - 1, c32, c32 + 1] if with_c32 else [])
    assert all(0 <= c < N for c in special)
    tiles = (N + TILE - 1) // TILE
    local = [r for t in (0, tiles // 2, tiles - 1) for r in range(t * TILE, min((t + 1) * TILE, N))]
    assert len(local) <= 512
    cnt = torch.zeros(T * N, dtype=torch.int64)
    cols, rid = [], []
    for j, r in enumerate(local):
        L = ROW_LENGTHS[j % len(ROW_LENGTHS)]
        c = torch.randint(0, N, (L,), generator=g, dtype=torch.int64)
        take = min(L, len(special))
        c[:take] = torch.tensor([special[(j + i) % len(special)] for i in range(take)])
        cols.append(c[torch.randperm(L, generator=g)])
        rid.append(torch.full((L,), j, dtype=torch.int64))
        cnt[slice_with_rows * N + r] = L
    assert {int(c[0]) for c in cols if c.numel() == 1} == set(special), "the one-entry rows do not cover every special column"
    rowptr = torch.zeros(T * N + 1, dtype=torch.int64)
    torch.cumsum(cnt, 0, out=rowptr[1:])
    col, rid = torch.cat(cols), torch.cat(rid)
    val = 0.1 + 0.9 * torch.rand(col.numel(), generator=g)
    rows = slice_with_rows * N + torch.tensor(local, dtype=torch.int64)
    return base.BatchedCSR(rowptr, col.int(), val, T, N), rows, rid, col, val


def run_big(flat, T, N, K, slice_with_rows, with_c32, want_ax, group):
    Nf = 8
    assert flat.numel() >= T * N * K
    X = flat[:T * N * K].view(T, N, K)
    csr, rows, rid, col, val = sparse_big_csr(T, N, K, slice_with_rows, with_c32, seed=52 + K)
    W = base.weight(K, Nf, False, False, T)
    # fp64 reference of the non-empty rows from the gathered rows of X alone (X never leaves the device as a whole)
    uniq, inv = torch.unique(col, return_inverse=True)
    Xg = X[slice_with_rows].index_select(0, uniq.to(DEV)).cpu().double()
    AXr = torch.zeros(rows.numel(), K, dtype=torch.float64).index_add_(0, rid, val.double()[:, None] * Xg[inv])
    Yr = AXr @ W.double()
    Y, AX, _ = launch(csr.to(DEV), X, W.to(DEV), want_ax=want_ax)
    worst = Worst(group)
    rows_d = rows.to(DEV)
    for name, out, ref in (("Y", Y, Yr), ("AX", AX, AXr)):
        if out is None:
            assert name == "AX" and not want_ax
            continue
        flat_out = out.view(T * N, -1)
        worst.f32(flat_out[rows_d].cpu(), ref, f"{name} of the non-empty rows, N={N} K={K}")
        flat_out[rows_d] = 0
        assert not bool(flat_out.any()), f"{name}: a row without entries is not zero, N={N} K={K}"
    worst.report()


def test_off32_offsets_at_their_limit(big_x):
    """K = 128, N = 2^24 - 1: a slice of X ends 256 bytes below 2^32, and the rows lie in slice 1, whose base
    is 4 GiB into X."""
    N = OFF32_LIMIT_N
    assert N == off32_limit(128) and N * 128 * 2 <= 0xffffffff < (N + 1) * 128 * 2
    run_big(big_x, 2, N, 128, slice_with_rows=1, with_c32=False, want_ax=True, group="OFF32 at its limit, K=128")


@pytest.mark.parametrize("K", [128, 120, 112])
def test_64_bit_offset_kernels(big_x, K):
    """N = the 32-bit limit + 4 097: the launcher takes the <16, 2, OFF32 = false> kernel of this K, and the columns from
    c32 on have byte offsets beyond 2^32."""
    N = off32_limit(K) + 4097
    assert N * K * 2 > 0xffffffff
    run_big(big_x, 1, N, K, slice_with_rows=0, with_c32=True, want_ax=K == 128, group=f"64-bit offsets, K={K}")
