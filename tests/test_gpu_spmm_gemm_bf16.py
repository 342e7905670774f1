"""GPU: the fused SpMM+GEMM on a bf16-stored operand (csrc/spmm_gemm_bf16.hip) against the C oracle.

Reference: tests/_util.load_c_oracle (ref_spmm, ref_gemm: fp64 accumulation, fp32 store) fed the WIDENED input
X_bf16.float() — widening is exact, so the fp32 outputs (AX, pre, Y) keep the project's bar max|Δ| <= 1e-5·max|ref|;
the outputs written in bf16 (Y with out_dtype=bf16, dX) are held to that bar plus one rounding to 8 significant bits
(tests/_bf16_bound.py).  Inputs: X ~ N(0,1) rounded to bf16, val uniform in [0.1, 1], W ~ N(0,1), seeded.
"""
import ctypes as C
import functools

import pytest
import torch

from _bf16_bound import assert_bf16_close
from _util import REL_TOL, assert_close, cptr, load_c_oracle, max_rel_err, record_tolerance
from tmgcn_amd import _lib, ops, synth
from tmgcn_amd.csr import BatchedCSR

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
WIDTHS = [(16, 8), (24, 40), (64, 64), (120, 40), (128, 128), (128, 16)]


def ref_spmm(csr, X):
    Y = torch.empty_like(X)
    load_c_oracle().ref_spmm(cptr(csr.rowptr), cptr(csr.col), cptr(csr.val), cptr(X), cptr(Y), csr.n_rows, csr.N, X.shape[2])
    return Y


def ref_gemm(A, W, trans_w=False, per_slice=False):
    T, N, K = A.shape
    Nf = W.shape[-2] if trans_w else W.shape[-1]
    Y = torch.empty(T, N, Nf)
    load_c_oracle().ref_gemm(cptr(A), cptr(W), cptr(Y), T * N, K, Nf, int(trans_w), N if per_slice else 0,
                             W.shape[-1] * W.shape[-2] if per_slice else 0)
    return Y


ACTS = {None: lambda x: x, "relu": torch.relu, "leaky": lambda x: torch.nn.functional.leaky_relu(x, 0.01), "selu": torch.selu}


def csr_from_lengths(T, N, cnt, seed):
    """CPU BatchedCSR with cnt[k*N + i] entries in row i of slice k: random columns (a row of N entries: every column
    once), values uniform in [0.1, 1]."""
    g = torch.Generator().manual_seed(seed)
    rowptr = torch.zeros(T * N + 1, dtype=torch.int64)
    torch.cumsum(cnt, 0, out=rowptr[1:])
    nnz = int(rowptr[-1])
    col = torch.randint(0, N, (nnz,), generator=g, dtype=torch.int32)
    for r in (cnt == N).nonzero().flatten().tolist():
        col[int(rowptr[r]):int(rowptr[r + 1])] = torch.randperm(N, generator=g).int()
    val = 0.1 + 0.9 * torch.rand(nnz, generator=g)
    return BatchedCSR(rowptr, col, val, T, N)


@functools.lru_cache(maxsize=None)
def mixed_csr(T=3, N=333):
    """Rows of 0, 1 and about 33 entries and, in slice 1, one row holding all N columns (beyond the four-wave threshold
    of 256).  3 x 333 rows: no multiple of 64, the last tile of every slice is ragged."""
    g = torch.Generator().manual_seed(5)
    kind = torch.randint(0, 4, (T * N,), generator=g)
    cnt = torch.where(kind == 0, 0, torch.where(kind == 1, 1, torch.randint(25, 42, (T * N,), generator=g)))
    cnt[N + 77] = N
    cnt[0], cnt[1] = 0, 1
    return csr_from_lengths(T, N, cnt.long(), seed=6)


@functools.lru_cache(maxsize=None)
def operands(T, N, K, seed=1):
    """(X bf16 on the CPU, its exact fp32 widening) — computed once per shape and never modified."""
    X = torch.randn(T, N, K, generator=torch.Generator().manual_seed(seed)).bfloat16()
    return X, X.float()


@functools.lru_cache(maxsize=None)
def ref_ax(K):
    csr = mixed_csr()
    return ref_spmm(csr, operands(csr.T, csr.N, K)[1])


def weight(K, Nf, trans_w, per_slice, T, seed=2):
    shape = ((T,) if per_slice else ()) + ((Nf, K) if trans_w else (K, Nf))
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def check_y(Y, ref, out_dtype, what):
    if out_dtype is BF16:
        assert_bf16_close(Y, ref, what)
    else:
        assert Y.dtype == torch.float32
        assert_close(Y, ref, REL_TOL, what)


# ------------------------------------------------------------------------------------- widths x options
@pytest.mark.parametrize("out_dtype", [None, BF16], ids=["y_f32", "y_bf16"])
@pytest.mark.parametrize("trans_w", [False, True], ids=["W", "Wt"])
@pytest.mark.parametrize("per_slice", [False, True], ids=["shared", "per_slice"])
@pytest.mark.parametrize("K,Nf", WIDTHS)
def test_kernel_vs_oracle(K, Nf, per_slice, trans_w, out_dtype):
    csr = mixed_csr()
    Xb, _ = operands(csr.T, csr.N, K)
    W = weight(K, Nf, trans_w, per_slice, csr.T)
    AXr = ref_ax(K)
    pre_r = ref_gemm(AXr, W, trans_w, per_slice)
    A, Xd, Wd = csr.to(DEV), Xb.to(DEV), W.to(DEV)
    for act in (None, "relu", "leaky", "selu"):
        for want_ax in (False, True):
            what = f"K={K} Nf={Nf} act={act} ax={want_ax}"
            Y, AX, pre = ops.kernels.spmm_gemm_bf16(A, Xd, Wd, trans_w=trans_w, act=act, want_ax=want_ax, want_pre=True,
                                                    out_dtype=out_dtype)
            check_y(Y, ACTS[act](pre_r), out_dtype, "Y " + what)
            assert (AX is not None) == want_ax
            if want_ax:
                assert AX.dtype == torch.float32
                assert_close(AX, AXr, REL_TOL, "AX " + what)
            assert (pre is not None) == (act is not None)
            if pre is not None:
                assert pre.dtype == torch.float32
                assert_close(pre, pre_r, REL_TOL, "pre " + what)


# ------------------------------------------------------------------------------------- row lengths and structure
def test_row_beyond_the_giant_threshold():
    """T = 1, N = 40 001, K = 16: row 0 holds 40 000 entries (more than TMGCN_GIANT_ROW = 32 768; walked whole by the
    four waves), every other row its self loop only."""
    N, K, Nf = 40001, 16, 16
    cnt = torch.ones(N, dtype=torch.int64)
    cnt[0] = 40000
    csr = csr_from_lengths(1, N, cnt, seed=8)
    csr.col[40000:] = torch.arange(1, N, dtype=torch.int32)          # the self loops
    Xb, Xw = operands(1, N, K, seed=3)
    W = weight(K, Nf, False, False, 1)
    AXr = ref_spmm(csr, Xw)
    Y, AX, _ = ops.kernels.spmm_gemm_bf16(csr.to(DEV), Xb.to(DEV), W.to(DEV), want_ax=True)
    assert_close(AX, AXr, REL_TOL, "AX, 40 000-entry row")
    assert_close(Y, ref_gemm(AXr, W), REL_TOL, "Y, 40 000-entry row")


@pytest.mark.parametrize("T,N,deg", [(2, 70, 0), (3, 1, 1), (3, 128, 5), (3, 96, 5)],
                         ids=["all_empty", "N=1", "slice_end_on_a_tile", "slice_end_on_half_a_tile"])
def test_structure(T, N, deg):
    K, Nf = 32, 24
    cnt = torch.full((T * N,), min(deg, N), dtype=torch.int64)
    csr = csr_from_lengths(T, N, cnt, seed=9)
    Xb, Xw = operands(T, N, K, seed=4)
    W = weight(K, Nf, False, True, T)
    AXr = ref_spmm(csr, Xw)
    for out_dtype in (None, BF16):
        Y, AX, pre = ops.kernels.spmm_gemm_bf16(csr.to(DEV), Xb.to(DEV), W.to(DEV), act="selu", want_ax=True, want_pre=True,
                                                out_dtype=out_dtype)
        pre_r = ref_gemm(AXr, W, False, True)
        if deg == 0:
            assert not AX.any() and not pre.any() and not Y.float().any()
        assert_close(AX, AXr, REL_TOL, "AX")
        assert_close(pre, pre_r, REL_TOL, "pre")
        check_y(Y, torch.selu(pre_r), out_dtype, "Y")


# ------------------------------------------------------------------------------------- alignment
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_misaligned_x_is_copied_once_by_ops_and_refused_by_the_c_entry(shift):
    """An X that starts `shift` elements (2·shift bytes) into its allocation: ops copies it once and gives the result
    of the aligned operand, bit for bit; the same pointer at the C ABI is TMGCN_ERR_INVALID."""
    csr = mixed_csr()
    K, Nf = 64, 64
    Xb, _ = operands(csr.T, csr.N, K)
    W = weight(K, Nf, False, False, csr.T).to(DEV)
    A = csr.to(DEV)
    buf = torch.empty(Xb.numel() + 8, dtype=BF16, device=DEV)
    Xs = buf[shift:shift + Xb.numel()].view(Xb.shape)
    Xs.copy_(Xb)
    assert Xs.data_ptr() % 16 == 2 * shift and Xs.is_contiguous()
    want = ops.spmm_feature_gemm(A, Xb.to(DEV), W, act="relu")
    got = ops.spmm_feature_gemm(A, Xs, W, act="relu")
    assert torch.equal(got, want)
    Y = torch.empty(csr.T, csr.N, Nf, device=DEV)
    lib = _lib.load()
    rc = lib.tmgcn_spmm_gemm_bf16(cptr(A.rowptr), cptr(A.col), cptr(A.val), cptr(Xs), csr.n_rows, csr.N, K, cptr(W), Nf, 0, 0, 0, 0,
                                  cptr(Y), 0, None, None, 0, -1.0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == -1 and b"aligned" in lib.tmgcn_last_error()


# ------------------------------------------------------------------------------------- reproducibility
@pytest.mark.parametrize("K,Nf", [(128, 128), (24, 40)])
def test_two_launches_give_the_same_bits(K, Nf):
    csr = mixed_csr()
    A, Xd, Wd = csr.to(DEV), operands(csr.T, csr.N, K)[0].to(DEV), weight(K, Nf, False, False, csr.T).to(DEV)
    Y1, AX1, _ = ops.kernels.spmm_gemm_bf16(A, Xd, Wd, act="leaky", want_ax=True)
    Y2, AX2, _ = ops.kernels.spmm_gemm_bf16(A, Xd, Wd, act="leaky", want_ax=True)
    assert torch.equal(Y1, Y2) and torch.equal(AX1, AX2)


# ------------------------------------------------------------------------------------- autograd
def _layer_refs(csr, Xw, W, act, dY, dY_rounded_for_dw):
    """Oracle forward and gradients of Y = act((Â ⋆ X)·W) for the upstream gradient dY: the dX reference is fed dY rounded
    to bf16 once (what the backward gather reads), dW the fp64 product of the oracle's AX and the fp32 gradient (or the
    rounded one, where the gradient itself arrives in bf16)."""
    AXr = ref_spmm(csr, Xw)
    pre = ref_gemm(AXr, W)
    mask = torch.ones_like(pre) if act is None else (pre > 0).float()                   # relu
    d_dx = dY.bfloat16().float() * mask                                                 # rounding commutes with a 0/1 mask
    d_dw = (dY.bfloat16().float() if dY_rounded_for_dw else dY) * mask
    dXr = ref_spmm(csr.transpose(), ref_gemm(d_dx, W, trans_w=True))
    dWr = torch.einsum("tnk,tnf->kf", AXr.double(), d_dw.double())
    return ACTS[act](pre), dXr, dWr


@pytest.mark.parametrize("out_dtype", [None, BF16], ids=["y_f32", "y_bf16"])
@pytest.mark.parametrize("act", [None, "relu"])
@pytest.mark.parametrize("K,Nf", [(64, 64), (24, 40)])
def test_autograd(K, Nf, act, out_dtype):
    csr = mixed_csr()
    Xb, Xw = operands(csr.T, csr.N, K)
    W = weight(K, Nf, False, False, csr.T)
    dY = torch.randn(csr.T, csr.N, Nf, generator=torch.Generator().manual_seed(12))
    Yr, dXr, dWr = _layer_refs(csr, Xw, W, act, dY, out_dtype is BF16)
    Xd, Wd = Xb.to(DEV).requires_grad_(True), W.to(DEV).requires_grad_(True)
    Y = ops.spmm_feature_gemm(csr.to(DEV), Xd, Wd, act=act, out_dtype=out_dtype)
    check_y(Y, Yr, out_dtype, "Y")
    Y.backward(dY.to(DEV).to(Y.dtype))
    assert Xd.grad.dtype == BF16 and Wd.grad.dtype == torch.float32
    assert_close(Wd.grad, dWr, REL_TOL, "dW")
    assert_bf16_close(Xd.grad, dXr, "dX")


def test_graph_capture_replays_the_eager_bits():
    csr = mixed_csr()
    K = Nf = 64
    A = csr.to(DEV)
    A.transpose()                                                # built outside the capture
    Xd = operands(csr.T, csr.N, K)[0].to(DEV).requires_grad_(True)
    Wd = weight(K, Nf, False, False, csr.T).to(DEV).requires_grad_(True)
    dY = torch.randn(csr.T, csr.N, Nf, generator=torch.Generator().manual_seed(13)).to(DEV)

    def step():
        Xd.grad = Wd.grad = None
        Y = ops.spmm_feature_gemm(A, Xd, Wd, act="relu")
        Y.backward(dY)
        return Y

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Y = step()
        eager = (Y.detach().clone(), Xd.grad.clone(), Wd.grad.clone())
    torch.cuda.current_stream().wait_stream(side)
    Xd.grad = Wd.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Yg = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(Yg, eager[0]) and torch.equal(Xd.grad, eager[1]) and torch.equal(Wd.grad, eager[2])


# ------------------------------------------------------------------------------------- model
BF16_MODEL_TOL = 2e-2     # the project's stated bound for bf16 storage


@pytest.mark.parametrize("branch", [dict(use_Minv=False, apply_M_twice=True), dict(use_Minv=False), dict(use_Minv=True)],
                         ids=["M_twice", "default", "Minv"])
def test_model_with_bf16_activations(branch):
    """EmbeddingGCN2 with act_dtype=bf16 against the same model in fp32: the layer-2 operand is rounded once, the
    deviation is that rounding propagated through layer 2, the head and the backward."""
    import tmgcn_amd.layers as ehf
    g = synth.dynamic_graph(T=4, N=200, edges_per_slice=300, seed=1, no_diag=2)
    At, X, M = g.At_list(), torch.from_numpy(g.X), torch.from_numpy(g.M)
    edges, labels = torch.from_numpy(g.edges), torch.from_numpy(g.labels).to(DEV)
    crit = torch.nn.CrossEntropyLoss(weight=torch.tensor([0.9, 0.1], device=DEV))
    out = {}
    for name, act_dtype in (("f32", None), ("bf16", BF16)):
        torch.manual_seed(0)
        m = ehf.EmbeddingGCN2(At, X, edges, M, hidden_feat=[16, 16, 2], condensed_W=True, nonlin2="selu", device=DEV,
                              act_dtype=act_dtype, **branch)
        logits = m()
        crit(logits, labels).backward()
        assert logits.dtype == torch.float32 and all(p.dtype == torch.float32 and p.grad.dtype == torch.float32 for p in m.parameters())
        out[name] = {"logits": logits.detach(), **{"d" + n: p.grad for n, p in m.named_parameters()}}
    for k, ref in out["f32"].items():
        err = max_rel_err(out["bf16"][k], ref)
        print(f"bf16 activations, {k}: max|Δ|/max|ref| = {err:.3e}")
        record_tolerance(f"EmbeddingGCN2 act_dtype=bf16 {k}", err, BF16_MODEL_TOL)
        assert err <= BF16_MODEL_TOL, (k, err)
    assert any(max_rel_err(out["bf16"][k], out["f32"][k]) > 0 for k in out["f32"]), "act_dtype=bf16 changed nothing: the bf16 path did not run"


def test_model_refuses_what_the_bf16_path_cannot_do():
    import tmgcn_amd.layers as ehf
    g = synth.dynamic_graph(T=4, N=200, edges_per_slice=300, seed=1, no_diag=2)
    args = (g.At_list(), torch.from_numpy(g.X), torch.from_numpy(g.edges), torch.from_numpy(g.M))
    with pytest.raises(RuntimeError, match="hidden_feat"):
        ehf.EmbeddingGCN2(*args, hidden_feat=[6, 6, 2], condensed_W=True, use_Minv=False, device=DEV, act_dtype=BF16)
    with pytest.raises(RuntimeError, match="group"):
        ehf.EmbeddingGCN2(*args, hidden_feat=[16, 16, 2], condensed_W=True, use_Minv=False, device=DEV, act_dtype=BF16,
                          group=object())
