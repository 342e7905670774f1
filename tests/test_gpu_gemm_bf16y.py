"""GPU: the layer-1 GEMM that stores its result in bf16 (tmgcn_gemm_bf16y) and the weight gradient that reads a bf16 dY and
applies act'(pre) as it loads (tmgcn_gemm_dw_act_bf16) — kernel launchers, ops.feature_gemm(out_dtype=bf16) with autograd,
KernelTimer, hipGraph capture, and EmbeddingGCN2(act_dtype=bf16) in its default branch.

The bar is BIT equality with the launches the fused ones replace, run by the untouched fp32 kernels of the same build:
    forward   round_bf16(gemm(A, W, act))  and the fp32 pre-activation of that launch
    backward  gemm_dw(A, act_bwd(pre, widen(dY), act))
Only storage changes, so no tolerance is needed.  One group is also held to the suite's own bound against fp64 (REL_TOL for
fp32 values, tests/_bf16_bound.py for bf16 ones), so that being equal to a wrong composition cannot pass."""
import ctypes as C

import pytest
import torch

from _bf16_bound import assert_bf16_close
from _util import REL_TOL, assert_close
from tmgcn_amd import _lib, ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
ACTS = [None, "relu", "leaky", "selu"]
K_X3, NF_X3 = [16, 20, 124, 128], [16, 24, 40, 128]          # the bf16-split matrix-core kernels
K_SM, NF_SM = [1, 2, 6, 15], [16, 24, 40, 64]                # the thread-per-row kernels: Nf 16, 24 staged exit, 40, 64 direct


def randn(shape, seed, dtype=F32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def fwd_composition(A, W, act):
    if act is None:
        return ops.round_bf16(ops.kernels.gemm(A, W)), None
    Y, pre = ops.kernels.gemm(A, W, act=act, want_pre=True)
    return ops.round_bf16(Y), pre


def fwd_fused(A, W, act):
    if act is None:
        return ops.kernels.gemm(A, W, out_dtype=BF16), None
    return ops.kernels.gemm(A, W, act=act, want_pre=True, out_dtype=BF16)


def check_forward(A, W, act, what):
    Y, pre = fwd_fused(A, W, act)
    Yc, prec = fwd_composition(A, W, act)
    assert Y.dtype == BF16 and Y.shape == Yc.shape
    assert same_bits(Y, Yc), f"{what}: Y differs from round_bf16(gemm)"
    assert (pre is None) == (prec is None)
    if pre is not None:
        assert pre.dtype == F32 and same_bits(pre, prec), f"{what}: pre differs from the fp32 launch's"
    return Y, pre


ACT_F64 = {
    None: lambda x: x,
    "relu": lambda x: x.clamp_min(0),
    "leaky": lambda x: torch.where(x > 0, x, 0.01 * x),
    "selu": lambda x: torch.nn.functional.selu(x),
}


def grad_f64(pre, act):
    """act'(pre) in fp64 at the fp32 pre-activation (the side of zero is decided by the stored value, as in the kernels)."""
    p = pre.double()
    if act == "relu":
        return (p > 0).double()
    if act == "leaky":
        return torch.where(p > 0, 1.0, 0.01).double()
    if act == "selu":
        scale, alpha = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717
        return torch.where(p > 0, scale, scale * alpha * torch.exp(p.clamp_max(0)))
    return torch.ones_like(p)


# ------------------------------------------------------------------------------------- 1. forward, both routes
@pytest.mark.parametrize("Nf", NF_X3)
@pytest.mark.parametrize("K", K_X3)
def test_forward_x3_route_is_bitwise_the_composition(K, Nf):
    Amax, W = randn((1, 200, K), 10 + K + Nf), randn((K, Nf), 20 + K + Nf) * 0.3
    for R in (1, 63, 64, 65, 200):                                          # the 64-row tile and its edges
        A = Amax[:, :R].contiguous()
        for act in ACTS:
            Y, pre = check_forward(A, W, act, f"K={K} Nf={Nf} R={R} act={act}")
    ref_pre = A.double() @ W.double()                                       # R = 200, selu: the suite's own bound
    assert_close(pre, ref_pre, REL_TOL, f"pre K={K} Nf={Nf}")
    assert_bf16_close(Y, ACT_F64["selu"](ref_pre), f"Y K={K} Nf={Nf}")


@pytest.mark.parametrize("Nf", NF_SM)
@pytest.mark.parametrize("K", K_SM)
def test_forward_small_route_is_bitwise_the_composition(K, Nf):
    Amax, W = randn((1, 700, K), 30 + K + Nf), randn((K, Nf), 40 + K + Nf) * 0.5
    for R in (1, 255, 256, 257, 700):                                       # the 256-row block and its edges
        A = Amax[:, :R].contiguous()
        for act in ACTS:
            Y, pre = check_forward(A, W, act, f"K={K} Nf={Nf} R={R} act={act}")
    ref_pre = A.double() @ W.double()
    assert_close(pre, ref_pre, REL_TOL, f"pre K={K} Nf={Nf}")
    assert_bf16_close(Y, ACT_F64["selu"](ref_pre), f"Y K={K} Nf={Nf}")


@pytest.mark.parametrize("K,Nf,T,N", [(20, 24, 3, 50), (128, 128, 3, 50), (2, 16, 3, 100), (6, 64, 3, 100)])
def test_forward_per_slice_weights(K, Nf, T, N):
    """One weight per slice with batches that end inside a 64-row tile (N = 50) / inside a 256-row block (N = 100)."""
    A, W = randn((T, N, K), 50 + K), randn((T, K, Nf), 51 + K) * 0.3
    for act in ACTS:
        Y, _ = check_forward(A, W, act, f"per-slice K={K} Nf={Nf} act={act}")
    assert_bf16_close(Y, ACT_F64["selu"](torch.einsum("tnk,tkf->tnf", A.double(), W.double())), f"per-slice K={K} Nf={Nf}")


def test_forward_blocks_take_several_tiles():
    """More 64-row tiles than the persistent grid holds, so blocks walk their tile list and both staging sets turn over."""
    R, K, Nf = 100_003, 128, 128
    A, W = randn((1, R, K), 60), randn((K, Nf), 61) * 0.1
    check_forward(A, W, "leaky", "R=100003")


def _raw_forward(A, W, act, Y, pre):
    """tmgcn_gemm_bf16y on caller-provided (views of) outputs: the torch operator always allocates aligned ones."""
    T, N, K = A.shape
    rc = _lib.load().tmgcn_gemm_bf16y(ops._ptr(A), ops._ptr(W), C.c_void_p(Y.data_ptr()), ops._ptr(pre), T * N, K, W.shape[-1],
                                      N if W.dim() == 3 else 0, K * W.shape[-1] if W.dim() == 3 else 0, _lib.ACT_IDS[act],
                                      ops._stream(A))
    assert rc == 0, _lib.load().tmgcn_last_error()


@pytest.mark.parametrize("K,Nf,R", [(20, 24, 130), (128, 128, 65), (2, 16, 300), (6, 40, 300)])
@pytest.mark.parametrize("shift_y,shift_pre", [(1, 0), (0, 1), (2, 0)], ids=["Y+2B", "pre+4B", "Y+4B"])
def test_forward_misaligned_outputs_take_the_scalar_epilogue(K, Nf, R, shift_y, shift_pre):
    """A Y that is not 8-byte aligned (or a pre that is not 16-byte aligned) cannot leave through the vector stores: the
    element-wise epilogue must write the same bits, and nothing outside the views."""
    A, W = randn((1, R, K), 70 + K), randn((K, Nf), 71 + K) * 0.3
    Yc, prec = fwd_composition(A, W, "selu")
    ybuf = torch.full((R * Nf + 16,), 7.0, dtype=BF16, device=DEV)
    pbuf = torch.full((R * Nf + 16,), 7.0, dtype=F32, device=DEV)
    Y = ybuf[shift_y:shift_y + R * Nf].view(1, R, Nf)
    pre = pbuf[shift_pre:shift_pre + R * Nf].view(1, R, Nf)
    _raw_forward(A, W, "selu", Y, pre)
    assert same_bits(Y, Yc) and same_bits(pre, prec)
    assert bool((ybuf[:shift_y] == 7).all()) and bool((ybuf[shift_y + R * Nf:] == 7).all())
    assert bool((pbuf[:shift_pre] == 7).all()) and bool((pbuf[shift_pre + R * Nf:] == 7).all())


# ------------------------------------------------------------------------------------- 2. rounding
@pytest.mark.parametrize("K,Nf", [(16, 16), (2, 16)], ids=["x3", "small"])
def test_rounding_is_to_nearest_even_and_specials_survive(K, Nf):
    R = 8
    A = torch.zeros(1, R, K)
    W = torch.zeros(K, Nf)
    A[0, :, 0] = 1.0
    W[0, 0], W[0, 1], W[0, 2], W[0, 3] = 257.0, 259.0, -257.0, -259.0        # ties at a bf16 ulp of 2: to the even neighbour
    W[0, 4], W[0, 5] = 4.0, -4.0
    A[0, 1, 0] = 2.0 ** 127                                                  # 2^127 · ±4 overflows fp32
    A[0, 2, 0] = float("nan")
    Y, _ = check_forward(A.to(DEV), W.to(DEV), None, f"rounding K={K}")
    Y = Y.cpu().float()
    assert Y[0, 0, :4].tolist() == [256.0, 260.0, -256.0, -260.0]
    assert Y[0, 1, 4] == float("inf") and Y[0, 1, 5] == float("-inf")
    assert bool(torch.isnan(Y[0, 2, :6]).all())
    assert Y[0, 3, :6].tolist() == [256.0, 260.0, -256.0, -260.0, 4.0, -4.0]


# ------------------------------------------------------------------------------------- 3. dW, both routes
def dw_composition(A, dYb, pre, act, per_slice):
    dY = dYb.float()                                                        # exact
    if act is not None:
        dY = ops.kernels.act_bwd(pre, dY, act)
    return ops.kernels.gemm_dw(A, dY, per_slice)


def pre_tensor(shape, seed):
    """Pre-activations on both sides of zero, some exactly 0 and -0."""
    p = randn(shape, seed)
    flat = p.view(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    return p


def check_dw(A, dYb, pre, act, per_slice, what):
    got = ops.kernels.gemm_dw(A, dYb, per_slice, pre=pre if act is not None else None, act=act)
    want = dw_composition(A, dYb, pre, act, per_slice)
    assert got.dtype == F32 and same_bits(got, want), f"{what}: dW differs from gemm_dw(act_bwd(widen(dY)))"
    return got


@pytest.mark.parametrize("Nf", NF_X3)
@pytest.mark.parametrize("K", K_X3)
def test_dw_x3_route_is_bitwise_the_composition(K, Nf):
    Amax, dmax, pmax = randn((1, 1000, K), 80 + K + Nf), randn((1, 1000, Nf), 81 + K + Nf, BF16), pre_tensor((1, 1000, Nf), 82 + K + Nf)
    for R in (1, 31, 32, 33, 127, 129, 1000):                               # steps of 32 rows, a flush every 128
        A, dY, pre = Amax[:, :R].contiguous(), dmax[:, :R].contiguous(), pmax[:, :R].contiguous()
        for act in ACTS:
            dW = check_dw(A, dY, pre, act, False, f"K={K} Nf={Nf} R={R} act={act}")
    ref = A[0].double().T @ (dY[0].double() * grad_f64(pre[0], "selu"))     # R = 1000, selu
    assert_close(dW, ref, REL_TOL, f"dW K={K} Nf={Nf}")


@pytest.mark.parametrize("Nf", NF_SM)
@pytest.mark.parametrize("K", K_SM)
def test_dw_small_route_is_bitwise_the_composition(K, Nf):
    Amax, dmax, pmax = randn((1, 1000, K), 90 + K + Nf), randn((1, 1000, Nf), 91 + K + Nf, BF16), pre_tensor((1, 1000, Nf), 92 + K + Nf)
    for R in (1, 31, 32, 33, 127, 129, 1000):
        A, dY, pre = Amax[:, :R].contiguous(), dmax[:, :R].contiguous(), pmax[:, :R].contiguous()
        for act in ACTS:
            dW = check_dw(A, dY, pre, act, False, f"K={K} Nf={Nf} R={R} act={act}")
    ref = A[0].double().T @ (dY[0].double() * grad_f64(pre[0], "selu"))
    assert_close(dW, ref, REL_TOL, f"dW K={K} Nf={Nf}")


@pytest.mark.parametrize("K,Nf,T,N", [(20, 24, 3, 50), (128, 128, 3, 75), (2, 16, 3, 100), (15, 64, 3, 45)])
def test_dw_per_slice_weights(K, Nf, T, N):
    """One dW per slice, N no multiple of the 32-row step: every slice ends in a tail step that re-reads its last row."""
    A, dY, pre = randn((T, N, K), 100 + K), randn((T, N, Nf), 101 + K, BF16), pre_tensor((T, N, Nf), 102 + K)
    for act in ACTS:
        dW = check_dw(A, dY, pre, act, True, f"per-slice K={K} Nf={Nf} act={act}")
    assert dW.shape == (T, K, Nf)
    ref = torch.einsum("tnk,tnf->tkf", A.double(), dY.double() * grad_f64(pre, "selu"))
    assert_close(dW, ref, REL_TOL, f"per-slice dW K={K} Nf={Nf}")


@pytest.mark.parametrize("K,Nf", [(32, 24), (2, 16), (4, 8)], ids=["split", "small", "narrow"])
def test_dw_of_no_rows_is_each_entry_points_own_rule(K, Nf):
    """R = 0 through the one dW launcher: tmgcn_gemm_dw_f32 and tmgcn_gemm_dw_act_f32 zero-fill the dW they are given and
    return OK; tmgcn_gemm_dw_act_bf16 returns OK and leaves dW as it is (the operator allocates zeros instead)."""
    lib = _lib.load()
    dW = torch.full((K, Nf), 7.0, device=DEV)
    ws = torch.empty(64, dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if lib.tmgcn_gemm_bf16y_supported(K, Nf):
        assert lib.tmgcn_gemm_dw_act_bf16(None, None, None, 0, dW.data_ptr(), 0, K, Nf, 0, ws.data_ptr(), ws.numel(), st) == 0
        torch.cuda.synchronize()
        assert bool((dW == 7.0).all())
    if lib.tmgcn_gemm_dw_act_supported(K, Nf):
        assert lib.tmgcn_gemm_dw_act_f32(None, None, ws.data_ptr(), 3, dW.data_ptr(), 0, K, Nf, 0, None, 0, st) == 0
        torch.cuda.synchronize()
        assert bool((dW == 0).all())
        dW.fill_(7.0)
    assert lib.tmgcn_gemm_dw_f32(None, None, dW.data_ptr(), 0, K, Nf, 0, 0, None, 0, st) == 0
    torch.cuda.synchronize()
    assert bool((dW == 0).all())
    A, dY = torch.empty(2, 0, K, device=DEV), torch.empty(2, 0, Nf, device=DEV)
    got = ops.kernels.gemm_dw(A, dY, False)
    assert got.shape == (K, Nf) and not bool(got.any())
    for per_slice, shape in ((False, (K, Nf)), (True, (2, K, Nf))):
        if lib.tmgcn_gemm_bf16y_supported(K, Nf):
            got = ops.kernels.gemm_dw(A, dY.to(BF16), per_slice)
            assert got.shape == shape and got.dtype == F32 and not bool(got.any())


def test_dw_long_chunks_run_the_ring_and_the_flush():
    """Enough rows per chunk for the steady-state loop (unconditional loads, a flush every four steps) and its drain."""
    R, K, Nf = 40_000, 128, 128
    A, dY, pre = randn((1, R, K), 110), randn((1, R, Nf), 111, BF16), pre_tensor((1, R, Nf), 112)
    for act in (None, "selu"):
        check_dw(A, dY, pre, act, False, f"R={R} act={act}")


# ------------------------------------------------------------------------------------- 4. autograd
def _autograd_case(K=20, Nf=24, T=3, N=50, per_slice=False):
    A = randn((T, N, K), 120 + K)
    W = randn((T, K, Nf) if per_slice else (K, Nf), 121 + K) * 0.3
    g = randn((T, N, Nf), 122 + K, BF16)
    return A, W, g


def _run(fn, A, W, g, act, a_grad):
    A2, W2 = A.clone().requires_grad_(a_grad), W.clone().requires_grad_()
    Y = fn(A2, W2, act)
    Y.backward(g)
    return Y.detach(), W2.grad, A2.grad


def _fused_op(A, W, act):
    return ops.feature_gemm(A, W, act=act, out_dtype=BF16)


def _composed_op(A, W, act):
    return ops.round_bf16(ops.feature_gemm(A, W, act=act))


@pytest.mark.parametrize("a_grad", [False, True], ids=["dW_only", "dA_and_dW"])
@pytest.mark.parametrize("K,Nf,per_slice", [(20, 24, False), (128, 128, True), (2, 16, False), (6, 64, True)])
def test_autograd_equals_the_composition(K, Nf, per_slice, a_grad):
    assert ops.gemm_bf16y_fused(K, Nf)
    A, W, g = _autograd_case(K, Nf, per_slice=per_slice)
    for act in ACTS:
        Y, dW, dA = _run(_fused_op, A, W, g, act, a_grad)
        Yc, dWc, dAc = _run(_composed_op, A, W, g, act, a_grad)
        assert Y.dtype == BF16 and same_bits(Y, Yc), act
        assert dW.dtype == F32 and same_bits(dW, dWc), act
        assert (dA is None) == (not a_grad)
        if a_grad:
            assert same_bits(dA, dAc), act


def test_autograd_takes_an_fp32_gradient():
    A, W, g = _autograd_case()
    gf = randn(tuple(g.shape), 131)                                         # not representable in bf16
    Y, dW, _ = _run(_fused_op, A, W, gf, "selu", False)
    Yc, dWc, _ = _run(_composed_op, A, W, gf, "selu", False)
    assert same_bits(Y, Yc) and same_bits(dW, dWc)


def test_autograd_with_a_bf16_stored_weight():
    """A parameter stored in bf16 keeps the composition (the bf16-Y kernel reads an fp32 W): same Y, dW rounded once."""
    A, W, g = _autograd_case()
    Wb = W.bfloat16()
    Y, dW, _ = _run(_fused_op, A, Wb, g, "selu", False)
    Yc, dWc, _ = _run(_composed_op, A, Wb, g, "selu", False)
    assert Y.dtype == BF16 and dW.dtype == BF16
    assert same_bits(Y, Yc) and same_bits(dW, dWc)


def test_unsupported_widths_keep_the_composition():
    A, W, g = _autograd_case(K=18, Nf=24)                                   # K no multiple of 4: the exact-f32 MFMA route
    assert not ops.gemm_bf16y_fused(18, 24)
    Y, dW, _ = _run(_fused_op, A, W, g, "relu", False)
    Yc, dWc, _ = _run(_composed_op, A, W, g, "relu", False)
    assert same_bits(Y, Yc) and same_bits(dW, dWc)
    with pytest.raises(RuntimeError, match="bf16-Y"):
        ops.kernels.gemm(A, W, out_dtype=BF16)


@pytest.mark.parametrize("K,Nf", [(20, 24), (2, 16)])
def test_autograd_under_a_kernel_timer_takes_the_two_tagged_launches(K, Nf):
    A, W, g = _autograd_case(K, Nf)
    Yc, dWc, _ = _run(_composed_op, A, W, g, "selu", False)
    ops.kernels.timer = ops.KernelTimer()
    try:
        Y, dW, _ = _run(_fused_op, A, W, g, "selu", False)
        tags = ops.kernels.timer.summary()
    finally:
        ops.kernels.timer = None
    assert same_bits(Y, Yc) and same_bits(dW, dWc)
    assert set(tags) == {"gemm_bf16y", "gemm_dw_act_bf16"}, tags          # no gemm, no act_bwd, no cast
    assert tags["gemm_bf16y"]["launches"] == 1 and tags["gemm_dw_act_bf16"]["launches"] == 1


def test_no_fp32_temporary():
    """The fused forward allocates the bf16 Y and the fp32 pre only: the peak rises by less than the 4 + 4 + 2 bytes per
    element of the composition (fp32 Y, fp32 pre, bf16 Y)."""
    A, W, _ = _autograd_case(128, 128, T=4, N=4096)
    n = A.shape[0] * A.shape[1] * W.shape[-1]
    with torch.no_grad():
        ops.feature_gemm(A, W, act="selu", out_dtype=BF16)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        Y = ops.feature_gemm(A, W, act="selu", out_dtype=BF16)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
    assert Y.dtype == BF16
    assert rise < 10 * n, f"peak rose by {rise} B; the composition needs {10 * n} B"


def test_graph_capture_replays_the_eager_bits():
    A, W, g = _autograd_case()
    Wp = W.clone().requires_grad_()

    def step():
        Wp.grad = None
        Y = ops.feature_gemm(A, Wp, act="selu", out_dtype=BF16)
        Y.backward(g)
        return Y

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Y = step()
        eager = (Y.detach().clone(), Wp.grad.clone())
    torch.cuda.current_stream().wait_stream(side)
    Wp.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Yg = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert same_bits(Yg.detach(), eager[0]) and same_bits(Wp.grad, eager[1])


# ------------------------------------------------------------------------------------- 5. model, default branch
@pytest.fixture(scope="module")
def graph_data():
    g = synth.dynamic_graph(T=4, N=200, edges_per_slice=300, seed=1, no_diag=2)
    return (g.At_list(), torch.from_numpy(g.X), torch.from_numpy(g.M), torch.from_numpy(g.edges),
            torch.from_numpy(g.labels).to(DEV))


@pytest.mark.parametrize("nonlin", ["relu", "leaky", "selu"])
@pytest.mark.parametrize("condensed", [True, False], ids=["shared_W", "per_slice_W"])
@pytest.mark.parametrize("hidden", [[16, 16, 2], [64, 128, 2]], ids=["16x16", "64x128"])
def test_model_default_branch_has_no_cast_launch_and_keeps_the_bits(graph_data, hidden, condensed, nonlin, monkeypatch):
    """EmbeddingGCN2(act_dtype=bf16) in the as-run default branch (no M in front of layer 2): the model runs with
    ops.round_bf16 raising, and logits and gradients are bit for bit those of feature_gemm + round_bf16 +
    spmm_feature_gemm on the same parameters."""
    import tmgcn_amd.layers as ehf
    At, X, M, edges, labels = graph_data
    crit = torch.nn.CrossEntropyLoss(weight=torch.tensor([0.9, 0.1], device=DEV))
    torch.manual_seed(0)
    m = ehf.EmbeddingGCN2(At, X, edges, M, hidden_feat=hidden, condensed_W=condensed, use_Minv=False, nonlin2=nonlin, device=DEV,
                          act_dtype=BF16)
    assert ops.gemm_bf16y_fused(m.AtXt.shape[-1], hidden[0])

    def no_cast(x):
        raise AssertionError("the model still casts with ops.round_bf16 in front of layer 2")

    with monkeypatch.context() as mp:
        mp.setattr(ops, "round_bf16", no_cast)
        logits = m()
        crit(logits, labels).backward()
    got = {"logits": logits.detach().clone(), **{n: p.grad.clone() for n, p in m.named_parameters()}}

    P = {n: p.detach().clone().requires_grad_() for n, p in m.named_parameters()}
    Y = ops.round_bf16(ops.feature_gemm(m.AtXt, P["W1"], act=nonlin))
    Z = ops.spmm_feature_gemm(m.At, Y, P["W2"])
    ref_logits = m._head(Z, m._edges, P["U"])
    crit(ref_logits, labels).backward()
    assert same_bits(got["logits"], ref_logits.detach())
    for n, p in P.items():
        assert same_bits(got[n], p.grad), n
