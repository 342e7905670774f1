"""GPU: the band M-transform on bf16-stored operands (csrc/mtransform_bf16.hip) through the kernel launcher, ops.m_transform
with autograd, hipGraph capture and EmbeddingGCN2(act_dtype=bf16).

The bar is BIT equality with the composition the fused launch replaces: a bf16 X is widened exactly, every output element
is the fp32 band kernel's value (the same taps in the same order through fmaf), a bf16 Y is that value rounded to nearest
even once — so  fused(X) == round_bf16(mtransform(widen(X)))  needs no tolerance.  The fp32-stored outputs are also held
against the C oracle at REL_TOL and the bf16-stored ones at the bound of tests/_bf16_bound.py."""
import pytest
import torch

from _bf16_bound import assert_bf16_close
from _util import REL_TOL, assert_close, cptr, load_c_oracle
from tmgcn_amd import ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
FORMS = [(F32, BF16), (BF16, F32), (BF16, BF16)]           # (X stored as, Y stored as)


def band_op(T, b):
    M = torch.from_numpy(synth.band_M(T, b, "matlab")).contiguous()
    return M, ops.MOperator(M, DEV)


def ref_mt(M64, X, transpose=False):
    lib = load_c_oracle()
    T = X.shape[0]
    Y = torch.empty_like(X)
    lib.ref_mtransform(cptr(M64), T, int(transpose), cptr(X), cptr(Y), X.numel() // T)
    return Y


def composition(op, X, y_dtype, **kw):
    """The launches the fused one replaces: widen (exact), the fp32 transform, one rounding."""
    Y = ops.kernels.mtransform(op, X.float(), **kw)
    return ops.round_bf16(Y) if y_dtype is BF16 else Y


def randn(shape, seed, dtype=F32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


# ------------------------------------------------------------------------------------- 1. bits against the composition
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("N,F", [(37, 2), (64, 16), (11, 3)])          # C = 74, 33: one column per lane; 1024: four
@pytest.mark.parametrize("T,b", [(1, 1), (5, 3), (34, 20), (95, 20), (600, 3)])   # 34, 95: row chunks; 600: two tap tables
def test_fused_launch_is_bitwise_the_composition(T, b, N, F, transpose):
    M, op = band_op(T, b)
    assert ops.m_transform_bf16_fused(op)
    X = randn((T, N, F), 100 + T + N)
    refs = {}
    for x_dtype, y_dtype in FORMS:
        Xs = X.to(x_dtype)                                               # what is stored; widening it back is exact
        Xd = Xs.to(DEV)
        got = ops.kernels.mtransform(op, Xd, transpose=transpose, out_dtype=y_dtype)
        assert got.dtype == y_dtype and got.shape == Xd.shape
        assert torch.equal(got, composition(op, Xd, y_dtype, transpose=transpose)), (x_dtype, y_dtype)
        if x_dtype not in refs:
            refs[x_dtype] = ref_mt(M, Xs.float(), transpose)
        if y_dtype is BF16:
            assert_bf16_close(got, refs[x_dtype], f"T={T} b={b} {x_dtype}->{y_dtype}")
        else:
            assert_close(got, refs[x_dtype], REL_TOL, f"T={T} b={b} {x_dtype}->{y_dtype}")


# ------------------------------------------------------------------------------------- 2. row window
def test_windowed_rows():
    """row/col offsets as in test_gpu_kernels.py::test_mtransform_windowed_rows: a slab of the output rows, fp32 -> bf16."""
    T, N, F = 24, 40, 4
    M, op = band_op(T, 6)
    Xd = randn((T, N, F), 9).to(DEV)
    part = ops.kernels.mtransform(op, Xd, row_off=8, col_off=0, T_out=8, out_dtype=BF16)
    assert part.shape == (8, N, F) and part.dtype == BF16
    assert torch.equal(part, composition(op, Xd, BF16, row_off=8, col_off=0, T_out=8))
    assert_bf16_close(part, ref_mt(M, Xd.cpu())[8:16], "row window")
    # the adjoint of that window on a bf16 gradient, written in fp32
    dY = randn((8, N, F), 10, BF16).to(DEV)
    dX = ops.kernels.mtransform(op, dY, transpose=True, row_off=0, col_off=8, T_out=T, out_dtype=F32)
    assert torch.equal(dX, composition(op, dY, F32, transpose=True, row_off=0, col_off=8, T_out=T))


# ------------------------------------------------------------------------------------- 3. misaligned base
@pytest.mark.parametrize("x_dtype,y_dtype", FORMS, ids=["f32->bf16", "bf16->f32", "bf16->bf16"])
def test_misaligned_base_gives_the_aligned_bits(x_dtype, y_dtype):
    """An X that starts one element (2 bytes bf16 / 4 bytes fp32) off its 16-byte aligned allocation takes the
    one-column-per-lane form: the same bits as the aligned call, which takes four."""
    T, N, F = 34, 64, 16
    _, op = band_op(T, 20)
    X = randn((T, N, F), 21, x_dtype).to(DEV)
    buf = torch.zeros(X.numel() + 8, dtype=x_dtype, device=DEV)
    Xo = buf[1:1 + X.numel()].view(T, N, F)
    Xo.copy_(X)
    assert X.data_ptr() % 16 == 0 and Xo.data_ptr() % 16 == X.element_size() and Xo.is_contiguous()
    for transpose in (False, True):
        assert torch.equal(ops.kernels.mtransform(op, Xo, transpose=transpose, out_dtype=y_dtype),
                           ops.kernels.mtransform(op, X, transpose=transpose, out_dtype=y_dtype))


# ------------------------------------------------------------------------------------- 4. dense operator
def test_dense_operator_composes_the_fp32_transform_and_the_casts():
    T, N, F = 40, 64, 16
    _, op = band_op(T, 40)
    assert not ops.m_transform_bf16_fused(op)
    X = randn((T, N, F), 31).to(DEV)
    assert torch.equal(ops.m_transform(X, op, out_dtype=BF16), composition(op, X, BF16))
    Xb = X.bfloat16()
    assert torch.equal(ops.m_transform(Xb, op), composition(op, Xb, F32))
    assert torch.equal(ops.m_transform(Xb, op, out_dtype=BF16), composition(op, Xb, BF16))
    with pytest.raises(RuntimeError, match="band"):                      # the kernel-level launcher has the band kernel only
        ops.kernels.mtransform(op, X, out_dtype=BF16)


# ------------------------------------------------------------------------------------- 5. autograd
def _autograd_case():
    T, N, F = 34, 64, 16
    _, op = band_op(T, 20)
    return op, randn((T, N, F), 41).to(DEV), randn((T, N, F), 42, BF16).to(DEV)


def test_autograd_runs_the_transposed_product_on_the_gradients_dtype():
    op, X, g = _autograd_case()
    want = ops.kernels.mtransform(op, g.float(), transpose=True)          # fp32 Mᵀ on the widened bf16 gradient
    Xf = X.clone().requires_grad_()
    Y = ops.m_transform(Xf, op, out_dtype=BF16)
    assert Y.dtype == BF16 and torch.equal(Y, composition(op, X, BF16))
    Y.backward(g)
    assert Xf.grad.dtype == F32 and torch.equal(Xf.grad, want)
    Xb = X.bfloat16().requires_grad_()
    ops.m_transform(Xb, op, out_dtype=BF16).backward(g)
    assert Xb.grad.dtype == BF16 and torch.equal(Xb.grad, ops.round_bf16(want))
    # an fp32 result of a bf16 X: the fp32 gradient is rounded once into X's dtype
    Xb2 = X.bfloat16().requires_grad_()
    gf = g.float()
    ops.m_transform(Xb2, op).backward(gf)
    assert Xb2.grad.dtype == BF16 and torch.equal(Xb2.grad, ops.round_bf16(want))


def test_autograd_under_a_kernel_timer_takes_the_tagged_launches():
    """With a KernelTimer attached the operator runs through the Python autograd function: the same bits, and the launches
    show up under mtransform_bf16 / mtransform_bf16_T."""
    op, X, g = _autograd_case()
    want = ops.kernels.mtransform(op, g.float(), transpose=True)
    ops.kernels.timer = ops.KernelTimer()
    try:
        Xf = X.clone().requires_grad_()
        Y = ops.m_transform(Xf, op, out_dtype=BF16)
        Y.backward(g)
        tags = ops.kernels.timer.summary()
    finally:
        ops.kernels.timer = None
    assert torch.equal(Y, composition(op, X, BF16)) and torch.equal(Xf.grad, want)
    assert tags["mtransform_bf16"]["launches"] == 1 and tags["mtransform_bf16_T"]["launches"] == 1
    assert "mtransform" not in tags and "mtransform_T" not in tags


# ------------------------------------------------------------------------------------- 6. no fp32 temporary
def test_no_fp32_temporary():
    """The fused launch allocates its bf16 result only: the peak rises by less than the fp32 [T, N, F] tensor that the
    composition needs for the transform's result."""
    T, N, F = 24, 512, 64
    _, op = band_op(T, 20)
    X = randn((T, N, F), 51).to(DEV)
    with torch.no_grad():
        ops.m_transform(X, op, out_dtype=BF16)                           # warm-up: library, operator lookup
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        Y = ops.m_transform(X, op, out_dtype=BF16)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
    assert Y.dtype == BF16
    assert rise < 4 * X.numel(), f"peak rose by {rise} B; an fp32 temporary is {4 * X.numel()} B"


# ------------------------------------------------------------------------------------- 7. graph capture
def test_graph_capture_replays_the_eager_bits():
    op, X, g = _autograd_case()
    Xf = X.clone().requires_grad_()

    def step():
        Xf.grad = None
        Y = ops.m_transform(Xf, op, out_dtype=BF16)
        Y.backward(g)
        return Y

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Y = step()
        eager = (Y.detach().clone(), Xf.grad.clone())
    torch.cuda.current_stream().wait_stream(side)
    Xf.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Yg = step()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(Yg, eager[0]) and torch.equal(Xf.grad, eager[1])


# ------------------------------------------------------------------------------------- 8. model, through the fused path
@pytest.mark.parametrize("branch", [dict(use_Minv=False, apply_M_twice=True), dict(use_Minv=True)], ids=["M_twice", "Minv"])
def test_model_takes_the_fused_path_and_keeps_the_bits(branch, monkeypatch):
    """EmbeddingGCN2(act_dtype=bf16) in the branches with an M product in front of layer 2: no cast launch is left (the
    model runs with ops.round_bf16 raising), and logits and gradients are bit for bit those of the two-launch path
    (fp32 M-transform, then round_bf16), restated here from the operators on the same parameters."""
    import tmgcn_amd.layers as ehf
    g = synth.dynamic_graph(T=4, N=200, edges_per_slice=300, seed=1, no_diag=2)
    At, X, M = g.At_list(), torch.from_numpy(g.X), torch.from_numpy(g.M)
    edges, labels = torch.from_numpy(g.edges), torch.from_numpy(g.labels).to(DEV)
    crit = torch.nn.CrossEntropyLoss(weight=torch.tensor([0.9, 0.1], device=DEV))
    torch.manual_seed(0)
    m = ehf.EmbeddingGCN2(At, X, edges, M, hidden_feat=[16, 16, 2], condensed_W=True, nonlin2="selu", device=DEV, act_dtype=BF16,
                          **branch)
    assert ops.m_transform_bf16_fused(m.Mop)

    def no_cast(x):
        raise AssertionError("the model still casts with ops.round_bf16 in front of layer 2")

    with monkeypatch.context() as mp:
        mp.setattr(ops, "round_bf16", no_cast)
        logits = m()
        crit(logits, labels).backward()
    got = {"logits": logits.detach().clone(), **{n: p.grad.clone() for n, p in m.named_parameters()}}

    # the two-launch path on the same parameters (ops.round_bf16 is itself again)
    P = {n: p.detach().clone().requires_grad_() for n, p in m.named_parameters()}
    if branch.get("use_Minv"):
        Y = ops.activation(ops.m_transform(ops.feature_gemm(m.AtXt, P["W1"]), m.Minv), "selu")
    else:
        Y = ops.feature_gemm(m.AtXt, P["W1"], act="selu")
    Z = ops.spmm_feature_gemm(m.At, ops.round_bf16(ops.m_transform(Y, m.Mop)), P["W2"])
    if branch.get("use_Minv"):
        Z = ops.m_transform(Z, m.Minv)
    ref_logits = m._head(Z, m._edges, P["U"])
    crit(ref_logits, labels).backward()
    assert torch.equal(got["logits"], ref_logits.detach())
    for n, p in P.items():
        assert torch.equal(got[n], p.grad), n
