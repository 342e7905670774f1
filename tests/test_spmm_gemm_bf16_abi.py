"""CPU: the host side of the bf16-stored fused SpMM+GEMM — the domain query, the argument checks of the C entry point
(every case returns before anything is launched, so no GPU is needed), the dtype rules of ops.spmm_feature_gemm and
the bf16 error-bound helper the GPU tests use."""
import ctypes as C

import pytest
import torch

from _bf16_bound import assert_bf16_close, bf16_excess
from _util import load_c_oracle, cptr
from tmgcn_amd import _lib, ops

INVALID = -1   # TMGCN_ERR_INVALID


def test_supported_is_exactly_the_documented_domain():
    lib = _lib.load()
    for K in list(range(-8, 140)) + [136, 144, 256]:
        for Nf in (-1, 0, 1, 2, 7, 8, 16, 127, 128, 129, 256):
            want = 1 if (K % 8 == 0 and 16 <= K <= 128 and 1 <= Nf <= 128) else 0
            assert lib.tmgcn_spmm_gemm_bf16_supported(K, Nf) == want, (K, Nf)
    assert ops.kernels.spmm_gemm_bf16_supported(64, 64) and not ops.kernels.spmm_gemm_bf16_supported(8, 8)


def _call(**over):
    """tmgcn_spmm_gemm_bf16 on made-up, never dereferenced, 16-byte aligned addresses; `over` replaces arguments."""
    a = dict(rowptr=0x1000, col=0x2000, val=0x3000, X=0x4000, n_rows=128, N=64, K=64, W=0x5000, Nf=32, trans_w=0,
             rows_per_batch=0, w_batch_stride=0, act=0, Y=0x6000, y_bf16=0, AX=0x7000, pre=0x8000, grid_reserve=0, avg=-1.0,
             stream=None)
    a.update(over)
    order = ("rowptr", "col", "val", "X", "n_rows", "N", "K", "W", "Nf", "trans_w", "rows_per_batch", "w_batch_stride", "act", "Y",
             "y_bf16", "AX", "pre", "grid_reserve", "avg", "stream")
    return _lib.load().tmgcn_spmm_gemm_bf16(*(a[k] for k in order))


@pytest.mark.parametrize("over", [
    dict(K=8), dict(K=20), dict(K=136), dict(K=0), dict(Nf=0), dict(Nf=129),           # widths outside the domain
    dict(rowptr=None), dict(X=None), dict(W=None), dict(Y=None),                       # NULL operands
    dict(X=0x4002), dict(X=0x4008), dict(AX=0x7004), dict(Y=0x6008),                   # not 16-byte aligned
    dict(y_bf16=2), dict(y_bf16=-1),
    dict(act=9), dict(N=0), dict(n_rows=100), dict(grid_reserve=-1), dict(rows_per_batch=-1),
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_invalid_arguments_are_refused_without_a_launch(over):
    assert _call(**over) == INVALID
    assert len(_lib.load().tmgcn_last_error()) > 0


def test_out_dtype_rules_of_the_python_operator():
    X, W = torch.zeros(1, 4, 16), torch.zeros(16, 16)
    with pytest.raises(RuntimeError, match="bf16"):
        ops.spmm_feature_gemm(None, X, W, out_dtype=torch.bfloat16)           # fp32 X: an fp32 Y only
    with pytest.raises(RuntimeError, match="out_dtype"):
        ops.spmm_feature_gemm(None, X, W, out_dtype=torch.float16)
    with pytest.raises(RuntimeError, match="K=12, Nf=16"):                     # bf16 X outside the domain: named, not widened
        ops.spmm_feature_gemm(None, torch.zeros(1, 4, 12, dtype=torch.bfloat16), torch.zeros(12, 16))
    with pytest.raises(RuntimeError, match="K=16, Nf=200"):
        ops.spmm_feature_gemm(None, torch.zeros(1, 4, 16, dtype=torch.bfloat16), torch.zeros(16, 200))


def test_bf16_bound_helper_on_the_oracles_own_output():
    """The oracle's product rounded to bf16 once lies inside the bound (with room: the fp32 term is unused); a value moved
    by two more bf16 steps, and an fp32 tensor passed where bf16 is expected, are caught."""
    lib = load_c_oracle()
    g = torch.Generator().manual_seed(11)
    A, W = torch.randn(1, 300, 64, generator=g), torch.randn(64, 48, generator=g)
    ref = torch.empty(1, 300, 48)
    lib.ref_gemm(cptr(A), cptr(W), cptr(ref), 300, 64, 48, 0, 0, 0)
    got = ref.bfloat16()
    assert bf16_excess(got, ref) <= 1.0
    assert_bf16_close(got, ref, "oracle output rounded once")
    # half a bf16 unit is reached for values just above a power of two: the bound is not slack by a factor of two
    x = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20])
    assert 0.9 < bf16_excess(x.bfloat16(), x) <= 1.0
    off = got.clone()
    i = int(ref.abs().flatten().argmax())
    off.view(-1)[i] = off.view(-1)[i] * (1 + 2.0 ** -6)                        # two units in the last place
    assert bf16_excess(off, ref) > 1.0
    with pytest.raises(AssertionError):
        assert_bf16_close(off, ref)
    with pytest.raises(AssertionError, match="bf16"):
        assert_bf16_close(ref, ref)
