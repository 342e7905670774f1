"""The error bound of an output that the bf16-stored fused SpMM+GEMM writes in bf16 (Y with out_dtype=bf16, dX), shared
by tests/test_gpu_spmm_gemm_bf16.py and tests/test_spmm_gemm_bf16_abi.py.

Derivation.  The kernel forms the fp32 value y and stores got = rne_bf16(y).  The project's bar for the fp32 value is
|y - ref| <= eps * M with eps = REL_TOL = 1e-5 and M = max|ref|.  bf16 keeps 8 significant bits, so round-to-nearest-even
moves y by at most half a unit in the last place: |got - y| <= 2^-8 * |y|.  Hence, per element,

    |got - ref| <= |got - y| + |y - ref| <= 2^-8 * (|ref| + eps * M) + eps * M = 2^-8 * |ref| + (1 + 2^-8) * eps * M.

Nothing in it comes from a run: it is the fp32 bar plus one rounding to 8 significant bits.
"""
import torch

from _util import REL_TOL

BF16_HALF_ULP = 2.0 ** -8


def bf16_excess(got, ref):
    """max over the elements of |got - ref| / bound(ref): <= 1 exactly when every element is inside the bound."""
    got = torch.as_tensor(got).double().cpu()
    ref = torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    scale = max(float(ref.abs().max()), 1e-30)
    bound = BF16_HALF_ULP * ref.abs() + (1.0 + BF16_HALF_ULP) * REL_TOL * scale
    return float(((got - ref).abs() / bound).max())


def assert_bf16_close(got, ref, what=""):
    assert torch.as_tensor(got).dtype == torch.bfloat16, f"{what}: expected a bf16 tensor, got {torch.as_tensor(got).dtype}"
    ex = bf16_excess(got, ref)
    assert ex <= 1.0, f"{what}: |got - ref| reaches {ex:.3f} x (2^-8 |ref| + (1 + 2^-8) 1e-5 max|ref|)"
