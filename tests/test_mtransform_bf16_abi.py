"""CPU: the host side of the band M-transform on bf16-stored operands — the domain query, the argument checks of the C
entry point (every case returns before anything is launched, so no GPU is needed) and the dtype rules of ops.m_transform."""
import pytest
import torch

from tmgcn_amd import _lib, ops

OK, INVALID = 0, -1   # TMGCN_OK, TMGCN_ERR_INVALID


def test_supported_is_exactly_the_documented_domain():
    lib = _lib.load()
    for lo in range(-1, 26):
        for hi in range(-1, 26):
            want = 1 if (lo >= 0 and hi >= 0 and lo + hi + 1 <= 20) else 0
            assert lib.tmgcn_mtransform_bf16_supported(lo, hi) == want, (lo, hi)
    assert ops.kernels.mtransform_bf16_supported(19, 0) and not ops.kernels.mtransform_bf16_supported(10, 10)


def _call(**over):
    """tmgcn_mtransform_bf16 on made-up, never dereferenced, 16-byte aligned addresses; `over` replaces arguments."""
    a = dict(M=0x1000, Tm=8, ldm=8, transpose=0, row_off=0, col_off=0, T_out=8, T_in=8, band_lo=3, band_hi=0, X=0x4000, x_bf16=0,
             Y=0x6000, y_bf16=1, C=64, stream=None)
    a.update(over)
    order = ("M", "Tm", "ldm", "transpose", "row_off", "col_off", "T_out", "T_in", "band_lo", "band_hi", "X", "x_bf16", "Y", "y_bf16",
             "C", "stream")
    return _lib.load().tmgcn_mtransform_bf16(*(a[k] for k in order))


@pytest.mark.parametrize("over", [
    dict(x_bf16=2), dict(x_bf16=-1), dict(y_bf16=2), dict(y_bf16=-1),                            # a flag outside {0, 1}
    dict(x_bf16=0, y_bf16=0),                                                                    # both fp32
    dict(band_lo=20, band_hi=0), dict(band_lo=10, band_hi=10), dict(band_lo=0, band_hi=20),   # unsupported band
    dict(band_lo=-1), dict(band_hi=-1),
    dict(M=None), dict(X=None), dict(Y=None), dict(Y=0x4000),                                    # NULL, X == Y
    dict(x_bf16=1, X=0x4001), dict(y_bf16=1, Y=0x6001),                                          # bf16 operand not 2-byte aligned
    dict(x_bf16=0, X=0x4002), dict(x_bf16=1, y_bf16=0, Y=0x6002),                                # fp32 operand not 4-byte aligned
    dict(Tm=0), dict(ldm=4), dict(T_out=-1), dict(T_in=-1), dict(C=-1),                          # the shape errors of the fp32 entry
    dict(row_off=1), dict(col_off=1), dict(row_off=-1), dict(T_out=9),
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_invalid_arguments_are_refused_without_a_launch(over):
    assert _call(**over) == INVALID
    assert len(_lib.load().tmgcn_last_error()) > 0


def test_both_fp32_names_the_fp32_entry_point():
    assert _call(x_bf16=0, y_bf16=0) == INVALID
    assert b"tmgcn_mtransform_f32" in _lib.load().tmgcn_last_error()


@pytest.mark.parametrize("over", [dict(T_out=0), dict(C=0), dict(C=0, X=None, Y=None)], ids=str)
def test_empty_extent_is_ok_without_a_launch(over):
    assert _call(**over) == OK


def test_dtype_rules_of_the_python_operator():
    op = ops.MOperator(torch.tril(torch.ones(4, 4)), "cpu")
    X = torch.zeros(4, 8, 4)
    with pytest.raises(RuntimeError, match="out_dtype"):
        ops.m_transform(X, op, out_dtype=torch.float16)
    with pytest.raises(RuntimeError, match="out_dtype"):
        ops.kernels.mtransform(op, X, out_dtype=torch.float16)
    with pytest.raises(RuntimeError, match="x_group_rows"):
        ops.m_transform(X.bfloat16(), op, x_group_rows=2)
    with pytest.raises(RuntimeError, match="y_group_rows"):
        ops.m_transform(X, op, y_group_rows=2, out_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="x_group_rows"):
        ops.kernels.mtransform(op, X.bfloat16(), x_group_rows=2)
    assert ops.m_transform_bf16_fused(op)                                            # 4 diagonals: one launch each way
    assert not ops.m_transform_bf16_fused(ops.MOperator(torch.ones(24, 24), "cpu"))  # dense: the fp32 transform and the casts
