"""CPU: the host side of the layer-1 GEMM that stores its result in bf16 and of the dW that reads a bf16 gradient — the domain
query, the argument checks of the two C entry points (every case returns before anything is launched, so no GPU is needed)
and the out_dtype rule of ops.feature_gemm."""
import pytest
import torch

from tmgcn_amd import _lib, ops

OK, INVALID, WORKSPACE = 0, -1, -3   # TMGCN_OK, TMGCN_ERR_INVALID, TMGCN_ERR_WORKSPACE


def documented(K, Nf):
    """Nf is the K of the bf16 gather that reads Y; K takes the split kernel (one k-chunk) or the thread-per-row kernel."""
    if not (16 <= Nf <= 128 and Nf % 8 == 0):
        return 0
    if 16 <= K <= 128 and K % 4 == 0:
        return 1
    return 1 if (1 <= K < 16 and Nf <= 64) else 0


def test_supported_is_exactly_the_documented_domain():
    lib = _lib.load()
    for K in range(0, 141):
        for Nf in range(0, 141):
            assert lib.tmgcn_gemm_bf16y_supported(K, Nf) == documented(K, Nf), (K, Nf)
    assert lib.tmgcn_gemm_bf16y_supported(-4, 16) == 0 and lib.tmgcn_gemm_bf16y_supported(16, -8) == 0
    assert lib.tmgcn_gemm_bf16y_supported(256, 128) == 0                   # the k-chunked form
    assert ops.kernels.gemm_bf16y_supported(128, 128) and ops.kernels.gemm_bf16y_supported(2, 64)
    assert not ops.kernels.gemm_bf16y_supported(2, 128) and not ops.kernels.gemm_bf16y_supported(18, 16)


def _fwd(**over):
    """tmgcn_gemm_bf16y on made-up, never dereferenced, 16-byte aligned addresses; `over` replaces arguments."""
    a = dict(A=0x10000, W=0x20000, Y=0x30000, pre=0x40000, R=100, K=32, Nf=24, rows_per_batch=0, w_batch_stride=0, act=3, stream=None)
    a.update(over)
    order = ("A", "W", "Y", "pre", "R", "K", "Nf", "rows_per_batch", "w_batch_stride", "act", "stream")
    return _lib.load().tmgcn_gemm_bf16y(*(a[k] for k in order))


def _dw(**over):
    """tmgcn_gemm_dw_act_bf16, likewise; the default workspace size is the one the library asks for."""
    a = dict(A=0x10000, dY=0x30000, pre=0x40000, act=3, dW=0x50000, R=100, K=32, Nf=24, rows_per_batch=0, ws=0x60000, ws_bytes=None,
             stream=None)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = _lib.load().tmgcn_gemm_dw_workspace_bytes(max(a["R"], 1), max(a["K"], 1), max(a["Nf"], 1),
                                                                  max(a["rows_per_batch"], 0))
    order = ("A", "dY", "pre", "act", "dW", "R", "K", "Nf", "rows_per_batch", "ws", "ws_bytes", "stream")
    return _lib.load().tmgcn_gemm_dw_act_bf16(*(a[k] for k in order))


_ids = lambda o: ",".join(f"{k}={v}" for k, v in o.items())  # noqa: E731


@pytest.mark.parametrize("over", [
    dict(A=None), dict(W=None), dict(Y=None),                                                   # NULL
    dict(A=0x10004), dict(A=0x10008), dict(K=2, A=0x10002),                                     # A: 16 bytes (4 below K = 16)
    dict(W=0x20002), dict(Y=0x30001), dict(pre=0x40002),                                        # fp32 / bf16 element alignment
    dict(act=-1), dict(act=4),
    dict(K=0), dict(Nf=0), dict(R=-1), dict(rows_per_batch=-1), dict(w_batch_stride=-1),
    dict(K=132), dict(K=256), dict(K=18), dict(K=17), dict(Nf=20), dict(Nf=8), dict(Nf=136), dict(K=2, Nf=128), dict(K=8, Nf=72),
], ids=_ids)
def test_forward_refuses_invalid_arguments_without_a_launch(over):
    assert _fwd(**over) == INVALID
    assert len(_lib.load().tmgcn_last_error()) > 0


@pytest.mark.parametrize("over", [
    dict(A=None), dict(dY=None), dict(dW=None),
    dict(pre=None), dict(pre=None, act=1),                                                      # an activation needs its pre
    dict(A=0x10004), dict(K=2, A=0x10002), dict(dY=0x30002), dict(dY=0x30004), dict(K=2, dY=0x30001),
    dict(pre=0x40004), dict(pre=0x40008), dict(K=2, pre=0x40002), dict(dW=0x50002),
    dict(act=-1), dict(act=4),
    dict(K=0), dict(Nf=0), dict(R=-1), dict(rows_per_batch=-1),
    dict(K=132), dict(K=256), dict(K=18), dict(Nf=20), dict(Nf=8), dict(Nf=136), dict(K=2, Nf=128),
], ids=_ids)
def test_dw_refuses_invalid_arguments_without_a_launch(over):
    assert _dw(**over) == INVALID
    assert len(_lib.load().tmgcn_last_error()) > 0


@pytest.mark.parametrize("over", [dict(ws=None), dict(ws_bytes=0), dict(ws_bytes=-1)], ids=_ids)
def test_dw_refuses_a_workspace_that_is_too_small(over):
    """As tmgcn_gemm_dw_f32 does: its own status, and nothing launched."""
    need = _lib.load().tmgcn_gemm_dw_workspace_bytes(100, 32, 24, 0)
    assert need > 0
    assert _dw(**over) == WORKSPACE
    assert _dw(ws_bytes=need - 1) == WORKSPACE
    assert b"workspace" in _lib.load().tmgcn_last_error()


def test_misaligned_operands_of_the_small_route_are_accepted_as_far_as_the_checks_go():
    """K < 16: 4-byte A / pre and 2-byte dY are fine — with R = 0 the call returns before a launch, after the checks that do
    not need rows; act = none does not look at pre."""
    assert _fwd(R=0, K=2, A=0x10004) == OK
    assert _dw(R=0, act=0, pre=None) == OK


@pytest.mark.parametrize("over", [dict(R=0), dict(R=0, A=None, W=None, Y=None, pre=None)], ids=_ids)
def test_empty_extent_is_ok_without_a_launch(over):
    assert _fwd(**over) == OK
    over = {("dY" if k == "Y" else k): v for k, v in over.items() if k != "W"}
    assert _dw(**over) == OK


def _fwd_f32(**over):
    """tmgcn_gemm_f32, likewise."""
    a = dict(A=0x10000, W=0x20000, Y=0x30000, pre=0x40000, R=100, K=32, Nf=24, trans_w=0, rows_per_batch=0, w_batch_stride=0, act=3,
             algo=0, stream=None)
    a.update(over)
    order = ("A", "W", "Y", "pre", "R", "K", "Nf", "trans_w", "rows_per_batch", "w_batch_stride", "act", "algo", "stream")
    return _lib.load().tmgcn_gemm_f32(*(a[k] for k in order))


def _dw_f32(fold, **over):
    """tmgcn_gemm_dw_f32, or with fold tmgcn_gemm_dw_act_f32 (the narrow kernel's fold of act'), likewise."""
    a = dict(A=0x10000, dY=0x30000, pre=0x40000, act=3, dW=0x50000, R=100, K=32, Nf=24, rows_per_batch=0, algo=0, ws=0x60000,
             ws_bytes=None, stream=None)
    a.update(over)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = _lib.load().tmgcn_gemm_dw_workspace_bytes(a["R"], a["K"], a["Nf"], a["rows_per_batch"])
    if fold:
        order = ("A", "dY", "pre", "act", "dW", "R", "K", "Nf", "rows_per_batch", "ws", "ws_bytes", "stream")
        return _lib.load().tmgcn_gemm_dw_act_f32(*(a[k] for k in order))
    order = ("A", "dY", "dW", "R", "K", "Nf", "rows_per_batch", "algo", "ws", "ws_bytes", "stream")
    return _lib.load().tmgcn_gemm_dw_f32(*(a[k] for k in order))


def test_fp32_entries_keep_their_own_rule_for_an_empty_extent():
    """The launchers are shared with the bf16 entries; the fp32 ones keep their own R = 0 rule.  The forward launches nothing
    and returns OK before it looks at an operand.  dW zero-fills what it is given — a launch, so its OK return is held on the
    GPU (test_gpu_gemm_bf16y.py) — and here refuses only a dW that is not there, where the bf16 entry returns OK."""
    assert _fwd_f32(R=0) == OK
    assert _fwd_f32(R=0, A=None, W=None, Y=None, pre=None) == OK
    assert _fwd_f32(R=0, K=256) == OK and _fwd_f32(R=0, K=132, trans_w=1, algo=1) == OK       # no bf16-Y domain here
    for fold in (False, True):
        k = dict(K=4, Nf=8) if fold else {}
        assert _dw_f32(fold, R=0, A=None, dY=None, ws=None, ws_bytes=0, dW=None, **k) == INVALID
        assert b"dW" in _lib.load().tmgcn_last_error()
    assert _dw(R=0, A=None, dY=None, ws=None, ws_bytes=0, dW=None) == OK


@pytest.mark.parametrize("K", [132, 256])
def test_forward_never_reaches_a_k_chunked_launch(K):
    """128 < K <= 512 is the k-chunked form of the fp32 entry, whose chunks add to an fp32 Y: the bf16-Y entry names the
    width and refuses, aligned operands or not."""
    lib = _lib.load()
    assert _fwd(K=K) == INVALID
    msg = lib.tmgcn_last_error()
    assert len(msg) > 0 and f"K={K}".encode() in msg
    assert _fwd(K=K, R=0) == INVALID


@pytest.mark.parametrize("K", [2, 32], ids=["small_route", "split_route"])
def test_every_dw_entry_asks_for_the_same_workspace(K):
    """One byte short of tmgcn_gemm_dw_workspace_bytes is the workspace status for the bf16 entry on both of its routes
    and for the two fp32 entries, with that same value."""
    lib = _lib.load()
    need = lib.tmgcn_gemm_dw_workspace_bytes(100, K, 24, 0)
    assert need > 0
    for call in (lambda **o: _dw(K=K, **o), lambda **o: _dw_f32(False, K=K, **o)):
        assert call(ws_bytes=need - 1) == WORKSPACE
        assert b"workspace" in lib.tmgcn_last_error()
        assert call(ws=None) == WORKSPACE
    # the fold of tmgcn_gemm_dw_act_f32 exists for even K, Nf <= 8 only
    need8 = lib.tmgcn_gemm_dw_workspace_bytes(100, K if K <= 8 else 8, 8, 0)
    assert _dw_f32(True, K=K if K <= 8 else 8, Nf=8, ws_bytes=need8 - 1) == WORKSPACE
    assert b"workspace" in lib.tmgcn_last_error()


def test_out_dtype_rule_of_the_python_operator():
    A, W = torch.zeros(2, 8, 16), torch.zeros(16, 16)
    for bad in (torch.float16, torch.float64, torch.int32):
        with pytest.raises(RuntimeError, match="out_dtype"):
            ops.feature_gemm(A, W, out_dtype=bad)
        with pytest.raises(RuntimeError, match="out_dtype"):
            ops.kernels.gemm(A, W, out_dtype=bad)
    assert ops.gemm_bf16y_fused(128, 128) and ops.gemm_bf16y_fused(2, 64) and ops.gemm_bf16y_fused(20, 24)
    assert not ops.gemm_bf16y_fused(256, 128) and not ops.gemm_bf16y_fused(2, 128) and not ops.gemm_bf16y_fused(16, 12)
