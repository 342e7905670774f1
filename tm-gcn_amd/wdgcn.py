"""Drop-in WD-GCN modules (TensorGCN-master/wd_gcn_functions.py, "wgf"): the third model family the reference's drivers
compare (experiment_*_wd-gcn*.py, graph_SEIR_wd_gcn.py), computed by the HIP kernels of csrc/wdgcn.hip (widths up to
8 x 8) and csrc/wdgcn_wide.hip (up to 64 x 64).

    WD_GCN       wgf:21-98    relu(AX·W), an LSTM over the T slices (sigmoid candidate), the edge head
    WD_GCN_reg   wgf:100-170  the same embedding with a per-node linear regression head (the SEIR script)

Contract kept from the reference
  * Constructor draws on the CPU generator with ``t.randn``: W [F0,H], Wf Wj Wc Wo, Uf Uj Uc Uo [H,H], bf bj bc bo [H]
    (the 13 parameters, registered in that order), then h_init [H], c_init [H] and U [2H,C] — three plain tensors, never
    trained, not in ``state_dict()``.  WD_GCN_reg builds ``lin1 = nn.Linear(H, 1)`` before W is drawn (wgf:111).
  * ``AX`` is a [self.T, N, F0] buffer whose first len(A) slices are Â_k·X_k and whose other slices are zero
    (wgf:80-84; layers.EmbeddingKWGCN.compute_AX).  ``gcn(A_list, X, edges)`` builds it again for that window, still
    over the model's T slices (wgf:61-64).  WD_GCN_reg's ``__call__(A, X)`` passes no edges, so the recompute branch
    never runs there and every call returns the training window's output (wgf:131-138).
  * The recurrence is causal: WD_GCN runs it only up to the last slice its edges read (``early_stop``), the logits are
    the same bits.  This spares the validation calls of the chess scripts 70 of 80 steps over zero-padded slices.
  * ops.wdgcn_lstm_route(F0, H) names the implementation: the lane-group kernels up to 8 x 8, the MFMA kernels up to
    64 x 64 (the paper's hidden sizes 32 and 64), and only beyond that (H > 64 or F0 > 64) the reference's statements as
    torch operators on the device (ops.wdgcn_lstm_torch).  There is no CPU path.  ``group=`` (slice sharding) does not apply — the recurrence couples
    all slices — and parameters are fp32 only: both raise.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .csr import BatchedCSR
from .layers import (AdjLike, EmbeddingKWGCN, _adj, _default_device, _Deliver, _feat, _Head, _is_recompute_call, _param,
                     _Sharding)


def _refuse(cls: str, param_dtype, group):
    if group is not None:
        raise RuntimeError(f"{cls}: slice sharding (group=) does not apply — the LSTM couples every slice to the next")
    if param_dtype != torch.float32:
        raise RuntimeError(f"{cls}: parameters are fp32 only (param_dtype={param_dtype})")


class _WdgcnBase(nn.Module):
    """What both models share: the cached AX (wgf:47, 80-84) and the 13 LSTM-model parameters + 3 plain tensors."""

    _shard = None          # compute_AX is layers.EmbeddingKWGCN's, which asks (never sharded here)

    def _init_common(self, A: AdjLike, X: torch.Tensor, device, param_dtype, group):
        _refuse(type(self).__name__, param_dtype, group)
        dev = torch.device(device) if device is not None else _default_device()
        self.T, self.N = int(X.shape[0]), int(X.shape[1])
        n_slices = A.T if isinstance(A, BatchedCSR) else len(A)
        if n_slices > self.T:
            raise RuntimeError(f"adjacency has {n_slices} slices but X has T={self.T}")
        self.dev = dev
        self.A = _adj(A, self.N, dev)
        self.AX = self.compute_AX(self.A, _feat(X, dev))
        return dev

    def _draw(self, F0: int, hidden_feat, dev):
        H = int(hidden_feat[0])
        self.W = _param(torch.randn(F0, H), dev, torch.float32)                             # wgf:39
        for name in ops.WDGCN_PARAM_NAMES[1:9]:                                             # wgf:42-49
            setattr(self, name, _param(torch.randn(H, H), dev, torch.float32))
        for name in ops.WDGCN_PARAM_NAMES[9:]:                                              # wgf:50-53
            setattr(self, name, _param(torch.randn(H), dev, torch.float32))
        self.h_init = torch.randn(H).to(dev)                                                # wgf:54-55: not parameters
        self.c_init = torch.randn(H).to(dev)
        self.U = torch.randn(2 * H, int(hidden_feat[1])).to(dev)                            # wgf:58: never trained

    def compute_AX(self, A: BatchedCSR, X: torch.Tensor) -> torch.Tensor:
        """wgf:80-84 — the statement of ehf:469-473 (layers.EmbeddingKWGCN.compute_AX): a [self.T, N, F0] buffer, the
        first A.T slices Â_k·X_k, the rest zero."""
        return EmbeddingKWGCN.compute_AX(self, A, X)

    def _recompute_AX(self, A, X) -> torch.Tensor:
        n_call = A.T if isinstance(A, BatchedCSR) else len(A)
        if n_call > self.T:
            raise RuntimeError(f"adjacency has {n_call} slices but the model was built for T={self.T} (wgf:80-84)")
        A_csr = _adj(A, self.N, self.dev) if n_call else \
            BatchedCSR(torch.zeros(1, dtype=torch.int64, device=self.dev), torch.zeros(0, dtype=torch.int32, device=self.dev),
                       torch.zeros(0, dtype=torch.float32, device=self.dev), 0, self.N)
        return self.compute_AX(A_csr, _feat(X, self.dev))

    def lstm_params(self):
        return [getattr(self, n) for n in ops.WDGCN_PARAM_NAMES]

    def _lstm(self, AX: torch.Tensor, T_run=None) -> torch.Tensor:
        return ops.wdgcn_lstm(AX, self.lstm_params(), self.h_init, self.c_init, T_run)       # wgf:70, 86-98


def _steps(edges: torch.Tensor) -> int:
    """Slices the recurrence has to run for an edge set: one past the last slice any edge reads."""
    return int(edges[0].max()) + 1 if edges.numel() else 1


class WD_GCN(_Head, _Deliver, _Sharding, _WdgcnBase):
    """WD-GCN with the edge head (wgf:21-98): logits [E, C] = [Z[src], Z[dst]]·U, Z the LSTM's output."""

    early_stop = True      # run the recurrence up to the last slice the edges read (the same logits, bit for bit)

    def __init__(self, A: AdjLike, X: torch.Tensor, edges: torch.Tensor, hidden_feat=[2, 2], device=None,
                 param_dtype=torch.float32, group=None):
        super().__init__()
        dev = self._init_common(A, X, device, param_dtype, group)
        self.F = [int(X.shape[-1])] + [int(h) for h in hidden_feat]
        self._edges = ops.EdgeIndex(edges, self.N, dev, T=self.T)                           # wgf:29-30
        self._t_run = _steps(edges)
        self._draw(self.F[0], hidden_feat, dev)

    def __call__(self, A=None, X=None, edges=None):                                         # wgf:60-61
        return self.forward(A, X, edges)

    def _embed_impl(self, A=None, X=None, edges=None):
        if _is_recompute_call(A, X, edges):                                                  # wgf:62-65
            AX, eidx, t_run = self._recompute_AX(A, X), ops.EdgeIndex(edges, self.N, self.dev, T=self.T), _steps(edges)
        else:
            AX, eidx, t_run = self.AX, self._edges, self._t_run
        Z = self._lstm(AX, t_run if self.early_stop else self.T)
        return Z, eidx, self.U, None                                                         # wgf:72-76: the edge head


class WD_GCN_reg(_Deliver, _WdgcnBase):
    """WD-GCN with a per-node linear regression head (wgf:100-170): returns lin1(Z).squeeze(2), [T, N]."""

    def __init__(self, A: AdjLike, X: torch.Tensor, hidden_feat=[2, 2], device=None, param_dtype=torch.float32,
                 group=None):
        super().__init__()
        dev = self._init_common(A, X, device, param_dtype, group)
        self.F = [int(X.shape[-1])] + [int(h) for h in hidden_feat]
        self.lin1 = nn.Linear(self.F[1], 1).to(dev)                                          # wgf:111: before W is drawn
        self._draw(self.F[0], hidden_feat, dev)

    def __call__(self, A=None, X=None):                                                      # wgf:131-132: edges never passed
        return self.forward(A, X)

    def forward(self, A=None, X=None, edges=None):
        AX = self._recompute_AX(A, X) if _is_recompute_call(A, X, edges) else self.AX        # wgf:134-138
        return self._deliver(self.lin1(self._lstm(AX)).squeeze(2))                           # wgf:140-145
