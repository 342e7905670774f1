"""Drop-in EvolveGCN-H modules (TensorGCN-master/evolvegcn_functions.py, "ef"): the fourth model family the reference's
drivers compare (experiment_*_evolvegcn*.py, graph_SEIR_evolvegcn.py), the weight evolution computed by the HIP kernels
of csrc/evolvegcn.hip / csrc/evolvegcn_wide.hip and the GCONVs by the batched per-slice GEMM / SpMM+GEMM of the other layers.

    EvolveGCN_1_layer  ef:22-101   W_t = GRU(summary(X_t), W_{t-1}), Y_t = (A_t·X_t)·W_t, the edge head
    EvolveGCN_2_layer  ef:104-213  two such layers, ReLU after the first
    EvolveGCN_reg      ef:310-381  the 1-layer embedding with a per-node linear regression head (the SEIR script)

Structure: a layer's summaries depend on its input only, so the forward is a fixed number of launches whatever T is —
summary + merge + chain (ops.egcn_evolve), then ONE batched GCONV with a per-slice W: ``feature_gemm(AX, W1_seq)``
on the cached AX for layer 1, ``spmm_feature_gemm(A, H1, W2_seq)`` for layer 2 — then the head.

Contract kept from the reference
  * Constructor draws on the CPU generator with ``t.randn`` (then ``.double()``): per layer p [F], W_Z U_Z [F,F], B_Z
    [F,k], W_R U_R, B_R, W_H U_H, B_H and W_init [F,k] (a plain tensor); layer 2 the same with the ``*2`` names; then U
    [2·F_{-2}, C] (an fp32 parameter); EvolveGCN_reg then ``lin1 = nn.Linear(F1, 1)``.  p and the gates are fp64
    parameters on the device, U and lin1 fp32.
  * ``gcn()`` returns ``(logits, W_T)`` / ``(logits, W_T, W2_T)``: the W are fp64 device tensors that carry autograd and
    go back in as ``W_init`` (``gcn(C_val, X_val, edges_val, W_val, W2_val)``).  The 1-layer model and EvolveGCN_reg
    recompute only when W_init is a tensor too (ef:55, 342), else they return the training output; the 2-layer model
    recomputes on (list, tensor, tensor) alone (ef:151) and raises where the reference would fail on a None W.
  * The output buffer has the model's T slices (ef:66): a call over fewer slices leaves the others zero.
  * Scores, summary and GRU are fp64 (the reference's precision); the GCONVs and the head fp32.  Layer 2 ranks the
    fp32 H1 its GCONV uses and forms the k selected rows again in fp64 from Â, X and the fp64 W_t of layer 1.  Equal
    scores select the lower node index (include/tmgcn.h).
  * ops.egcn_evolve_route(F, k) names the implementation of a layer's evolution: csrc/evolvegcn.hip up to 8 x 8,
    csrc/evolvegcn_wide.hip up to 64 x 64; widths beyond (F or k > 64) run the reference's statements as torch
    operators on the device (ops.egcn_evolve_torch).  There is no CPU path.  ``group=`` (slice sharding) does not apply — the GRU couples all
    slices — and ``param_dtype`` other than the reference's: both raise.
  * Train with ``torch.optim.SGD`` as the drivers do (it takes the fp64 / fp32 mix).  tmgcn_amd.optim.FusedSGD and
    layers.fused_train_step do not apply to these models (FusedSGD refuses fp64 parameters); graphs.GraphedTrainStep
    does, through ``.loss``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .csr import BatchedCSR
from .layers import AdjLike, _adj, _default_device, _Deliver, _feat, _Head, _param, _Sharding

GATES = ops.EGCN_GATE_NAMES


def _refuse(cls: str, param_dtype, group):
    if group is not None:
        raise RuntimeError(f"{cls}: slice sharding (group=) does not apply — the GRU couples every slice to the next")
    if param_dtype not in (None, torch.float64):
        raise RuntimeError(f"{cls}: the GRU parameters are fp64 as in the reference (param_dtype={param_dtype})")


def _is_list(A) -> bool:
    return type(A) == list or isinstance(A, BatchedCSR)


class _EgcnBase(nn.Module):
    """What the three models share: the adjacency, X and the cached AX (the layer-1 GCONV's A_t·X_t), the per-layer
    draws and the evolution + GCONV of one call."""

    _shard = None

    def _init_common(self, A: AdjLike, X: torch.Tensor, hidden_feat, device, param_dtype, group):
        _refuse(type(self).__name__, param_dtype, group)
        dev = torch.device(device) if device is not None else _default_device()
        self.T, self.N = int(X.shape[0]), int(X.shape[1])
        n_slices = A.T if isinstance(A, BatchedCSR) else len(A)
        if n_slices < self.T:
            raise RuntimeError(f"adjacency has {n_slices} slices but X has T={self.T} (ef:67-70)")
        self.dev = dev
        self.F = [int(X.shape[-1])] + [int(h) for h in hidden_feat]
        self.A = _adj(A, self.N, dev)
        if self.A.T > self.T:                                    # the loop reads A[t] for t < T only (ef:67-70)
            self.A = self.A.slices(0, self.T)
        self.X = _feat(X, dev)
        self.AX = ops.spmm(self.A, self.X)
        return dev

    def _draw_layer(self, i: int, suffix: str, dev):
        F, k = self.F[i], self.F[i + 1]
        setattr(self, "p" + suffix, _param(torch.randn(F).double(), dev, torch.float64))              # ef:37
        for g, name in enumerate(GATES):                                                             # ef:38-46
            shape = (F, k) if name.startswith("B_") else (F, F)
            setattr(self, name + suffix, _param(torch.randn(*shape).double(), dev, torch.float64))
        setattr(self, "W_init" + suffix, torch.randn(F, k).double().to(dev))                         # ef:47: no parameter

    def gates(self, suffix: str = ""):
        return [getattr(self, n + suffix) for n in GATES]

    def _call_inputs(self, A, X):
        """(A as BatchedCSR, X fp32, AX, T_run) of a recompute call: the loop runs over the call's X slices (ef:67)."""
        T_run = int(X.shape[0])
        if T_run > self.T:
            raise RuntimeError(f"X has {T_run} slices but the model was built for T={self.T} (ef:66)")
        A_csr = _adj(A, self.N, self.dev)
        if A_csr.T < T_run:
            raise RuntimeError(f"adjacency has {A_csr.T} slices but X has {T_run} (ef:67-70)")
        if A_csr.T > T_run:
            A_csr = A_csr.slices(0, T_run)
        Xf = _feat(X, self.dev)
        AX = ops.spmm(A_csr, Xf) if T_run else Xf.new_zeros(0, self.N, Xf.shape[-1])
        return A_csr, Xf, AX, T_run

    def _w0(self, W, name):
        if W is None:
            raise RuntimeError(f"{type(self).__name__}: {name} is None — the reference's GRU would fail on it "
                               f"(ef:151-155 take the W of a recompute call unchecked); pass the W a previous call returned")
        return W.detach().to(self.dev, torch.float64) if W.device != self.dev or W.dtype != torch.float64 else W

    def _layers(self, A_csr, X, AX, T_run, W0, W02=None):
        """The embedding [self.T, N, F_{-2}] (zero beyond T_run, ef:66) and the final W of each layer."""
        W1s, W1 = ops.egcn_evolve(X, self.p, self.gates(), W0, T_run)                     # ef:69 / 167
        two = W02 is not None
        Y = ops.feature_gemm(AX, W1, act="relu" if two else None) if T_run else AX.new_zeros(0, self.N, W1.shape[-1])
        Ws = [W1s[-1]]
        if two:
            W2s, W2 = ops.egcn_evolve(Y, self.p2, self.gates("2"), W02, T_run, rows=(A_csr, X, W1s))   # ef:169
            Y = ops.spmm_feature_gemm(A_csr, Y, W2) if T_run else Y.new_zeros(0, self.N, W2.shape[-1])   # ef:170
            Ws.append(W2s[-1])
        if T_run < self.T:
            Y = torch.cat((Y, Y.new_zeros(self.T - T_run, self.N, Y.shape[-1])), dim=0)
        return Y, Ws


class _EgcnEdge(_Head, _Deliver, _Sharding, _EgcnBase):
    """The edge-head models: ``__call__`` keeps the W arguments for ``_embed_impl`` and returns the reference's tuple."""

    _layers_n = 1

    def _init_edge(self, A, X, edges, hidden_feat, device, param_dtype, group):
        dev = self._init_common(A, X, hidden_feat, device, param_dtype, group)
        self._edges = ops.EdgeIndex(edges, self.N, dev, T=self.T)                          # ef:29-30
        self._W_args, self._W_want, self._W_out = (None, None), False, ()
        return dev

    def _embed_impl(self, A=None, X=None, edges=None):
        W_init, W_init2 = self._W_args
        two = self._layers_n == 2
        recompute = _is_list(A) and type(X) == torch.Tensor and type(edges) == torch.Tensor
        if not two:
            recompute = recompute and isinstance(W_init, torch.Tensor)                     # ef:55
        if recompute:                                                                       # ef:56-58 / 152-155
            A_csr, Xf, AX, T_run = self._call_inputs(A, X)
            eidx = ops.EdgeIndex(edges, self.N, self.dev, T=self.T)
            W0 = self._w0(W_init, "W_init")
            W02 = self._w0(W_init2, "W_init2") if two else None
        else:                                                                               # ef:60-64 / 157-162
            A_csr, Xf, AX, T_run, eidx = self.A, self.X, self.AX, self.T, self._edges
            W0 = self.W_init
            W02 = self.W_init2 if two else None
        Y, Ws = self._layers(A_csr, Xf, AX, T_run, W0, W02)
        if self._W_want:
            self._W_out = Ws                                     # handed to __call__, which clears it again
        return Y, eidx, self.U, None                                                        # ef:73-76: the edge head

    def __call__(self, A=None, X=None, edges=None, W_init=None, W_init2=None):
        # the returned W carry this call's autograd graph: they live as long as the caller keeps them, not on the module
        self._W_args, self._W_want = (W_init, W_init2), True
        try:
            out = self.forward(A, X, edges)
            return (out, *self._W_out)
        finally:
            self._W_args, self._W_want, self._W_out = (None, None), False, ()


class EvolveGCN_1_layer(_EgcnEdge):
    """1-layer EvolveGCN-H with the edge head (ef:22-101): ``gcn(...)`` -> (logits [E, C], W_T)."""

    def __init__(self, A: AdjLike, X: torch.Tensor, edges: torch.Tensor, hidden_feat=[2, 2], device=None,
                 param_dtype=None, group=None):
        super().__init__()
        dev = self._init_edge(A, X, edges, hidden_feat, device, param_dtype, group)
        self._draw_layer(0, "", dev)
        self.U = _param(torch.randn(self.F[-2] * 2, self.F[-1]), dev, torch.float32)      # ef:48

    def __call__(self, A=None, X=None, edges=None, W_init=None):                           # ef:50-52
        return super().__call__(A, X, edges, W_init)


class EvolveGCN_2_layer(_EgcnEdge):
    """2-layer EvolveGCN-H with the edge head (ef:104-213): ``gcn(...)`` -> (logits [E, C], W_T, W2_T)."""

    _layers_n = 2

    def __init__(self, A: AdjLike, X: torch.Tensor, edges: torch.Tensor, hidden_feat=[2, 2, 2], device=None,
                 param_dtype=None, group=None):
        super().__init__()
        dev = self._init_edge(A, X, edges, hidden_feat, device, param_dtype, group)
        self._draw_layer(0, "", dev)
        self._draw_layer(1, "2", dev)
        self.U = _param(torch.randn(self.F[-2] * 2, self.F[-1]), dev, torch.float32)      # ef:144


class EvolveGCN_reg(_Deliver, _EgcnBase):
    """1-layer EvolveGCN-H with a per-node linear regression head (ef:310-381): returns lin1(Y).squeeze(2), [T, N].
    U is drawn (ef:334) but never used; it stays a parameter, as in the reference."""

    def __init__(self, A: AdjLike, X: torch.Tensor, hidden_feat=[2, 2], device=None, param_dtype=None, group=None):
        super().__init__()
        dev = self._init_common(A, X, hidden_feat, device, param_dtype, group)
        self._draw_layer(0, "", dev)
        self.U = _param(torch.randn(self.F[-2] * 2, self.F[-1]), dev, torch.float32)      # ef:334
        self.lin1 = nn.Linear(self.F[1], 1).to(dev)                                         # ef:335

    def __call__(self, A=None, X=None, W_init=None):                                        # ef:337-339
        return self.forward(A, X, W_init)

    def forward(self, A=None, X=None, W_init=None):
        if _is_list(A) and type(X) == torch.Tensor and isinstance(W_init, torch.Tensor):    # ef:342-343
            A_csr, Xf, AX, T_run = self._call_inputs(A, X)
            W0 = self._w0(W_init, "W_init")
        else:                                                                               # ef:344-347
            A_csr, Xf, AX, T_run, W0 = self.A, self.X, self.AX, self.T, self.W_init
        Y, _ = self._layers(A_csr, Xf, AX, T_run, W0)
        return self._deliver(self.lin1(Y).squeeze(2))                                       # ef:356-358
