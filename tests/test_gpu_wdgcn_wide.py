"""GPU: the wide WD-GCN kernels (csrc/wdgcn_wide.hip: exact-f32 MFMA, widths up to 64 x 64) behind ops.wdgcn_lstm —
routing, every padding case of the widths, node-tile and length edges, saturated gates, a realistic size, reproducible
bits, the no-gradient forward, the models of tmgcn_amd.wdgcn at wide H, hipGraph capture, and the narrow kernels
unchanged.  The checker is test_gpu_wdgcn.py's: Z and the 13 gradients against tests/_wdgcn_ref.py in fp64, no further
from it than max(1e-5, twice the reference's own fp32 arithmetic)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wdgcn_ref as ref  # noqa: E402
from _util import max_rel_err  # noqa: E402

from tmgcn_amd import ops, synth, wdgcn  # noqa: E402
from tmgcn_amd.graphs import GraphedTrainStep  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rand_params(F0, H, scale=1.0, seed=0):
    gen = torch.Generator().manual_seed(seed)
    shapes = [(F0, H)] + [(H, H)] * 8 + [(H,)] * 4
    return [torch.randn(*s, generator=gen) * scale for s in shapes], torch.randn(H, generator=gen), torch.randn(H, generator=gen)


def _inputs(T, N, F0, H, seed=0, ax_scale=1.0, p_scale=1.0, zero_from=None):
    gen = torch.Generator().manual_seed(seed + 100)
    AX = torch.rand(T, N, F0, generator=gen) * ax_scale * (2 * (torch.rand(T, N, F0, generator=gen) > 0.3).float() - 1)
    if zero_from is not None:
        AX[zero_from:] = 0
    params, h0, c0 = _rand_params(F0, H, p_scale, seed)
    R = torch.randn(T, N, H, generator=gen)
    return AX, params, h0, c0, R


def _device_run(AX, params, h0, c0, R, T_run=None):
    dp = [p.to(DEV).requires_grad_(True) for p in params]
    Z = ops.wdgcn_lstm(AX.to(DEV), dp, h0.to(DEV), c0.to(DEV), T_run)
    Z.backward(R[:Z.shape[0]].to(DEV))
    return Z.detach(), [p.grad for p in dp]


def _check_kernel(T, N, F0, H, seed=0, ax_scale=1.0, p_scale=1.0, zero_from=None):
    assert ops.wdgcn_lstm_route(F0, H) == "wide"
    AX, params, h0, c0, R = _inputs(T, N, F0, H, seed, ax_scale, p_scale, zero_from)
    Z, grads = _device_run(AX, params, h0, c0, R)
    outs = {}
    for dt in (torch.float32, torch.float64):
        q = {n: p.detach().to(dt).clone().requires_grad_(True) for n, p in zip(ref.NAMES, params)}
        Zr = ref.lstm(AX.to(dt), q, h0.to(dt), c0.to(dt))
        Zr.backward(R.to(dt))
        outs[dt] = (Zr.detach(), [q[n].grad for n in ref.NAMES])
    (Z32, g32), (Z64, g64) = outs[torch.float32], outs[torch.float64]
    # no worse than the reference's own fp32 arithmetic, measured against the fp64 truth
    for what, got, r32, r64 in [("Z", Z.cpu(), Z32, Z64)] + [("d" + n, g.cpu(), a, b) for n, g, a, b in zip(ref.NAMES, grads, g32, g64)]:
        own, theirs = max_rel_err(got, r64), max_rel_err(r32, r64)
        print(f"T={T} N={N} F0={F0} H={H} {what}: own {own:.2e} reference fp32 {theirs:.2e}")
        assert own <= max(1e-5, 2 * theirs), f"T={T} N={N} F0={F0} H={H} {what}: {own:.2e} from fp64 (reference fp32 {theirs:.2e})"


def test_routing(monkeypatch):
    for w in [(2, 6), (8, 8)]:
        assert ops.wdgcn_lstm_route(*w) == "narrow", w
    for w in [(2, 9), (9, 8), (2, 12), (16, 6), (64, 64), (1, 64)]:
        assert ops.wdgcn_lstm_route(*w) == "wide" and ops.wdgcn_wide_supported(*w) and not ops.wdgcn_supported(*w), w
    for w in [(2, 65), (65, 2)]:
        assert ops.wdgcn_lstm_route(*w) == "torch" and not ops.wdgcn_wide_supported(*w), w

    def refuse(*a, **k):
        raise AssertionError("the torch path ran at a width the wide kernels cover")
    monkeypatch.setattr(ops, "wdgcn_lstm_torch", refuse)
    AX, params, h0, c0, _ = _inputs(3, 20, 16, 32)
    Z = ops.wdgcn_lstm(AX.to(DEV), [p.to(DEV) for p in params], h0.to(DEV), c0.to(DEV))
    assert Z.shape == (3, 20, 32) and bool(torch.isfinite(Z).all())


# padding in each dimension, the first widths past the narrow kernels, both maxima
@pytest.mark.parametrize("F0,H", [(2, 9), (2, 12), (2, 16), (7, 33), (9, 8), (16, 6), (17, 32), (40, 48), (33, 64), (64, 64),
                                  (1, 64), (64, 9)])
def test_kernel_widths(F0, H):
    _check_kernel(5, 65, F0, H, seed=H * 10 + F0)


# a wave owns 16 nodes, a block 64
@pytest.mark.parametrize("N", [1, 15, 16, 17, 63, 64, 65, 129])
def test_kernel_node_counts(N):
    _check_kernel(5, N, 16, 32, seed=N)


@pytest.mark.parametrize("T", [1, 80, 150])
def test_kernel_lengths(T):
    _check_kernel(T, 63, 16, 32, seed=T)


def test_early_stop_is_causal():
    AX, params, h0, c0, _ = _inputs(5, 63, 16, 32, seed=3)
    dp = [p.to(DEV) for p in params]
    with torch.no_grad():
        full = ops.wdgcn_lstm(AX.to(DEV), dp, h0.to(DEV), c0.to(DEV))
        part = ops.wdgcn_lstm(AX.to(DEV), dp, h0.to(DEV), c0.to(DEV), 3)
    assert part.shape == (3, 63, 32) and torch.equal(part, full[:3])


def test_kernel_saturated_gates_and_zero_slices():
    _check_kernel(5, 64, 64, 64, seed=7, ax_scale=50.0)
    _check_kernel(80, 65, 16, 32, seed=9, zero_from=10)


def test_kernel_realistic_size():
    _check_kernel(80, 7301, 16, 32, seed=5)


def test_bit_identical_across_runs():
    AX, params, h0, c0, R = _inputs(20, 1000, 16, 32, seed=11)
    (Za, ga), (Zb, gb) = _device_run(AX, params, h0, c0, R), _device_run(AX, params, h0, c0, R)
    assert torch.equal(Za, Zb)
    for n, a, b in zip(ref.NAMES, ga, gb):
        assert torch.equal(a, b), n


def test_no_grad_forward_and_empty_graph():
    AX, params, h0, c0, R = _inputs(5, 65, 16, 32, seed=13)
    Zg, _ = _device_run(AX, params, h0, c0, R)
    with torch.no_grad():
        Zn = ops.wdgcn_lstm(AX.to(DEV), [p.to(DEV) for p in params], h0.to(DEV), c0.to(DEV))
    assert torch.equal(Zn, Zg)
    Z0 = ops.wdgcn_lstm(torch.zeros(5, 0, 16, device=DEV), [p.to(DEV).requires_grad_(True) for p in params], h0.to(DEV), c0.to(DEV))
    assert Z0.shape == (5, 0, 32)


def test_narrow_widths_unchanged():
    AX, params, h0, c0, _ = _inputs(5, 65, 2, 6, seed=17)
    dp = [p.to(DEV) for p in params]
    assert ops.wdgcn_lstm_route(2, 6) == "narrow"
    with torch.no_grad():
        via_ops = ops.wdgcn_lstm(AX.to(DEV), dp, h0.to(DEV), c0.to(DEV))
        direct = torch.ops.tmgcn.wdgcn_lstm(AX.to(DEV), torch.cat([p.reshape(-1) for p in dp]), h0.to(DEV), c0.to(DEV), 6, 5)
    assert torch.equal(via_ops, direct)


# ---- model level -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    return synth.dynamic_graph(T=6, N=50, edges_per_slice=60, seed=3, no_diag=3)


def _model(g, hidden=(32, 3), seed=0):
    torch.manual_seed(seed)
    return wdgcn.WD_GCN(g.At_list(), torch.from_numpy(g.X), torch.from_numpy(g.edges), list(hidden), device=DEV)


def _bar(own, theirs, what):
    print(f"{what}: own {own:.2e} reference fp32 {theirs:.2e}")
    assert own <= max(1e-5, 2 * theirs), (what, own, theirs)


def test_model_against_reference(small):
    g = small
    m = _model(g)
    assert m.F[0] == 2 and ops.wdgcn_lstm_route(m.F[0], 32) == "wide"
    labels = torch.from_numpy(g.labels)
    out = m()
    loss = torch.nn.CrossEntropyLoss(weight=torch.tensor([0.5, 0.3, 0.2], device=DEV))(out, labels.to(DEV))
    loss.backward()
    p = {n: getattr(m, n).detach().cpu() for n in ref.NAMES}
    r = {dt: ref.train_step(m.AX.cpu(), p, m.h_init.cpu(), m.c_init.cpu(), m.U.cpu(), g.edges, labels,
                            torch.tensor([0.5, 0.3, 0.2]), dt) for dt in (torch.float32, torch.float64)}
    r32, r64 = r[torch.float32], r[torch.float64]
    _bar(max_rel_err(out.detach().cpu(), r64[0]), max_rel_err(r32[0], r64[0]), "logits")
    _bar(abs(float(loss.detach()) - float(r64[1])) / abs(float(r64[1])), abs(float(r32[1]) - float(r64[1])) / abs(float(r64[1])), "loss")
    for n in ref.NAMES:
        _bar(max_rel_err(getattr(m, n).grad.cpu(), r64[2][n]), max_rel_err(r32[2][n], r64[2][n]), "d" + n)

    # the recompute call on a shorter window (wgf:61-64), with and without the early stop
    keep = g.edges[0] < 2
    e_val = g.edges[:, keep]
    coo = [(c.tocoo().row, c.tocoo().col, c.tocoo().data) for c in g.Ct[:3]]
    AX_val = ref.compute_AX(coo, g.X, g.T)
    args = (g.At_list()[:3], torch.from_numpy(g.X[:3]), torch.from_numpy(e_val))
    with torch.no_grad():
        early = m(*args).clone()
        m.early_stop = False
        full = m(*args).clone()
    assert torch.equal(early, full)
    v = {}
    for dt in (torch.float32, torch.float64):
        q = {n: p[n].to(dt) for n in ref.NAMES}
        Z = ref.lstm(AX_val.to(dt), q, m.h_init.cpu().to(dt), m.c_init.cpu().to(dt))
        v[dt] = ref.edge_logits(Z, e_val, m.U.cpu().to(dt))
    _bar(max_rel_err(early.cpu(), v[torch.float64]), max_rel_err(v[torch.float32], v[torch.float64]), "validation logits")


def test_wd_gcn_reg_against_reference(small):
    g = small
    torch.manual_seed(4)
    m = wdgcn.WD_GCN_reg(g.At_list(), torch.from_numpy(g.X), [16, 2], device=DEV)
    assert ops.wdgcn_lstm_route(m.F[0], 16) == "wide"
    y = m()
    assert y.shape == (g.T, g.N)
    p = {n: getattr(m, n).detach().cpu() for n in ref.NAMES}
    r = {dt: ref.reg_forward(m.AX.cpu(), p, m.h_init.cpu(), m.c_init.cpu(), m.lin1.weight.detach().cpu(),
                             m.lin1.bias.detach().cpu(), dt) for dt in (torch.float32, torch.float64)}
    _bar(max_rel_err(y.detach().cpu(), r[torch.float64]), max_rel_err(r[torch.float32], r[torch.float64]), "WD_GCN_reg output")
    (y ** 2).mean().backward()
    assert all(getattr(m, n).grad is not None and bool(torch.isfinite(getattr(m, n).grad).all()) for n in ref.NAMES)


def test_graphed_step_equals_eager_step(small):
    g = small
    target = torch.from_numpy(g.labels).to(DEV)
    crit = torch.nn.CrossEntropyLoss(weight=torch.tensor([0.5, 0.3, 0.2], device=DEV))
    eager, graphed = _model(g), _model(g)
    opt_e = torch.optim.SGD(eager.parameters(), lr=0.01, momentum=0.9)
    opt_g = torch.optim.SGD(graphed.parameters(), lr=0.01, momentum=0.9)
    step = GraphedTrainStep(graphed, crit, opt_g, target, warmup=1)
    # the eager twin takes the same warm-up step and then the three steps the graph replays
    for _ in range(4):
        opt_e.zero_grad(set_to_none=True)
        le = eager.loss(crit, target, unit_grad=True)
        le.backward(gradient=ops.unit_gradient(DEV))
        opt_e.step()
    for _ in range(3):
        lg = step()
    torch.cuda.synchronize()
    assert abs(float(lg) - float(le)) <= 1e-6 * abs(float(le))
    for n in ref.NAMES:
        assert max_rel_err(getattr(graphed, n).detach().cpu(), getattr(eager, n).detach().cpu()) <= 1e-6, n
