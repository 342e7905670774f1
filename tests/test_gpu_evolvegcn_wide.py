"""GPU: EvolveGCN-H at widths up to 64 x 64 (csrc/evolvegcn_wide.hip through ops.egcn_evolve and tmgcn_amd.evolvegcn)
against the CPU restatement tests/_evolvegcn_ref.py in fp64: routing, the kernels over widths / node counts / lengths,
the tie rule and NaN, layer 2's fp64 rows, early stop, reproducibility, the three models (forward, every gradient, a
validation-style call, 10 SGD steps against a restatement twin), hipGraph capture, and the narrow route unchanged.

Bars.  fp64 quantities at operator level (W_seq, y_sel, the gradients of p, the gates and W_init): 1e-9·max|ref|, the
project's bar for W in test_gpu_evolvegcn.py.  dH is the fp64 gradient stored once in fp32: 2^-24 (the rounding of one
store, relative to the element, so at most that relative to max|ref|) + 1e-9.  H_sel of layer 2: 1e-12.  Everything that
passes through the fp32 GCONVs: the README's parity bar (`_bar`).
Selection is discontinuous, so every comparison over a random selection runs with the `gap` fixture: the restatement's
k-th and (k+1)-th score of every slice and layer must differ by more than 1e-5·max|score| (ten times the fp32 GCONV's
parity bar).  The gates and W_init are drawn both as the reference draws them, N(0,1) (which saturates the gates at
width 64), and scaled by 1/sqrt(F) (which does not)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _evolvegcn_ref as ref  # noqa: E402
from _util import max_rel_err, record_tolerance  # noqa: E402

from tmgcn_amd import evolvegcn, ops  # noqa: E402
from tmgcn_amd.graphs import GraphedTrainStep  # noqa: E402
from tmgcn_amd.layers import _adj  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64_BAR = 1e-9
DH_BAR = 2.0 ** -24 + 1e-9
GAP = 1e-5
SELECT_BLOCK = 1024                      # nodes a selection block covers (kEgwSort)
DRAWS = ("n01", "scaled")


def _bar(got, r32, r64, what):
    """The README's bar: <= 1e-5·max|ref|; where the reference's own fp32 result is more than 1e-5 from the fp64 truth,
    within 1e-6 of the truth and at least 10x closer to it than the reference."""
    err = max_rel_err(got, r32)
    print(f"{what}: {err:.3e} from the fp32 restatement")
    if err <= 1e-5:
        return
    ref_dev, own = max_rel_err(r32, r64), max_rel_err(got, r64)
    assert ref_dev > 1e-5 and own <= 1e-6 and own * 10 <= ref_dev, \
        f"{what}: {err:.2e} from the reference, {own:.2e} from the fp64 truth (reference: {ref_dev:.2e})"


_summarize = ref.summarize


def _checked_summarize(H, p, k):
    y = (torch.matmul(H.detach().double(), p.detach()) / torch.norm(p.detach(), 2))
    assert not bool(torch.isnan(y).any())
    if y.numel() > k:
        s = torch.sort(y, descending=True).values
        gap, scale = float(s[k - 1] - s[k]), float(y.abs().max())
        assert gap > GAP * scale, f"the restatement's scores {k} and {k + 1} are {gap:.2e} apart (max|score| {scale:.2e}): choose another seed"
    return _summarize(H, p, k)


@pytest.fixture
def gap(monkeypatch):
    """Every ref.summarize of the test asserts the gap condition on the restatement's own scores first."""
    monkeypatch.setattr(ref, "summarize", _checked_summarize)


def _shape(name, F, k):
    return (F, k) if name.startswith("B_") else (F, F)


def _draw(T, N, F, k, seed, draw="n01"):
    gen = torch.Generator().manual_seed(seed)
    s = 1.0 / math.sqrt(F) if draw == "scaled" else 1.0
    H = torch.randn(T, N, F, generator=gen)
    p = torch.randn(F, generator=gen).double()
    gates = [torch.randn(*_shape(n, F, k), generator=gen).double() * s for n in ref.GATES]
    W0 = torch.randn(F, k, generator=gen).double() * s
    R1, R2 = torch.randn(T + 1, F, k, generator=gen).double(), torch.randn(T, F, k, generator=gen)
    return H, p, gates, W0, R1, R2


def _summary(Ht, p, k):
    """ref.summarize; a slice with NaN scores: the numbers only, unfilled places idx = -1 with a zero row."""
    if not bool(torch.isnan(Ht).any()):
        return ref.summarize(Ht, p, k)
    y = torch.matmul(torch.nan_to_num(Ht.detach().double()), p.detach()) / torch.norm(p.detach(), 2)
    y[torch.isnan(Ht).any(dim=1)] = float("nan")
    idx = ref.topk_tie_rule(y, k)
    rows = Ht.double()[idx, :]
    ys = torch.matmul(rows, p) / torch.norm(p, 2)
    pad = k - len(idx)
    return (torch.cat((idx, torch.full((pad,), -1, dtype=torch.int64))), torch.cat((ys, ys.new_zeros(pad))),
            torch.cat((rows * ys.unsqueeze(1), rows.new_zeros(pad, Ht.shape[1]))))


def _ref_evolve(H, p, gates, W0, R1=None, R2=None, rank=None):
    """The restatement over all slices of H: (W_seq, idx, y_sel, rows, gradients of H, p, the gates and W0 for
    L = Σ W_seq·R1 + Σ W_seq[1:]·R2).  rank: the fp32 tensor whose scores rank (layer 2), H then being the fp64 rows."""
    want = R1 is not None
    leaves = [H.double().clone().requires_grad_(want), p.clone().requires_grad_(want)] + \
             [g.clone().requires_grad_(want) for g in gates] + [W0.clone().requires_grad_(want)]
    Hr, pr, W = leaves[0], leaves[1], leaves[11]
    q = dict(zip(ref.GATES, leaves[2:11]))
    k = W0.shape[1]
    seq, idx, ys, rows = [W], [], [], []
    for t in range(H.shape[0]):
        if rank is None:
            i, y, Zs = _summary(Hr[t], pr, k)
        else:
            i = ref.summarize(rank[t], pr, k)[0]
            y = torch.matmul(Hr[t][i, :], pr) / torch.norm(pr, 2)
            Zs = Hr[t][i, :] * y.unsqueeze(1)
        idx.append(i)
        ys.append(y.detach())
        rows.append(torch.where((i >= 0).unsqueeze(1), Hr[t].detach()[i.clamp(min=0), :], torch.zeros(())))
        W = ref.gru(Zs.t(), W, q)
        seq.append(W)
    Wseq = torch.stack(seq)
    if want:
        ((Wseq * R1).sum() + (Wseq[1:] * R2.double()).sum()).backward()
    st = (lambda v: torch.stack(v)) if idx else (lambda v: torch.zeros(0))
    return Wseq.detach(), st(idx), st(ys), st(rows), [x.grad for x in leaves]


def _packed(p, gates):
    return torch.cat([p.detach().reshape(-1)] + [g.detach().reshape(-1) for g in gates])


def _dev_leaves(H, p, gates, W0, H_grad):
    return [H.to(DEV).requires_grad_(H_grad), p.to(DEV).requires_grad_(True)] + \
           [g.to(DEV).requires_grad_(True) for g in gates] + [W0.to(DEV).requires_grad_(True)]


def _run(dev, R1, R2, rows=None):
    Wseq, W32 = ops.egcn_evolve(dev[0], dev[1], dev[2:11], dev[11], rows=rows)
    ((Wseq * R1.to(DEV)).sum() + (W32 * R2.to(DEV)).sum().double()).backward()
    return Wseq.detach(), W32.detach()


def _close(got, want, bar, what):
    scale = max(float(want.abs().max()), 1e-300)
    err = float((got.cpu().double() - want).abs().max()) / scale
    print(f"{what}: {err:.3e} (bar {bar:.1e})")
    assert err <= bar, f"{what}: {err:.3e} > {bar:.1e}"


def _check_evolve(T, N, F, k, seed, draw, H_grad=True):
    H, p, gates, W0, R1, R2 = _draw(T, N, F, k, seed, draw)
    Wr, idx_r, y_r, rows_r, gr = _ref_evolve(H, p, gates, W0, R1, R2)
    assert ops.egcn_evolve_route(F, k) == "wide"
    dev = _dev_leaves(H, p, gates, W0, H_grad)
    Wseq, W32 = _run(dev, R1, R2)
    what = f"T={T} N={N} F={F} k={k} {draw}"
    with torch.no_grad():
        out = ops.kernels.ops.egcn_wide_fwd(dev[0].detach(), _packed(dev[1], dev[2:11]), dev[11].detach(), k, T, False)
    np.testing.assert_array_equal(out[2].cpu().numpy(), idx_r.numpy(), err_msg=what)
    assert torch.equal(out[0], Wseq) and torch.equal(out[1], W32)
    _close(Wseq, Wr, F64_BAR, what + " W_seq")
    _close(out[3], y_r, F64_BAR, what + " y_sel")
    _close(out[4], rows_r, 0.0, what + " H_sel")
    assert torch.equal(W32.cpu(), Wseq[1:].float().cpu())
    names = ["H", "p"] + list(ref.GATES) + ["W_init"]
    for n, a, b in list(zip(names, dev, gr))[0 if H_grad else 1:]:
        if n == "p" and F == 1:
            # dp of F = 1 is zero in exact arithmetic (y = h·sign(p)): the restatement's is rounding noise
            assert float(a.grad.abs().max()) <= 1e-9 * max(float(gr[11].abs().max()), 1e-300)
            continue
        _close(a.grad, b, DH_BAR if n == "H" else F64_BAR, f"{what} d{n}")
    if not H_grad:
        assert dev[0].grad is None


# ---- routing --------------------------------------------------------------------------------------------------------
def test_routing(monkeypatch):
    for F, k in ((2, 6), (8, 8)):
        assert ops.egcn_evolve_route(F, k) == "narrow" and ops.egcn_supported(F, k) and not ops.egcn_wide_supported(F, k)
    for F, k in ((2, 9), (9, 8), (12, 3), (64, 64), (1, 64)):
        assert ops.egcn_evolve_route(F, k) == "wide" and ops.egcn_wide_supported(F, k) and not ops.egcn_supported(F, k)
    for F, k in ((2, 65), (65, 2)):
        assert ops.egcn_evolve_route(F, k) == "torch" and not ops.egcn_wide_supported(F, k)

    def refuse(*a, **kw):
        raise AssertionError("the torch path ran")
    monkeypatch.setattr(ops, "egcn_evolve_torch", refuse)
    H, p, gates, W0, _, _ = _draw(3, 50, 16, 32, 5)
    Wseq, W32 = ops.egcn_evolve(H.to(DEV), p.to(DEV), [g.to(DEV) for g in gates], W0.to(DEV))
    assert Wseq.shape == (4, 16, 32) and W32.shape == (3, 16, 32) and bool(torch.isfinite(Wseq).all())
    with pytest.raises(AssertionError, match="torch path"):
        H, p, gates, W0, _, _ = _draw(2, 70, 2, 65, 5)
        ops.egcn_evolve(H.to(DEV), p.to(DEV), [g.to(DEV) for g in gates], W0.to(DEV))


def test_narrow_route_unchanged():
    H, p, gates, W0, _, _ = _draw(5, 100, 6, 6, 66)
    assert ops.egcn_evolve_route(6, 6) == "narrow"
    d = [H.to(DEV), p.to(DEV)] + [g.to(DEV) for g in gates] + [W0.to(DEV)]
    with torch.no_grad():
        Wseq, W32 = ops.egcn_evolve(d[0], d[1], d[2:11], d[11])
        out = ops.kernels.ops.egcn_fwd(d[0], _packed(d[1], d[2:11]), d[11], 6, 5, False)
    assert torch.equal(Wseq, out[0]) and torch.equal(W32, out[1])
    with pytest.raises(RuntimeError, match="1..64"):
        ops.kernels.ops.egcn_wide_fwd(d[0], _packed(d[1], d[2:11]), d[11], 6, 5, False)


# ---- the kernels over their domain ----------------------------------------------------------------------------------
@pytest.mark.parametrize("draw", DRAWS)
@pytest.mark.parametrize("F,k", [(2, 9), (9, 2), (9, 9), (2, 12), (12, 3), (16, 16), (17, 33), (33, 17), (40, 48), (1, 64),
                                 (64, 1), (64, 9), (64, 64)])
def test_widths(gap, F, k, draw):
    _check_evolve(5, 130, F, k, seed=1000 + 100 * F + k, draw=draw)


@pytest.mark.parametrize("N", [32, 33, SELECT_BLOCK - 1, SELECT_BLOCK, SELECT_BLOCK + 1, 2 * SELECT_BLOCK + 1])
def test_node_counts(gap, N):
    """N = k (everything selected, the order still matters) and k + 1; one below, at and one above the nodes of one
    selection block; three blocks."""
    _check_evolve(5, N, 16, 32, seed=N, draw="scaled")


def test_large_slice():
    """2^18 + 3 nodes per slice, 257 selection blocks and the folds of the merge: indices and y_sel."""
    T, N, F, k = 2, 2 ** 18 + 3, 16, 32
    H, p, gates, W0, _, _ = _draw(T, N, F, k, seed=18, draw="scaled")
    with torch.no_grad():
        out = ops.kernels.ops.egcn_wide_fwd(H.to(DEV), _packed(p, gates).to(DEV), W0.to(DEV), k, T, False)
    for t in range(T):
        y = torch.matmul(H[t].double(), p) / torch.norm(p, 2)
        idx = ref.topk_tie_rule(y, k)
        np.testing.assert_array_equal(out[2][t].cpu().numpy(), idx.numpy())
        _close(out[3][t], y[idx], F64_BAR, f"y_sel slice {t}")


@pytest.mark.parametrize("T", [1, 2, 5, 7, 80])
def test_lengths(gap, T):
    _check_evolve(T, 63, 16, 32, seed=T, draw="scaled")


def test_tie_rule_across_the_cut_and_blocks():
    """80 identical rows (>= 2k) spread over the three selection blocks, ten better rows above them: the cut at k = 32
    falls inside the identical rows and takes the 22 lowest node indices, in order."""
    T, N, F, k = 3, 2500, 16, 32
    H, p, gates, W0, R1, R2 = _draw(T, N, F, k, seed=7, draw="scaled")
    H = H * 0.01
    v = torch.sign(p).float()                             # not parallel to p: dp does not cancel
    gen = torch.Generator().manual_seed(70)
    same = 900 + torch.randperm(N - 900, generator=gen)[:90]   # the selected identical rows span two selection blocks
    for t in range(T):
        H[t, same[:80]] = v * 5.0
        for r, n in enumerate(same[80:]):
            H[t, n] = v * (6.0 + r)
    Wr, idx_r, y_r, _, gr = _ref_evolve(H, p, gates, W0, R1, R2)
    want = sorted(same[80:].tolist(), key=lambda n: -same.tolist().index(n)) + sorted(same[:80].tolist())[:22]
    assert idx_r[0].tolist() == want and want[10] < SELECT_BLOCK <= want[31]
    dev = _dev_leaves(H, p, gates, W0, True)
    Wseq, _ = _run(dev, R1, R2)
    with torch.no_grad():
        out = ops.kernels.ops.egcn_wide_fwd(dev[0].detach(), _packed(dev[1], dev[2:11]), dev[11].detach(), k, T, False)
    np.testing.assert_array_equal(out[2].cpu().numpy(), idx_r.numpy())
    _close(Wseq, Wr, F64_BAR, "W_seq")
    for n, a, b in zip(["H", "p"] + list(ref.GATES) + ["W_init"], dev, gr):
        _close(a.grad, b, DH_BAR if n == "H" else F64_BAR, "d" + n)


def test_fewer_than_k_numbers():
    """Slice 1 has 20 numbers and 110 NaN scores: idx = -1 and a zero column in the 12 unfilled places; the NaN rows are
    never selected; the gradients are finite and those of the restatement."""
    T, N, F, k = 3, 130, 16, 32
    H, p, gates, W0, R1, R2 = _draw(T, N, F, k, seed=9, draw="scaled")
    H[1, 20:, 3] = float("nan")
    H[0, 5, 0] = float("nan")
    Wr, idx_r, y_r, rows_r, gr = _ref_evolve(H, p, gates, W0, R1, R2)
    assert idx_r[1, 20:].tolist() == [-1] * 12 and 5 not in idx_r[0].tolist()
    dev = _dev_leaves(H, p, gates, W0, True)
    Wseq, _ = _run(dev, R1, R2)
    with torch.no_grad():
        out = ops.kernels.ops.egcn_wide_fwd(dev[0].detach(), _packed(dev[1], dev[2:11]), dev[11].detach(), k, T, False)
    np.testing.assert_array_equal(out[2].cpu().numpy(), idx_r.numpy())
    assert float(out[5][1, :, 20:].abs().max()) == 0.0 and float(out[3][1, 20:].abs().max()) == 0.0     # X_g, y_sel
    _close(out[3], y_r, F64_BAR, "y_sel")
    _close(Wseq, Wr, F64_BAR, "W_seq")
    for n, a, b in zip(["H", "p"] + list(ref.GATES) + ["W_init"], dev, gr):
        assert bool(torch.isfinite(a.grad).all()), n
        _close(a.grad, torch.nan_to_num(b), DH_BAR if n == "H" else F64_BAR, "d" + n)
    assert float(dev[0].grad[1, 20:].abs().sum()) == 0.0 and float(dev[0].grad[0, 5].abs().sum()) == 0.0


@pytest.mark.parametrize("Fp", [12, 64])
def test_layer2_rows(gap, Fp):
    """rows = (A, X_prev, W_prev_seq): the fp32 H ranks, the selected rows are formed again in fp64."""
    T, N, F, k = 5, 130, 16, 32
    H, p, gates, W0, R1, R2 = _draw(T, N, F, k, seed=Fp, draw="scaled")
    gen = torch.Generator().manual_seed(1000 + Fp)
    A = []
    for _ in range(T):
        r, c = torch.randint(0, N, (4 * N,), generator=gen), torch.randint(0, N, (4 * N,), generator=gen)
        a = torch.sparse_coo_tensor(torch.stack([r, c]), torch.rand(4 * N, generator=gen).double(), (N, N)).coalesce()
        # fp32-representable values after the duplicates are summed, as the device CSR is fp32
        A.append(torch.sparse_coo_tensor(a.indices(), a.values().float().double(), (N, N)).coalesce())
    Xp = torch.randn(T, N, Fp, generator=gen)
    Wp = torch.randn(T + 1, Fp, F, generator=gen).double() / math.sqrt(Fp)
    H64 = torch.stack([torch.relu(torch.sparse.mm(A[t], Xp[t].double()) @ Wp[t + 1]) for t in range(T)])
    H32 = H64.float()
    Wr, idx_r, y_r, rows_r, gr = _ref_evolve(H64, p, gates, W0, R1, R2, rank=H32)
    dev = _dev_leaves(H32, p, gates, W0, True)
    A_csr, Xd, Wd = _adj(A, N, torch.device(DEV)), Xp.to(DEV), Wp.to(DEV)
    Wseq, _ = _run(dev, R1, R2, rows=(A_csr, Xd, Wd))
    with torch.no_grad():
        out = ops.kernels.ops.egcn_wide_fwd(dev[0].detach(), _packed(dev[1], dev[2:11]), dev[11].detach(), k, T, False,
                                            A_csr.rowptr, A_csr.col, A_csr.val, Xd, Wd)
    np.testing.assert_array_equal(out[2].cpu().numpy(), idx_r.numpy())
    _close(out[4], rows_r, 1e-12, "H_sel")
    _close(out[3], y_r, 1e-12, "y_sel")
    _close(Wseq, Wr, F64_BAR, "W_seq")
    for n, a, b in zip(["H", "p"] + list(ref.GATES) + ["W_init"], dev, gr):
        _close(a.grad, b, DH_BAR if n == "H" else F64_BAR, "d" + n)


def test_early_stop():
    T, N, F, k = 5, 130, 16, 32
    H, p, gates, W0, _, _ = _draw(T, N, F, k, seed=3, draw="scaled")
    d = [H.to(DEV), p.to(DEV)] + [g.to(DEV) for g in gates] + [W0.to(DEV)]
    with torch.no_grad():
        full, full32 = ops.egcn_evolve(d[0], d[1], d[2:11], d[11])
        part, part32 = ops.egcn_evolve(d[0], d[1], d[2:11], d[11], T_run=3)
        none, none32 = ops.egcn_evolve(d[0], d[1], d[2:11], d[11], T_run=0)
    assert part.shape == (4, F, k) and torch.equal(part, full[:4]) and torch.equal(part32, full32[:3])
    assert none.shape == (1, F, k) and torch.equal(none[0], d[11]) and none32.shape == (0, F, k)
    leaves = _dev_leaves(H, p, gates, W0, False)                  # T_run = 0 with a backward: dW_init = dW_seq[0]
    Wseq, _ = ops.egcn_evolve(leaves[0], leaves[1], leaves[2:11], leaves[11], T_run=0)
    (Wseq * 2.0).sum().backward()
    assert float((leaves[11].grad - 2.0).abs().max()) == 0.0 and float(leaves[1].grad.abs().max()) == 0.0


@pytest.mark.parametrize("F,k,N", [(33, 17, 1100), (64, 64, 130)])
def test_same_bits_on_every_run(F, k, N):
    H, p, gates, W0, R1, R2 = _draw(5, N, F, k, seed=11, draw="scaled")
    runs = []
    for _ in range(2):
        dev = _dev_leaves(H, p, gates, W0, True)
        Wseq, W32 = _run(dev, R1, R2)
        runs.append([Wseq.cpu(), W32.cpu()] + [x.grad.cpu() for x in dev])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- the models -----------------------------------------------------------------------------------------------------
SHAPES = {"w32": (5, 300, 12, [32, 16, 3], 1), "w64": (5, 130, 64, [64, 64, 3], 2), "w12": (5, 300, 2, [12, 2], 3)}


def _case(name):
    T, N, F0, hidden, seed = SHAPES[name]
    gen = torch.Generator().manual_seed(seed)
    A = []
    for _ in range(T):
        # 4·N entries of mean 1/4: rows sum to 1 on average, as those of a normalised adjacency do.  With entries of
        # mean 1/2 the first loss is 53 and SGD at the drivers' lr = 0.01 does not settle: no two implementations stay
        # within 1e-5 over 10 such steps (measured: the torch route leaves the restatement twin at step 4 as well)
        r, c = torch.randint(0, N, (4 * N,), generator=gen), torch.randint(0, N, (4 * N,), generator=gen)
        A.append(torch.sparse_coo_tensor(torch.stack([r, c]), torch.rand(4 * N, generator=gen).double() / 2, (N, N)).coalesce())
    X = torch.randn(T, N, F0, generator=gen).double()    # fp32-representable values, as the device copies are fp32
    E = 400
    edges = torch.stack([torch.randint(0, T, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen),
                         torch.randint(0, N, (E,), generator=gen)])
    target = torch.randint(0, hidden[-1], (E,), generator=gen)
    return T, N, F0, hidden, seed, A, X, edges, target


def _model(name, draw, cls=None):
    T, N, F0, hidden, seed, A, X, edges, target = _case(name)
    layers = len(hidden) - 1
    torch.manual_seed(seed)
    if cls is None:
        cls = evolvegcn.EvolveGCN_1_layer if layers == 1 else evolvegcn.EvolveGCN_2_layer
    m = cls(A, X, edges, hidden, device=DEV) if cls is not evolvegcn.EvolveGCN_reg else cls(A, X, hidden, device=DEV)
    if draw == "scaled":
        with torch.no_grad():
            for i, s in enumerate(["", "2"][:layers]):
                f = 1.0 / math.sqrt(m.F[i])
                for g in m.gates(s):
                    g.mul_(f)
                getattr(m, "W_init" + s).mul_(f)
    d = {n + "0": getattr(m, n).detach().cpu().numpy() for n in ref.names(layers)}
    d["W_init"] = m.W_init.cpu().numpy()
    if layers == 2:
        d["W_init2"] = m.W_init2.cpu().numpy()
    return m, d


@pytest.mark.parametrize("draw", DRAWS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_models_against_restatement(gap, name, draw):
    T, N, F0, hidden, seed, A, X, edges, target = _case(name)
    layers = len(hidden) - 1
    m, d = _model(name, draw)
    for i in range(layers):
        assert ops.egcn_evolve_route(m.F[i], m.F[i + 1]) == "wide"
    res = m()
    loss = torch.nn.CrossEntropyLoss()(res[0], target.to(DEV))
    loss.backward()
    w = torch.ones(hidden[-1])
    r32 = ref.train_step(A, X, d, layers, edges.numpy(), target.numpy(), w)
    r64 = ref.train_step(A, X, d, layers, edges.numpy(), target.numpy(), w, out_dtype=torch.float64)
    what = f"{name} {draw}"
    _bar(res[0].detach().cpu(), r32[0], r64[0], what + " logits")
    _bar(torch.tensor([float(loss.detach())]), torch.tensor([float(r32[1])]), torch.tensor([float(r64[1])]), what + " loss")
    _close(res[1].detach(), r64[3][0].detach(), F64_BAR, what + " W_T")
    if layers == 2:
        _bar(res[2].detach().cpu(), r32[3][1].detach(), r64[3][1].detach(), what + " W2_T")
    for n in ref.names(layers):
        _bar(getattr(m, n).grad.cpu(), r32[2][n], r64[2][n], f"{what} d{n}")
    # a validation-style call: the first three slices with the returned W going back in
    q = ref.params(d, layers, grad=False)
    ev = torch.stack([torch.randint(0, 3, (50,)), torch.randint(0, N, (50,)), torch.randint(0, N, (50,))])
    with torch.no_grad():
        rv = m(A[:3], X[:3], ev, *res[1:])
        W_in = [x.detach().cpu() for x in res[1:]]
        out = []
        for dt in (torch.float32, torch.float64):
            Y, Ws = ref.embed(A[:3], X[:3], q, W_in[0], T, W_in[1] if layers == 2 else None, dt)
            out.append((ref.edge_logits(Y, ev.numpy(), q["U"].to(dt)), Ws))
    _bar(rv[0].cpu(), out[0][0], out[1][0], what + " validation logits")
    _close(rv[1], out[1][1][0], F64_BAR, what + " validation W_T")


@pytest.mark.parametrize("draw", DRAWS)
def test_reg_against_restatement(gap, draw):
    T, N, F0, _, seed, A, X, _, _ = _case("w12")
    hidden = [16, 2]
    gen = torch.Generator().manual_seed(31)
    A = A[:T]
    torch.manual_seed(seed)
    m = evolvegcn.EvolveGCN_reg(A, X, hidden, device=DEV)
    if draw == "scaled":
        with torch.no_grad():
            for g in m.gates():
                g.mul_(1.0 / math.sqrt(F0))
            m.W_init.mul_(1.0 / math.sqrt(F0))
    assert ops.egcn_evolve_route(F0, 16) == "wide"
    y = m()
    R = torch.randn(T, N, generator=gen)
    (torch.as_tensor(y) * R.to(DEV)).sum().backward()
    names = ref.names(1)[:-1]
    res = []
    for dt in (torch.float32, torch.float64):
        q = {n: getattr(m, n).detach().cpu().clone().requires_grad_(True) for n in names}
        Y, Ws = ref.embed(A, X, q, m.W_init.cpu(), T, None, dt)
        lw, lb = m.lin1.weight.detach().cpu().to(dt).requires_grad_(True), m.lin1.bias.detach().cpu().to(dt)
        out = (Y @ lw.t() + lb).squeeze(2)
        (out * R.to(dt)).sum().backward()
        res.append((out.detach(), {n: q[n].grad for n in names}, lw.grad))
    _bar(torch.as_tensor(y).detach().cpu(), res[0][0], res[1][0], f"reg {draw} output")
    for n in names:
        _bar(getattr(m, n).grad.cpu(), res[0][1][n], res[1][1][n], f"reg {draw} d{n}")
    _bar(m.lin1.weight.grad.cpu(), res[0][2], res[1][2], f"reg {draw} dlin1.weight")
    with torch.no_grad():
        y3 = m(A[:3], X[:3], m.W_init.cpu())
        q = {n: getattr(m, n).detach().cpu() for n in names}
        Y, _ = ref.embed(A[:3], X[:3], q, m.W_init.cpu(), T, None, torch.float32)
        want = (Y @ m.lin1.weight.detach().cpu().t() + m.lin1.bias.detach().cpu()).squeeze(2)
    assert max_rel_err(torch.as_tensor(y3).cpu(), want) <= 1e-5


@pytest.mark.parametrize("name", list(SHAPES))
def test_models_sgd_10_steps(gap, name):
    """10 steps of torch.optim.SGD against a restatement twin on the CPU, with the bars of test_chess_sgd_20_epochs.
    lr = 0.001: the selection changes as p moves, so the loss jumps from step to step, and at the drivers' lr = 0.01 the
    restatement's own fp32-output and fp64-output runs of the 64-wide shape part ways (2.9e-1 in the losses of these 10
    steps); at 0.001 they stay within 2e-7 of each other on all three shapes."""
    T, N, F0, hidden, seed, A, X, edges, target = _case(name)
    layers = len(hidden) - 1
    m, d = _model(name, "scaled")
    opt = torch.optim.SGD(m.parameters(), lr=0.001, momentum=0.9)
    q = ref.params(d, layers)
    opt_r = torch.optim.SGD(list(q.values()), lr=0.001, momentum=0.9)
    crit = torch.nn.CrossEntropyLoss()
    w = torch.ones(hidden[-1])
    losses, losses_r = [], []
    for _ in range(10):
        opt.zero_grad()
        loss = crit(m()[0], target.to(DEV))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        opt_r.zero_grad()
        losses_r.append(float(ref.train_step(A, X, d, layers, edges.numpy(), target.numpy(), w, q=q)[1]))
        opt_r.step()
    err = max_rel_err(torch.tensor(losses), torch.tensor(losses_r))
    record_tolerance(f"EvolveGCN wide {name} SGD losses", err, 1e-5)
    assert err <= 1e-5, err
    for n in ref.names(layers):
        e = max_rel_err(getattr(m, n).detach().cpu(), q[n].detach())
        record_tolerance(f"EvolveGCN wide {name} SGD final {n}", e, 1e-4)
        assert e <= 1e-4, (n, e)


def test_graphed_step_equals_eager_step():
    T, N, F0, hidden, seed, A, X, edges, target = _case("w32")
    target = target.to(DEV)
    crit = torch.nn.CrossEntropyLoss(weight=torch.ones(3, device=DEV))
    eager, graphed = _model("w32", "scaled")[0], _model("w32", "scaled")[0]
    opt_e = torch.optim.SGD(eager.parameters(), lr=0.01, momentum=0.9)
    opt_g = torch.optim.SGD(graphed.parameters(), lr=0.01, momentum=0.9)
    step = GraphedTrainStep(graphed, crit, opt_g, target, warmup=1)
    for _ in range(2):
        opt_e.zero_grad(set_to_none=True)
        le = eager.loss(crit, target, unit_grad=True)
        le.backward(gradient=ops.unit_gradient(DEV))
        opt_e.step()
    lg = step()
    torch.cuda.synchronize()
    assert float(lg.detach()) == float(le.detach())
    for n in ref.names(2):
        assert torch.equal(getattr(eager, n).detach(), getattr(graphed, n).detach()), n
