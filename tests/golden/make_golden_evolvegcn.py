"""Generate the EvolveGCN fixtures tests/golden/g13_egcn_*.npz by running the REAL reference model.

Run where the reference is checked out (the GPU tests need only the committed .npz files):

    python tests/golden/make_golden_evolvegcn.py PATH/TO/TensorGCN-master

It imports TensorGCN-master/evolvegcn_functions.py ("ef", with the empty torchvision stub of make_golden.py) and runs
  * g13_egcn_chess     EvolveGCN_2_layer(C_train, X_train, edges_train, [6,6,3]) on the whole chess data set of G10,
                       built the way experiment_chess_evolvegcn.py builds it (slices 0..79 of the normalised adjacency,
                       degree features, class weights .33): initial parameters and W_inits, logits, loss, every
                       gradient, the selected indices and scores of every summary call, the validation and test calls
                       with W chained, 20 SGD epochs (lr .01, momentum .9) and an fp64 truth of loss and
                       gradients (the same module under torch.set_default_dtype(float64), U cast to float64);
  * g13_egcn_chess_lp  EvolveGCN_1_layer(C[:79], X[:79], e_train, [6,2]) in the link-prediction shape: the labelled
                       edge set (the training edges of slices 1..79 moved one slice back, plus as many seeded
                       non-edges) is stored in the fixture, since the script samples its non-edges unseeded;
  * g13_egcn_small_*   T = 5, N in {6, 7, 200}: N = k, width 1 and [3,8,8,2]; and one EvolveGCN_reg case with the
                       no-W_init call quirk.
For every summary call it asserts that no tie or near-tie (relative gap < 1e-6) at the k-th rank involves rows that
differ, and records the smallest relative gap between the k-th and (k+1)-th score of each case.
Fixtures are data only (arrays): no reference source text is stored.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "evolvegcn_functions.py")):
    sys.exit("usage: make_golden_evolvegcn.py PATH/TO/TensorGCN-master (the directory that holds evolvegcn_functions.py)")
REF = os.path.abspath(sys.argv[1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

for m in ("torchvision", "torchvision.datasets"):
    sys.modules.setdefault(m, types.ModuleType(m))
sys.modules["torchvision"].datasets = sys.modules["torchvision.datasets"]
sys.path.insert(0, REF)
import evolvegcn_functions as ef  # noqa: E402  (the real reference)

from _g10 import G10  # noqa: E402

torch.set_num_threads(8)
GATES = ("W_Z", "U_Z", "B_Z", "W_R", "U_R", "B_R", "W_H", "U_H", "B_H")
NEAR = 1e-6


def names(layers):
    out = []
    for s in ([""] if layers == 1 else ["", "2"]):
        out += ["p" + s] + [g + s for g in GATES]
    return out + ["U"]


class Recorder:
    """Wraps a model's summarize: records (layer, idx, scores) of every call, checks the k-th rank."""

    def __init__(self, gcn):
        self.calls, self.min_gap = [], np.inf
        orig = gcn.summarize

        def wrapped(X, k, *l):
            p = gcn.p if not l or l[0] == 1 else gcn.p2
            with torch.no_grad():                 # the same operators as the model's summary, so the same indices
                y = (X @ p) / p.norm(2)
                idx = y.topk(k).indices
                self.check(X, y, k)
            self.calls.append((l[0] if l else 1, idx.numpy().astype(np.int32), y[idx].numpy().copy()))
            return orig(X, k, *l)

        gcn.summarize = wrapped

    def check(self, X, y, k):
        ys = torch.sort(y, descending=True).values
        if len(ys) <= k:
            return
        yk, yk1 = float(ys[k - 1]), float(ys[k])
        gap = (yk - yk1) / max(abs(yk), 1e-300)
        self.min_gap = min(self.min_gap, gap)
        if gap < NEAR:
            near = torch.nonzero((y - yk).abs() <= NEAR * max(abs(yk), 1e-300)).flatten()
            rows = X[near]
            assert bool((rows == rows[0]).all()), f"a near-tie at the k-th rank between rows that differ: nodes {near.tolist()}"

    def take(self, out, prefix):
        for layer in (1, 2):
            c = [x for x in self.calls if x[0] == layer]
            if c:
                out[f"{prefix}idx{layer}"] = np.stack([x[1] for x in c])
                out[f"{prefix}ysel{layer}"] = np.stack([x[2] for x in c])
        self.calls = []


def sparse_list(k, i, j, v, slices, N):
    out = []
    for s in slices:
        m = k == s
        out.append(torch.sparse_coo_tensor(torch.tensor(np.stack([i[m], j[m]]), dtype=torch.long),
                                           torch.tensor(v[m], dtype=torch.float64), (N, N)).coalesce())
    return out


def record_model(gcn, layers, out):
    for n in names(layers):
        out[n + "0"] = getattr(gcn, n).detach().numpy().copy()
    out["W_init"] = gcn.W_init.numpy().copy()
    if layers == 2:
        out["W_init2"] = gcn.W_init2.numpy().copy()
    out["param_names"] = np.array([n for n, _ in gcn.named_parameters()])
    out["param_dtypes"] = np.array([str(q.dtype) for _, q in gcn.named_parameters()])


def run_train(gcn, layers, crit, target, out, prefix=""):
    res = gcn()
    loss = crit(res[0], target)
    loss.backward()
    out[prefix + "logits"], out[prefix + "loss"] = res[0].detach().numpy(), np.float64(loss.item())
    for n in names(layers):
        out[prefix + "d" + n] = getattr(gcn, n).grad.numpy().copy()
    return res


def fp64_truth(gcn, layers, target, weight, out):
    """logits, loss and gradients with the Y buffer and U in float64 (everything else already is)."""
    gcn.U.data = gcn.U.data.double()
    for n in names(layers):
        getattr(gcn, n).grad = None
    torch.set_default_dtype(torch.float64)        # Y = t.zeros(...) takes the default dtype (ef:66, 164)
    try:
        res = gcn()
        loss = torch.nn.CrossEntropyLoss(weight=torch.tensor(weight, dtype=torch.float64))(res[0], target)
        loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    out["loss64"] = np.float64(loss.item())
    for n in names(layers):
        out["d" + n + "64"] = getattr(gcn, n).grad.numpy().copy()


def chess():
    g = G10()
    k, i, j, v = g.C()
    N, T = g.N, g.T
    C_train = sparse_list(k, i, j, v, range(T), N)
    C_val = sparse_list(k, i, j, v, range(T, T + g.S_val), N)
    C_test = sparse_list(k, i, j, v, range(T + g.S_val, g.TT), N)
    X_train, X_val, X_test = (torch.tensor(x) for x in (g.X[:T], g.X[T:T + g.S_val], g.X[T + g.S_val:]))
    ek = g.edges_all[0]
    te = ek >= T + g.S_val
    edges_test = g.edges_all[:, te].copy()
    edges_test[0] -= T + g.S_val
    edges_train, edges_val = torch.tensor(g.edges_train), torch.tensor(g.edges_val_b)
    target = torch.tensor(g.target_train)
    weight = np.array([.33, .33, .33], np.float32)
    crit = torch.nn.CrossEntropyLoss(weight=torch.tensor(weight))
    out = {"seed": np.int64(13)}
    torch.manual_seed(13)
    gcn = ef.EvolveGCN_2_layer(C_train, X_train, edges_train, [6, 6, 3])
    record_model(gcn, 2, out)
    rec = Recorder(gcn)
    _, W_val, W2_val = run_train(gcn, 2, crit, target, out)
    rec.take(out, "")
    with torch.no_grad():
        o_val, W_test, W2_test = gcn(C_val, X_val, edges_val, W_val, W2_val)
        rec.take(out, "val_")
        o_test, _, _ = gcn(C_test, X_test, torch.tensor(edges_test), W_test, W2_test)
        rec.take(out, "test_")
    out["logits_val"], out["logits_test"] = o_val.numpy(), o_test.numpy()
    out["W_val"], out["W2_val"], out["W_test"], out["W2_test"] = (w.detach().numpy() for w in (W_val, W2_val, W_test, W2_test))
    # 20 SGD epochs from the same start (the script's loop: zero_grad, gcn(), criterion, backward, step)
    torch.manual_seed(13)
    gcn = ef.EvolveGCN_2_layer(C_train, X_train, edges_train, [6, 6, 3])
    rec2 = Recorder(gcn)
    opt = torch.optim.SGD(gcn.parameters(), lr=0.01, momentum=0.9)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        l = crit(gcn()[0], target)
        l.backward()
        opt.step()
        losses.append(l.item())
        rec2.calls = []
    out["sgd_losses"] = np.array(losses, np.float64)
    for n in names(2):
        out["sgd_" + n] = getattr(gcn, n).detach().numpy().copy()
    torch.manual_seed(13)
    gcn = ef.EvolveGCN_2_layer(C_train, X_train, edges_train, [6, 6, 3])
    fp64_truth(gcn, 2, target, weight, out)
    out["min_gap"] = np.float64(min(rec.min_gap, rec2.min_gap))
    print("chess: smallest relative gap at the k-th rank", out["min_gap"])
    np.savez_compressed(os.path.join(HERE, "g13_egcn_chess.npz"), **out)


def chess_lp():
    g = G10()
    k, i, j, v = g.C()
    N, T = g.N, g.T
    C_train = sparse_list(k, i, j, v, range(T - 1), N)
    X_train = torch.tensor(g.X[:T - 1])
    rng = np.random.default_rng(13)
    pos = g.edges_train[:, g.edges_train[0] >= 1].copy()
    pos[0] -= 1                                              # slice t+1's edges, predicted from slice t
    neg = np.stack([pos[0], rng.integers(0, N, pos.shape[1]), rng.integers(0, N, pos.shape[1])])
    edges = np.concatenate([pos, neg], axis=1)
    target = np.concatenate([np.ones(pos.shape[1], np.int64), np.zeros(neg.shape[1], np.int64)])
    weight = np.array([.1, .9], np.float32)
    # the non-edges only (int16 node ids): the positives and the targets follow from G10 (tests/_evolvegcn_ref.lp_edges)
    out = {"seed": np.int64(14), "neg": neg[1:].astype(np.int16), "weight": weight}
    torch.manual_seed(14)
    gcn = ef.EvolveGCN_1_layer(C_train, X_train, torch.tensor(edges), [6, 2])
    record_model(gcn, 1, out)
    rec = Recorder(gcn)
    crit = torch.nn.CrossEntropyLoss(weight=torch.tensor(weight))
    _, W_T = run_train(gcn, 1, crit, torch.tensor(target), out)
    rec.take(out, "")
    out["W_T"] = W_T.detach().numpy()
    torch.manual_seed(14)
    gcn = ef.EvolveGCN_1_layer(C_train, X_train, torch.tensor(edges), [6, 2])
    fp64_truth(gcn, 1, torch.tensor(target), weight, out)
    out["min_gap"] = np.float64(rec.min_gap)
    print("chess LP: smallest relative gap at the k-th rank", out["min_gap"])
    np.savez_compressed(os.path.join(HERE, "g13_egcn_chess_lp.npz"), **out)


def small(name, T, N, F0, hidden, seed, reg=False):
    rng = np.random.default_rng(seed)
    ks, is_, js, vs = [], [], [], []
    for s in range(T):
        nnz = 3 * N
        key = np.unique(rng.integers(0, N, nnz) * N + rng.integers(0, N, nnz))
        ks.append(np.full(len(key), s))
        is_.append(key // N)
        js.append(key % N)
        vs.append(rng.random(len(key)).astype(np.float32))
    k, i, j, v = (np.concatenate(a) for a in (ks, is_, js, vs))
    X = rng.standard_normal((T, N, F0)).astype(np.float32).astype(np.float64)
    A = sparse_list(k, i, j, v, range(T), N)
    layers = len(hidden) - 1
    out = {"T": np.int64(T), "N": np.int64(N), "hidden": np.array(hidden), "A_k": k, "A_i": i, "A_j": j, "A_v": v,
           "X": X, "seed": np.int64(seed)}
    torch.manual_seed(seed)
    if reg:
        gcn = ef.EvolveGCN_reg(A, torch.tensor(X), list(hidden))
        record_model(gcn, 1, out)
        out["lin_w0"], out["lin_b0"] = gcn.lin1.weight.detach().numpy().copy(), gcn.lin1.bias.detach().numpy().copy()
        rec = Recorder(gcn)
        y = gcn()
        (y ** 2).mean().backward()
        out["out"] = y.detach().numpy()
        out["dlin_w"], out["dlin_b"] = gcn.lin1.weight.grad.numpy().copy(), gcn.lin1.bias.grad.numpy().copy()
        for n in names(1)[:-1]:
            out["d" + n] = getattr(gcn, n).grad.numpy().copy()
        with torch.no_grad():
            out["out_call"] = gcn(A[:3], torch.tensor(X[:3])).numpy()     # no W_init: the training output (ef:342)
            W0 = torch.tensor(out["W_init"]) * 0.5
            out["W_call"] = W0.numpy()
            out["out_call_w"] = gcn(A[:3], torch.tensor(X[:3]), W0).numpy()   # with W_init: 3 slices, the rest zero
    else:
        cls = ef.EvolveGCN_1_layer if layers == 1 else ef.EvolveGCN_2_layer
        C = hidden[-1]
        E = 4 * N
        edges = np.stack([rng.integers(0, T, E), rng.integers(0, N, E), rng.integers(0, N, E)])
        target = rng.integers(0, C, E)
        weight = rng.random(C).astype(np.float32) + 0.5
        out.update(edges=edges, target=target, weight=weight)
        gcn = cls(A, torch.tensor(X), torch.tensor(edges), list(hidden))
        record_model(gcn, layers, out)
        rec = Recorder(gcn)
        crit = torch.nn.CrossEntropyLoss(weight=torch.tensor(weight))
        res = run_train(gcn, layers, crit, torch.tensor(target), out)
        rec.take(out, "")
        for q, w in enumerate(res[1:]):
            out[f"W_T{q + 1}"] = w.detach().numpy()
        Ev = 2 * N
        edges_v = np.stack([rng.integers(0, 3, Ev), rng.integers(0, N, Ev), rng.integers(0, N, Ev)])
        out["edges_val"] = edges_v
        with torch.no_grad():
            rv = gcn(A[:3], torch.tensor(X[:3]), torch.tensor(edges_v), *res[1:])
        out["logits_val"] = rv[0].numpy()
        for q, w in enumerate(rv[1:]):
            out[f"W_val{q + 1}"] = w.numpy()
    out["min_gap"] = np.float64(rec.min_gap)
    print(name, "smallest relative gap at the k-th rank", out["min_gap"])
    np.savez_compressed(os.path.join(HERE, f"g13_egcn_small_{name}.npz"), **out)


if __name__ == "__main__":
    small("n6_k6", 5, 6, 2, [6, 2], 1)
    small("n7_w1", 5, 7, 1, [1, 1, 2], 2)
    small("n200_3882", 5, 200, 3, [8, 8, 2], 3)
    small("reg_n50", 5, 50, 2, [6, 2], 4, reg=True)
    chess_lp()
    chess()
