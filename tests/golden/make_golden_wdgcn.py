"""Generate the WD-GCN fixtures tests/golden/g12_wdgcn_*.npz by running the REAL reference model.

Run where the reference is checked out (the GPU tests need only the committed .npz files):

    python tests/golden/make_golden_wdgcn.py PATH/TO/TensorGCN-master

It imports TensorGCN-master/wd_gcn_functions.py ("wgf", with the empty torchvision stub of make_golden.py) and runs
  * g12_wdgcn_chess   WD_GCN(C_train, X_train, edges_train, [6,3]) on the whole chess data set of G10, built the way
                      experiment_chess_wd-gcn.py:36-90 builds it (slices 0..79 of the normalised adjacency C, degree
                      features, class weights .33): initial parameters and the three plain tensors, logits, loss, the
                      13 gradients, the validation logits on the 10 slices after the training block, 20 SGD epochs
                      (lr .01, momentum .9), and an fp64 truth of loss and gradients (the same module, every parameter
                      and plain tensor cast to float64);
  * g12_wdgcn_small_* T = 5, N = 7..200, H in {1, 6, 8}, synthetic inputs stored in the fixture, a validation call on
                      3 of the 5 slices (zero-padded AX) — and one WD_GCN_reg case.
Fixtures are data only (arrays): no reference source text is stored.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "wd_gcn_functions.py")):
    sys.exit("usage: make_golden_wdgcn.py PATH/TO/TensorGCN-master (the directory that holds wd_gcn_functions.py)")
REF = os.path.abspath(sys.argv[1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

for m in ("torchvision", "torchvision.datasets"):
    sys.modules.setdefault(m, types.ModuleType(m))
sys.modules["torchvision"].datasets = sys.modules["torchvision.datasets"]
sys.path.insert(0, REF)
import wd_gcn_functions as wgf  # noqa: E402  (the real reference)

from _g10 import G10  # noqa: E402

torch.set_num_threads(8)
NAMES = ("W", "Wf", "Wj", "Wc", "Wo", "Uf", "Uj", "Uc", "Uo", "bf", "bj", "bc", "bo")


def sparse_list(k, i, j, v, slices, N):
    out = []
    for s in slices:
        m = k == s
        out.append(torch.sparse_coo_tensor(torch.tensor(np.stack([i[m], j[m]]), dtype=torch.long),
                                           torch.tensor(v[m], dtype=torch.float64), (N, N)).coalesce())
    return out


def record_model(gcn, out, prefix=""):
    for n in NAMES:
        out[prefix + n + "0"] = getattr(gcn, n).detach().numpy().copy()
    for n in ("h_init", "c_init", "U"):
        out[prefix + n] = getattr(gcn, n).detach().numpy().copy()


def fp64_truth(gcn, target, weight, out, prefix=""):
    """loss and gradients of the same module with every parameter and plain tensor in float64."""
    for n in NAMES:
        getattr(gcn, n).data = getattr(gcn, n).data.double()
        getattr(gcn, n).grad = None
    for n in ("h_init", "c_init", "U"):
        setattr(gcn, n, getattr(gcn, n).double())
    gcn.AX = gcn.AX.double()
    torch.set_default_dtype(torch.float64)        # the LSTM's output buffer is a t.zeros of the default dtype (wgf:89)
    try:
        loss = torch.nn.CrossEntropyLoss(weight=torch.tensor(weight, dtype=torch.float64))(gcn(), target)
        loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    out[prefix + "loss64"] = np.float64(loss.item())
    for n in NAMES:
        out[prefix + "d" + n + "64"] = getattr(gcn, n).grad.numpy().copy()


def chess():
    g = G10()
    k, i, j, v = g.C()
    N, T = g.N, g.T
    C_train = sparse_list(k, i, j, v, range(T), N)
    C_val = sparse_list(k, i, j, v, range(T, T + g.S_val), N)
    X_train, X_val = torch.tensor(g.X[:T]), torch.tensor(g.X_val_b)
    edges_train, edges_val = torch.tensor(g.edges_train), torch.tensor(g.edges_val_b)
    target = torch.tensor(g.target_train)
    weight = np.array([.33, .33, .33], np.float32)
    crit = torch.nn.CrossEntropyLoss(weight=torch.tensor(weight))
    out = {"seed": np.int64(12)}
    torch.manual_seed(12)
    gcn = wgf.WD_GCN(C_train, X_train, edges_train, [6, 3])
    record_model(gcn, out)
    logits = gcn()
    loss = crit(logits, target)
    loss.backward()
    out["logits"], out["loss"] = logits.detach().numpy(), np.float64(loss.item())
    for n in NAMES:
        out["d" + n] = getattr(gcn, n).grad.numpy().copy()
    with torch.no_grad():
        out["logits_val"] = gcn(C_val, X_val, edges_val).numpy()
    # 20 SGD epochs from the same start (the script's loop: zero_grad, gcn(), criterion, backward, step)
    torch.manual_seed(12)
    gcn = wgf.WD_GCN(C_train, X_train, edges_train, [6, 3])
    opt = torch.optim.SGD(gcn.parameters(), lr=0.01, momentum=0.9)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        l = crit(gcn(), target)
        l.backward()
        opt.step()
        losses.append(l.item())
    out["sgd_losses"] = np.array(losses, np.float64)
    for n in NAMES:
        out["sgd_" + n] = getattr(gcn, n).detach().numpy().copy()
    torch.manual_seed(12)
    gcn = wgf.WD_GCN(C_train, X_train, edges_train, [6, 3])
    fp64_truth(gcn, target, weight, out)
    np.savez_compressed(os.path.join(HERE, "g12_wdgcn_chess.npz"), **out)


def small(name, T, N, H, C, nnz_per_slice, seed, reg=False):
    rng = np.random.default_rng(seed)
    ks, is_, js, vs = [], [], [], []
    for s in range(T):
        r = rng.integers(0, N, nnz_per_slice)
        c = rng.integers(0, N, nnz_per_slice)
        key = np.unique(r * N + c)
        ks.append(np.full(len(key), s))
        is_.append(key // N)
        js.append(key % N)
        vs.append(rng.random(len(key)).astype(np.float32))
    k, i, j, v = (np.concatenate(a) for a in (ks, is_, js, vs))
    X = rng.integers(0, 4, (T, N, 2)).astype(np.float64)
    A = sparse_list(k, i, j, v, range(T), N)
    out = {"T": np.int64(T), "N": np.int64(N), "H": np.int64(H), "C": np.int64(C), "A_k": k, "A_i": i, "A_j": j,
           "A_v": v, "X": X}
    torch.manual_seed(seed)
    if reg:
        gcn = wgf.WD_GCN_reg(A, torch.tensor(X), [H, C])
        out["lin_w0"], out["lin_b0"] = gcn.lin1.weight.detach().numpy().copy(), gcn.lin1.bias.detach().numpy().copy()
        record_model(gcn, out)
        y = gcn()
        (y ** 2).mean().backward()
        out["out"] = y.detach().numpy()
        out["dlin_w"], out["dlin_b"] = gcn.lin1.weight.grad.numpy().copy(), gcn.lin1.bias.grad.numpy().copy()
        out["param_order"] = np.array([n for n, _ in gcn.named_parameters()])
        with torch.no_grad():
            out["out_call"] = gcn(A[:3], torch.tensor(X[:3])).numpy()      # __call__ passes no edges: the training output
    else:
        E = 4 * N
        edges = np.stack([rng.integers(0, T, E), rng.integers(0, N, E), rng.integers(0, N, E)])
        target = rng.integers(0, C, E)
        weight = rng.random(C).astype(np.float32) + 0.5
        out.update(edges=edges, target=target, weight=weight)
        gcn = wgf.WD_GCN(A, torch.tensor(X), torch.tensor(edges), [H, C])
        record_model(gcn, out)
        crit = torch.nn.CrossEntropyLoss(weight=torch.tensor(weight))
        logits = gcn()
        loss = crit(logits, torch.tensor(target))
        loss.backward()
        out["logits"], out["loss"] = logits.detach().numpy(), np.float64(loss.item())
        # the validation call: 3 of the T slices (AX zero-padded to T, wgf:80-84)
        Ev = 2 * N
        edges_v = np.stack([rng.integers(0, 3, Ev), rng.integers(0, N, Ev), rng.integers(0, N, Ev)])
        out["edges_val"] = edges_v
        with torch.no_grad():
            out["logits_val"] = gcn(A[:3], torch.tensor(X[:3]), torch.tensor(edges_v)).numpy()
    for n in NAMES:
        out["d" + n] = getattr(gcn, n).grad.numpy().copy()
    np.savez_compressed(os.path.join(HERE, f"g12_wdgcn_small_{name}.npz"), **out)


if __name__ == "__main__":
    small("h1_n7", 5, 7, 1, 2, 12, 1)
    small("h6_n200", 5, 200, 6, 3, 600, 2)
    small("h8_n63", 5, 63, 8, 3, 200, 3)
    small("reg_h6_n50", 5, 50, 6, 2, 150, 4, reg=True)
    chess()
