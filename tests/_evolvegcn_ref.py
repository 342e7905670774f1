"""CPU restatement of EvolveGCN-H (TensorGCN-master/evolvegcn_functions.py, "ef") for the tests: the summary with the
project's tie rule (equal scores: lower node index first), the matrix GRU, the GCONVs and the two heads, in the dtype
of the tensors handed in.  Pinned to the fixtures of the real reference (G13) by tests/test_evolvegcn_ref_golden.py,
and used as the checker at sizes the fixtures do not cover.  torch CPU only."""
import numpy as np
import torch

GATES = ("W_Z", "U_Z", "B_Z", "W_R", "U_R", "B_R", "W_H", "U_H", "B_H")


def names(layers):
    out = []
    for s in ([""] if layers == 1 else ["", "2"]):
        out += ["p" + s] + [g + s for g in GATES]
    return out + ["U"]


def topk_tie_rule(y, k):
    """Indices of the k largest scores, equal scores by the lower index, NaN never selected."""
    yy = y.detach().double().numpy()
    order = np.lexsort((np.arange(len(yy)), -np.nan_to_num(yy, nan=-np.inf)))
    order = [i for i in order if not np.isnan(yy[i])][:k]
    return torch.as_tensor(np.array(order, np.int64))


def summarize(H, p, k):
    """ef:80-84 in fp64: (idx, y[idx], Zs [k, F])."""
    y = torch.matmul(H.double(), p) / torch.norm(p, 2)
    idx = topk_tie_rule(y, k)
    return idx, y[idx], H.double()[idx, :] * y[idx].unsqueeze(1)


def gru(X, W, q, s=""):
    """ef:86-91: X = Zsᵀ [F, k], W = W_{t-1}."""
    Z = torch.sigmoid(q["W_Z" + s] @ X + q["U_Z" + s] @ W + q["B_Z" + s])
    R = torch.sigmoid(q["W_R" + s] @ X + q["U_R" + s] @ W + q["B_R" + s])
    Ht = torch.tanh(q["W_H" + s] @ X + q["U_H" + s] @ (R * W) + q["B_H" + s])
    return (1 - Z) * W + Z * Ht


def embed(A, X, q, W0, T, W02=None, out_dtype=torch.float32, record=None):
    """Y [T, N, F_{-2}] (zero beyond X's slices, ef:66) and the final W of each layer.  A: list of dense or sparse
    [N, N] fp64 tensors, X: [T_run, N, F0] fp64.  record: a list that receives (layer, idx) of every summary."""
    T_run, N = X.shape[0], X.shape[1]
    W, W2 = W0, W02
    Y = None
    for t in range(T_run):
        idx, _, Zs = summarize(X[t], q["p"], W.shape[1])
        if record is not None:
            record.append((1, idx))
        W = gru(Zs.t(), W, q)
        H = torch.sparse.mm(A[t], X[t].double()) @ W if A[t].is_sparse else A[t] @ X[t].double() @ W
        if W2 is not None:
            H = torch.relu(H)
            idx, _, Zs = summarize(H, q["p2"], W2.shape[1])
            if record is not None:
                record.append((2, idx))
            W2 = gru(Zs.t(), W2, q, "2")
            H = (torch.sparse.mm(A[t], H) if A[t].is_sparse else A[t] @ H) @ W2
        if Y is None:
            Y = torch.zeros(T, N, H.shape[1], dtype=out_dtype)
        Y[t] = H
    return Y, (W,) if W2 is None else (W, W2)


def edge_logits(Y, edges, U):
    """cat(Y[t·N+src], Y[t·N+dst])·U (ef:73-76); edges int64 [3, E]."""
    N, F = Y.shape[1], Y.shape[2]
    Yf = Y.reshape(-1, F)
    src = torch.as_tensor(edges[0] * N + edges[1])
    dst = torch.as_tensor(edges[0] * N + edges[2])
    return torch.cat((Yf[src], Yf[dst]), dim=1) @ U


def params(d, layers, suffix="0", grad=True):
    return {n: torch.tensor(d[n + suffix]).requires_grad_(grad) for n in names(layers)}


def train_step(A, X, d, layers, edges, target, weight, T=None, out_dtype=torch.float32, record=None, q=None):
    """(logits, loss, {name: grad}, W_T tuple) of nn.CrossEntropyLoss(weight)(gcn()[0], target); q: the parameters
    (default: the fixture's initial ones)."""
    q = params(d, layers) if q is None else q
    T = X.shape[0] if T is None else T
    W02 = torch.tensor(d["W_init2"]) if layers == 2 else None
    Y, Ws = embed(A, X, q, torch.tensor(d["W_init"]), T, W02, out_dtype, record)
    out = edge_logits(Y, edges, q["U"].to(out_dtype))
    loss = torch.nn.CrossEntropyLoss(weight=torch.as_tensor(weight).to(out_dtype))(out, torch.as_tensor(target))
    loss.backward()
    return out.detach(), loss.detach(), {n: q[n].grad for n in q}, Ws


def sparse_slices(d, N):
    k, i, j, v = d["A_k"], d["A_i"], d["A_j"], d["A_v"]
    return [torch.sparse_coo_tensor(torch.tensor(np.stack([i[k == s], j[k == s]])), torch.tensor(v[k == s], dtype=torch.float64),
                                    (N, N)).coalesce() for s in range(int(d["T"]))]


def lp_edges(g, d):
    """The labelled edge set of g13_egcn_chess_lp: slice t+1's training edges at slice t, then the stored non-edges."""
    pos = g.edges_train[:, g.edges_train[0] >= 1].copy()
    pos[0] -= 1
    neg = np.stack([pos[0], d["neg"][0].astype(np.int64), d["neg"][1].astype(np.int64)])
    edges = np.concatenate([pos, neg], axis=1)
    target = np.concatenate([np.ones(pos.shape[1], np.int64), np.zeros(neg.shape[1], np.int64)])
    return edges, target
