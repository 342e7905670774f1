"""CPU restatement of WD-GCN (TensorGCN-master/wd_gcn_functions.py, "wgf") for the tests: the embedding, the edge head
and the per-node regression head, in the dtype of the tensors handed in — fp32 for the reference's own arithmetic,
fp64 for a truth to measure both against.  Pinned to the fixtures of the real reference (G12) by
tests/test_wdgcn_ref_golden.py, and used as the checker at sizes the fixtures do not cover.  torch CPU only."""
import numpy as np
import torch

NAMES = ("W", "Wf", "Wj", "Wc", "Wo", "Uf", "Uj", "Uc", "Uo", "bf", "bj", "bc", "bo")


def compute_AX(coo, X, T):
    """[T, N, F0]: slice k = Â_k·X_k (fp64 products, as the scripts' X is .double()) stored in fp32 for k < len(coo),
    zero beyond.  coo: list of (rows, cols, vals) numpy arrays, X: [>= len(coo), N, F0]."""
    N, F0 = X.shape[1], X.shape[2]
    AX = np.zeros((T, N, F0), np.float32)
    for k, (r, c, v) in enumerate(coo):
        acc = np.zeros((N, F0), np.float64)
        np.add.at(acc, r, v.astype(np.float64)[:, None] * X[k, c].astype(np.float64))
        AX[k] = acc
    return torch.from_numpy(AX)


def lstm(AX, p, h0, c0):
    """Z [T, N, H] of wgf:70, 86-98; p: dict name -> tensor."""
    Y = torch.relu(AX @ p["W"])
    N = AX.shape[1]
    h = h0.expand(N, -1)
    c = c0.expand(N, -1)
    out = []
    for t in range(AX.shape[0]):
        y = Y[t]
        f = torch.sigmoid(y @ p["Wf"] + h @ p["Uf"] + p["bf"])
        j = torch.sigmoid(y @ p["Wj"] + h @ p["Uj"] + p["bj"])
        o = torch.sigmoid(y @ p["Wo"] + h @ p["Uo"] + p["bo"])
        ct = torch.sigmoid(y @ p["Wc"] + h @ p["Uc"] + p["bc"])
        c = j * ct + f * c
        h = o * torch.tanh(c)
        out.append(h)
    return torch.stack(out)


def edge_logits(Z, edges, U):
    """cat(Z[t·N+src], Z[t·N+dst])·U (wgf:72-76); edges int64 [3, E]."""
    N, H = Z.shape[1], Z.shape[2]
    Zf = Z.reshape(-1, H)
    src = torch.as_tensor(edges[0] * N + edges[1])
    dst = torch.as_tensor(edges[0] * N + edges[2])
    return torch.cat((Zf[src], Zf[dst]), dim=1) @ U


def train_step(AX, p, h0, c0, U, edges, target, weight, dtype=torch.float32):
    """(logits, loss, {name: grad}) of nn.CrossEntropyLoss(weight)(WD_GCN(), target) in `dtype`."""
    q = {n: torch.as_tensor(p[n]).to(dtype).clone().requires_grad_(True) for n in NAMES}
    Z = lstm(torch.as_tensor(AX).to(dtype), q, torch.as_tensor(h0).to(dtype), torch.as_tensor(c0).to(dtype))
    out = edge_logits(Z, edges, torch.as_tensor(U).to(dtype))
    loss = torch.nn.CrossEntropyLoss(weight=torch.as_tensor(weight).to(dtype))(out, torch.as_tensor(target))
    loss.backward()
    return out.detach(), loss.detach(), {n: q[n].grad for n in NAMES}


def reg_forward(AX, p, h0, c0, lin_w, lin_b, dtype=torch.float32):
    """WD_GCN_reg's output [T, N] = lin1(Z).squeeze(2) (wgf:140-145)."""
    q = {n: torch.as_tensor(p[n]).to(dtype) for n in NAMES}
    Z = lstm(torch.as_tensor(AX).to(dtype), q, torch.as_tensor(h0).to(dtype), torch.as_tensor(c0).to(dtype))
    return (Z @ torch.as_tensor(lin_w).to(dtype).t() + torch.as_tensor(lin_b).to(dtype)).squeeze(2)
