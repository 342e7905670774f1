"""EvolveGCN-H training-epoch time (forward, weighted cross entropy, backward, SGD step) on the chess data of G10, from
device events, in two configurations: the chess script's EvolveGCN_2_layer [6,6,3] (T = 80) and the link-prediction
shape's EvolveGCN_1_layer [6,2] (T = 79, the labelled edges of tests/golden/g13_egcn_chess_lp.npz):

    graph      tmgcn_amd.evolvegcn, the epoch captured once with graphs.GraphedTrainStep and replayed
    eager      the same model, one epoch per Python call (csrc/evolvegcn.hip + the batched GEMMs + the fused head + loss)
    naive      the reference's statements as torch operators on the GPU (ops.egcn_evolve_torch for the weight evolution,
               then the same batched GCONVs and head)
    cpu        the CPU restatement (tests/_evolvegcn_ref.py) at <= 16 threads, forward + backward

    python tools/evolvegcn_epoch.py [--out profiles/evolvegcn_epoch.json] [--reps 50] [--kernel-db DIR]
                                    [--dispatch-db T=DIR:EPOCHS ...] [--profile-only --T T --epochs E]

Kernel times come from separate runs: --profile-only builds the 2-layer chess model over the first T slices, runs E
eager epochs and nothing else, the program to trace with

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/evolvegcn_epoch.py --profile-only --T 80 --epochs 20

--kernel-db DIR reads that trace's results database and adds the median time of each EvolveGCN kernel.  The dispatches
per training step come from two traces of the same T with E1 < E2 epochs: (dispatches(E2) - dispatches(E1)) / (E2 - E1)
— the set-up's dispatches cancel.  --dispatch-db T=DIR1:E1,DIR2:E2 adds that count for T.
"""
import argparse
import glob
import json
import os
import sqlite3
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tmgcn_amd import evolvegcn, ops  # noqa: E402
from tmgcn_amd.graphs import GraphedTrainStep  # noqa: E402

DEV = "cuda:0"


def _slices(g, n):
    k, i, j, v = g.C()
    out = []
    for s in range(n):
        m = k == s
        out.append(torch.sparse_coo_tensor(torch.tensor(np.stack([i[m], j[m]])), torch.tensor(v[m], dtype=torch.float64),
                                           (g.N, g.N)).coalesce())
    return out


def chess_inputs(T=None):
    from _g10 import G10
    g = G10()
    T = g.T if T is None else T
    keep = g.edges_train[0] < T
    return (evolvegcn.EvolveGCN_2_layer, _slices(g, T), torch.tensor(g.X[:T]), torch.tensor(g.edges_train[:, keep]),
            torch.tensor(g.target_train[keep]), torch.tensor(g.class_weights), [6, 6, 3])


def lp_inputs():
    from _g10 import G10
    import _evolvegcn_ref as ref
    g = G10()
    d = np.load(os.path.join(ROOT, "tests", "golden", "g13_egcn_chess_lp.npz"))
    edges, target = ref.lp_edges(g, d)
    return (evolvegcn.EvolveGCN_1_layer, _slices(g, g.T - 1), torch.tensor(g.X[:g.T - 1]), torch.tensor(edges),
            torch.tensor(target), torch.tensor(d["weight"]), [6, 2])


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "reps": reps}


def _model(inputs):
    cls, A, X, edges, target, w, hf = inputs
    torch.manual_seed(0)
    return cls(A, X, edges, hf, device=DEV)


def measure(inputs, reps):
    cls, A, X, edges, target, w, hf = inputs
    m = _model(inputs)
    layers = 2 if cls is evolvegcn.EvolveGCN_2_layer else 1
    tgt, crit = target.to(DEV), torch.nn.CrossEntropyLoss(weight=w.to(DEV))
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9)

    def eager():
        opt.zero_grad()
        crit(m()[0], tgt).backward()
        opt.step()
    for _ in range(3):
        eager()
    res = {"model": cls.__name__, "T": m.T, "N": m.N, "E": int(edges.shape[1]), "hidden_feat": hf,
           "eager": timed(eager, reps)}
    step = GraphedTrainStep(m, crit, opt, tgt, warmup=2)
    step()
    res["graph"] = timed(step, reps)

    # the naive port: the reference's loop of topk + GRU as torch operators on the GPU, autograd through it
    names = [n for n, _ in m.named_parameters()]
    params = {n: getattr(m, n).detach().clone().requires_grad_(True) for n in names}
    opt_n = torch.optim.SGD(list(params.values()), lr=0.01, momentum=0.9)
    eidx = m._edges

    def naive():
        opt_n.zero_grad()
        g1 = [params[n] for n in ops.EGCN_GATE_NAMES]
        _, W1 = ops.egcn_evolve_torch(m.X, params["p"], g1, m.W_init)
        Y = ops.feature_gemm(m.AX, W1, act="relu" if layers == 2 else None)
        if layers == 2:
            g2 = [params[n + "2"] for n in ops.EGCN_GATE_NAMES]
            _, W2 = ops.egcn_evolve_torch(Y, params["p2"], g2, m.W_init2)
            Y = ops.spmm_feature_gemm(m.A, Y, W2)
        Yf = Y.reshape(-1, Y.shape[-1])
        out = torch.cat((Yf[eidx.src.long()], Yf[eidx.dst.long()]), 1) @ params["U"]
        crit(out, tgt).backward()
        opt_n.step()
    naive()
    res["naive"] = timed(naive, max(3, reps // 10))

    import _evolvegcn_ref as ref
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    d = {n + "0": getattr(m, n).detach().cpu().numpy() for n in names}
    d["W_init"] = m.W_init.cpu().numpy()
    if layers == 2:
        d["W_init2"] = m.W_init2.cpu().numpy()
    e_np, Xd = edges.numpy(), X.double()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref.train_step(A, Xd, d, layers, e_np, target, w)
        ts.append((time.perf_counter() - t0) * 1e3)
    res["cpu"] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "reps": 3, "threads": torch.get_num_threads(),
                  "what": "forward + backward of the restatement (no optimizer step)"}
    return res


CLOCK_GHZ = 2.4           # MI355X peak engine clock


def _kernels(trace_dir):
    """(name, duration ns) of every kernel dispatch of a rocprofv3 trace: its results database, or its CSV."""
    rows = []
    for db in sorted(glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True)):
        con = sqlite3.connect(db)
        rows += list(con.execute("select name, duration from kernels"))
        con.close()
    if not rows:
        import csv
        for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)):
            with open(path) as f:
                rows += [(r["Kernel_Name"], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in csv.DictReader(f)]
    if not rows:
        raise SystemExit(f"no rocprofv3 kernel trace under {trace_dir}")
    return rows


def kernel_times(trace_dir, T):
    """Median duration of each EvolveGCN kernel in the rocprofv3 results database(s) under trace_dir."""
    by = {}
    for name, dur in _kernels(trace_dir):
        for kind in ("egcn_topk", "egcn_select", "egcn_chain_fwd", "egcn_chain_bwd", "egcn_grad"):
            if kind in name:
                by.setdefault(kind, []).append(dur)
    if not by:
        raise SystemExit(f"no EvolveGCN kernel in the trace under {trace_dir}")
    out = {k: {"median_us": round(statistics.median(v) / 1e3, 2), "calls": len(v)} for k, v in sorted(by.items())}
    out["chain_cycles_per_step"] = {k: round(out[k]["median_us"] * 1e3 * CLOCK_GHZ / T)
                                    for k in ("egcn_chain_fwd", "egcn_chain_bwd") if k in out}
    out["what"] = (f"rocprofv3 --kernel-trace of tools/evolvegcn_epoch.py --profile-only (eager chess epochs of the 2-layer "
                   f"model, T = {T}); two launches of each kernel per epoch (one per layer); cycles per step = median "
                   f"kernel time / T at {CLOCK_GHZ} GHz")
    return out


def dispatches_per_step(spec):
    """'DIR1:E1,DIR2:E2' -> (dispatches(E2) - dispatches(E1)) / (E2 - E1)."""
    (d1, e1), (d2, e2) = [(p.rsplit(":", 1)[0], int(p.rsplit(":", 1)[1])) for p in spec.split(",")]
    n1, n2 = len(_kernels(d1)), len(_kernels(d2))
    return {"per_step": (n2 - n1) / (e2 - e1), "dispatches": {str(e1): n1, str(e2): n2}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evolvegcn_epoch.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--kernel-db", default=None, help="directory of a rocprofv3 trace of --profile-only --T 80")
    ap.add_argument("--dispatch-db", action="append", default=[], help="T=DIR1:E1,DIR2:E2")
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--T", type=int, default=80)
    ap.add_argument("--epochs", type=int, default=20)
    a = ap.parse_args()
    if a.profile_only:
        inputs = chess_inputs(a.T)
        m = _model(inputs)
        tgt, crit = inputs[4].to(DEV), torch.nn.CrossEntropyLoss(weight=inputs[5].to(DEV))
        opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9)
        for _ in range(a.epochs):
            opt.zero_grad()
            crit(m()[0], tgt).backward()
            opt.step()
        torch.cuda.synchronize()
        return
    out = {"device": torch.cuda.get_device_name(0), "configs": {}}
    if a.kernel_db:
        out["chess_kernels_rocprofv3"] = kernel_times(a.kernel_db, 80)
    if a.dispatch_db:
        out["dispatches_per_training_step"] = {s.split("=", 1)[0]: dispatches_per_step(s.split("=", 1)[1])
                                               for s in a.dispatch_db}
        out["dispatches_per_training_step"]["what"] = (
            "kernel dispatches of one eager chess epoch of the 2-layer model (forward, loss, backward, SGD step) at T "
            "slices, from two rocprofv3 traces of --profile-only with different epoch counts")
    for name, inp in (("chess_2layer", chess_inputs), ("chess_lp_1layer", lp_inputs)):
        out["configs"][name] = measure(inp(), a.reps)
        print(name, json.dumps(out["configs"][name]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
