"""WD-GCN training-epoch time (forward, weighted cross entropy, backward, SGD step) on the chess data of G10 and on
S1- / S3-shaped synthetic inputs ([6,3] / [6,2], F0 = 2), from device events:

    eager      tmgcn_amd.wdgcn.WD_GCN, one epoch per Python call (csrc/wdgcn.hip + the fused head + loss)
    graph      the same epoch captured once with graphs.GraphedTrainStep and replayed
    naive      the reference's statements as torch operators on the GPU (ops.wdgcn_lstm_torch + gather/matmul head)
    cpu        the CPU restatement (tests/_wdgcn_ref.py) at <= 16 threads

    python tools/wdgcn_epoch.py [--out profiles/wdgcn_epoch.json] [--reps 50] [--kernel-db DIR] [--profile-only]

Kernel times come from a separate run: --profile-only runs 20 eager epochs of the chess config and nothing else, the
program to trace with

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/wdgcn_epoch.py --profile-only

and --kernel-db DIR then reads that trace's results database and adds the median time of each WD-GCN kernel, and of
the two LSTM kernels also as cycles per time step (kernel time / T at the 2.4 GHz peak engine clock), to the JSON.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tmgcn_amd import ops, synth, wdgcn  # noqa: E402
from tmgcn_amd.graphs import GraphedTrainStep  # noqa: E402

DEV = "cuda:0"


def chess_inputs():
    from _g10 import G10
    g = G10()
    k, i, j, v = g.C()
    A = []
    for s in range(g.T):
        m = k == s
        A.append(torch.sparse_coo_tensor(torch.tensor(np.stack([i[m], j[m]])), torch.tensor(v[m], dtype=torch.float64), (g.N, g.N)).coalesce())
    return A, torch.tensor(g.X[:g.T]), torch.tensor(g.edges_train), torch.tensor(g.target_train), torch.tensor(g.class_weights), [6, 3]


def synth_inputs(name):
    g = synth.dynamic_graph(**synth.CONFIGS[name], seed=0)
    return g.At_list(), torch.from_numpy(g.X), torch.from_numpy(g.edges), torch.from_numpy(g.labels), torch.tensor([0.9, 0.1]), [6, 2]


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


def measure(name, inputs, reps):
    A, X, edges, target, w, hf = inputs
    torch.manual_seed(0)
    m = wdgcn.WD_GCN(A, X, edges, hf, device=DEV)
    tgt, crit = target.to(DEV), torch.nn.CrossEntropyLoss(weight=w.to(DEV))
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9)

    def eager():
        opt.zero_grad()
        crit(m(), tgt).backward()
        opt.step()
    for _ in range(3):
        eager()
    res = {"T": m.T, "N": m.N, "E": int(edges.shape[1]), "hidden_feat": hf, "eager": timed(eager, reps)}
    step = GraphedTrainStep(m, crit, opt, tgt, warmup=2)
    step()
    res["graph"] = timed(step, reps)

    # the naive port: the reference's statements on the GPU, autograd through the 80-step loop
    params = [getattr(m, n).detach().clone().requires_grad_(True) for n in ops.WDGCN_PARAM_NAMES]
    opt_n = torch.optim.SGD(params, lr=0.01, momentum=0.9)
    AX, U, h0, c0 = m.AX, m.U, m.h_init, m.c_init
    src = (edges[0] * m.N + edges[1]).to(DEV)
    dst = (edges[0] * m.N + edges[2]).to(DEV)

    def naive():
        opt_n.zero_grad()
        Z = ops.wdgcn_lstm_torch(AX, params, h0, c0).reshape(-1, hf[0])
        crit(torch.cat((Z[src], Z[dst]), 1) @ U, tgt).backward()
        opt_n.step()
    naive()
    res["naive"] = timed(naive, max(3, reps // 10))

    import _wdgcn_ref as ref
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    p = {n: getattr(m, n).detach().cpu() for n in ops.WDGCN_PARAM_NAMES}
    AXc, e_np = AX.cpu(), edges.numpy()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        ref.train_step(AXc, p, h0.cpu(), c0.cpu(), U.cpu(), e_np, target, w)
        ts.append((time.perf_counter() - t0) * 1e3)
    res["cpu"] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "reps": 3, "threads": torch.get_num_threads(),
                  "what": "forward + backward of the restatement (no optimizer step)"}
    return res


PROFILE_T = 80            # the chess config's slices: what --profile-only runs
CLOCK_GHZ = 2.4           # MI355X peak engine clock


def kernel_times(trace_dir):
    """Median duration of each WD-GCN kernel in the rocprofv3 results database(s) under trace_dir."""
    import glob
    import sqlite3
    dbs = sorted(glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True))
    if not dbs:
        raise SystemExit(f"no rocprofv3 results database under {trace_dir}")
    by = {}
    for db in dbs:
        con = sqlite3.connect(db)
        for name, dur, grid in con.execute("select name, duration, grid_x from kernels where name like '%wdgcn%'"):
            kind = "fwd" if "wdgcn_fwd" in name else "bwd" if "wdgcn_bwd" in name else "slab_sum"
            by.setdefault(kind, []).append((dur, grid))
        con.close()
    if not by:
        raise SystemExit(f"no WD-GCN kernel in the trace under {trace_dir}")
    out = {k: {"median_us": round(statistics.median(d for d, _ in v) / 1e3, 2), "calls": len(v), "grid_x_threads": v[0][1]}
           for k, v in sorted(by.items())}
    out["cycles_per_step"] = {k: round(out[k]["median_us"] * 1e3 * CLOCK_GHZ / PROFILE_T) for k in ("fwd", "bwd") if k in out}
    out["what"] = (f"rocprofv3 --kernel-trace of tools/wdgcn_epoch.py --profile-only (20 eager chess epochs, T = {PROFILE_T}); "
                   f"cycles per step = median kernel time / T at {CLOCK_GHZ} GHz")
    out["instruction_issue_estimate_cycles_per_step"] = "a few hundred (forward), 2-3x that (backward)"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wdgcn_epoch.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--kernel-db", default=None, help="directory of a rocprofv3 trace of --profile-only")
    ap.add_argument("--profile-only", action="store_true")
    a = ap.parse_args()
    if a.profile_only:
        A, X, edges, target, w, hf = chess_inputs()
        m = wdgcn.WD_GCN(A, X, edges, hf, device=DEV)
        tgt, crit = target.to(DEV), torch.nn.CrossEntropyLoss(weight=w.to(DEV))
        opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9)
        for _ in range(20):
            opt.zero_grad()
            crit(m(), tgt).backward()
            opt.step()
        torch.cuda.synchronize()
        return
    out = {"device": torch.cuda.get_device_name(0), "configs": {}}
    if a.kernel_db:
        out["chess_kernels_rocprofv3"] = kernel_times(a.kernel_db)
    for name, inp in (("chess", chess_inputs), ("S1", lambda: synth_inputs("S1")), ("S3", lambda: synth_inputs("S3"))):
        out["configs"][name] = measure(name, inp(), a.reps)
        print(name, json.dumps(out["configs"][name]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
