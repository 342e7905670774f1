"""Forward + backward time of the EvolveGCN-H weight evolution at widths beyond the narrow kernels, from device events, on
synthetic H at the chess shape (N = 7 301 nodes, T = 80 slices) and (F, k) = (2, 16), (16, 32), (64, 64), (12, 6):

    wide       ops.egcn_evolve through csrc/evolvegcn_wide.hip (five forward launches, five backward launches)
    torch      ops.egcn_evolve_torch: the reference's statements as torch operators on the same device, autograd through
               the T-step loop — what these widths ran before the wide kernels existed, so the baseline

and the forward chain alone in cycles per step at the 2.4 GHz peak engine clock.  The chain is the only part of the
forward whose time grows with T (selection, rows and the W_g·X products are grids over T), so it is taken as the
difference between a 160-step and an 80-step forward at N = 64, divided by 80: launches and the parallel parts cancel.

    python tools/evolvegcn_wide_epoch.py [--out profiles/evolvegcn_wide_epoch.json] [--reps 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tmgcn_amd import ops  # noqa: E402

DEV = "cuda:0"
N, T = 7301, 80
SHAPES = [(2, 16), (16, 32), (64, 64), (12, 6)]
CLOCK_GHZ = 2.4           # MI355X peak engine clock


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": reps}


def draw(F, k, n, t, gen):
    H = torch.randn(t, n, F, generator=gen).to(DEV)
    p = torch.randn(F, generator=gen).double().to(DEV).requires_grad_(True)
    gates = [(torch.randn(*((F, k) if i % 3 == 2 else (F, F)), generator=gen).double() / F ** 0.5).to(DEV).requires_grad_(True)
             for i in range(9)]
    W0 = (torch.randn(F, k, generator=gen).double() / F ** 0.5).to(DEV).requires_grad_(True)
    return H, p, gates, W0


def measure(F, k, reps):
    gen = torch.Generator().manual_seed(F * 100 + k)
    H, p, gates, W0 = draw(F, k, N, T, gen)
    R1, R2 = torch.randn(T + 1, F, k, generator=gen).double().to(DEV), torch.randn(T, F, k, generator=gen).to(DEV)

    def run(evolve):
        def step():
            for q in [p, W0] + gates:
                q.grad = None
            Wseq, W32 = evolve(H, p, gates, W0)
            ((Wseq * R1).sum() + (W32 * R2).sum().double()).backward()
        return step
    assert ops.egcn_wide_supported(F, k)
    wide = run(ops.egcn_evolve if ops.egcn_evolve_route(F, k) == "wide" else
               lambda H, p, g, W0: torch.ops.tmgcn.egcn_evolve_wide(H, p, g, W0, k, T))
    naive = run(ops.egcn_evolve_torch)
    for _ in range(3):
        wide()
    naive()
    res = {"F": F, "k": k, "N": N, "T": T, "wide_fwd_bwd": timed(wide, reps), "torch_fwd_bwd": timed(naive, max(3, reps // 5))}
    res["speedup_over_torch"] = round(res["torch_fwd_bwd"]["median_ms"] / res["wide_fwd_bwd"]["median_ms"], 1)
    P = torch.cat([p.detach().reshape(-1)] + [g.detach().reshape(-1) for g in gates])
    W0d = W0.detach()
    fwd = torch.ops.tmgcn.egcn_wide_fwd
    res["fwd_five_launches_no_grad"] = timed(lambda: fwd(H, P, W0d, k, T, False), reps)
    res["fwd_five_launches_with_gates"] = timed(lambda: fwd(H, P, W0d, k, T, True), reps)
    out = fwd(H, P, W0d, k, T, True)
    res["bwd_five_launches"] = timed(lambda: torch.ops.tmgcn.egcn_wide_bwd(H, P, W0d, out[5], out[2], out[3], out[4], out[0],
                                                                          out[6], R1, R2, False), reps)
    Hs = torch.randn(2 * T, 64, F, generator=gen).to(DEV)
    fwd(Hs, P, W0d, k, 2 * T, False)
    t1 = timed(lambda: fwd(Hs, P, W0d, k, T, False), reps)
    t2 = timed(lambda: fwd(Hs, P, W0d, k, 2 * T, False), reps)
    res["fwd_n64_80_steps"], res["fwd_n64_160_steps"] = t1, t2
    res["chain_fwd_cycles_per_step"] = round((t2["median_ms"] - t1["median_ms"]) * 1e6 * CLOCK_GHZ / T)
    res["route"] = ops.egcn_evolve_route(F, k)
    # beyond the run-to-run spread: the slowest wide repetition against the fastest torch one
    res["wide_faster_than_torch_beyond_spread"] = res["wide_fwd_bwd"]["max_ms"] < res["torch_fwd_bwd"]["min_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evolvegcn_wide_epoch.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0),
           "what": ("forward + backward of the EvolveGCN-H weight evolution on synthetic H, device events; chain cycles per "
                    f"step = (160-step forward - 80-step forward at N = 64) / 80 at {CLOCK_GHZ} GHz; the event times of the "
                    "operators include their launches and output allocations"),
           "shapes": {}}
    for F, k in SHAPES:
        out["shapes"][f"{F}x{k}"] = measure(F, k, a.reps)
        print(f"{F}x{k}", json.dumps(out["shapes"][f"{F}x{k}"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
