"""Forward + backward time of the WD-GCN recurrence at widths beyond the narrow kernels, from device events, on synthetic
AX at the chess shape (N = 7 301 nodes, T = 80 slices) and (F0, H) = (2, 16), (16, 32), (64, 64):

    wide       ops.wdgcn_lstm through csrc/wdgcn_wide.hip (one forward launch, three backward launches)
    torch      ops.wdgcn_lstm_torch: the reference's statements as torch operators on the same device, autograd through
               the T-step loop — what these widths ran before the wide kernels existed, so the baseline

and the forward kernel alone (no gradient: Z only; with gradient: Z and the saved activations), converted to cycles per
time step at the 2.4 GHz peak engine clock and set against the MFMA issue floor of one wave's step
((4·NT·nj + 32·NT²) v_mfma_f32_16x16x4_f32 of 32 cycles each, NT = ⌈H/16⌉, nj = ⌈F0/16⌉; the 457 waves of this shape
are at most one per SIMD).

    python tools/wdgcn_wide_epoch.py [--out profiles/wdgcn_wide_epoch.json] [--reps 20]
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
SHAPES = [(2, 16), (16, 32), (64, 64)]
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
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "reps": reps}


def measure(F0, H, reps):
    gen = torch.Generator().manual_seed(F0 * 100 + H)
    AX = (torch.rand(T, N, F0, generator=gen) * (2 * (torch.rand(T, N, F0, generator=gen) > 0.3).float() - 1)).to(DEV)
    shapes = [(F0, H)] + [(H, H)] * 8 + [(H,)] * 4
    params = [(torch.randn(*s, generator=gen) / max(H, F0) ** 0.5).to(DEV).requires_grad_(True) for s in shapes]
    h0, c0 = torch.randn(H, generator=gen).to(DEV), torch.randn(H, generator=gen).to(DEV)
    R = torch.randn(T, N, H, generator=gen).to(DEV)
    P = torch.cat([p.detach().reshape(-1) for p in params])

    def run(lstm):
        def step():
            for p in params:
                p.grad = None
            lstm(AX, params, h0, c0).backward(R)
        return step
    assert ops.wdgcn_wide_supported(F0, H)
    wide, naive = run(ops.wdgcn_lstm if ops.wdgcn_lstm_route(F0, H) == "wide" else
                      lambda AX, p, h0, c0: torch.ops.tmgcn.wdgcn_lstm_wide(AX, torch.cat([q.reshape(-1) for q in p]), h0, c0, H, T)), \
        run(ops.wdgcn_lstm_torch)
    for _ in range(3):
        wide()
    naive()
    res = {"F0": F0, "H": H, "N": N, "T": T, "wide_fwd_bwd": timed(wide, reps), "torch_fwd_bwd": timed(naive, max(3, reps // 5))}
    res["speedup_over_torch"] = round(res["torch_fwd_bwd"]["median_ms"] / res["wide_fwd_bwd"]["median_ms"], 1)
    fwd = torch.ops.tmgcn.wdgcn_wide_fwd
    res["fwd_kernel_no_grad"] = timed(lambda: fwd(AX, P, h0, c0, H, T, False), reps)
    res["fwd_kernel_with_saved"] = timed(lambda: fwd(AX, P, h0, c0, H, T, True), reps)
    Z, saved = fwd(AX, P, h0, c0, H, T, True)
    res["bwd_three_launches"] = timed(lambda: torch.ops.tmgcn.wdgcn_wide_bwd(AX, P, h0, c0, Z, saved, R), reps)
    NT, nj = (H + 15) // 16, (F0 + 15) // 16
    floor = (4 * NT * nj + 32 * NT * NT) * 32
    cyc = res["fwd_kernel_no_grad"]["median_ms"] * 1e6 * CLOCK_GHZ / T
    res["fwd_cycles_per_step"] = round(cyc)
    res["fwd_mfma_issue_floor_cycles_per_step"] = floor
    res["fwd_cycles_over_floor"] = round(cyc / floor, 2)
    res["route"] = ops.wdgcn_lstm_route(F0, H)
    res["wide_faster_than_torch"] = res["wide_fwd_bwd"]["median_ms"] < res["torch_fwd_bwd"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wdgcn_wide_epoch.json"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0),
           "what": ("forward + backward of the WD-GCN recurrence on synthetic AX, device events; cycles per step = forward "
                    f"kernel time (no gradient) / T at {CLOCK_GHZ} GHz; the event times of the single kernels include the "
                    "launch and the output allocation"),
           "shapes": {}}
    for F0, H in SHAPES:
        out["shapes"][f"{F0}x{H}"] = measure(F0, H, a.reps)
        print(f"{F0}x{H}", json.dumps(out["shapes"][f"{F0}x{H}"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
