#!/usr/bin/env python3
"""A/B of the fused SpMM+GEMM launch with the gathered operand stored in fp32 and in bf16, in ONE process.

Operand: the S4 rows on a quarter of the slices — T = 4, N = 2 M, 32 random neighbours + the self loop per row, K = Nf =
128 — so a run finishes in seconds.  Timed, interleaved (fp32, bf16, fp32, ...) so that drift hits both alike:

  forward   Y = (Â ⋆ X)·W with AX stored (what a training step launches): fp32 X | bf16 X, Y fp32 | bf16 X, Y bf16
  backward  dX = (Âᵀ ⋆ dY)·Wᵀ, no AX:                                     fp32 dY | bf16 dY, dX bf16

Each launch is timed by device events around it, after warm-up launches of every variant; min and median over the
repetitions are reported, and the byte model of DESIGN.md §4 (B per edge-slice) beside them.  The baseline is the fp32
kernel of this build in this run.  Writes one JSON file (default profiles/bf16_gather_ab.json).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def model_bytes_per_edge(F, d, x_bytes, y_bytes):
    """SURVEY §8d no-reuse model: col + val, the gathered row, and per row the row pointer and the Y row."""
    return 8 + F * x_bytes + (4 + F * y_bytes) / d


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--T", type=int, default=4)
    ap.add_argument("--N", type=int, default=2_000_000)
    ap.add_argument("--deg", type=int, default=32, help="random neighbours per row (plus the self loop)")
    ap.add_argument("--F", type=int, default=128)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_gather_ab.json"))
    a = ap.parse_args()

    import torch
    from tmgcn_amd import ops, synth
    if not torch.cuda.is_available():
        sys.exit("bf16_gather_ab: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    k = ops.kernels
    A = synth.device_er_csr(a.T, a.N, a.deg, dev)
    At = A.transpose()
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.randn(a.T, a.N, a.F, generator=g, device=dev)
    dY = torch.randn(a.T, a.N, a.F, generator=g, device=dev)
    W = torch.randn(a.F, a.F, generator=g, device=dev) * 0.1
    Xb, dYb = X.bfloat16(), dY.bfloat16()
    bf16 = torch.bfloat16

    variants = {
        "fwd_f32": lambda: k.spmm_gemm(A, X, W, want_ax=True),
        "fwd_bf16_y_f32": lambda: k.spmm_gemm_bf16(A, Xb, W, want_ax=True),
        "fwd_bf16_y_bf16": lambda: k.spmm_gemm_bf16(A, Xb, W, want_ax=True, out_dtype=bf16),
        "bwd_f32": lambda: k.spmm_gemm(At, dY, W, trans_w=True),
        "bwd_bf16": lambda: k.spmm_gemm_bf16(At, dYb, W, trans_w=True, out_dtype=bf16),
    }
    # the two paths compute the same thing: the bf16 launch against the fp32 launch on the widened operand
    chk = k.spmm_gemm(A, Xb.float(), W)[0]
    got = k.spmm_gemm_bf16(A, Xb, W)[0]
    agree = float((got - chk).abs().max() / chk.abs().max())
    del chk, got

    for _ in range(a.warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    ms = {n: [] for n in variants}
    for _ in range(a.reps):
        for n, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = f()
            e1.record()
            e1.synchronize()
            ms[n].append(e0.elapsed_time(e1))
            del out
    d = a.deg + 1
    edges = a.T * a.N * d
    model = {"fwd_f32": model_bytes_per_edge(a.F, d, 4, 4), "fwd_bf16_y_f32": model_bytes_per_edge(a.F, d, 2, 4),
             "fwd_bf16_y_bf16": model_bytes_per_edge(a.F, d, 2, 2), "bwd_f32": model_bytes_per_edge(a.F, d, 4, 4),
             "bwd_bf16": model_bytes_per_edge(a.F, d, 2, 2)}
    res = {"tool": "tools/bf16_gather_ab.py", "device": torch.cuda.get_device_name(dev),
           "operand": {"T": a.T, "N": a.N, "entries_per_row": d, "K": a.F, "Nf": a.F, "edge_slices": edges},
           "reps": a.reps, "warmup": a.warmup, "bf16_vs_f32_on_widened_x_max_rel": agree, "variants": {}}
    for n, v in ms.items():
        mn, md = min(v), statistics.median(v)
        res["variants"][n] = {"min_ms": round(mn, 4), "median_ms": round(md, 4), "max_ms": round(max(v), 4),
                              "model_bytes_per_edge_slice": round(model[n], 2),
                              "model_TB_per_s_at_median": round(model[n] * edges / (md * 1e-3) / 1e12, 3)}
    r = res["variants"]
    res["speedup_median"] = {"fwd_y_f32": round(r["fwd_f32"]["median_ms"] / r["fwd_bf16_y_f32"]["median_ms"], 3),
                             "fwd_y_bf16": round(r["fwd_f32"]["median_ms"] / r["fwd_bf16_y_bf16"]["median_ms"], 3),
                             "bwd": round(r["bwd_f32"]["median_ms"] / r["bwd_bf16"]["median_ms"], 3)}
    res["model_byte_ratio"] = {"fwd_y_f32": round(model["fwd_f32"] / model["fwd_bf16_y_f32"], 3),
                               "fwd_y_bf16": round(model["fwd_f32"] / model["fwd_bf16_y_bf16"], 3),
                               "bwd": round(model["bwd_f32"] / model["bwd_bf16"], 3)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
