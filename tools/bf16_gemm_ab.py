#!/usr/bin/env python3
"""A/B of the layer-1 GEMM in front of the bf16 gather: the fp32 launches and their casts against the fused launches of
tmgcn_gemm_bf16y / tmgcn_gemm_dw_act_bf16 (csrc/gemm.hip), in ONE process.

Shapes (K = input width, F = layer-1 width; one shared weight, selu):
  wide    K = F = 128, T = 4 of the bench workload's slices of N = 2 M nodes      (the bf16-split matrix-core kernels)
  narrow  K = 2, F = 64, T = 16, N = 2 M                                          (the thread-per-row kernels)

Timed, interleaved (composition, fused, composition, ...) so that drift hits both alike:
  forward   gemm (fp32 Y + fp32 pre) + round_bf16                   | gemm_bf16y (bf16 Y + fp32 pre)
  backward  widen + act_bwd + gemm_dW (+ its slab reduction)         | gemm_dw_act_bf16 (+ the same reduction)

Each variant is timed by device events around it (a composition: around all its launches, and around each of them), after
warm-up runs of every variant; min and median over the repetitions are reported with the byte model beside them, per row
of the operand: forward 4K + 14F composed, 4K + 6F fused; backward 4K + 22F composed, 4K + 6F fused.  The baseline is the
composition of this build in this run.  Keep criterion per direction: the fused launch is faster than the composition in
EVERY interleaved pair of repetitions, at both shapes.  Writes one JSON file (default profiles/bf16_gemm_ab.json).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"wide": dict(K=128, F=128, T=4), "narrow": dict(K=2, F=64, T=16)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--N", type=int, default=2_000_000)
    ap.add_argument("--act", default="selu", choices=["relu", "leaky", "selu"])
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_gemm_ab.json"))
    a = ap.parse_args()

    import torch
    from tmgcn_amd import ops
    if not torch.cuda.is_available():
        sys.exit("bf16_gemm_ab: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    k = ops.kernels
    bf16 = torch.bfloat16

    def timed(*steps):
        """Runs the steps back to back, each fed the previous one's result; ms of each step and of the whole."""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(steps) + 1)]
        out = None
        ev[0].record()
        for i, f in enumerate(steps):
            out = f(out)
            ev[i + 1].record()
        ev[-1].synchronize()
        del out
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(len(steps))] + [ev[0].elapsed_time(ev[-1])]

    res = {"tool": "tools/bf16_gemm_ab.py", "device": torch.cuda.get_device_name(dev), "act": a.act, "reps": a.reps,
           "warmup": a.warmup, "shapes": {}}
    for name in a.shapes:
        K, F, T = SHAPES[name]["K"], SHAPES[name]["F"], SHAPES[name]["T"]
        if not ops.kernels.gemm_bf16y_supported(K, F):
            sys.exit(f"bf16_gemm_ab: K={K}, F={F} has no fused launch")
        g = torch.Generator(device=dev).manual_seed(1)
        A = torch.empty(T, a.N, K, device=dev)
        dYb = torch.empty(T, a.N, F, device=dev, dtype=bf16)
        for t in range(T):                                  # slice by slice: no second full-size fp32 tensor
            A[t] = torch.randn(a.N, K, generator=g, device=dev)
            dYb[t] = torch.randn(a.N, F, generator=g, device=dev).to(bf16)
        W = torch.randn(K, F, generator=g, device=dev) * (0.5 / K ** 0.5)
        _, pre = k.gemm(A, W, act=a.act, want_pre=True)     # the saved pre-activation both backward routes read

        variants = {
            "fwd_composed": (("gemm", lambda _: k.gemm(A, W, act=a.act, want_pre=True)), ("round_bf16", lambda yp: ops.round_bf16(yp[0]))),
            "fwd_fused": (("gemm_bf16y", lambda _: k.gemm(A, W, act=a.act, want_pre=True, out_dtype=bf16)),),
            "bwd_composed": (("widen", lambda _: k.ops.widen_params([dYb])[0]), ("act_bwd", lambda d: k.act_bwd(pre, d, a.act)),
                             ("gemm_dW", lambda d: k.gemm_dw(A, d, False))),
            "bwd_fused": (("gemm_dw_act_bf16", lambda _: k.gemm_dw(A, dYb, False, pre=pre, act=a.act)),),
        }
        launches = {"fwd_composed": 2, "fwd_fused": 1, "bwd_composed": 3, "bwd_fused": 1}   # the dW slab reduction aside: both have it

        # the two routes compute the same bits
        Yf, pf = k.gemm(A, W, act=a.act, want_pre=True, out_dtype=bf16)
        Yc, pc = k.gemm(A, W, act=a.act, want_pre=True)
        agree_fwd = bool(torch.equal(Yf, ops.round_bf16(Yc)) and torch.equal(pf, pc))
        del Yf, pf, Yc, pc
        agree_bwd = bool(torch.equal(k.gemm_dw(A, dYb, False, pre=pre, act=a.act),
                                     k.gemm_dw(A, k.act_bwd(pre, k.ops.widen_params([dYb])[0], a.act), False)))

        for _ in range(a.warmup):
            for steps in variants.values():
                timed(*(f for _, f in steps))
        torch.cuda.synchronize()
        ms = {n: [] for n in variants}
        for _ in range(a.reps):
            for n, steps in variants.items():
                ms[n].append(timed(*(f for _, f in steps)))

        rows = T * a.N
        model = {"fwd_composed": 4 * K + 14 * F, "fwd_fused": 4 * K + 6 * F, "bwd_composed": 4 * K + 22 * F, "bwd_fused": 4 * K + 6 * F}
        out = {"operand": {"T": T, "N": a.N, "K": K, "F": F, "rows": rows}, "fused_equals_composition_bitwise": {"fwd": agree_fwd, "bwd": agree_bwd},
               "variants": {}}
        for n, reps in ms.items():
            total = [r[-1] for r in reps]
            md = statistics.median(total)
            v = {"min_ms": round(min(total), 4), "median_ms": round(md, 4), "max_ms": round(max(total), 4), "launches": launches[n],
                 "model_bytes_per_row": model[n], "model_TB_per_s_at_median": round(model[n] * rows / (md * 1e-3) / 1e12, 3)}
            if len(variants[n]) > 1:
                v["steps_median_ms"] = {tag: round(statistics.median(r[i] for r in reps), 4) for i, (tag, _) in enumerate(variants[n])}
            out["variants"][n] = v
        r = out["variants"]
        out["speedup_median"] = {d: round(r[d + "_composed"]["median_ms"] / r[d + "_fused"]["median_ms"], 3) for d in ("fwd", "bwd")}
        out["model_byte_ratio"] = {d: round(model[d + "_composed"] / model[d + "_fused"], 3) for d in ("fwd", "bwd")}
        out["pairs_ms"] = {d: [[round(c[-1], 4), round(f[-1], 4)] for c, f in zip(ms[d + "_composed"], ms[d + "_fused"])] for d in ("fwd", "bwd")}
        out["fused_faster_in_every_pair"] = {d: all(f < c for c, f in out["pairs_ms"][d]) for d in ("fwd", "bwd")}
        res["shapes"][name] = out
        del A, dYb, pre, variants
        torch.cuda.empty_cache()
    res["keep"] = {d: all(s["fused_faster_in_every_pair"][d] for s in res["shapes"].values()) for d in ("fwd", "bwd")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
