#!/usr/bin/env python3
"""A/B of the band M-transform in front of / behind the bf16 gather: the fp32 kernel plus a cast launch against the one
fused launch of csrc/mtransform_bf16.hip, in ONE process.

Operand: the bench workload's activation — T = 16, N = 2 M, F = 128, the 20-diagonal band_M.  Timed, interleaved (pair,
fused, pair, ...) so that drift hits both alike:

  forward   fp32 X -> bf16 Y:   mtransform + round_bf16                 | fused f32 -> bf16
  backward  bf16 dY -> fp32 dX: widen + mtransform_T                     | fused bf16 -> f32 (transposed)
  and the fp32 kernel alone each way (mtransform, mtransform_T): the rate the fused launches are held against.

Each variant is timed by device events around it (a pair: around both launches, and around each of them), after warm-up
runs of every variant; min and median over the repetitions are reported, with the byte model beside them: 14 B per element
for a pair (4 + 4 transform, 4 + 2 cast), 6 B fused, 8 B for the fp32 kernel alone.  The cast launch takes fewer than 2^31
elements, so at this size the pair's cast runs as a few launches over slabs of slices (their sum is what is reported).
The baseline is the pair of this build in this run.  Keep criterion per direction: the fused launch's median is below the
pair's fastest repetition.  Writes one JSON file (default profiles/bf16_mtransform_ab.json).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAST_MAX = 2 ** 31 - 1   # elements per cast launch (tmgcn_cast_multi)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--T", type=int, default=16)
    ap.add_argument("--N", type=int, default=2_000_000)
    ap.add_argument("--F", type=int, default=128)
    ap.add_argument("--band", type=int, default=20, help="diagonals of the lower-banded M")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_mtransform_ab.json"))
    a = ap.parse_args()

    import torch
    from tmgcn_amd import ops, synth
    if not torch.cuda.is_available():
        sys.exit("bf16_mtransform_ab: needs the GPU (a CPU run measures nothing)")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    k = ops.kernels
    bf16, f32 = torch.bfloat16, torch.float32
    op = ops.MOperator(synth.band_M(a.T, a.band, "matlab"), dev)
    if not ops.m_transform_bf16_fused(op):
        sys.exit(f"bf16_mtransform_ab: a band of {a.band} diagonals has no fused launch")
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.empty(a.T, a.N, a.F, device=dev)
    dYb = torch.empty(a.T, a.N, a.F, device=dev, dtype=bf16)
    for t in range(a.T):                                   # slice by slice: no second full-size fp32 tensor
        X[t] = torch.randn(a.N, a.F, generator=g, device=dev)
        dYb[t] = torch.randn(a.N, a.F, generator=g, device=dev).to(bf16)
    slab = max(1, CAST_MAX // (a.N * a.F))                 # slices per cast launch

    def cast(Z, to_bf16):
        return [ops.round_bf16(Z[t:t + slab]) if to_bf16 else k.ops.widen_params([Z[t:t + slab]])[0] for t in range(0, a.T, slab)]

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

    # backward pair: the cast launches widen the bf16 gradient slab by slab; the fp32 transposed launch then runs on a resident
    # fp32 tensor of the same shape (X — a launch's time does not depend on the values), since the slabs are separate tensors
    variants = {
        "fwd_pair": (("mtransform", lambda _: k.mtransform(op, X)), ("round_bf16", lambda Y: cast(Y, True))),
        "fwd_fused": (("mtransform_bf16", lambda _: k.mtransform(op, X, out_dtype=bf16)),),
        "fwd_f32_kernel": (("mtransform", lambda _: k.mtransform(op, X)),),
        "bwd_pair": (("widen", lambda _: cast(dYb, False)), ("mtransform_T", lambda _: k.mtransform(op, X, transpose=True))),
        "bwd_fused": (("mtransform_bf16_T", lambda _: k.mtransform(op, dYb, transpose=True, out_dtype=f32)),),
        "bwd_f32_kernel": (("mtransform_T", lambda _: k.mtransform(op, X, transpose=True)),),
    }

    # the two routes compute the same bits (on one slab: the cast launch's size limit)
    s = min(slab, a.T)
    small = ops.MOperator(synth.band_M(s, min(a.band, s), "matlab"), dev)
    agree_fwd = bool(torch.equal(k.mtransform(small, X[:s], out_dtype=bf16), ops.round_bf16(k.mtransform(small, X[:s]))))
    agree_bwd = bool(torch.equal(k.mtransform(small, dYb[:s], transpose=True, out_dtype=f32),
                                 k.mtransform(small, dYb[:s].float(), transpose=True)))

    for _ in range(a.warmup):
        for steps in variants.values():
            timed(*(f for _, f in steps))
    torch.cuda.synchronize()
    ms = {n: [] for n in variants}
    for _ in range(a.reps):
        for n, steps in variants.items():
            ms[n].append(timed(*(f for _, f in steps)))

    elements = a.T * a.N * a.F
    model = {"fwd_pair": 14, "fwd_fused": 6, "fwd_f32_kernel": 8, "bwd_pair": 14, "bwd_fused": 6, "bwd_f32_kernel": 8}
    res = {"tool": "tools/bf16_mtransform_ab.py", "device": torch.cuda.get_device_name(dev),
           "operand": {"T": a.T, "N": a.N, "F": a.F, "band_diagonals": a.band, "elements": elements, "cast_launches_per_pair": -(-a.T // slab)},
           "reps": a.reps, "warmup": a.warmup, "fused_equals_pair_bitwise": {"fwd": agree_fwd, "bwd": agree_bwd}, "variants": {}}
    for n, rows in ms.items():
        total = [r[-1] for r in rows]
        mn, md = min(total), statistics.median(total)
        v = {"min_ms": round(mn, 4), "median_ms": round(md, 4), "max_ms": round(max(total), 4), "model_bytes_per_element": model[n],
             "model_TB_per_s_at_median": round(model[n] * elements / (md * 1e-3) / 1e12, 3)}
        if len(variants[n]) > 1:
            v["steps_median_ms"] = {tag: round(statistics.median(r[i] for r in rows), 4) for i, (tag, _) in enumerate(variants[n])}
        res["variants"][n] = v
    r = res["variants"]
    res["speedup_median"] = {d: round(r[d + "_pair"]["median_ms"] / r[d + "_fused"]["median_ms"], 3) for d in ("fwd", "bwd")}
    res["model_byte_ratio"] = round(14 / 6, 3)
    res["keep"] = {d: bool(r[d + "_fused"]["median_ms"] < r[d + "_pair"]["min_ms"]) for d in ("fwd", "bwd")}
    res["fused_rate_vs_f32_kernel"] = {d: round(r[d + "_fused"]["model_TB_per_s_at_median"] / r[d + "_f32_kernel"]["model_TB_per_s_at_median"], 3)
                                       for d in ("fwd", "bwd")}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
