#!/usr/bin/env python3
"""bench.py — TM-GCN layer forward+backward throughput, (edges×T)/s  (BASELINE.json metric).

A "step" is one pass of the hot path over one batch of synthetic input:
    forward   Y  = ((Â ⋆ (M ×₁ X)) · W)            P1 -> [exchange] -> P2 -> P3
    backward  dX, dW from a given dY               P3ᵀ (dA, dW) -> P2ᵀ -> [exchange] -> P1ᵀ
Workload (SURVEY §8d "S4", the config the metric is quoted on): per GPU 16 frontal slices of an
N = 2,000,000-node graph, 32 random out-neighbours per row + self loop (66 M stored non-zeros
per slice), F = 128 -> 128 features, band M with 20 diagonals, fp32.  Weak scaling: T = 16·G.
Inputs are generated on the device (seeded by global slice index) and are resident in HBM
before the timed region.  One unit of work = one stored non-zero of one slice ("edge-slice").

    python bench.py --gpus 1 --steps 10 --warmup 3
    python bench.py --gpus 1 --steps 10 --warmup 3 --full # every leg below as well
    python bench.py --gpus 8 --steps 10 --warmup 3        # starts its own 8 ranks (see launch())
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
        --master-port 29500 bench.py --gpus 8 --steps 10 --warmup 3

A plain run is lean: it sets up, warms up, times --steps steps, writes the last step's outputs if --dump-outputs DIR is
given, and prints the result line (metric, value, unit, higher_is_better, dtype, ms_per_step, the in-run per-kernel
times and the roofline on them, the traffic of the committed PMC record).  Everything that takes checks or runs of its
own — the verify leg, the measured traffic, the hbm-only and side legs, the exchange comparison, the epochs and the CPU
baseline — runs with --full only (FULL_ONLY).

Rank 0 prints ONE JSON line (driver contract), the last line of the job's stdout, with (--full: all of them)
  roofline      dominant kernel = the fused SpMM+GEMM kernel (its forward and backward launches: the average rocprofv3's
                per-kernel row reports; each direction beside it), HIP events on the launch stream; `traffic` measured in
                the run (two PMC child runs); `roofline.legs` = the side legs' figures:
  roofline_skewed / roofline_T128 / roofline_real_structure   (N = 1 only) the same layer as child runs of this script on
                capped-Zipf row lengths, on S4's own T (128 slices of N·16/128 nodes, a true 20-diagonal band) and on the
                reference's real operand (its chess Ât replicated on the block diagonal), each with its own verify leg and
                its own two PMC passes; every launch quoted on the SURVEY §8d model bytes, or on the MEASURED bytes where
                those are below 0.8x the model (launch_roofline)
  cpu_baseline  the oracle executed the reference's way on the host cores (N = 1 only, bounded sample: about 30 s), the
                GPU/CPU ratio, and `cpu_baseline.epochs` (the training-epoch times below, GPU beside CPU, condensed)
  epochs        training-epoch time of the reference-shaped configs S1-S3 (GPU eager / hipGraph /
                untouched-script mode vs the CPU oracle; north_star's >= 10x Reddit-LP target) and of the reference's
                own chess data from its raw edge list (`epochs.chess`, tools/chess_epoch.py), N = 1 only
  ranks         world size as RCCL itself reports it, and the device every rank ran on
  verify        after the timed region every rank checks sampled rows of Y and dX and the all-reduced dW of
                the last step against the CPU oracle, from regenerated seeded inputs (tools/bench_verify.py);
                a miss makes the job exit non-zero
  plan          per-rank HBM plan of both exchange modes, computed before anything is allocated
Every rank carries a hard deadline (--deadline): stacks are dumped and the process exits non-zero,
so a stalled multi-rank job ends instead of hanging until somebody's timeout.
"""
import argparse
import gc
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
F32_MATRIX_PEAK_TFLOPS = 157.3  # MI355X fp32 matrix (v_mfma_f32_*_f32) dense peak: 256 CUs x 256 flop/clk x 2.4 GHz
T0 = time.perf_counter()


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--nodes", type=int, default=2_000_000)
    p.add_argument("--slices-per-gpu", type=int, default=16)
    p.add_argument("--deg", type=int, default=32)
    p.add_argument("--feat", type=int, default=128)
    p.add_argument("--band", type=int, default=20)
    p.add_argument("--graph", choices=["er", "powerlaw", "powerlaw_sym", "chess_tiled"], default="er",
                   help="adjacency of the S4 layer: er = SURVEY §8d (every row deg+1 entries, the headline); powerlaw = the same N, "
                        "mean row length and uniform columns with capped-Zipf row lengths (synth.device_powerlaw_csr: hubs of up to "
                        "100 000 entries); powerlaw_sym = that with every pair stored both ways (forward AND backward skewed); "
                        "chess_tiled = the reference's own operand (Ât of its chess data, read_data.py:116-127, 204-223: 4 entries per "
                        "row, two rows of three the self loop only, community-local columns) replicated on the block diagonal to "
                        "about --nodes nodes (synth.device_chess_tiled_csr; --deg unused)")
    p.add_argument("--exchange", choices=["a2a", "allgather"], default="a2a")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-epochs", action="store_true", help="skip the S1-S3 training-epoch block (N = 1 only)")
    p.add_argument("--no-compare-exchange", action="store_true",
                   help="skip the a2a / allgather side-by-side leg of multi-rank runs")
    p.add_argument("--no-compare-full", action="store_true",
                   help="skip the full-N run of the OTHER exchange mode (by default it runs whenever its memory plan fits: "
                        "the all-gather is node-chunked, so it fits at every world size)")
    p.add_argument("--gather-chunk-nodes", type=int, default=None,
                   help="nodes per chunk of the chunked all-gather (default: ~8 GB chunk buffers; 0 = the literal "
                        "unchunked form, which materialises [T,N,F] twice per GPU)")
    p.add_argument("--no-measure-traffic", action="store_true",
                   help="do not measure roofline.traffic in this run (two short child runs of this script under "
                        "`rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE`, N = 1 only); the committed PMC record is quoted instead")
    p.add_argument("--no-hbm-only", action="store_true",
                   help="skip the roofline.frac_hbm_only leg (N = 1 only): the same edge-slices per launch as 2 slices of "
                        "N x slices/2 nodes, i.e. one multi-GB gather window per slice that the 256 MB Infinity Cache cannot help")
    p.add_argument("--no-skewed", action="store_true",
                   help="skip the roofline_skewed leg (N = 1 only): the same layer on --graph powerlaw — the mean row length, N and "
                        "uniform columns of S4 with capped-Zipf row lengths (hubs of 100 000 entries) — as a child run of this script")
    p.add_argument("--no-t128", action="store_true",
                   help="skip the roofline_T128 leg (N = 1 only): S4's own T — 128 slices of N·slices/128 nodes, the same edge-slices and "
                        "bytes per tensor, a true 20-diagonal band over 128 slices — as a child run of this script")
    p.add_argument("--no-real-structure", action="store_true",
                   help="skip the roofline_real_structure leg (N = 1 only): the same layer on --graph chess_tiled, as a child run")
    p.add_argument("--no-legs", action="store_true", help="skip every side leg (what the child runs of this script are given)")
    p.add_argument("--no-leg-traffic", action="store_true",
                   help="do not measure the side legs' traffic (two more PMC child runs per leg); their frac then stays on the model bytes")
    p.add_argument("--verify-slices", type=int, default=0,
                   help="check the rows of Y on this many evenly spaced local slices only (0 = all; the T = 128 leg passes 16)")
    p.add_argument("--no-verify", action="store_true",
                   help="skip the verify leg (sampled rows of Y / dX and the all-reduced dW against the CPU oracle)")
    p.add_argument("--verify-rows", type=int, default=128, help="sampled rows per slice (Y) and sampled nodes (dX) per rank")
    p.add_argument("--no-fuse", action="store_true", help="run P2 and P3 as separate kernels")
    p.add_argument("--no-pipeline", action="store_true", help="exchange all slices before computing")
    p.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for "
                   "the single-device diagnostic below)")
    p.add_argument("--single-device", action="store_true",
                   help="diagnostic: all ranks share cuda:0 (needs --backend gloo; RCCL refuses it)")
    p.add_argument("--grid-reserve", type=int, default=None,
                   help="block slots the fused kernel leaves free for RCCL's kernels (default: the layer's choice)")
    p.add_argument("--cu-reserve", type=int, default=None,
                   help="CUs the pipelined path's compute streams leave free for RCCL's kernels (CU-masked streams; default: the layer's choice)")
    p.add_argument("--force-collectives", action="store_true",
                   help="run the exchange (RCCL) code path even at --gpus 1 (diagnostic)")
    p.add_argument("--cpu-nodes", type=int, default=250_000, help="N of the repeated CPU-baseline sample")
    p.add_argument("--cpu-full-nodes", type=int, default=0,
                   help="N of an additional CPU point at the headline's own N (one repetition, about a minute at N = 2 M); "
                        "-1 = --nodes, 0 = skip (default: the bounded sample at --cpu-nodes is the baseline)")
    p.add_argument("--compare-nodes", type=int, default=250_000,
                   help="N of the reduced-size a2a / allgather comparison (fits at every world size)")
    p.add_argument("--epoch-reps", type=int, default=50, help="GPU epochs timed per config in the epochs block")
    p.add_argument("--cpu-epoch-reps", type=int, default=5, help="CPU epochs timed per config and thread count")
    p.add_argument("--watchdog", type=int, default=600,
                   help="dump every thread's Python stack to stderr once after this many seconds (0 disables)")
    p.add_argument("--selftest-stall", action="store_true",
                   help="diagnostic (tests/test_bench_launcher.py): every rank stops making progress before it touches "
                        "the GPU, so that the deadline path can be exercised on a CPU-only machine")
    p.add_argument("--deadline", type=int, default=900,
                   help="hard limit: after this many seconds every rank dumps its stacks and exits non-zero (0 disables)")
    p.add_argument("--full", action="store_true",
                   help="run everything beyond the headline as well: the verify leg, the measured traffic, the hbm-only and side "
                        "legs, the exchange comparison, the epochs and the CPU baseline (a plain run skips them: FULL_ONLY)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last step computed (Y, dX, dW of rank 0's shard) as DIR/<name>.npy, "
                        "float32; Y and dX as a fixed, seeded sample of their rows (dump_outputs)")
    return p.parse_args(argv)


# what a plain run leaves out (the --no-* switches a run without --full gets)
FULL_ONLY = ("no_verify", "no_measure_traffic", "no_hbm_only", "no_legs", "no_compare_exchange", "no_epochs", "no_cpu_baseline")


def stage(msg):
    """Progress marker on stderr (where a stalled run stopped is the first thing one needs)."""
    r = os.environ.get("RANK", "0")
    sys.stderr.write(f"[bench r{r} +{time.perf_counter() - T0:7.1f}s] {msg}\n")
    sys.stderr.flush()


# ---------------------------------------------------------------------------------------
# self-launch: `python bench.py --gpus N` with no torchrun around it
# ---------------------------------------------------------------------------------------
def launch(args):
    """Start the N ranks as FRESH processes (`python -m torch.distributed.run … bench.py …`) from a
    parent that never touches the GPU, relay their output, and return their exit code.  The
    parent enforces the deadline too: it kills the process group it started (and only that)."""
    import signal
    import socket
    import subprocess

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL needs it on this driver
    stage(f"launching {args.gpus} ranks: {' '.join(cmd[1:8])} …")
    p = subprocess.Popen(cmd, env=env, start_new_session=True)
    limit = (args.deadline + 120) if args.deadline > 0 else None
    try:
        return p.wait(timeout=limit)
    except subprocess.TimeoutExpired:
        stage(f"ranks still running after {limit} s: killing process group {p.pid}")
        for sig in (signal.SIGTERM, signal.SIGKILL):
            try:
                os.killpg(p.pid, sig)
            except ProcessLookupError:
                break
            try:
                p.wait(timeout=10)
                break
            except subprocess.TimeoutExpired:
                continue
        return 124
    except KeyboardInterrupt:
        os.killpg(p.pid, signal.SIGTERM)
        raise


def arm_deadlines(args):
    import faulthandler
    if args.deadline > 0:
        # C-level timer thread: needs no GIL, fires even when the main thread is stuck inside a
        # collective or a device synchronise.  Dumps every Python stack, then _exit(1); torchrun
        # then tears the other ranks down, so the whole job ends non-zero.
        faulthandler.dump_traceback_later(args.deadline, exit=True)
    if args.watchdog > 0 and (args.deadline <= 0 or args.watchdog < args.deadline):
        def soft():
            time.sleep(args.watchdog)
            sys.stderr.write(f"[bench r{os.environ.get('RANK', '0')}] watchdog: still running after {args.watchdog} s\n")
            faulthandler.dump_traceback(all_threads=True)
        threading.Thread(target=soft, daemon=True).start()


# ---------------------------------------------------------------------------------------
# CPU legs (the oracle is imported only here: bench.py's cpu_baseline leg)
# ---------------------------------------------------------------------------------------
def _cpu_model():
    try:
        return [l.split(":")[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
    except Exception:
        return "unknown"


def cpu_baseline(args):
    """The oracle's layer fwd+bwd (list of COO fp64, one sparse.mm per slice, fp32 GEMM, autograd: the reference's way) on
    the host cores, on a BOUNDED sample of the S4 workload: 2 slices of N = --cpu-nodes nodes (default 250 000 — the N of
    S4's own T = 128 on one GPU, the `roofline_T128` leg), the same degree and widths; slices are independent, so the rate
    extrapolates to T slices by T/2.  About 30 s of CPU work: a warm-up, one repetition at 8 and one at 32 threads (torch's
    sparse kernels do not scale further: 128 / 256 threads of the EPYC 9575F ran at 1.3-2x the time of 8 in rounds 1-5), and
    two more at the better count; `value` = the best repetition.  --cpu-full-nodes -1 adds one repetition at the headline's
    own N (a minute; rounds 1-5 measured it within 3 % of the sample's rate)."""
    import torch
    from oracle import tmgcn_oracle as orc
    from tmgcn_amd import synth

    ncpu = os.cpu_count() or 1
    Tc, F = 2, args.feat

    def inputs(Nc):
        A = synth.device_er_csr(Tc, Nc, args.deg, "cpu")
        At = A.to_coo_list(torch.float64)
        X = synth.device_features(Tc, Nc, F, "cpu").double()
        M = torch.from_numpy(synth.band_M(Tc, args.band, "matlab"))
        g = torch.Generator().manual_seed(1)
        W = torch.randn(F, F, generator=g) * 0.1
        dY = torch.randn(Tc, Nc, F, generator=g)
        return A.nnz, (M, At, X, W, dY)

    def timed(ops_in, reps):
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            orc.layer_fwd_bwd(*ops_in)
            times.append(time.perf_counter() - t0)
        return times

    Ns = min(args.nodes, args.cpu_nodes)
    nnz_s, ops_s = inputs(Ns)
    sweep = {}
    counts = sorted({min(c, ncpu) for c in (8, 32)})
    torch.set_num_threads(counts[0])
    stage(f"cpu_baseline: N={Ns} sample, thread sweep {counts}")
    orc.layer_fwd_bwd(*ops_s)                                   # warm-up (allocator, sparse kernels' first-call costs)
    for c in counts:
        torch.set_num_threads(c)
        sweep[c] = timed(ops_s, 1)[0]
    threads = min(sweep, key=sweep.get)
    torch.set_num_threads(threads)
    ts = [sweep[threads]] + timed(ops_s, 2)
    small = {"nodes": Ns, "slices": Tc, "edge_slices": nnz_s, "threads": threads, "reps_s": [round(t, 3) for t in ts],
             "rate_best": nnz_s / min(ts), "rate_mean": nnz_s * len(ts) / sum(ts),
             "thread_sweep_s": {str(c): round(t, 3) for c, t in sweep.items()},
             "thread_sweep_rate": {str(c): nnz_s / t for c, t in sweep.items()}}
    del ops_s
    full_n = args.nodes if args.cpu_full_nodes < 0 else args.cpu_full_nodes
    full = None
    if full_n and full_n > small["nodes"]:
        stage(f"cpu_baseline: identical-N point N={full_n}, {threads} threads")
        nnz_f, ops_f = inputs(full_n)
        tf = timed(ops_f, 1)
        full = {"nodes": full_n, "slices": Tc, "edge_slices": nnz_f, "threads": threads, "reps_s": [round(t, 3) for t in tf],
                "rate_best": nnz_f / min(tf), "rate_mean": nnz_f * len(tf) / sum(tf)}
        del ops_f
    return {"value": small["rate_best"], "unit": "edge-slices/s", "cores": threads, "kind": "port",
            "sample": f"oracle = the reference's way on torch CPU (COO fp64, sparse.mm per slice, autograd), {_cpu_model()}, "
                      f"{threads} of {ncpu} hardware threads (the better of {counts}); fwd+bwd of {Tc} slices of N={Ns} nodes, "
                      f"deg={args.deg}+1, F={F}->{F} — a bounded sample of S4 (its own T = 128 on one GPU has this N); value = best of "
                      f"{len(ts)} repetitions ({', '.join(str(round(t, 2)) for t in ts)} s); extrapolates to T slices by T/2 (slices are "
                      "independent)",
            "identical_n": full, "small_sample": small}


EPOCH_MODELS = {  # the scripts' model per config
    "S1": dict(kind="gcn2", hidden=[6, 6, 2], nonlin="selu"),   # experiment_bitcoin_our.py:107 (2-layer)
    "S2": dict(kind="gcn", hidden=[6, 2]),                      # experiment_reddit_our_link_prediction.py:65
    "S3": dict(kind="gcn2", hidden=[6, 6, 2], nonlin="selu", bf16=True),  # AMLSim, bf16 weights
    "P128": dict(kind="gcn2", hidden=[128, 128, 2], nonlin="relu", scale=0.05),  # BASELINE.md §2 probe, wide features
    "S2z": dict(kind="gcn", hidden=[6, 2]),                     # hub source nodes (synth.CONFIGS): the 1-layer …
    "S2z2": dict(kind="gcn2", hidden=[6, 6, 2], nonlin="selu"),  # … and the 2-layer link-prediction model
}


def gpu_epochs(g, spec, epochs, mode):
    """(first loss, median-pass and fastest-pass seconds per training epoch) — zero_grad, gcn(),
    weighted CE, backward, SGD step: the loop of experiment_reddit_our_link_prediction.py:75-81 —
    on the device; five timed passes of `epochs` epochs each.
    mode: "eager"   device targets + nn.CrossEntropyLoss on device logits
          "graph"   the same epoch captured into one hipGraph and replayed
          "fused"   eager with `gcn.loss(criterion, target)`: edge head + weighted CE + all their gradients in
                    one launch (csrc/head_loss.hip; the 1-layer model folds its AtXt·W into it as well)
          "graph_fused"  the fused epoch captured into one hipGraph and replayed
          "graph_fused8" eight consecutive fused epochs per hipGraph (one launch latency for eight epochs; the time is
                    still per epoch)
          "graph_onelaunch", "graph_onelaunch8"  the folded 1-layer model only (S2): loss, gradients AND the SGD update in ONE
                    launch per epoch (GraphedTrainStep(fold_optimizer=True)), one or eight epochs per hipGraph
          "script"  what an untouched reference script does: `import tmgcn_amd.ehf as ehf`,
                    host-side targets, class weights and criterion (hosted.DeviceResult)"""
    import torch
    if mode == "script":
        import tmgcn_amd.ehf as ehf
    else:
        import tmgcn_amd.layers as ehf
    At, X, M = g.At_list(), torch.from_numpy(g.X), torch.from_numpy(g.M)
    edges, labels = torch.from_numpy(g.edges), torch.from_numpy(g.labels)
    if mode != "script":
        labels = labels.cuda()
    torch.manual_seed(0)
    kw = dict(condensed_W=True, use_Minv=False, param_dtype=torch.bfloat16 if spec.get("bf16") else torch.float32)
    if spec["kind"] == "gcn":
        m = ehf.EmbeddingGCN(At, X, edges, M, hidden_feat=spec["hidden"], **kw)
    else:
        m = ehf.EmbeddingGCN2(At, X, edges, M, hidden_feat=spec["hidden"], nonlin2=spec["nonlin"], **kw)
    if "scale" in spec:  # N(0,1) weights at width 128 overflow the activations; both sides scale the same way
        with torch.no_grad():
            for q in m.parameters():
                q.mul_(spec["scale"])
    if mode in ("fused", "graph_fused", "graph_fused8", "graph_onelaunch", "graph_onelaunch8"):      # the opt-in fused pieces: one-launch head + loss + gradients, one-launch SGD
        from tmgcn_amd.optim import FusedSGD
        opt = FusedSGD(m.parameters(), lr=0.01, momentum=0.9)
    else:
        opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9)
    if mode in ("fused", "graph_fused", "graph_fused8", "graph_onelaunch", "graph_onelaunch8"):
        from tmgcn_amd.losses import WeightedCrossEntropy
        crit = WeightedCrossEntropy(torch.tensor([0.9, 0.1])).cuda()
    elif mode == "script":
        crit = torch.nn.CrossEntropyLoss(weight=torch.tensor([0.9, 0.1]))
    else:
        crit = torch.nn.CrossEntropyLoss(weight=torch.tensor([0.9, 0.1], device="cuda"))

    fused = mode in ("fused", "graph_fused", "graph_fused8", "graph_onelaunch", "graph_onelaunch8")
    per_run = 8 if mode in ("graph_fused8", "graph_onelaunch8") else 1
    fold = mode in ("graph_onelaunch", "graph_onelaunch8")

    def epoch():
        opt.zero_grad(set_to_none=True)
        loss = m.loss(crit, labels) if fused else crit(m(), labels)   # fused: head + criterion + gradients in one launch
        loss.backward()
        opt.step()
        return loss

    first = float(epoch().detach())
    for _ in range(3):
        epoch()
    if mode in ("graph", "graph_fused", "graph_fused8", "graph_onelaunch", "graph_onelaunch8"):
        from tmgcn_amd.graphs import GraphedTrainStep
        step = GraphedTrainStep(m, crit, opt, labels, fused_loss=fused, steps_per_replay=per_run, fold_optimizer=fold)
        if fold and not step.folded:
            raise RuntimeError("graph_onelaunch: the model / optimizer pair is not the one the one-launch step covers")
        for _ in range(3):
            step()
        run = step
    else:
        run = epoch
    # sub-millisecond epochs: one pass of `epochs` epochs lasts 15-250 ms, short enough for a clock
    # ramp or a host hiccup to double it (measured: the same mode 0.28 / 0.92 / 1.45 ms depending
    # on what ran before it).  Time five passes after a pass of warm-up; report the median pass.
    passes = []
    for rep in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(epochs // per_run):
            run()
        torch.cuda.synchronize()
        if rep:
            passes.append((time.perf_counter() - t0) / (epochs // per_run * per_run))
    passes.sort()
    return first, passes[len(passes) // 2], passes[0]


def cpu_epochs(g, spec, epochs, threads):
    """The same epoch on the CPU oracle (the reference's way), `threads` torch threads."""
    import torch
    from oracle import tmgcn_oracle as orc
    torch.set_num_threads(threads)
    At, X, M = g.At_list(), torch.from_numpy(g.X), torch.from_numpy(g.M)
    edges, labels = torch.from_numpy(g.edges), torch.from_numpy(g.labels)
    torch.manual_seed(0)
    F = [X.shape[-1]] + spec["hidden"]
    p = {k: torch.nn.Parameter(v * spec.get("scale", 1.0)) for k, v in orc.draw_params(spec["kind"], g.T, F).items()}
    AtXt = orc.compute_AtXt(M, At, X)  # cached at construction, as the reference does (ehf:195)
    src, dst = orc.flat_edge_index(edges, g.N)
    opt = torch.optim.SGD(list(p.values()), lr=0.01, momentum=0.9)
    crit = torch.nn.CrossEntropyLoss(weight=torch.tensor([0.9, 0.1]))

    def epoch():
        opt.zero_grad()
        if spec["kind"] == "gcn":
            out = orc.gcn_forward(AtXt, p["W"], p["U"], src, dst)
        else:
            out = orc.gcn2_forward(AtXt, At, M, p["W1"], p["W2"], p["U"], src, dst, nonlin=spec["nonlin"])
        loss = crit(out, labels)
        loss.backward()
        opt.step()
        return float(loss.detach())

    first = epoch()
    times = []
    for _ in range(epochs):
        t0 = time.perf_counter()
        epoch()
        times.append(time.perf_counter() - t0)
    times.sort()
    return first, times[len(times) // 2]


def epochs_block(args, configs=("S1", "S2", "S3", "S2z2", "chess"), modes=("eager", "graph", "fused", "graph_fused", "graph_fused8", "script")):
    """north_star's epoch-throughput target (>= 10x the reference's CPU epoch on Reddit link
    prediction at 1 GPU), as a record: per config the GPU epoch in every mode, the CPU oracle's
    epoch (median of --cpu-epoch-reps at 8 and at 32 threads, both recorded, the better one reported) and the
    ratio for an untouched script ("script" mode) and for the best mode."""
    from tmgcn_amd import synth
    ncpu = os.cpu_count() or 1
    out = {}
    for name in configs:
        if name == "chess":
            continue
        stage(f"epochs: {name}")
        spec = EPOCH_MODELS[name]
        g = synth.dynamic_graph(**synth.CONFIGS[name], seed=0)
        rec = {"model": spec["kind"], "T": g.T, "N": g.N, "E": int(g.edges.shape[1]),
               "nnz_At": int(sum(c.nnz for c in g.Ct)), "gpu_epochs_timed": args.epoch_reps, "gpu_passes": 5,
               "cpu_epochs_timed": args.cpu_epoch_reps}
        loss_gpu = None
        for mode in modes + (("graph_onelaunch", "graph_onelaunch8") if (spec["kind"] == "gcn" and "graph_fused" in modes) else ()):
            first, sec, sec_min = gpu_epochs(g, spec, args.epoch_reps, mode)
            rec[f"gpu_ms_{mode}"] = round(sec * 1e3, 4)
            rec.setdefault("gpu_ms_min_pass", {})[mode] = round(sec_min * 1e3, 4)
            loss_gpu = first if loss_gpu is None else loss_gpu
        rec["first_loss_gpu"] = loss_gpu
        if args.cpu_epoch_reps > 0:
            cpu = {}
            loss_cpu = None
            # 8 and 32 threads only: on these small per-slice ops (N = 1 000-6 000) more threads are pathological — with 128 / 256
            # threads one S1 epoch did not finish in ten minutes on the 256-thread EPYC 9575F (round 4; the layer leg's
            # cpu_baseline, whose operands are 100x larger, does sweep up to all hardware threads)
            for th in sorted({min(8, ncpu), min(32, ncpu)}):
                loss_cpu, cpu[th] = cpu_epochs(g, spec, args.cpu_epoch_reps, th)
            th_best = min(cpu, key=cpu.get)
            rec.update({"cpu_ms": round(cpu[th_best] * 1e3, 2), "cpu_threads": th_best,
                        "cpu_ms_by_threads": {str(k): round(v * 1e3, 2) for k, v in cpu.items()},
                        "first_loss_cpu": loss_cpu})
            best = min(v for k, v in rec.items() if k.startswith("gpu_ms_") and isinstance(v, float))
            rec["speedup_script_mode"] = round(rec["cpu_ms"] / rec["gpu_ms_script"], 1) if "script" in modes else None
            rec["speedup_best_mode"] = round(rec["cpu_ms"] / best, 1)
        out[name] = rec
        gc.collect()
    # the one REAL data set the reference ships (chess, 7 301 players x 80 training slices; raw edges of fixture G10 under
    # tests/golden): device adjacency pipeline + the script's 2-layer model, eager / captured epochs, the CPU oracle's epoch
    fixture = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "g10_chess_full.npz")
    if "chess" in configs and os.path.exists(fixture):
        stage("epochs: chess (real data)")
        try:
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
            import chess_epoch
            out["chess"] = chess_epoch.run(epochs=max(40, args.epoch_reps * 4), cpu=min(3, args.cpu_epoch_reps))
            out["chess"]["what"] = ("the reference's data/chess (experiment_chess_our.py: EmbeddingGCN2 2->6->6->3, class-weighted CE, SGD) from "
                                    "the raw edge list: real row-length skew (3.97 non-zeros per row, 14.9 in the longest of 64 neighbours)")
        except Exception as e:                    # the headline must not depend on an optional record
            out["chess"] = {"error": repr(e)}
        gc.collect()
    out["note"] = ("epoch = zero_grad, gcn(), class-weighted CE, backward, SGD step (experiment_reddit_our_link_prediction.py:75-81); "
                   "S1/S2/S3 are synthetic stand-ins of the Bitcoin-OTC / Reddit-LP / AMLSim shapes (SURVEY §8d), S2z2 the Reddit-LP shape "
                   "with Zipf(1.5) source nodes (hub rows of 3 800 entries in the adjacency, 19 700 in the labelled edges) under the "
                   "2-layer model; CPU = the oracle "
                   f"run the reference's way on {_cpu_model()}, median epoch")
    return out


# ---------------------------------------------------------------------------------------
# the layer bench proper
# ---------------------------------------------------------------------------------------
def build_problem(args, dev, rank, world, exchange, N, kernels_ok=True):
    """This rank's shard of the S4 layer at N nodes: adjacency, M, layer, inputs — and the three
    closures that REGENERATE any slice of the global inputs from its seed (the verify leg uses them
    for data other ranks hold)."""
    import torch
    from tmgcn_amd import synth
    from tmgcn_amd.dist import ShardedTMGCNLayer

    G, Tl, F = world, args.slices_per_gpu, args.feat
    T = Tl * G
    k0 = rank * Tl
    A = synth.device_csr(args.graph, Tl, N, args.deg, dev, first_slice=k0)
    A.transpose()  # backward operand, built once (plan time, not timed)
    M = synth.band_M(T, args.band, "matlab")
    layer = ShardedTMGCNLayer(A, M, T, group=None, exchange=exchange, fuse=False if args.no_fuse else None,
                              pipeline=not args.no_pipeline, force_collectives=args.force_collectives,
                              grid_reserve=args.grid_reserve, gather_chunk_nodes=args.gather_chunk_nodes, cu_reserve=args.cu_reserve)
    shape = layer.input_shape(F)
    node_sharded = layer.collective and exchange == "a2a"
    if node_sharded:
        # node shard of the synthetic features: slice j of rank q's shard is seeded by 1000*q + j
        X = synth.device_features(T, shape[1], F, dev, first_slice=1000 * rank)
    else:
        X = synth.device_features(shape[0], N, F, dev, first_slice=k0)
    X.requires_grad_(True)
    g = torch.Generator(device=dev).manual_seed(1234)
    W = (torch.randn(F, F, device=dev, generator=g) * 0.1).requires_grad_(True)  # same on every rank
    dY = synth.device_normal(Tl, N, F, dev, first_slice=k0)

    def x_slice(j):                       # [N, F] of global input slice j, whoever holds it
        if node_sharded:
            return torch.cat([synth.device_features(1, shape[1], F, dev, first_slice=1000 * q + j)[0] for q in range(G)], 0)
        return synth.device_features(1, N, F, dev, first_slice=j)[0]

    def dy_slice(k):                      # [N, F] of upstream-gradient slice k
        return synth.device_normal(1, N, F, dev, first_slice=k)[0]

    def a_slice(k):                       # one-slice CSR of adjacency slice k
        return synth.device_csr(args.graph, 1, N, args.deg, dev, first_slice=k)

    return dict(A=A, M=M, T=T, Tl=Tl, k0=k0, layer=layer, X=X, W=W, dY=dY, node_sharded=node_sharded,
                x_slice=x_slice, dy_slice=dy_slice, a_slice=a_slice)


def run_layer(args, dist, dev, rank, world, exchange, N, steps, warmup, want_timer=True, verify=False, dump_dir=None):
    """Build this rank's shard of the S4 layer at N nodes and time `steps` fwd+bwd steps; rank 0 writes the last step's
    outputs to `dump_dir` if given.  Returns a dict; every device tensor dies with this frame."""
    import torch
    from tmgcn_amd import ops

    pb = build_problem(args, dev, rank, world, exchange, N)
    A, layer, X, W, dY = pb["A"], pb["layer"], pb["X"], pb["W"], pb["dY"]
    F = args.feat
    last = {}

    phase_events = []                     # (start, after forward, after backward) per timed step, on the main stream

    def step(record=False):
        X.grad = None
        W.grad = None
        last.clear()                      # frees the previous Y before the next forward allocates
        if record:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
        Y = layer(X, W)
        if record:
            ev[1].record()
        Y.backward(dY)
        if record:
            ev[2].record()
            phase_events.append(ev)
        last["Y"] = Y.detach()

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    stage(f"layer[{exchange}, N={N}]: inputs resident, warm-up")
    for _ in range(warmup):
        step()
    if want_timer:
        ops.kernels.timer = ops.KernelTimer()
    fence()
    stage(f"layer[{exchange}, N={N}]: timing {steps} steps")
    t0 = time.perf_counter()
    for _ in range(steps):
        step(record=True)
    fence()
    elapsed = time.perf_counter() - t0
    # forward / backward split of the step (main-stream events; side streams are joined before each ends):
    # against the N = 1 figures it shows which pass an exchange is exposed in
    fwd = sum(e[0].elapsed_time(e[1]) for e in phase_events) / len(phase_events)
    bwd = sum(e[1].elapsed_time(e[2]) for e in phase_events) / len(phase_events)
    phases = torch.tensor([fwd, bwd], device=dev, dtype=torch.float64)
    if world > 1:
        pmax = phases.clone()
        dist.all_reduce(pmax, op=dist.ReduceOp.MAX)
        phases_rec = {"forward_ms_rank0": round(fwd, 3), "backward_ms_rank0": round(bwd, 3),
                      "forward_ms_max": round(float(pmax[0]), 3), "backward_ms_max": round(float(pmax[1]), 3)}
    else:
        phases_rec = {"forward_ms": round(fwd, 3), "backward_ms": round(bwd, 3)}
    kt = ops.kernels.timer.summary() if want_timer else {}
    ops.kernels.timer = None
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        n = torch.tensor([A.nnz], device=dev, dtype=torch.int64)
        dist.all_reduce(n)
        total_nnz = int(n.item())
    else:
        total_nnz = A.nnz
    stage(f"layer[{exchange}, N={N}]: {elapsed / steps * 1e3:.1f} ms/step")
    peak_gb = torch.cuda.max_memory_allocated(dev) / 1e9
    if dump_dir is not None and rank == 0:
        dump_outputs(dump_dir, {"Y": last["Y"], "dX": X.grad, "dW": W.grad})
        stage(f"layer[{exchange}, N={N}]: last step's outputs written to {dump_dir}")
    ver = None
    if verify:
        # the checker: the results of the LAST TIMED step against the CPU oracle, from regenerated inputs
        stage(f"layer[{exchange}, N={N}]: verify")
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from bench_verify import verify_layer
        ver = verify_layer(dist=dist, rank=rank, world=world, dev=dev, node_sharded_input=pb["node_sharded"], A=A,
                           M64=pb["M"], T=pb["T"], k0=pb["k0"], N=N, W=W, X=X, dY=dY, Y=last["Y"], dX=X.grad, dW=W.grad,
                           x_slice=pb["x_slice"], dy_slice=pb["dy_slice"], a_slice=pb["a_slice"], rows=args.verify_rows,
                           y_slices=args.verify_slices or None)
        stage(f"layer[{exchange}, N={N}]: verify {'ok' if ver['ok'] else 'FAILED'} in {ver['seconds']} s: "
              f"Y {ver['max_rel_err_Y']:.2e} dX {ver['max_rel_err_dX']:.2e} dW {ver['max_rel_err_dW']}")
    cnt = A.rowptr[1:] - A.rowptr[:-1]
    row_stats = {"max": int(cnt.max()), "median": int(cnt.median()), "min": int(cnt.min()), "mean": round(A.nnz / max(1, A.n_rows), 4),
                 "share_of_rows_with_one_entry": round(float((cnt == 1).sum()) / max(1, A.n_rows), 4),
                 "rows_over_256": int((cnt > 256).sum()),
                 "share_of_entries_in_rows_over_256": round(float(cnt[cnt > 256].sum()) / max(1, A.nnz), 4),
                 "share_of_entries_in_longest_tenth_of_rows": round(float(torch.sort(cnt, descending=True).values[:max(1, A.n_rows // 10)].sum()) / max(1, A.nnz), 4)}
    del cnt
    return {"elapsed": elapsed, "kt": kt, "nnz_rank": A.nnz, "rows_rank": A.n_rows, "total_nnz": total_nnz, "row_stats": row_stats,
            "collective": layer.collective, "grid_reserve": layer.grid_reserve, "cu_reserve": layer.cu_reserve, "T": pb["T"],
            "gather_chunks": len(layer.gather_chunks(F)) if (layer.collective and exchange == "allgather"
                                                               and layer.gather_chunk_nodes != 0) else None,
            "peak_gb": peak_gb, "verify": ver, "phases": phases_rec}


DUMP_BYTES = 20 << 20  # per array: Y and dX of the S4 shard (16 GB each) are sampled down to this, the three stay below 64 MB


def dump_outputs(dump_dir, arrays):
    """`arrays` (name -> device tensor [..., F]) as dump_dir/<name>.npy, float32.  An array larger than DUMP_BYTES is
    written as a sample of its rows (rows = every index but the last): a fixed number of distinct rows drawn by a
    generator seeded with 0, in ascending order, gathered in place — so two runs of the same shape write the same rows."""
    import numpy as np
    import torch
    os.makedirs(dump_dir, exist_ok=True)
    for name, t in arrays.items():
        t = t.detach()
        lead, F = tuple(t.shape[:-1]), t.shape[-1]
        n = int(np.prod(lead))
        k = max(1, DUMP_BYTES // (4 * F))
        if n > k:
            idx = np.sort(np.random.default_rng(0).choice(n, size=k, replace=False))
            t = t[tuple(torch.from_numpy(i).to(t.device) for i in np.unravel_index(idx, lead))]
        np.save(os.path.join(dump_dir, name + ".npy"), t.float().cpu().numpy())


def _child_env():
    """A clean environment for child runs of this script: should THIS process itself run under a profiler, its preload /
    tool variables must not leak into the children (a nested rocprofv3 sets its own)."""
    env = {k: v for k, v in os.environ.items()
           if k != "LD_PRELOAD" and not k.startswith(("ROCP_", "ROCPROF", "ROCTX", "HSA_TOOLS_", "ROCPROFILER_"))}
    env["TMPDIR"] = "/tmp"
    return env


CHILD_OFF = ["--no-epochs", "--no-cpu-baseline", "--no-measure-traffic", "--no-hbm-only", "--no-legs", "--no-compare-exchange",
             "--deadline", "400"]


def workload_flags(args, **over):
    """The flags that define a layer workload, the parent's unless overridden."""
    w = dict(nodes=args.nodes, slices_per_gpu=args.slices_per_gpu, deg=args.deg, feat=args.feat, band=args.band, graph=args.graph)
    w.update(over)
    return ["--gpus", "1", "--nodes", str(w["nodes"]), "--slices-per-gpu", str(w["slices_per_gpu"]), "--deg", str(w["deg"]),
            "--feat", str(w["feat"]), "--band", str(w["band"]), "--graph", w["graph"]]


def run_child(flags, what, timeout=420):
    """One child run of this script (an ordinary child process of a parent that has released its device memory; a profiler
    around the parent then sees the headline's launches only).  Returns (parsed JSON line or None, exit code, error text)."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__)] + flags + ["--full"] + CHILD_OFF
    stage(f"{what}: child run {' '.join(flags)}")
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=_child_env(), capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        return None, 124, f"the {what} child run timed out"
    lines = [l for l in (r.stdout or "").splitlines() if l.startswith("{")]
    if not lines:
        return None, r.returncode, f"the {what} child run exited {r.returncode}: {(r.stderr or '')[-300:]}"
    return json.loads(lines[-1]), r.returncode, None


def measure_hbm_only(args, N, Tl, F):
    """The headline figure leans on the Infinity Cache (a quarter of each slice's 1 GB gather window fits its 256 MB).
    The same kernel on the same number of edge-slices per launch, arranged as 2 slices of N·Tl/2 nodes (S4 default:
    16 M nodes, an 8 GB window per slice), is what HBM alone sustains.  A child run (3 steps, no other legs)."""
    nodes = N * (Tl // 2)
    c, rc, err = run_child(workload_flags(args, nodes=nodes, slices_per_gpu=2) + ["--steps", "3", "--warmup", "1", "--no-verify"], "hbm-only")
    if c is None or rc != 0:
        return {"error": err or f"the large-window child run exited {rc}"}
    cr = c["roofline"]
    return {"nodes": nodes, "slices": 2, "gather_window_gb": round(nodes * F * 4 / 1e9, 2), "frac": cr["frac"], "achieved": cr["achieved"],
            "avg_launch_ms": cr["avg_launch_ms"], "edge_slices_per_launch": cr["edge_slices_per_launch"],
            "ms_per_step": round(c["ms_per_step"], 3), "steps": c["steps"]}


def launch_roofline(model_bytes, measured_bytes, ms):
    """One launch against the HBM roof, on the bytes SURVEY §8d prescribes: the no-reuse gather model — unless the measured
    fabric-side bytes (FETCH_SIZE x 2 + WRITE_SIZE) are below 0.8x the model, i.e. a good part of the gather never left the
    L2s ("cache hits are not HBM traffic"), or the model bytes would put the launch ABOVE the roof (it moved less than the
    model says: 0.87x on the skewed graph's backward, whose hub rows of dY are re-read from L2); then the MEASURED bytes.
    A launch is never quoted above what it moved.  The measured bytes are fabric-side: Infinity-Cache hits are in them."""
    over_roof = model_bytes / (ms * 1e-3) / 1e9 > HBM_PEAK_GBS
    use_measured = measured_bytes is not None and (measured_bytes < 0.8 * model_bytes or (over_roof and measured_bytes < model_bytes))
    used = measured_bytes if use_measured else model_bytes
    return {"launch_ms": ms, "model_bytes": int(model_bytes), "measured_bytes": None if measured_bytes is None else int(measured_bytes),
            "basis": "measured" if use_measured else "model", "achieved": used / (ms * 1e-3) / 1e9,
            "frac": used / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "frac_model": model_bytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS}


LEGS = {
    "skewed": dict(over=dict(graph="powerlaw"), steps=5, warmup=2, extra=[],
                   what="powerlaw: N, mean row length and uniform columns of S4, capped-Zipf row lengths (alpha 0.8, cap 100 000), long rows "
                        "at random positions of every slice; the backward operand (the transpose) has Poisson row lengths and re-reads "
                        "the hubs' rows of dY from cache"),
    "T128": dict(over=None, steps=5, warmup=2, extra=["--verify-slices", "16"],
                 what="S4's own T on one GPU: 128 slices of N·slices/128 nodes — the headline's edge-slices per launch and bytes per tensor, "
                      "a true 20-diagonal band over 128 slices (read_data.m:116-124; at T = 16 it is a full lower triangle), a 128-slice "
                      "batched CSR; each slice's gather window (128 MB at the default size) fits the 256 MB Infinity Cache"),
    "real_structure": dict(over=dict(graph="chess_tiled"), steps=5, warmup=2, extra=[],
                           what="the reference's own operand — Ât of its chess data (read_data.py:116-127, 204-223; N = 7 301, 80 slices): "
                                "4 entries per row, two rows of three holding the self loop only, columns inside communities — every "
                                "fifth slice REPLICATED on the block diagonal to the headline's N (synth.device_chess_tiled_csr: a "
                                "replication, not a larger real graph; row lengths and column locality are kept exactly)"),
}


def measure_leg(args, name):
    """One side leg: the S4 layer on another adjacency / shape as a CHILD run of this script with its own verify leg against
    the CPU oracle, plus — unless --no-leg-traffic — two PMC child runs for the fabric-side bytes of its forward and backward
    launch.  Each launch is quoted on the bytes launch_roofline() prescribes; the leg's `frac` is (bytes used, forward +
    backward) / (time, forward + backward) / peak: a launch above the roof cannot enter it."""
    spec = LEGS[name]
    over = spec["over"] if spec["over"] is not None else dict(nodes=max(1, args.nodes * args.slices_per_gpu // 128), slices_per_gpu=128)
    flags = workload_flags(args, **over)
    c, rc, err = run_child(flags + ["--steps", str(spec["steps"]), "--warmup", str(spec["warmup"]), "--verify-rows", str(args.verify_rows)]
                           + spec["extra"], name)
    if c is None:
        return {"error": err}
    cr, v = c["roofline"], c.get("verify") or {}
    model = cr["bytes_per_edge_slice"] * cr["edge_slices_per_launch"]
    traffic = None
    if not args.no_leg_traffic:
        traffic, why = measure_traffic(args, what=name, **over)
        if traffic is None:
            traffic = {"error": why}
    tf = (traffic or {}).get("forward_bytes")
    tb = (traffic or {}).get("backward_bytes")
    fwd = launch_roofline(model, tf, cr["forward_launch_ms"])
    bwd = launch_roofline(model, tb, cr["backward_launch_ms"]) if cr.get("backward_launch_ms") else None
    both = [x for x in (fwd, bwd) if x]
    used = sum(x["achieved"] * x["launch_ms"] for x in both)           # GB/s x ms = MB
    ms = sum(x["launch_ms"] for x in both)
    rec = {"workload": c["config"]["workload"], "graph": spec["what"], "row_lengths": c["config"].get("row_lengths"),
           "bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "achieved": used / ms, "frac": used / ms / HBM_PEAK_GBS,
           "frac_forward_only": fwd["frac"], "forward": fwd, "backward": bwd,
           "frac_is": "bytes used (forward + backward launch) / their time / 8 TB/s; per launch the SURVEY §8d no-reuse model bytes, or "
                      "the MEASURED fabric-side bytes (FETCH_SIZE x 2 + WRITE_SIZE) where those are below 0.8x the model — `basis` says "
                      "which; `frac_model` beside it is the model figure whatever the basis",
           "traffic": tf, "traffic_backward": tb, "traffic_source": traffic,
           "bytes_per_edge_slice": cr["bytes_per_edge_slice"], "edge_slices_per_launch": cr["edge_slices_per_launch"],
           "forward_launch_ms": cr["forward_launch_ms"], "backward_launch_ms": cr.get("backward_launch_ms"),
           "kernels_ms": c.get("kernels_ms"), "ms_per_step": round(c["ms_per_step"], 3), "steps": c["steps"], "value": c["value"],
           "verify_ok": v.get("ok"),
           "verify": {k: v.get(k) for k in ("max_rel_err_Y", "max_rel_err_dX", "max_rel_err_dW", "slices_checked", "seconds")},
           "child_exit_code": rc}
    if name == "real_structure":
        # d = 4: the exact-f32 products of the fused kernel (2·K·Nf flops per ROW, whatever the row holds) are as large a
        # term as its bytes — the matrix-core figure beside the byte figure
        rows = cr["edge_slices_per_launch"] / (c["config"]["row_lengths"] or {}).get("mean", float("nan"))
        fl = 2.0 * rows * args.feat * args.feat
        rec["mfma"] = {"flops_per_launch": fl, "tflops_forward": fl / (cr["forward_launch_ms"] * 1e-3) / 1e12,
                       "peak_tflops_f32_matrix": F32_MATRIX_PEAK_TFLOPS,
                       "frac_forward": fl / (cr["forward_launch_ms"] * 1e-3) / 1e12 / F32_MATRIX_PEAK_TFLOPS,
                       "note": "fp32-equivalent flops of the products (2·K·Nf per row) against the fp32 matrix peak; below 14 entries per "
                               "row they are formed as six bf16 plane products per term on v_mfma_f32_16x16x32_bf16 (csrc/spmm_gemm.hip "
                               "spmm_gemm_bx3_kernel): a third of the pipe time of the exact-f32 MFMAs, which at 4 entries per row took "
                               "as long on the matrix cores as the launch's compulsory bytes take on HBM"}
    return rec


def hbm_only_fields(h, dom, F):
    """roofline.frac_hbm_only (+ its provenance) from the large-gather-window run, same formula as `frac`."""
    if not h:
        return {}
    if "error" in h:
        return {"frac_hbm_only": None, "hbm_only_note": "large-window run failed: " + h["error"]}
    return {"frac_hbm_only": h["frac"], "achieved_hbm_only": h["achieved"],
            "hbm_only": {"what": f"the same kernel and edge-slices per launch as {h['slices']} slices of N = {h['nodes']} nodes: "
                                 f"one {h['gather_window_gb']} GB gather window per slice, of which the 256 MB Infinity Cache holds "
                                 "3 % (the headline's 1 GB windows: 25 %) — what HBM alone sustains; a child run of this script "
                                 "(so that a profiler around this process sees the headline's launches only)",
                         "avg_launch_ms": h["avg_launch_ms"], "edge_slices_per_launch": h["edge_slices_per_launch"],
                         "ms_per_step": h["ms_per_step"], "steps": h["steps"]}}


def free_device_memory():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def measure_traffic(args, what="headline", **over):
    """Fabric-side bytes of the dominant kernel's forward and backward launch, MEASURED IN THIS RUN (N = 1): two short child
    runs of this script — the workload of `over` (default: the parent's), 1 warm-up + 2 steps, no other legs — under
    `rocprofv3 --pmc FETCH_SIZE --kernel-trace` and `--pmc WRITE_SIZE --kernel-trace` (separate passes, kernel trace only:
    what the guide's HBM / rocprofv3 section prescribes and what gpurun allows), reduced by tools/pmc_traffic.py's reader:
    bytes per launch = FETCH_SIZE x 2 (gfx950 counts 16-B-per-lane reads at half their bytes; the factor is re-calibrated
    in the same pass on the band M-transform, whose bytes are known exactly) + WRITE_SIZE, KiB units.  The children are
    ordinary child processes of a parent that has already released its device memory.
    Returns (record, None) — record["forward_bytes"], ["backward_bytes"] — or (None, reason)."""
    import shutil
    import subprocess
    import tempfile
    if shutil.which("rocprofv3") is None:
        return None, "rocprofv3 not on PATH"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pmc_traffic
    flags = workload_flags(args, **over)
    common = flags + ["--steps", "2", "--warmup", "1", "--no-verify"] + CHILD_OFF
    got = {}
    with tempfile.TemporaryDirectory(prefix="tmgcn_pmc_", dir="/tmp") as tmp:
        for counter in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, counter)
            cmd = ["rocprofv3", "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", d, "--",
                   sys.executable, os.path.abspath(__file__)] + common
            stage(f"traffic[{what}]: rocprofv3 --pmc {counter} --kernel-trace … (child run)")
            try:
                r = subprocess.run(cmd, cwd="/tmp", env=_child_env(), capture_output=True, text=True, timeout=420)
            except subprocess.TimeoutExpired:
                return None, f"the {counter} pass timed out"
            if r.returncode != 0:
                return None, f"the {counter} pass exited {r.returncode}: {(r.stderr or '')[-300:]}"
            got[counter] = pmc_traffic.read_pass(d, counter)
    fused = lambda k: "spmm_gemm_kernel" in k or "spmm_gemm_bx3_kernel" in k     # (few entries per row: the bf16-product kernel)
    band_f = [v for k, v in got["FETCH_SIZE"].items() if "mtransform_band_kernel" in k]
    # (fetch, write) per dispatch, kernel by kernel: the two launches of a step may be different kernels (a plan for the giant
    # rows of A but none for those of its transpose), and each pass lists a kernel's dispatches in order
    pairs = [q for k, v in got["FETCH_SIZE"].items() if fused(k) and k in got["WRITE_SIZE"] for q in zip(v, got["WRITE_SIZE"][k])]
    if not pairs:
        return None, "no spmm_gemm_kernel / spmm_gemm_bx3_kernel dispatch in the counter output"
    fwd = max(pairs, key=lambda q: q[1])                            # forward also stores AX and Y
    bwd = min(pairs, key=lambda q: q[1])
    # calibration: the band M-transform reads one [T,N,F] fp32 tensor exactly once (chess_tiled rounds N by < 0.03 %)
    w = dict(nodes=args.nodes, slices_per_gpu=args.slices_per_gpu, feat=args.feat)
    w.update(over)
    slab = w["slices_per_gpu"] * w["nodes"] * w["feat"] * 4
    cal = round(slab / (band_f[0][0] * 1024), 4) if band_f and band_f[0] and band_f[0][0] else None
    return {"kind": "measured in this run", "how": "two child runs of bench.py (1 warm-up + 2 steps) under rocprofv3 --pmc FETCH_SIZE / "
            "--pmc WRITE_SIZE with --kernel-trace (separate passes); FETCH_SIZE x 2 on gfx950 + WRITE_SIZE, KiB units",
            "forward_bytes": int(fwd[0] * 1024 * 2.0 + fwd[1] * 1024), "backward_bytes": int(bwd[0] * 1024 * 2.0 + bwd[1] * 1024),
            "fetch_size_kib_raw": fwd[0], "write_size_kib": fwd[1], "backward_fetch_size_kib_raw": bwd[0], "backward_write_size_kib": bwd[1],
            "dispatches": len(pairs), "fetch_x2_calibration_on_band_mtransform": cal,
            "calibration_is": "bytes of one [T,N,F] fp32 tensor / raw FETCH_SIZE of the band M-transform in the same pass (it reads its input once)",
            "meaning": "fabric-side bytes between L2 and the Infinity Fabric, Infinity-Cache hits included: an upper bound on "
                       "what HBM itself moved"}, None


def traffic_record(N, F, Tl):
    """HBM-side traffic of the dominant kernel from the committed PMC passes (tools/pmc_traffic.py);
    None when the passes were taken at another problem size."""
    pmc = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        rec = json.load(open(pmc))
        if rec.get("nodes") == N and rec.get("feat") == F and rec.get("slices_per_gpu") == Tl:
            return rec["spmm_hbm_bytes_per_launch"], {
                "kind": "committed file", "file": "profiles/pmc_traffic.json", "profile": rec.get("profile"),
                "derived_by": rec.get("derived_by", "tools/pmc_traffic.py"),
                "meaning": "fabric-side bytes (L2 <-> Infinity Fabric: FETCH_SIZE x2 on gfx950 + WRITE_SIZE) from separate "
                           "rocprofv3 --pmc passes of this workload, NOT measured in this run; Infinity-Cache hits are "
                           "included, so HBM itself moves at most this"}
    except Exception:
        pass
    return None, None


def plain_or_full(args):
    """A run without --full is the headline alone: it gets every FULL_ONLY switch."""
    if not args.full:
        for k in FULL_ONLY:
            setattr(args, k, True)
    return args


def worker(args):
    plain_or_full(args)
    arm_deadlines(args)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.selftest_stall:
        stage("selftest: stalling on purpose")
        while True:
            time.sleep(3600)
    stage("importing torch")
    import torch
    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs"
    if args.single_device:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    import torch.distributed as dist
    ranks_info = None
    if world > 1 or args.force_collectives:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:      # no launcher (--force-collectives at --gpus 1): any free port
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        # one node by contract: keep every bootstrap socket on loopback (the container hostname
        # may not resolve, and a resolver time-out looks exactly like a stalled first run)
        os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
        os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
        stage(f"init_process_group({args.backend}) world={world}")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)
        one = torch.ones(1, device=dev)
        dist.all_reduce(one)                       # first collective: communicator set-up happens here
        torch.cuda.synchronize()
        stage("first all-reduce done")
        prop = torch.cuda.get_device_properties(dev)
        mine = {"rank": rank, "local_rank": local, "device": f"cuda:{local}", "name": prop.name,
                "pci_bus_id": getattr(prop, "pci_bus_id", None), "uuid": str(getattr(prop, "uuid", "")) or None,
                "pid": os.getpid()}
        gathered = [None] * dist.get_world_size()
        dist.all_gather_object(gathered, mine)
        ranks_info = {"backend": dist.get_backend(), "world_size": dist.get_world_size(),
                      "rccl_ranks": int(one.item()) if args.backend == "nccl" else None,
                      "allreduce_sum_of_ones": int(one.item()), "devices": gathered}

    from tmgcn_amd import _lib
    _lib.load()  # fail loudly if the HIP library is missing

    N, F, Tl = args.nodes, args.feat, args.slices_per_gpu
    if args.graph == "chess_tiled":
        N = max(1, int(round(N / 7301))) * 7301          # whole copies of the 7 301-node operand (synth.device_chess_tiled_csr)
    from tmgcn_amd.dist import memory_plan
    collective = world > 1 or args.force_collectives
    nnz_rank = Tl * N * (args.deg + 1)

    def plan_of(ex, n_nodes):
        ex = ex if collective else "none"
        return memory_plan(ex, Tl * world, world, n_nodes, F, F, Tl * n_nodes * (args.deg + 1),
                           gather_chunk_nodes=args.gather_chunk_nodes)

    def fits(ex, n_nodes):
        """Collective decision, BEFORE anything is allocated: does the plan of mode `ex` at n_nodes fit
        on every rank with 10 % headroom?  (The verify leg sizes its own fp64 buffer against what is
        free when it runs, and does without it otherwise.)"""
        need = plan_of(ex, n_nodes)["total"]
        free_b, _total = torch.cuda.mem_get_info(dev)
        if args.single_device:
            free_b //= world                     # every rank of the emulation allocates on the same device
        ok = torch.tensor([1 if free_b > 1.10 * need else 0], device=dev)
        if dist.is_initialized():
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        return bool(int(ok.item())), need, free_b

    plans = {ex: plan_of(ex, N) for ex in (("a2a", "allgather") if collective else ("none",))}
    for ex, pl in plans.items():
        stage(f"plan[{ex}, N={N}]: {pl['total_gb']} GB per rank (exchange: {pl['exchange'] / 1e9:.1f} GB, {pl['exchange_note']})")
    ok, need, free_b = fits(args.exchange, N)
    if not ok:
        raise SystemExit(f"bench: the '{args.exchange}' plan needs {need / 1e9:.0f} GB per rank but only {free_b / 1e9:.0f} GB "
                         f"are free (rank {rank}); nothing was allocated")
    res = run_layer(args, dist, dev, rank, world, args.exchange, N, args.steps, args.warmup, verify=not args.no_verify,
                    dump_dir=args.dump_outputs)
    free_device_memory()
    hbm_only = None
    if world == 1 and not collective and not args.no_hbm_only and Tl >= 4:
        hbm_only = measure_hbm_only(args, N, Tl, F)
    legs = {}
    if world == 1 and not collective and not args.no_legs and args.graph == "er":
        for name, off in (("skewed", args.no_skewed), ("T128", args.no_t128 or Tl >= 128 or Tl * N < 128 * 64),
                          ("real_structure", args.no_real_structure)):
            if not off:
                legs[name] = measure_leg(args, name)
                free_device_memory()
    if rank == 0:
        # the headline measurement, on stderr, BEFORE the side legs (exchange comparison, epochs, CPU baseline):
        # should one of those die, the record of the run's purpose survives in the log (the JSON line on
        # stdout is printed once, at the end, as the driver's contract wants it)
        stage("headline: " + json.dumps({"n_gpus": world, "exchange": args.exchange if res["collective"] else "none",
                                         "ms_per_step": round(res["elapsed"] / args.steps * 1e3, 3),
                                         "edge_slices_per_s": res["total_nnz"] * args.steps / res["elapsed"],
                                         "verify_ok": (res["verify"] or {}).get("ok")}))

    compare = None
    if collective and not args.no_compare_exchange and res["collective"]:
        # a2a (node -> slice re-partition, the xGMI-first form) and the north-star's literal all-gather
        # (node-chunked, fused with its P1 consumer) side by side: at a reduced N, and at full N
        # whenever the other mode's memory plan fits (decided collectively, before allocating).
        n_cmp = min(N, args.compare_nodes)
        compare = {"reduced_n": {"nodes": n_cmp}}
        for ex in ("a2a", "allgather"):
            ok, need, _ = fits(ex, n_cmp)
            if ok:
                r = run_layer(args, dist, dev, rank, world, ex, n_cmp, 3, 1, want_timer=False)
                compare["reduced_n"][ex + "_ms_per_step"] = round(r["elapsed"] / 3 * 1e3, 3)
                free_device_memory()
            else:
                compare["reduced_n"][ex + "_ms_per_step"] = None
                compare["reduced_n"][ex + "_note"] = f"needs about {need / 1e9:.0f} GB per rank: does not fit here"
        other = "allgather" if args.exchange == "a2a" else "a2a"
        ok, need, _ = fits(other, N)
        compare["full_n"] = {"nodes": N, args.exchange + "_ms_per_step": round(res["elapsed"] / args.steps * 1e3, 3),
                             other + "_plan_gb_per_gpu": round(need / 1e9, 1)}
        if N == n_cmp:
            compare["full_n"][other + "_ms_per_step"] = compare["reduced_n"].get(other + "_ms_per_step")
        elif args.no_compare_full:
            compare["full_n"][other + "_ms_per_step"] = None
            compare["full_n"]["note"] = "not run (--no-compare-full); " + ("it would fit" if ok else "it would not fit at this world size")
        elif ok:
            r = run_layer(args, dist, dev, rank, world, other, N, 3, 1, want_timer=False, verify=not args.no_verify)
            compare["full_n"][other + "_ms_per_step"] = round(r["elapsed"] / 3 * 1e3, 3)
            compare["full_n"][other + "_gather_chunks"] = r["gather_chunks"]
            compare["full_n"][other + "_peak_hbm_gb_rank0"] = round(r["peak_gb"], 1)
            compare["full_n"][other + "_verify"] = r["verify"]
            free_device_memory()
        else:
            compare["full_n"][other + "_ms_per_step"] = None
            compare["full_n"]["note"] = f"the {other} plan ({need / 1e9:.0f} GB per rank) does not fit beside what is resident"

    out = None
    if rank == 0:
        elapsed, kt = res["elapsed"], res["kt"]
        # roofline of the dominant kernel (forward SpMM): SURVEY §8d no-reuse gather model,
        # bytes per edge-slice = 8 (col+val) + F*4 (gathered row) + (4 + F*4)/d (rowptr + output row)
        d = res["nnz_rank"] / res["rows_rank"]
        bytes_per_unit = 8 + F * 4 + (4 + F * 4) / d
        # dominant kernel: the forward SpMM — fused with the GEMM epilogue when the widths allow
        # (then it also writes Y; only P2's own bytes are counted, conservatively)
        dom = "spmm_gemm" if "spmm_gemm" in kt else "spmm"
        sp = kt[dom]
        # The same kernel runs twice per step: forward (Â, also stores AX and Y) and backward (Âᵀ on dY) —
        # the same number of edge-slices and the same algorithmic bytes per edge-slice ("backward
        # P2ᵀ identical").  rocprofv3's per-kernel row averages over ALL its launches, so `avg_launch_ms` does
        # too (it is the figure the committed kernel-stats summary must agree with); the two directions are
        # reported separately beside it.
        spT = kt.get(dom + "_T")
        both = [sp] + ([spT] if spT and spT["launches"] == sp["launches"] else [])
        avg_ms = sum(x["total_ms"] for x in both) / sum(x["launches"] for x in both)
        # one launch per step and direction at N = 1; the pipelined multi-GPU path launches slice by slice
        units_per_launch = res["nnz_rank"] * args.steps / sp["launches"]
        achieved = bytes_per_unit * units_per_launch / (avg_ms * 1e-3) / 1e9
        achieved_fwd = bytes_per_unit * units_per_launch / (sp["avg_ms"] * 1e-3) / 1e9
        traffic, traffic_source = None, None
        if world == 1 and not args.no_measure_traffic and sp["launches"] == args.steps:
            traffic_source, why = measure_traffic(args)
            if traffic_source is None:
                stage(f"traffic: not measured ({why}); quoting the committed PMC record")
                traffic, traffic_source = traffic_record(N, F, Tl)
                if traffic_source is not None:
                    traffic_source["not_measured_because"] = why
            else:
                traffic = traffic_source["forward_bytes"]
        elif sp["launches"] == args.steps:
            traffic, traffic_source = traffic_record(N, F, Tl)
        out = {
            "metric": "TM-GCN layer fwd+bwd throughput (edges x T)/s",
            "value": res["total_nnz"] * args.steps / elapsed,
            "unit": "edge-slices/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"S4 TM-GCN layer fwd+bwd: {Tl} slices/GPU (T={res['T']}), N={N}, "
                                   + (f"{res['total_nnz'] / (world * Tl * N):.2f} entries per row (the chess operand's own row lengths), "
                                      if args.graph == "chess_tiled" else
                                      f"deg={args.deg}+self{'' if args.graph == 'er' else ' on average (' + args.graph + ' row lengths)'}, ") +
                                   f"F={F}->{F}, band-M b={args.band}, fp32",
                       "exchange": args.exchange if res["collective"] else "none", "grid_reserve": res["grid_reserve"],
                       "cu_reserve": res["cu_reserve"],
                       "edge_slices_per_step": res["total_nnz"]},
            "roofline": {"kernel": "spmm_gemm_kernel (P2 + fused P3: forward on Â and backward on Âᵀ, averaged over both launches)"
                         if dom == "spmm_gemm" else "spmm_vec4_kernel (P2, forward and backward launches)",
                         "bound": "hbm", "achieved": achieved,
                         "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": traffic, "traffic_source": traffic_source,
                         "achieved_is": "algorithmic bytes (SURVEY §8d no-reuse gather model) / measured launch time, as a "
                                        "fraction of the 8 TB/s spec; part of the gather is served by the 256 MB Infinity Cache",
                         "bytes_per_edge_slice": bytes_per_unit, "edge_slices_per_launch": units_per_launch,
                         "avg_launch_ms": avg_ms, "launches_averaged": sum(x["launches"] for x in both),
                         "forward_launch_ms": sp["avg_ms"], "backward_launch_ms": spT["avg_ms"] if spT else None,
                         "frac_forward_only": achieved_fwd / HBM_PEAK_GBS,
                         **hbm_only_fields(hbm_only, dom, F),
                         "traffic_is_for": "the forward launch (the larger of the two: it also stores AX and Y)",
                         "note": None if sp["launches"] == args.steps else
                         "pipelined multi-GPU path: one-slice launches alternate between two streams and are enqueued ahead, so a "
                         "launch's event-to-event time includes waiting for residency: achieved / frac are LOWER bounds here; "
                         "the N = 1 line carries the kernel's own figure"},
            "kernels_ms": {k: round(v["avg_ms"], 4) for k, v in kt.items()},
            "phases_ms": res["phases"],
            "peak_hbm_gb_rank0": round(res["peak_gb"], 1),
            "plan": {ex: {"total_gb": pl["total_gb"], "exchange_gb": round(pl["exchange"] / 1e9, 2), "exchange": pl["exchange_note"]}
                     for ex, pl in plans.items()},
            "verify": res["verify"],
        }
        if args.graph != "er":
            out["config"]["graph"] = args.graph
        out["config"]["row_lengths"] = res["row_stats"]
        # the side legs: full records at the top level, and the figures a reader needs first inside `roofline` (a container
        # the driver's parser keeps)
        for name, rec in legs.items():
            out["roofline_" + name] = rec
        out["roofline"]["legs"] = {name: ({"error": rec["error"]} if "error" in rec else
                                          {"frac": rec["frac"], "achieved": rec["achieved"], "frac_forward_only": rec["frac_forward_only"],
                                           "basis_forward": rec["forward"]["basis"], "basis_backward": (rec["backward"] or {}).get("basis"),
                                           "frac_model_forward": rec["forward"]["frac_model"],
                                           "forward_launch_ms": rec["forward_launch_ms"], "backward_launch_ms": rec["backward_launch_ms"],
                                           "traffic": rec["traffic"], "traffic_backward": rec["traffic_backward"],
                                           "model_bytes_per_launch": rec["forward"]["model_bytes"],
                                           "ms_per_step": rec["ms_per_step"], "verify_ok": rec["verify_ok"],
                                           **({"mfma_frac_forward": rec["mfma"]["frac_forward"]} if "mfma" in rec else {})})
                                   for name, rec in legs.items()}
        if res["gather_chunks"] is not None:
            out["config"]["gather_chunks"] = res["gather_chunks"]
        if ranks_info is not None:
            out["ranks"] = ranks_info
        if compare is not None:
            out["exchange_compare"] = compare
        if "gemm_dW" in kt:
            # the one GEMM that still runs as its own kernel (dW = AXᵀ·dY); the forward / dA GEMMs run
            # inside the fused SpMM kernels, hidden under the gather.  At 128x128 its arithmetic intensity
            # (192 bf16-flop per byte streamed) is on the MEMORY side of the bf16 ridge (312 flop/B): HBM is
            # its roof, the matrix-core figures are reported beside it.
            t_dw = kt["gemm_dW"]["avg_ms"] * 1e-3
            fp32_tf = 2.0 * res["rows_rank"] * F * F / t_dw / 1e12
            gbs = res["rows_rank"] * 2 * F * 4 / t_dw / 1e9
            out["dw_roofline"] = {"kernel": "gemm_dw_bf16x3_kernel (dW)", "bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS,
                                  "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS, "avg_launch_ms": kt["gemm_dW"]["avg_ms"],
                                  "bytes_per_row": 2 * F * 4,
                                  "mfma_tflops_bf16": 6.0 * fp32_tf, "mfma_frac_of_2500": 6.0 * fp32_tf / 2500.0,
                                  "fp32_equivalent_tflops": fp32_tf,
                                  "dtype": "bf16 planes of an exact 3-way fp32 split (v_mfma_f32_32x32x16_bf16), fp32 accumulate",
                                  "note": "6 bf16 MFMA products per fp32 term; runs at the 1400 W board cap with the shader clock "
                                          "pulled down (profiles/archive/r02t_power_probe.jsonl)"}
        if world == 1:  # the CPU legs are reported at N = 1 only
            if not args.no_epochs:
                out["epochs"] = epochs_block(args)
                # the four epoch times once more as FLAT top-level numbers (a driver that keeps only scalar keys keeps these):
                # best mode, the untouched-script mode, and the CPU oracle's epoch
                for name, rec in out["epochs"].items():
                    if not isinstance(rec, dict) or "error" in rec:
                        continue
                    gpu = {k: v for k, v in rec.items() if k.startswith("gpu_ms_") and isinstance(v, float)}
                    if gpu:
                        out[f"epoch_ms_{name}"] = min(gpu.values())
                    if "gpu_ms_script" in rec:
                        out[f"epoch_ms_script_{name}"] = rec["gpu_ms_script"]
                    if rec.get("cpu_ms") is not None:
                        out[f"epoch_ms_cpu_{name}"] = rec["cpu_ms"]
            if not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline(args)
                cb = out["cpu_baseline"]
                # the GPU/CPU ratio of the headline, inside a container the driver's parser keeps.  `vs_baseline` stays
                # null: BASELINE.md holds no published number for this metric (§1 "None")
                cb["gpu_over_cpu"] = out["value"] / cb["value"] if cb.get("value") else None
                # north_star's ">= 10x reference CPU epoch throughput on Reddit link prediction at 1 GPU": the epoch times
                # of the reference-shaped configs, GPU beside the CPU oracle (the same numbers as out["epochs"], condensed)
                if "epochs" in out:
                    ce = {}
                    for name, rec in out["epochs"].items():
                        if not isinstance(rec, dict) or "error" in rec:
                            continue
                        gpu = {k: v for k, v in rec.items() if k.startswith("gpu_ms_") and isinstance(v, float)}
                        if not gpu or rec.get("cpu_ms") is None:
                            continue
                        best = min(gpu, key=gpu.get)
                        e = {"gpu_captured_ms": gpu[best], "gpu_best_mode": best[len("gpu_ms_"):], "gpu_eager_ms": rec.get("gpu_ms_eager"),
                             "gpu_script_ms": rec.get("gpu_ms_script"), "cpu_ms": rec["cpu_ms"], "cpu_threads": rec.get("cpu_threads"),
                             "speedup_best": round(rec["cpu_ms"] / gpu[best], 1)}
                        if rec.get("gpu_ms_script"):
                            e["speedup_script"] = round(rec["cpu_ms"] / rec["gpu_ms_script"], 1)
                        ce[name] = e
                    ce["what"] = ("training epoch (zero_grad, gcn(), class-weighted CE, backward, SGD step: "
                                  "experiment_reddit_our_link_prediction.py:75-81) in ms; S2 = the Reddit-LP-shaped config of north_star's "
                                  ">= 10x target; gpu_script = an untouched reference script on `import tmgcn_amd.ehf as ehf`; cpu = the "
                                  "oracle run the reference's way, median epoch")
                    cb["epochs"] = ce
    # RCCL prints its version banner through C stdio, which is flushed only at exit when stdout is
    # a pipe/file: every rank flushes it BEFORE the last barrier so that rank 0's JSON line is the
    # last line of the job's stdout.
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.flush()
    if dist.is_initialized():
        stage("final barrier")
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        # a reader's summary on stderr (the JSON line on stdout stays the last line of stdout, alone)
        try:
            r = out["roofline"]
            stage(f"summary: {out['ms_per_step']:.1f} ms/step, {out['value'] / 1e9:.2f} G edge-slices/s, roofline.frac {r['frac']:.3f}"
                  + (f" (hbm-only {r['frac_hbm_only']:.3f})" if r.get("frac_hbm_only") is not None else "")
                  + (f", verify {'ok' if (out.get('verify') or {}).get('ok') else 'FAILED'}" if out.get("verify") else ""))
            for name, leg in (r.get("legs") or {}).items():
                if "error" in leg:
                    stage(f"summary: leg {name}: {leg['error']}")
                else:
                    stage(f"summary: leg {name}: forward {leg['forward_launch_ms']:.1f} ms / backward {leg['backward_launch_ms']:.1f} ms, "
                          f"frac {leg['frac']:.3f} (forward {leg['frac_forward_only']:.3f} on {leg['basis_forward']} bytes, backward on "
                          f"{leg['basis_backward']} bytes), {leg['ms_per_step']:.1f} ms/step, verify {'ok' if leg['verify_ok'] else 'FAILED'}")
            cb = out.get("cpu_baseline")
            if cb:
                stage(f"summary: cpu_baseline {cb['value'] / 1e6:.2f} M edge-slices/s on {cb['cores']} threads (GPU / CPU {cb.get('gpu_over_cpu') or 0:.0f}x)"
                      + "".join(f"; {k} epoch {v['gpu_captured_ms']:.3f} ms captured / {v.get('gpu_script_ms') or float('nan'):.3f} script / "
                                f"{v['cpu_ms']:.0f} CPU" for k, v in (cb.get("epochs") or {}).items() if isinstance(v, dict) and k in ("S2",)))
        except Exception as e:                       # never let a summary line cost the record
            stage(f"summary: not printed ({e!r})")
        print(json.dumps(out), flush=True)
    stage("done")
    bad = [v for v in (res.get("verify"), ((compare or {}).get("full_n") or {}).get(
        ("allgather" if args.exchange == "a2a" else "a2a") + "_verify")) if v is not None and not v["ok"]]
    for name, rec in legs.items():
        if "error" not in rec and rec.get("verify_ok") is False:
            bad.append({"roofline_" + name: rec.get("verify")})
    if bad:
        sys.stderr.write(f"[bench r{rank}] VERIFY FAILED: {json.dumps(bad)}\n")
        sys.exit(3)


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher around us: become one.  Nothing in this process has touched the GPU
        # (torch is not even imported), the ranks are fresh processes.
        sys.exit(launch(args))
    worker(args)


if __name__ == "__main__":
    main()
