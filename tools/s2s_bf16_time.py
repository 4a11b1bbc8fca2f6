"""fp32 against bf16 operands on the target-only seq2seq model, in one process, alternating.

Inference: the fused call (ops.seq2seq_decode, dtype f32 / bf16) at B 512 / 1024 / 4096, T 30 -> 30, H 256, with the
headline's protocol (bench.py --mode infer): inputs resident on the device, warm-up calls, then K calls between two HIP
events; the two forms alternate, `--repeats` times each.  Training: Seq2SeqTrainer.train_step (Adam) at B 1024,
T 30 -> 30, both forms alternating the same way.  One JSON line per (phase, batch, dtype) with the median, min and max
over the repeats, and per batch the largest difference between the two forms' outputs (inference) or losses (training).
The per-step time of the fused call is the call time / (tile rounds x (T_in + T_out)), rounds = ceil(tiles / groups) with
one group of eight workgroups per 16-sequence tile and at most CUs / 8 groups.

    python tools/s2s_bf16_time.py [--calls 200] [--repeats 5] [--batches 512,1024,4096] [--train-batch 1024] [--only-bf16]
"""
import argparse
import gc
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from longterm360fov_amd import ops  # noqa: E402
from longterm360fov_amd.training import Seq2SeqTrainer  # noqa: E402
from oracle import fov_oracle as O  # noqa: E402


def event_ms(fn, calls):
    gc.collect()
    gc.freeze()
    for _ in range(3):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "repeats": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", default="512,1024,4096")
    ap.add_argument("--train-batch", type=int, default=1024, help="0: no training phase")
    ap.add_argument("--train-steps", type=int, default=50)
    ap.add_argument("--t-in", type=int, default=30)
    ap.add_argument("--t-out", type=int, default=30)
    ap.add_argument("--only-bf16", action="store_true", help="the bf16 fused call alone (a profiler run)")
    args = ap.parse_args()
    T_in, T_out, H = args.t_in, args.t_out, 256
    dtypes = ("bf16",) if args.only_bf16 else ("f32", "bf16")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    w = O.init_seq2seq(1234, 90, 6, H, bias_noise=0.05)
    dw = {k: torch.from_numpy(v).cuda() for k, v in w.items()}
    for B in [int(b) for b in args.batches.split(",") if b]:
        enc, dec0, _ = O.synthetic_batch(1234, B, T_in, T_out)
        d_enc, d_dec0 = torch.from_numpy(enc).cuda(), torch.from_numpy(dec0).cuda()
        ws = {dt: ops.Workspace() for dt in dtypes}
        out = {dt: torch.empty((B, T_out, 6), dtype=torch.float32, device="cuda") for dt in dtypes}
        call = {dt: (lambda dt=dt: ops.seq2seq_decode(d_enc, d_dec0, dw, T_out, workspace=ws[dt], out=out[dt], dtype=dt))
                for dt in dtypes}
        for dt in dtypes:
            for _ in range(args.warmup):
                call[dt]()
        torch.cuda.synchronize()
        times = {dt: [] for dt in dtypes}
        for _ in range(args.repeats):
            for dt in dtypes:
                times[dt].append(event_ms(call[dt], args.calls))
        for dt in dtypes:
            ws[dt].check()
        tiles = (B + 15) // 16
        rounds = -(-tiles // min(tiles, cus // 8))
        for dt in dtypes:
            s = stats(times[dt])
            line = {"phase": "infer", "dtype": dt, "B": B, "T_in": T_in, "T_out": T_out, "H": H, "calls": args.calls, **s,
                    "sequences_per_s": B / (s["median_ms"] * 1e-3)}
            if dt == "bf16":
                line["tile_rounds"] = rounds
                line["us_per_step"] = s["median_ms"] * 1e3 / (rounds * (T_in + T_out))
            print(json.dumps(line), flush=True)
        if len(dtypes) == 2:
            a, b = out["f32"].cpu().numpy(), out["bf16"].cpu().numpy()
            print(json.dumps({"phase": "infer", "B": B, "max_abs_diff_bf16_vs_f32": float(np.abs(a - b).max()),
                              "bf16_speedup": float(np.median(times["f32"]) / np.median(times["bf16"]))}), flush=True)
    if args.train_batch and not args.only_bf16:
        B = args.train_batch
        enc, dec0, tgt = O.synthetic_batch(99, B, T_in, T_out)
        dec_in = np.concatenate([dec0, tgt[:, :-1]], axis=1)
        d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (enc, dec_in, tgt)]
        tr = {dt: Seq2SeqTrainer(w, dtype=dt) for dt in dtypes}
        loss = {}

        def step(dt):
            loss[dt] = tr[dt].train_step(*d)

        for dt in dtypes:
            for _ in range(args.warmup):
                step(dt)
        torch.cuda.synchronize()
        times = {dt: [] for dt in dtypes}
        for _ in range(args.repeats):
            for dt in dtypes:
                times[dt].append(event_ms(lambda dt=dt: step(dt), args.train_steps))
        for dt in dtypes:
            tr[dt].check()
            s = stats(times[dt])
            print(json.dumps({"phase": "train", "dtype": dt, "B": B, "T_in": T_in, "T_out": T_out, "H": H, "steps": args.train_steps,
                              **s, "loss": float(loss[dt].item())}), flush=True)
        print(json.dumps({"phase": "train", "B": B, "bf16_speedup": float(np.median(times["f32"]) / np.median(times["bf16"])),
                          "loss_rel_diff_bf16_vs_f32": abs(float(loss["bf16"].item()) / float(loss["f32"].item()) - 1.0)}), flush=True)


if __name__ == "__main__":
    main()
