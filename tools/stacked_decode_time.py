"""What decoding the 2- and 3-layer seq2seq LSTM models in ONE launch (fov_stacked_seq2seq_decode_fwd) is worth against the
host loop it replaces - per predicted second one launch per layer plus one Dense, plus a launch per encoder layer - which is
the parent commit's code path, unchanged.

One process, device-resident inputs and weights, HIP events around `--calls` back-to-back calls; the fused call and the loop
alternate, `--repeats` times each (StackedSeq2SeqLSTM.decode_device with fused=True / fused=False; the library's knob is
cached per process, so it is not what switches here).  A row reports median / min / max; the verdict row of a shape says
whether the fused call's SLOWEST repeat beats the loop's FASTEST one (the rule of DESIGN.md section 5), the time per
layer-step the fused call implies (the slope between the full lengths and T 2 -> 2, so without launch and weight prologue)
next to the arithmetic estimate of 32 cycles x (K_in + H) MFMAs per wave, and the launches the loop pays.

Shapes: the scripts' own (B 64, F 6, H 32, T 10 -> 10) and the metric's horizon at scale (B 1024 and 4096, F 90, H 64,
T 30 -> 30), L = 2 and 3.

    python tools/stacked_decode_time.py [--repeats 5] [--calls 50] [--out profiles/stacked_decode_time.jsonl]
"""
import argparse
import gc
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(64, 6, 32, 10, 10), (1024, 90, 64, 30, 30), (4096, 90, 64, 30, 30)]      # B, F_enc, H, T_in, T_out
CLOCK_GHZ = 2.4


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "repeats": len(v)}


def event_ms(torch, fn, calls):
    gc.collect()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join("profiles", "stacked_decode_time.jsonl"))
    a = ap.parse_args()
    import torch
    from longterm360fov_amd.models import StackedSeq2SeqLSTM
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for B, F, H, T_in, T_out in SHAPES:
        for L in (2, 3):
            m = StackedSeq2SeqLSTM(num_encoder_tokens=F, latent_dim=H, num_layers=L, recurrent_activation="sigmoid", seed=L)
            rng = np.random.default_rng(B + L)
            e = torch.from_numpy(rng.uniform(-1, 1, (B, T_in, F)).astype(np.float32)).cuda()
            d0 = torch.from_numpy(rng.uniform(-1, 1, (B, 1, 6)).astype(np.float32)).cuda()
            legs = {"fused": lambda: m.decode_device(e, d0, T_out, fused=True), "loop": lambda: m.decode_device(e, d0, T_out, fused=False)}
            outs = {k: fn() for k, fn in legs.items()}      # warm-up: weights uploaded and padded, LDS attribute set
            for fn in legs.values():
                fn()
            torch.cuda.synchronize()
            m._ws.check()
            diff = float((outs["fused"] - outs["loop"]).abs().max().item())
            times = {k: [] for k in legs}
            for _ in range(a.repeats):
                for k, fn in legs.items():
                    times[k].append(event_ms(torch, fn, a.calls))
            shape = {"B": B, "F_enc": F, "H": H, "L": L, "T_in": T_in, "T_out": T_out}
            for k in legs:
                emit({**shape, "call": k, "calls": a.calls, **stats(times[k])})
            e2 = e[:, :2].contiguous()
            legs["fused, T 2 -> 2"] = lambda: m.decode_device(e2, d0, 2, fused=True)
            times["fused, T 2 -> 2"] = [event_ms(torch, legs["fused, T 2 -> 2"], a.calls) for _ in range(a.repeats)]
            emit({**shape, "call": "fused, T 2 -> 2", "calls": a.calls, **stats(times["fused, T 2 -> 2"])})
            # slope between the two lengths: a layer-step without the launch and the weight prologue
            per_step_us = (float(np.median(times["fused"])) - float(np.median(times["fused, T 2 -> 2"]))) * 1e3 / (L * (T_in + T_out - 4))
            emit({**shape, "tiles": (B + 15) // 16, "loop_launches": L + T_out * (L + 1), "max_abs_fused_minus_loop": diff,
                  "speedup_median": float(np.median(times["loop"]) / np.median(times["fused"])),
                  "slowest_fused_ms": float(np.max(times["fused"])), "fastest_loop_ms": float(np.min(times["loop"])),
                  "slowest_fused_beats_fastest_loop": bool(np.max(times["fused"]) < np.min(times["loop"])),
                  "fused_us_per_layer_step": per_step_us,
                  "fused_cycles_per_layer_step_at_%.1f_GHz" % CLOCK_GHZ: per_step_us * CLOCK_GHZ * 1e3,
                  "mfma_cycles_per_layer_step_estimate": 32 * (H + H)})
            del m, e, d0, outs
            gc.collect()
            torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
