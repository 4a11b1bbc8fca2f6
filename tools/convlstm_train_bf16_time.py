"""fp32 against bf16 head operands in the ConvLSTM heat-map model's TRAINING step (configs[3]), in one process, alternating.

(a) `layers`: the three head layers Conv2D 56 -> 512 -> 1024 -> 30 (k = 5) on 36 x 18 maps, each of the three products of a
    training step in both dtypes, ms and TFLOP/s from HIP events: forward and data gradient per decoder step (B maps),
    weight gradient as the trainer forms it, ONE product over the T_out * B maps of all steps.  The last layer's data
    gradient (30 input channels) is timed both ways: on the 30-channel dy (plain forward kernel) and on the dy padded to 32
    channels (map-resident kernel), which is what ConvLSTMTrainer(head_dtype='bf16') runs.
(b) `packs`: what rebuilding the six bf16 packs from the fp32 master weights costs per step.
(c) `step`: ConvLSTMTrainer.train_step at B 256, T 10 -> 10, head_dtype f32 and bf16 alternated, `--repeats` times each; the
    feature is a win when the slowest bf16 repeat beats the fastest fp32 repeat.
One JSON line per row on stdout and in --out (default profiles/convlstm_train_bf16_time.jsonl, written anew; '-': no file).

    python tools/convlstm_train_bf16_time.py [--batch 256] [--reps 3] [--repeats 5] [--no-layers] [--no-step] [--out FILE]
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
from longterm360fov_amd.training import ConvLSTMTrainer  # noqa: E402
from oracle import fov_oracle as O  # noqa: E402

H, W, C, T = 36, 18, 30, 10
PEAK = {"f32": 157.3, "bf16": 2500.0}       # matrix peak, TFLOP/s
OUT = None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def event_ms(fn, calls):
    gc.collect()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "repeats": len(v)}


def alternate(call, reps, repeats):
    for fn in call.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in call}
    for _ in range(repeats):
        for k, fn in call.items():
            times[k].append(event_ms(fn, reps))
    return times


def layers(B, reps, repeats):
    sc = ops.Scratch()
    for name, c, n in (("head0 56->512", 56, 512), ("head1 512->1024", 512, 1024), ("head2 1024->30", 1024, 30)):
        xs = torch.rand((T * B, H, W, c), device="cuda")            # the layer's input over all steps
        dys = torch.rand((T * B, H, W, n), device="cuda") - 0.5
        x, dy = xs[:B], dys[:B]
        dys_b = dys       # what the bf16 weight gradient reads: for a ragged N the view of a buffer padded to a multiple of 4
        if n % 4:
            dys_b = torch.zeros((T * B, H, W, n + (-n) % 4), device="cuda")
            dys_b[..., :n] = dys
            dys_b = dys_b[..., :n]
        w = (torch.rand((5, 5, c, n), device="cuda") - 0.5) * 0.02
        b = torch.zeros(n, device="cuda")
        y, dx = torch.empty((B, H, W, n), device="cuda"), torch.empty((B, H, W, c), device="cuda")
        dw = torch.empty_like(w)
        packed = ops.conv2d_pack_bf16(w)
        wt = ops.conv2d_weight_transpose(w)
        wtb, wtp = ops.conv2d_bwd_data_pack_bf16(w)
        rows = [("forward", B, {"f32": lambda: ops.conv2d(x, w, b, activation="relu", out=y),
                                "bf16": lambda: ops.conv2d_bf16(x, w, b, activation="relu", out=y, packed=packed)}),
                ("data gradient", B, {"f32": lambda: ops.conv2d(dy, wt, out=dx),
                                      "bf16": lambda: ops.conv2d_bf16(dy, wtb, out=dx, packed=wtp)}),
                ("weight gradient", T * B, {"f32": lambda: ops.conv2d_wgrad(xs, dys, 5, 5, dw=dw, scratch=sc),
                                            "bf16": lambda: ops.conv2d_wgrad_bf16(xs, dys_b, 5, 5, dw=dw, scratch=sc)})]
        pad = (-n) % 4
        if pad:       # the padded dy of the last layer
            dyp = torch.zeros((B, H, W, n + pad), device="cuda")
            dyp[..., :n] = dy
            wtb2, wtp2 = ops.conv2d_bwd_data_pack_bf16(w, pad)
            rows.append(("data gradient, dy padded to %d channels" % (n + pad), B,
                         {"bf16": lambda: ops.conv2d_bf16(dyp, wtb2, out=dx, packed=wtp2)}))
        for prod, maps, call in rows:
            times = alternate(call, reps, repeats)
            flop = 2.0 * 25 * c * n * maps * H * W
            for dt in call:
                s = stats(times[dt])
                tf = flop / s["median_ms"] / 1e9
                emit({"phase": "layers", "layer": name, "product": prod, "dtype": dt, "maps": maps, "launches": reps, **s, "tflops": tf,
                      "frac_of_peak": tf / PEAK[dt]})
            if len(call) == 2:
                emit({"phase": "layers", "layer": name, "product": prod, "bf16_speedup": float(np.median(times["f32"]) / np.median(times["bf16"]))})
        del xs, dys, dys_b, x, dy, y, dx, rows
        torch.cuda.empty_cache()


def packs(repeats):
    w = O.init_convlstm_seq2seq(1, C=C, latent_dim=16, head="conv2d")
    ws = [torch.from_numpy(w["head%d_W" % i]).cuda() for i in range(3)]

    def all_packs():
        for i, v in enumerate(ws):
            ops.conv2d_pack_bf16(v)
            ops.conv2d_bwd_data_pack_bf16(v, 2 if i == 2 else 0)
    times = alternate({"packs": all_packs}, 3, repeats)
    emit({"phase": "packs", "what": "three forward packs + three transposed packs (transpose, pack) per step", **stats(times["packs"]),
          "fp32_weight_mbytes": sum(v.numel() for v in ws) * 4 / 1e6})


def step(B, repeats):
    w = O.init_convlstm_seq2seq(1, C=C, latent_dim=16, head="conv2d")
    enc = torch.rand((B, T, H, W, C), device="cuda")
    dec0 = enc[:, -1:].contiguous()
    tgt = torch.rand((B, T, H, W, C), device="cuda")
    tgt = tgt / tgt.sum(-1, keepdim=True)
    tr = {dt: ConvLSTMTrainer(w, head="conv2d", head_dtype=dt) for dt in ("f32", "bf16")}
    losses = {dt: float(tr[dt].train_step(enc, dec0, tgt).item()) for dt in tr}      # warm-up: allocator, scratch
    times = alternate({dt: (lambda dt=dt: tr[dt].train_step(enc, dec0, tgt)) for dt in tr}, 1, repeats)
    for dt in tr:
        tr[dt].check()
        s = stats(times[dt])
        emit({"phase": "step", "head_dtype": dt, "B": B, "T_in": T, "T_out": T, **s, "first_loss": losses[dt],
              "sequences_per_s": B / (s["median_ms"] * 1e-3)})
    emit({"phase": "step", "B": B, "bf16_speedup": float(np.median(times["f32"]) / np.median(times["bf16"])),
          "slowest_bf16_ms": float(np.max(times["bf16"])), "fastest_f32_ms": float(np.min(times["f32"])),
          "slowest_bf16_beats_fastest_f32": bool(np.max(times["bf16"]) < np.min(times["f32"]))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3, help="launches per timed region of a head layer")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "convlstm_train_bf16_time.jsonl"))
    a = ap.parse_args()
    global OUT
    if a.out != "-":
        OUT = a.out
        open(OUT, "w").close()
    if not a.no_layers:
        layers(a.batch, a.reps, a.repeats)
    packs(a.repeats)
    if not a.no_step:
        step(a.batch, a.repeats)


if __name__ == "__main__":
    main()
