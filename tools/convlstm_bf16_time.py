"""fp32 against bf16 operands on the ConvLSTM heat-map model's Conv2D head (configs[3]), in one process, alternating.

(a) `layers`: the three head layers Conv2D 56 -> 512 -> 1024 -> 30 (k = 5, relu) at B x 36 x 18, ops.conv2d against
    ops.conv2d_bf16 on packed weights, ms and TFLOP/s per launch from HIP events.
(b) `predict`: ConvLSTMSeq2Seq.predict_device at B 256, T 10 -> 10 with the maps resident on the device (bench.py --mode
    convlstm's protocol and inputs), dtype f32 and bf16 alternated, `--repeats` times each: median / min / max, the largest
    difference between the two outputs, and the time of the sixty ConvLSTM cell launches alone (thirty encoder, thirty
    decoder steps: fp32 in both models - what a bf16 cell would still have to win).
One JSON line per row.

    python tools/convlstm_bf16_time.py [--batch 256] [--reps 10] [--repeats 5] [--calls 2] [--only-bf16] [--no-layers]
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
from longterm360fov_amd.models import ConvLSTMSeq2Seq  # noqa: E402
from oracle import fov_oracle as O  # noqa: E402

H, W, C, T = 36, 18, 30, 10
PEAK = {"f32": 157.3, "bf16": 2500.0}       # matrix peak, TFLOP/s


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


def layers(B, reps, repeats, dtypes):
    for name, c, n in (("head0 56->512", 56, 512), ("head1 512->1024", 512, 1024), ("head2 1024->30", 1024, 30)):
        x = torch.rand((B, H, W, c), device="cuda")
        w = torch.rand((5, 5, c, n), device="cuda") * 0.01
        b = torch.zeros(n, device="cuda")
        y = torch.empty((B, H, W, n), device="cuda")
        packed = ops.conv2d_pack_bf16(w)
        call = {"f32": lambda: ops.conv2d(x, w, b, activation="relu", out=y),
                "bf16": lambda: ops.conv2d_bf16(x, w, b, activation="relu", out=y, packed=packed)}
        for dt in dtypes:
            call[dt]()
            call[dt]()
        torch.cuda.synchronize()
        times = {dt: [] for dt in dtypes}
        for _ in range(repeats):
            for dt in dtypes:
                times[dt].append(event_ms(call[dt], reps))
        flop = 2.0 * 25 * c * n * B * H * W
        for dt in dtypes:
            s = stats(times[dt])
            tf = flop / s["median_ms"] / 1e9
            print(json.dumps({"phase": "layers", "layer": name, "dtype": dt, "B": B, "launches": reps, **s, "tflops": tf,
                              "frac_of_peak": tf / PEAK[dt]}), flush=True)
        if len(dtypes) == 2:
            print(json.dumps({"phase": "layers", "layer": name, "B": B,
                              "bf16_speedup": float(np.median(times["f32"]) / np.median(times["bf16"]))}), flush=True)
        del x, w, y, packed
        torch.cuda.empty_cache()


def predict(B, calls, repeats, dtypes):
    w = O.init_convlstm_seq2seq(1, C=C, latent_dim=16, head="conv2d")
    x0 = torch.rand((B, T, H, W, C), device="cuda")
    dec0 = x0[:, -1:].contiguous()
    models = {dt: ConvLSTMSeq2Seq(w, head="conv2d", dtype=dt) for dt in dtypes}
    out = {}
    for dt in dtypes:
        out[dt] = models[dt].predict_device(x0, dec0, T)       # warm-up: device weights, packed head, allocator
    torch.cuda.synchronize()
    times = {dt: [] for dt in dtypes}
    for _ in range(repeats):
        for dt in dtypes:
            times[dt].append(event_ms(lambda dt=dt: models[dt].predict_device(x0, dec0, T), calls))
    head_flop = 2.0 * 25 * (56 * 512 + 512 * 1024 + 1024 * 30) * H * W * B * T
    for dt in dtypes:
        s = stats(times[dt])
        print(json.dumps({"phase": "predict", "dtype": dt, "B": B, "T_in": T, "T_out": T, "calls": calls, **s,
                          "sequences_per_s": B / (s["median_ms"] * 1e-3), "head_tflop_per_call": head_flop / 1e12}), flush=True)
    if len(dtypes) == 2:
        a, b = out["f32"].cpu().numpy(), out["bf16"].cpu().numpy()
        print(json.dumps({"phase": "predict", "B": B, "max_abs_diff_bf16_vs_f32": float(np.abs(a - b).max()),
                          "bf16_speedup": float(np.median(times["f32"]) / np.median(times["bf16"]))}), flush=True)
    # the sixty cell launches of one predict call: the encoder's thirty and the decoder's thirty (on a fixed input map)
    dw = next(iter(models.values()))._dw
    filters = (32, 16, 8)
    xe = torch.cat([x0, torch.zeros((B, T, H, W, 2), device="cuda")], -1)

    def cells():
        seq = [xe[:, t] for t in range(T)]
        states = []
        for l, F in enumerate(filters):
            h = torch.zeros((B, H, W, F), device="cuda")
            c = torch.zeros((B, H, W, F), device="cuda")
            nxt = []
            for t in range(T):
                hn = torch.empty((B, H, W, F), device="cuda")
                ops.convlstm_cell(seq[t], h, dw["enc%d_KR" % l], dw["enc%d_b" % l], c, hn, "hard_sigmoid")
                h = hn
                nxt.append(h)
            seq = nxt
            states.append([h, c])
        for t in range(T):
            feat = torch.empty((B, H, W, sum(filters)), device="cuda")
            cur, off = xe[:, -1], 0
            for l, F in enumerate(filters):
                hslot = feat[..., off:off + F]
                ops.convlstm_cell(cur, states[l][0], dw["dec%d_KR" % l], dw["dec%d_b" % l], states[l][1], hslot, "hard_sigmoid")
                states[l][0] = hslot
                cur = hslot
                off += F

    cells()
    torch.cuda.synchronize()
    s = stats([event_ms(cells, calls) for _ in range(repeats)])
    print(json.dumps({"phase": "predict", "part": "sixty fp32 cell launches", "B": B, **s}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10, help="launches per timed region of a head layer")
    ap.add_argument("--calls", type=int, default=2, help="predict_device calls per timed region")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only-bf16", action="store_true", help="the bf16 model alone (a profiler run)")
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--no-predict", action="store_true")
    a = ap.parse_args()
    dtypes = ("bf16",) if a.only_bf16 else ("f32", "bf16")
    if not a.no_layers:
        layers(a.batch, a.reps, a.repeats, dtypes)
    if not a.no_predict:
        predict(a.batch, a.calls, a.repeats, dtypes)


if __name__ == "__main__":
    main()
