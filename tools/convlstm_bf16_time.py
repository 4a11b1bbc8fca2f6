"""fp32 against bf16 operands on the ConvLSTM heat-map model's Conv2D head (configs[3]), in one process, alternating.

(a) `layers`: the three head layers Conv2D 56 -> 512 -> 1024 -> 30 (k = 5, relu) at B x 36 x 18, ops.conv2d against
    ops.conv2d_bf16 on packed weights, ms and TFLOP/s per launch from HIP events.
(b) `predict`: ConvLSTMSeq2Seq.predict_device at B 256, T 10 -> 10 with the maps resident on the device (bench.py --mode
    convlstm's protocol and inputs), three models alternated, `--repeats` times each - dtype f32, dtype bf16 (fp32 cells) and
    dtype bf16 with cell_dtype bf16 ("bf16+cells") -: median / min / max, the largest difference between the outputs, and
    the time of the sixty ConvLSTM cell launches alone (thirty encoder, thirty decoder steps), fp32 cells and bf16 cells
    alternated.
(c) `cells`: the three cell shapes of configs[3] (32 + 32, 32 + 16, 16 + 8 channels -> 4F gate columns, k = 5),
    ops.convlstm_cell against ops.convlstm_cell_bf16 on packed weights, ms and TFLOP/s per launch from HIP events.
    Each row carries the two floors arithmetic gives a launch: the matrix work at the bf16 peak and the fp32 maps it moves
    (x, h_prev, c_prev in; c, h out) at the measured 6.29 TB/s copy rate.
One JSON line per row on stdout.  A run with the bf16 cells in it also writes the lines to --out (default
profiles/convlstm_cell_bf16_time.jsonl, written anew by every run; `--out -` writes no file).  --no-bf16-cells leaves the
third model leg, the bf16 pass over the sixty cells and phase (c) out: the tool as it was before the bf16 cells, for
profiles/convlstm_bf16_time.jsonl and the rocprofv3 recipe of profiles/README.md.

    python tools/convlstm_bf16_time.py [--batch 256] [--reps 10] [--repeats 5] [--calls 2] [--only-bf16] [--no-layers]
                                       [--no-predict] [--no-cells] [--no-bf16-cells] [--out FILE]
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
COPY_TBS = 6.29                             # measured device copy rate, TB/s


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
            emit({"phase": "layers", "layer": name, "dtype": dt, "B": B, "launches": reps, **s, "tflops": tf,
                  "frac_of_peak": tf / PEAK[dt]})
        if len(dtypes) == 2:
            emit({"phase": "layers", "layer": name, "B": B, "bf16_speedup": float(np.median(times["f32"]) / np.median(times["bf16"]))})
        del x, w, y, packed
        torch.cuda.empty_cache()


def predict(B, calls, repeats, dtypes, bf16_cells):
    w = O.init_convlstm_seq2seq(1, C=C, latent_dim=16, head="conv2d")
    x0 = torch.rand((B, T, H, W, C), device="cuda")
    dec0 = x0[:, -1:].contiguous()
    kinds = {"f32": dict(dtype="f32"), "bf16": dict(dtype="bf16"), "bf16+cells": dict(dtype="bf16", cell_dtype="bf16")}
    heads = tuple(dtypes)
    dtypes = heads + (("bf16+cells",) if bf16_cells else ())
    models = {dt: ConvLSTMSeq2Seq(w, head="conv2d", **kinds[dt]) for dt in dtypes}
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
        emit({"phase": "predict", "dtype": dt, "B": B, "T_in": T, "T_out": T, "calls": calls, **s,
              "sequences_per_s": B / (s["median_ms"] * 1e-3), "head_tflop_per_call": head_flop / 1e12})
    if len(heads) == 2:
        a, b = out["f32"].cpu().numpy(), out["bf16"].cpu().numpy()
        emit({"phase": "predict", "B": B, "max_abs_diff_bf16_vs_f32": float(np.abs(a - b).max()),
              "bf16_speedup": float(np.median(times["f32"]) / np.median(times["bf16"]))})
        if bf16_cells:
            emit({"phase": "predict", "B": B,
                  "max_abs_diff_bf16_cells_vs_f32": float(np.abs(a - out["bf16+cells"].cpu().numpy()).max())})
    if bf16_cells:
        b, c = out["bf16"].cpu().numpy(), out["bf16+cells"].cpu().numpy()
        emit({"phase": "predict", "B": B, "max_abs_diff_bf16_cells_vs_bf16": float(np.abs(b - c).max()),
              "bf16_cells_speedup_over_bf16": float(np.median(times["bf16"]) / np.median(times["bf16+cells"])),
              "slowest_bf16_cells_ms": float(np.max(times["bf16+cells"])), "fastest_bf16_ms": float(np.min(times["bf16"])),
              "all_bf16_slowest_beats_fp32_cells_fastest": bool(np.max(times["bf16+cells"]) < np.min(times["bf16"]))})
    # the sixty cell launches of one predict call: the encoder's thirty and the decoder's thirty (on a fixed input map)
    dw = models[dtypes[-1]]._dw
    filters = (32, 16, 8)
    xe = torch.cat([x0, torch.zeros((B, T, H, W, 2), device="cuda")], -1)

    def cells(bf16):
        def cell(x, h, name, c, h_out):
            if bf16:
                ops.convlstm_cell_bf16(x, h, dw[name + "_KR"], dw[name + "_b"], c, h_out, "hard_sigmoid", packed=dw[name + "_P"])
            else:
                ops.convlstm_cell(x, h, dw[name + "_KR"], dw[name + "_b"], c, h_out, "hard_sigmoid")
        seq = [xe[:, t] for t in range(T)]
        states = []
        for l, F in enumerate(filters):
            h = torch.zeros((B, H, W, F), device="cuda")
            c = torch.zeros((B, H, W, F), device="cuda")
            nxt = []
            for t in range(T):
                hn = torch.empty((B, H, W, F), device="cuda")
                cell(seq[t], h, "enc%d" % l, c, hn)
                h = hn
                nxt.append(h)
            seq = nxt
            states.append([h, c])
        for t in range(T):
            feat = torch.empty((B, H, W, sum(filters)), device="cuda")
            cur, off = xe[:, -1], 0
            for l, F in enumerate(filters):
                hslot = feat[..., off:off + F]
                cell(cur, states[l][0], "dec%d" % l, states[l][1], hslot)
                states[l][0] = hslot
                cur = hslot
                off += F

    forms = (False, True) if bf16_cells else (False,)
    for bf16 in forms:
        cells(bf16)
    torch.cuda.synchronize()
    ct = {bf16: [] for bf16 in forms}
    for _ in range(repeats):
        for bf16 in forms:
            ct[bf16].append(event_ms(lambda bf16=bf16: cells(bf16), calls))
    emit({"phase": "predict", "part": "sixty fp32 cell launches", "B": B, **stats(ct[False])})
    if bf16_cells:
        emit({"phase": "predict", "part": "sixty bf16 cell launches", "B": B, **stats(ct[True])})


def cell_layers(B, reps, repeats):
    """fp32 cell against bf16 cell on the three cell shapes of configs[3], x a 32-channel map / a slot of the concat map."""
    for name, c, f in (("cell0 32+32 -> 128", 32, 32), ("cell1 32+16 -> 64", 32, 16), ("cell2 16+8 -> 32", 16, 8)):
        x = torch.rand((B, H, W, c), device="cuda")
        h = torch.rand((B, H, W, f), device="cuda") - 0.5
        cs = torch.rand((B, H, W, f), device="cuda") - 0.5
        w = (torch.rand((5, 5, c + f, 4 * f), device="cuda") - 0.5) * 0.1
        b = torch.zeros(4 * f, device="cuda")
        ho, cn = torch.empty((B, H, W, f), device="cuda"), torch.empty((B, H, W, f), device="cuda")
        packed = ops.convlstm_cell_pack_bf16(w)
        call = {"f32": lambda: ops.convlstm_cell(x, h, w, b, cs, ho, "hard_sigmoid", c_new=cn),
                "bf16": lambda: ops.convlstm_cell_bf16(x, h, w, b, cs, ho, "hard_sigmoid", c_new=cn, packed=packed)}
        for dt in call:
            call[dt]()
            call[dt]()
        torch.cuda.synchronize()
        times = {dt: [] for dt in call}
        for _ in range(repeats):
            for dt in call:
                times[dt].append(event_ms(call[dt], reps))
        flop = 2.0 * 25 * (c + f) * 4 * f * B * H * W
        gbytes = 4.0 * (c + 4 * f) * B * H * W / 1e9          # x, h_prev, c_prev in; c, h out
        for dt in call:
            s = stats(times[dt])
            tf = flop / s["median_ms"] / 1e9
            emit({"phase": "cells", "layer": name, "dtype": dt, "B": B, "launches": reps, **s, "tflops": tf,
                  "frac_of_peak": tf / PEAK[dt], "map_gbytes_per_s": gbytes / (s["median_ms"] * 1e-3),
                  "floor_ms_matrix_peak": flop / PEAK[dt] / 1e9, "floor_ms_map_traffic": gbytes / COPY_TBS})
        emit({"phase": "cells", "layer": name, "B": B, "bf16_speedup": float(np.median(times["f32"]) / np.median(times["bf16"]))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10, help="launches per timed region of a head layer")
    ap.add_argument("--calls", type=int, default=2, help="predict_device calls per timed region")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only-bf16", action="store_true", help="the bf16 model alone (a profiler run)")
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--no-predict", action="store_true")
    ap.add_argument("--no-cells", action="store_true", help="without the per-layer cell rows")
    ap.add_argument("--no-bf16-cells", action="store_true", help="without anything that runs a bf16 cell")
    ap.add_argument("--out", default=os.path.join("profiles", "convlstm_cell_bf16_time.jsonl"),
                    help="file the JSON lines of a run with bf16 cells also go to, written anew ('-': none)")
    a = ap.parse_args()
    global OUT
    if not a.no_bf16_cells and a.out != "-":
        OUT = a.out
        open(OUT, "w").close()
    dtypes = ("bf16",) if a.only_bf16 else ("f32", "bf16")
    if not a.no_layers:
        layers(a.batch, a.reps, a.repeats, dtypes)
    if not a.no_predict:
        predict(a.batch, a.calls, a.repeats, dtypes, not a.no_bf16_cells)
    if not a.no_cells and not a.no_bf16_cells:
        cell_layers(a.batch, a.reps, a.repeats)


if __name__ == "__main__":
    main()
