"""What decoding the heat-map model's predictions on the device is worth, at configs[3]'s shape (B 256, T 10 -> 10,
36 x 18 x 30), for the fp32 model and the bf16-head model.

Without --phase this is the driver: it runs the phases below one after the other, each as a child process of its own under
`timeout -k 10`, chained so that the first failure ends the run, and leaves their JSON lines in --out (default
profiles/heatmap_decode_time.jsonl, written anew).  The driver itself never touches the GPU.  Inside a phase the legs
alternate in one process, --repeats times each, and a row reports median / min / max.

  end2end  ConvLSTMSeq2Seq.predict_trajectories, host xyz in, NumPy out, wall clock around the call: output 'maps' (the
           code path before the decode existed: the yardstick) against 'index' and 'xyz'.
  device   predict_index_device against predict_device on device-resident 32-channel maps, HIP events.
  kernel   fov_heatmap_argmax on one step's softmax output (256 maps) alternated with fov_softmax_lastdim on the same
           tensor, and one call on all 2 560 maps of a predict call; bytes read per second against the 6.29 TB/s copy rate.

    python tools/heatmap_decode_time.py [--batch 256] [--repeats 5] [--out FILE] [--phase end2end|device|kernel]
"""
import argparse
import gc
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, C, T = 36, 18, 30, 10
COPY_TBS = 6.29                             # measured device copy rate, TB/s
PHASES = (("end2end", 420), ("device", 300), ("kernel", 180))      # name, time limit of the child in seconds
OUT = None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


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


def wall_ms(torch, fn):
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()                                    # ends in NumPy arrays: the copy to the host has synchronised
    return (time.perf_counter() - t0) * 1e3


def unit_xyz(seed, *lead):
    v = np.random.default_rng(seed).standard_normal(lead + (30, 3))
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def models():
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    from oracle import fov_oracle as O
    w = O.init_convlstm_seq2seq(1, C=C, latent_dim=16, head="conv2d")
    return {"f32": ConvLSTMSeq2Seq(w, head="conv2d"), "bf16": ConvLSTMSeq2Seq(w, head="conv2d", dtype="bf16")}


def end2end(B, repeats):
    import torch
    enc = unit_xyz(1, B, T)
    dec = enc[:, -1:]
    for dt, m in models().items():
        legs = ("maps", "index", "xyz")
        res = {o: m.predict_trajectories(enc, dec, predict_step=T, output=o) for o in legs}      # warm-up
        same = bool((res["index"] == np.argmax(res["maps"].reshape(B, T, -1, C), axis=-2)).all())
        times = {o: [] for o in legs}
        for _ in range(repeats):
            for o in legs:
                times[o].append(wall_ms(torch, lambda o=o: m.predict_trajectories(enc, dec, predict_step=T, output=o)))
        for o in legs:
            emit({"phase": "end2end", "dtype": dt, "output": o, "B": B, "T_out": T, "result_mbytes": res[o].nbytes / 1e6,
                  **stats(times[o])})
        emit({"phase": "end2end", "dtype": dt, "B": B, "index_equals_numpy_argmax_of_maps": same,
              "median_saving_ms_index_vs_maps": float(np.median(times["maps"]) - np.median(times["index"])),
              "slowest_index_ms": float(np.max(times["index"])), "fastest_maps_ms": float(np.min(times["maps"])),
              "slowest_index_beats_fastest_maps": bool(np.max(times["index"]) < np.min(times["maps"])),
              "slowest_xyz_beats_fastest_maps": bool(np.max(times["xyz"]) < np.min(times["maps"]))})
        del res, m
        gc.collect()
        torch.cuda.empty_cache()


def device(B, repeats, calls=2):
    import torch
    from longterm360fov_amd import ops
    enc = torch.from_numpy(unit_xyz(1, B, T)).cuda()
    e32, d32 = ops.one_hot_maps(enc, channels=32), ops.one_hot_maps(enc[:, -1:], channels=32)
    for dt, m in models().items():
        legs = {"predict_device": lambda: m.predict_device(e32, d32, T),
                "predict_index_device": lambda: m.predict_index_device(e32, d32, T)}
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(repeats):
            for k, fn in legs.items():
                times[k].append(event_ms(torch, fn, calls))
        for k in legs:
            emit({"phase": "device", "dtype": dt, "call": k, "B": B, "T_out": T, "calls": calls, **stats(times[k])})
        emit({"phase": "device", "dtype": dt, "B": B,
              "median_index_minus_maps_ms": float(np.median(times["predict_index_device"]) - np.median(times["predict_device"])),
              "maps_spread_ms": float(np.max(times["predict_device"]) - np.min(times["predict_device"]))})
        del m
        gc.collect()
        torch.cuda.empty_cache()


def kernel(B, repeats, reps=50):
    import torch
    from longterm360fov_amd import ops
    x = torch.randn((B, H, W, C), device="cuda")
    y = ops.softmax_lastdim(x)
    y2 = torch.empty_like(y)
    index = torch.empty((B, C), dtype=torch.int32, device="cuda")
    allmaps = ops.softmax_lastdim(torch.randn((B, T, H, W, C), device="cuda"))
    allindex = torch.empty((B, T, C), dtype=torch.int32, device="cuda")
    legs = {"heatmap_argmax, one step (%d maps)" % B: (lambda: ops.heatmap_argmax(y, out=index), y.numel() * 4),
            "softmax_lastdim, same tensor": (lambda: ops.softmax_lastdim(y, out=y2), 2 * y.numel() * 4),
            "heatmap_argmax, all steps (%d maps)" % (B * T): (lambda: ops.heatmap_argmax(allmaps, out=allindex), allmaps.numel() * 4)}
    for fn, _ in legs.values():
        fn()
        fn()
    torch.cuda.synchronize()
    assert (index.cpu().numpy() == np.argmax(y.cpu().numpy().reshape(B, -1, C), axis=1)).all()
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, (fn, _) in legs.items():
            times[k].append(event_ms(torch, fn, reps))
    for k, (_, nbytes) in legs.items():
        s = stats(times[k])
        tbs = nbytes / (s["median_ms"] * 1e-3) / 1e12
        emit({"phase": "kernel", "call": k, "launches": reps, **s, "mbytes_moved": nbytes / 1e6, "tbytes_per_s": tbs,
              "frac_of_copy_rate": tbs / COPY_TBS})
    a, s_ = times["heatmap_argmax, one step (%d maps)" % B], times["softmax_lastdim, same tensor"]
    emit({"phase": "kernel", "argmax_median_over_softmax_median": float(np.median(a) / np.median(s_)),
          "slowest_argmax_not_above_fastest_softmax": bool(np.max(a) <= np.min(s_))})


def drive(a):
    open(a.out, "w").close()
    for name, limit in PHASES:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--phase", name, "--batch", str(a.batch),
               "--repeats", str(a.repeats), "--out", a.out]
        print("+ " + " ".join(cmd), flush=True)
        code = subprocess.call(cmd, cwd=ROOT)
        if code != 0:       # a fault, an abort or a time limit: nothing more is started on the GPU
            print("phase %s ended with status %d: stopping" % (name, code), flush=True)
            return code
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "heatmap_decode_time.jsonl"))
    ap.add_argument("--phase", choices=[p for p, _ in PHASES], help="run one phase in this process (what the driver starts)")
    a = ap.parse_args()
    if a.phase is None:
        sys.exit(drive(a))
    global OUT
    OUT = a.out
    {"end2end": end2end, "device": device, "kernel": kernel}[a.phase](a.batch, a.repeats)


if __name__ == "__main__":
    main()
