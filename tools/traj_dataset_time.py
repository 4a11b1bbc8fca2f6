"""What keeping the FoV tracks on the device is worth for the seq2seq LSTM models, at configs[2]'s shape (B 512, 34 users,
T 10 -> 10 and 30 -> 30): one video of 34 users, stride 1, just long enough for 544 windows.

Without --phase this is the driver: it runs the phases below one after the other, each as a child process of its own under
`timeout -k 10`, chained so that the first failure ends the run, and leaves their JSON lines in --out (default
profiles/traj_dataset_time.jsonl, written anew).  The driver itself never touches the GPU.  Inside a phase the legs
alternate in one process, --repeats times each, and a row reports median / min / max.

  batch    one TrajectoryDataset.batch of 512 windows (sample rows uploaded, one gather launch; wall clock to a device
           synchronise) against the same batch made on the host in the same process: slices of utility.get_data's arrays,
           get_gt_target_xyz / get_gt_target_xyz_oth of them (given_others...py:675-695) and four uploads.  What is paid
           once per dataset is reported apart: utility.get_data against TrajectoryDataset's construction.
  predict  OthersMixingSeq2Seq(latent_dim 256).predict_dataset against predict on the host arrays of the same windows,
           batch_size 512, NumPy out, wall clock.
  kernel   fov_window_inputs writing all five outputs of 512 windows, HIP events over --launches launches, alternated with
           one device copy of as many bytes as it writes; bytes moved (read + written) per second for both.

    python tools/traj_dataset_time.py [--batch 512] [--repeats 5] [--out FILE] [--phase batch|predict|kernel]
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

NUM_USER = 34
LENGTHS = (10, 30)
PHASES = (("batch", 420), ("predict", 300), ("kernel", 180))      # name, time limit of the child in seconds
OUT = None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "repeats": len(v)}


def wall_ms(torch, fn):
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(torch, fn, calls):
    gc.collect()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / calls


def datadb(T, B):
    """One video of NUM_USER users, the fewest whole seconds that give at least B windows at stride 1."""
    windows = -(-B // NUM_USER)
    S = windows + 2 * T - 1
    v = np.random.default_rng(T).standard_normal((NUM_USER, S * 30, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    return {"video": {"x": v[..., 0].copy(), "y": v[..., 1].copy(), "z": v[..., 2].copy()}}


def setup(T):
    from longterm360fov_amd.config import cfg
    cfg.running_length = cfg.predict_step = T
    cfg.data_chunk_stride = 1


def host_batch(arrays, lo, hi):
    """The mixing model's inputs and target of windows lo .. hi-1 as the reference's test loop makes them, float32."""
    from longterm360fov_amd import utility as U
    enc, fut, oth_fut = arrays[0][lo:hi], arrays[1][lo:hi], arrays[4][:, lo:hi]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return [f32(enc), f32(U.get_gt_target_xyz_oth(U.reshape_others_data(oth_fut))), f32(U.get_gt_target_xyz(enc[:, -1:]))], \
        f32(U.get_gt_target_xyz(fut))


def batch(B, repeats, launches):
    import torch
    from longterm360fov_amd import utility as U
    from longterm360fov_amd.trajectories import TrajectoryDataset
    for T in LENGTHS:
        setup(T)
        db = datadb(T, B)
        once = {"utility.get_data": [], "TrajectoryDataset": []}
        for _ in range(repeats):
            t0 = time.perf_counter()
            arrays = U.get_data(db, pick_user=True, num_user=NUM_USER)
            once["utility.get_data"].append((time.perf_counter() - t0) * 1e3)
            once["TrajectoryDataset"].append(wall_ms(torch, lambda: TrajectoryDataset(db, True, num_user=NUM_USER)))
        ds = TrajectoryDataset(db, True, num_user=NUM_USER)
        index = np.arange(B)
        up = lambda a: torch.from_numpy(a).cuda()

        def host_leg():
            x, y = host_batch(arrays, 0, B)
            return [up(a) for a in x] + [up(y)]

        legs = {"ds.batch": lambda: ds.batch(index), "host slices + helpers + upload": host_leg}
        got, ref = legs["ds.batch"](), legs["host slices + helpers + upload"]()
        worst = max(float((a - b).abs().max()) for a, b in zip((got["enc"], got["others"], got["dec_in"], got["target"]), ref))
        times = {k: [] for k in legs}
        for _ in range(repeats):
            for k, fn in legs.items():
                times[k].append(wall_ms(torch, fn))
        for k in once:
            emit({"phase": "batch", "T": T, "paid": "once per dataset", "call": k, "windows": len(ds), "num_user": NUM_USER,
                  "host_mbytes": sum(a.nbytes for a in arrays) / 1e6 if k == "utility.get_data" else ds.tables()["secs"].nbytes / 1e6,
                  **stats(once[k])})
        for k in legs:
            emit({"phase": "batch", "T": T, "paid": "per batch", "call": k, "B": B, "num_user": NUM_USER, **stats(times[k])})
        emit({"phase": "batch", "T": T, "B": B, "max_abs_difference_device_vs_host_batch": worst,
              "median_host_over_device": float(np.median(times["host slices + helpers + upload"]) / np.median(times["ds.batch"])),
              "slowest_device_beats_fastest_host": bool(np.max(times["ds.batch"]) < np.min(times["host slices + helpers + upload"]))})
        del arrays, ds, got, ref
        gc.collect()
        torch.cuda.empty_cache()


def predict(B, repeats, launches):
    import torch
    from longterm360fov_amd import utility as U
    from longterm360fov_amd.models import OthersMixingSeq2Seq
    from longterm360fov_amd.trajectories import TrajectoryDataset
    for T in LENGTHS:
        setup(T)
        db = datadb(T, B)
        ds = TrajectoryDataset(db, True, num_user=NUM_USER)
        arrays = U.get_data(db, pick_user=True, num_user=NUM_USER)
        x, _ = host_batch(arrays, 0, len(ds))
        del arrays
        m = OthersMixingSeq2Seq(latent_dim=256, num_user=NUM_USER, seed=1)
        legs = {"predict_dataset": lambda: m.predict_dataset(ds, batch_size=B), "predict on host arrays": lambda: m.predict(x, batch_size=B)}
        res = {k: fn() for k, fn in legs.items()}                      # warm-up
        times = {k: [] for k in legs}
        for _ in range(repeats):
            for k, fn in legs.items():
                times[k].append(wall_ms(torch, fn))
        for k in legs:
            emit({"phase": "predict", "T": T, "call": k, "windows": len(ds), "batch_size": B, "num_user": NUM_USER, "latent_dim": 256,
                  **stats(times[k])})
        emit({"phase": "predict", "T": T, "max_abs_difference": float(np.abs(res["predict_dataset"] - res["predict on host arrays"]).max()),
              "median_saving_ms": float(np.median(times["predict on host arrays"]) - np.median(times["predict_dataset"])),
              "slowest_dataset_beats_fastest_host": bool(np.max(times["predict_dataset"]) < np.min(times["predict on host arrays"]))})
        del m, ds, x
        gc.collect()
        torch.cuda.empty_cache()


def kernel(B, repeats, launches):
    import torch
    from longterm360fov_amd import ops
    from longterm360fov_amd.trajectories import TrajectoryDataset
    for T in LENGTHS:
        setup(T)
        ds = TrajectoryDataset(datadb(T, B), True, num_user=NUM_USER)
        d = ds._dev
        sample = d["sample"][:B].contiguous()
        gather = lambda: ops.window_inputs(d["secs"], d["feat"], sample, d["others_base"], T, T, ds.fut_offset,
                                           outputs=ops.WINDOW_INPUT_NAMES)
        written = sum(t.numel() * 4 for t in gather().values())
        src = torch.randn(written // 4, device="cuda")
        dst = torch.empty_like(src)
        legs = {"fov_window_inputs, five outputs": gather, "device copy of the bytes it writes": lambda: dst.copy_(src)}
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(repeats):
            for k, fn in legs.items():
                times[k].append(event_ms(torch, fn, launches))
        for k in legs:
            s = stats(times[k])
            emit({"phase": "kernel", "T": T, "B": B, "num_user": NUM_USER, "call": k, "launches": launches, **s,
                  "mbytes_written": written / 1e6, "tbytes_moved_per_s": 2 * written / (s["median_ms"] * 1e-3) / 1e12,
                  "note": "the gather's time includes its five torch.empty calls and the ctypes call" if "fov" in k else
                          "Tensor.copy_ into an existing tensor"})
        emit({"phase": "kernel", "T": T, "gather_median_over_copy_median": float(
            np.median(times["fov_window_inputs, five outputs"]) / np.median(times["device copy of the bytes it writes"]))})
        del ds, src, dst
        gc.collect()
        torch.cuda.empty_cache()


def drive(a):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").close()
    for name, limit in PHASES:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--phase", name, "--batch", str(a.batch),
               "--repeats", str(a.repeats), "--launches", str(a.launches), "--out", a.out]
        print("+ " + " ".join(cmd), flush=True)
        code = subprocess.call(cmd, cwd=ROOT)
        if code != 0:       # a fault, an abort or a time limit: nothing more is started on the GPU
            print("phase %s ended with status %d: stopping" % (name, code), flush=True)
            return code
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200, help="launches per timed window of the kernel phase")
    ap.add_argument("--out", default=os.path.join("profiles", "traj_dataset_time.jsonl"))
    ap.add_argument("--phase", choices=[p for p, _ in PHASES], help="run one phase in this process (what the driver starts)")
    a = ap.parse_args()
    if a.phase is None:
        sys.exit(drive(a))
    global OUT
    OUT = a.out
    {"batch": batch, "predict": predict, "kernel": kernel}[a.phase](a.batch, a.repeats, a.launches)


if __name__ == "__main__":
    main()
