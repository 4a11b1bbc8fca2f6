#!/usr/bin/env python3
"""Measures the one-hot heat-map inputs of BASELINE.json configs[3] (ConvLSTM seq2seq on 36x18x30 maps, B = 256, T 10 -> 10).

--mode kernel   launches fov_onehot_maps on the configs[3] encoder maps (256 x 10 slabs of 648 x 32 fp32, 212 MB written;
                also the 30-channel and the index-input forms) --iters times each, cycling over --buffers output buffers
                (1: the same 212 MB rewritten, resident in the 256 MiB Infinity Cache; 3: a 636 MB footprint, the HBM
                write rate).  Run it under
                `rocprofv3 --kernel-trace --stats`, then `--stats <..._kernel_stats.csv>` turns the kernel times into write
                bandwidth.
--mode predict  times, with the profiler off and the forms alternated, at B = 256:
                  predict_device        maps resident in HBM (the bench's form; 30 channels, padded inside)
                  xyz_device            xyz resident -> one_hot_maps(channels=32) -> predict_device (device tensor out)
                  predict_trajectories  host xyz in, NumPy out
                  predict               host maps in (built beforehand), NumPy out
                  host_maps             utility.theta_phi_index_for_onehot + create_one_hot + transpose on the host
Writes JSON to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, T, FR = 256, 10, 30
SLAB = 36 * 18


def _xyz(rng, shape):
    v = rng.standard_normal(shape + (3,))
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def kernel_mode(a):
    import torch
    from longterm360fov_amd import ops, utility
    host = _xyz(np.random.default_rng(0), (B, T, FR))
    xyz = torch.from_numpy(host).cuda()
    # indices from the host mirror: an index-only launch would join the 30-channel kernel's statistics
    ti, pi = (torch.from_numpy(a.astype(np.int32)).cuda() for a in utility.theta_phi_index_for_onehot(host))
    outs = {C: [torch.empty((B, T, 36, 18, C), device="cuda") for _ in range(a.buffers)] for C in (30, 32)}
    forms = [("xyz_c32", xyz, 32), ("xyz_c30", xyz, 30), ("index_c32", (ti, pi), 32)]
    res = {}
    for name, src, C in forms:
        for i in range(3):
            ops.one_hot_maps(src, channels=C, out=outs[C][i % a.buffers])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.iters):
            ops.one_hot_maps(src, channels=C, out=outs[C][i % a.buffers])      # each call reads the status word back
        torch.cuda.synchronize()
        res[name] = {"call_us": 1e6 * (time.perf_counter() - t0) / a.iters, "bytes_written": B * T * SLAB * C * 4,
                     "buffers": a.buffers}
        print(name, res[name])
    return res


def predict_mode(a):
    import torch
    from longterm360fov_amd import ops, utility
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    from oracle import fov_oracle as O       # Keras initialisers only
    w = O.init_convlstm_seq2seq(1234, C=30, latent_dim=16, k=5, head="conv2d")
    m = ConvLSTMSeq2Seq(w, head="conv2d")
    rng = np.random.default_rng(1)
    enc_xyz = _xyz(rng, (B, T, FR))
    dec_xyz = enc_xyz[:, -1:]

    def host_maps(x):
        ti, pi = utility.theta_phi_index_for_onehot(x)
        return np.ascontiguousarray(utility.create_one_hot(ti, pi).transpose(0, 1, 3, 4, 2), dtype=np.float32)

    t0 = time.perf_counter()
    enc_maps, dec_maps = host_maps(enc_xyz), host_maps(dec_xyz)
    host_ms = 1e3 * (time.perf_counter() - t0)
    enc_d, dec_d = torch.from_numpy(enc_maps).cuda(), torch.from_numpy(dec_maps).cuda()
    enc_x, dec_x = torch.from_numpy(enc_xyz).cuda(), torch.from_numpy(dec_xyz).cuda()

    def sync(f):
        def run():
            f()
            torch.cuda.synchronize()
        return run

    forms = {
        "predict_device": sync(lambda: m.predict_device(enc_d, dec_d, T)),
        "xyz_device": sync(lambda: m.predict_device(ops.one_hot_maps(enc_x, channels=32), ops.one_hot_maps(dec_x, channels=32), T)),
        "predict_trajectories": lambda: m.predict_trajectories(enc_xyz, dec_xyz, predict_step=T),
        "predict": lambda: m.predict([enc_maps, dec_maps], predict_step=T),
    }
    ref = m.predict_device(enc_d, dec_d, T).cpu().numpy()
    assert np.array_equal(m.predict_trajectories(enc_xyz, dec_xyz, predict_step=T), ref), "trajectory path differs"
    for f in forms.values():        # warm-up of every shape
        f()
    times = {k: [] for k in forms}
    for _ in range(a.repeats):       # alternate the forms: drift of the shared host hits all of them alike
        for k, f in forms.items():
            t0 = time.perf_counter()
            f()
            times[k].append(1e3 * (time.perf_counter() - t0))
    res = {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))} for k, v in times.items()}
    res["host_maps"] = {"ms": host_ms, "note": "vectorised NumPy mirror, once; the reference's triple loop is slower"}
    for k, v in res.items():
        print(k, v)
    return res


def stats_mode(path):
    import csv
    bytes_by = {"onehot_maps_kernel<32>": B * T * SLAB * 32 * 4, "onehot_maps_kernel<30>": B * T * SLAB * 30 * 4}
    res = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for key, nbytes in bytes_by.items():
                if key in name:
                    avg_ns = float(row["AverageNs"])
                    res[name] = {"calls": int(row["Calls"]), "avg_us": avg_ns / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                                 "max_us": float(row["MaxNs"]) / 1e3, "write_TBps": nbytes / avg_ns / 1e3}
    for k, v in res.items():
        print(k, v)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("kernel", "predict"), default="kernel")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--buffers", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stats", help="a rocprofv3 kernel_stats.csv: report kernel time and write bandwidth, no GPU needed")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.stats is not None:
        res = stats_mode(a.stats)
    else:
        import torch
        assert torch.cuda.is_available(), "onehot_probe measures on the GPU"
        res = kernel_mode(a) if a.mode == "kernel" else predict_mode(a)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
