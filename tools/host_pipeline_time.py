"""What the staging ring (longterm360fov_amd/hostpipe.py) is worth: the models' own predict / evaluate / fit on
host arrays, wall clock around the call ending in a device synchronise, in three legs -

  parent  a checkout of the parent commit (--parent DIR, with the built library copied in): the serial loop as it was
  off     this tree with model.host_pipeline = False: must be the parent within the parent's own spread
  on      this tree with model.host_pipeline = True

Without --leg this is the driver: it never touches the GPU, runs one child process per leg and round under `timeout -k 10`,
the legs alternating for --rounds rounds, then one `parts` child, stops at the first failure, and writes the children's JSON
lines and its own summary rows (median / min / max per leg, the default-on verdict per shape) to --out, written anew.

A child times every shape once, after a warm-up call; the first pipelined call (which allocates the ring) is reported on its
own as first_call_ms.  Shapes (--scale 1; a smaller scale divides the row counts, for rehearsal):
  s2s         Seq2SeqLSTM H 256, F 90, T 30 -> 30, 64 chunks of 1024 rows; float32 / float64 inputs, dtype f32 / bf16
  mixing      OthersMixingSeq2Seq H 256, 34 users, T 30 -> 30, 64 chunks of 512, float64 inputs (utility.get_data's)
  convlstm    ConvLSTMSeq2Seq on 36 x 18 x 30 maps, T 10 -> 10, 8 chunks of 32: predict (maps back) and predict_index
  evaluate    the s2s model on 64 chunks of 1024
  fit         the s2s model with FOV_FIT_RESIDENT_BYTES=0, one epoch: 256 steps of 32 rows, 32 steps of 1024
The `parts` child measures, per chunk of each predict shape and each alone: the host's narrowing into pinned memory, the
upload, the kernels on resident inputs with nothing copied back, the download - the pipelined chunk can at best take the
largest of the four - and, for the narrowing choice, a float64 chunk copied to pinned float64, uploaded and narrowed by
tensor.to(float32) on the device.

    python tools/host_pipeline_time.py --parent DIR [--rounds 5] [--scale 1] [--out FILE] [--only s2s,fit]
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
LIMIT = {"parent": 240, "off": 240, "on": 240, "parts": 300}      # a child's time limit in seconds
GROUPS = ("s2s", "mixing", "convlstm", "evaluate", "fit")


def stats(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "n": len(v)}


def uniform(seed, shape, dtype):
    a = np.random.default_rng(seed).random(shape, dtype=np.float32)
    a -= 0.5
    return a.astype(dtype) if dtype != np.float32 else a


def wall_ms(torch, fn):
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def cases(models, scale, only):
    """(name, chunks, make) - make() -> (model, fn): fn() is the timed call."""
    def s2s(dtype, in_dtype):
        def make():
            n = 64 * 1024 // scale
            m = models.Seq2SeqLSTM(num_encoder_tokens=90, latent_dim=256, seed=1, dtype=dtype)
            x = [uniform(1, (n, 30, 90), in_dtype), uniform(2, (n, 30, 6), in_dtype)]
            return m, lambda: m.predict(x, batch_size=1024)
        return make

    def mixing():
        n = 64 * 512 // scale
        m = models.OthersMixingSeq2Seq(num_encoder_tokens=90, latent_dim=256, num_user=34, seed=2)
        x = [uniform(3, (n, 30, 90), np.float64), uniform(4, (n, 30, 33, 6), np.float64), uniform(5, (n, 1, 6), np.float64)]
        return m, lambda: m.predict(x, batch_size=512)

    def convlstm(method):
        def make():
            from oracle import fov_oracle as O
            n = max(8 * 32 // scale, 64)
            w = O.init_convlstm_seq2seq(1, C=30, latent_dim=16, head="conv2d")
            m = models.ConvLSTMSeq2Seq(w, head="conv2d")
            maps = np.zeros((n, 10, 36, 18, 30), np.float32)
            maps.reshape(n * 10, 648, 30)[np.arange(n * 10)[:, None], np.random.default_rng(6).integers(0, 648, (n * 10, 30)), np.arange(30)] = 1
            x = [maps, maps[:, -1:]]
            return m, lambda: getattr(m, method)(x, batch_size=32, predict_step=10)
        return make

    def trained(n):
        m = models.Seq2SeqLSTM(num_encoder_tokens=90, latent_dim=256, seed=1)
        m.compile(optimizer="Adam", loss="mean_squared_error")
        return m, [uniform(1, (n, 30, 90), np.float32), uniform(2, (n, 30, 6), np.float32)], uniform(7, (n, 30, 6), np.float32)

    def evaluate():
        m, x, y = trained(64 * 1024 // scale)
        return m, lambda: m.evaluate(x, y, batch_size=1024)

    def fit(batch, steps):
        def make():
            m, x, y = trained(batch * max(steps // scale, 4))
            os.environ["FOV_FIT_RESIDENT_BYTES"] = "0"
            return m, lambda: m.fit(x, y, batch_size=batch, epochs=1, shuffle=True, verbose=0)
        return make

    table = [("s2s", "s2s f32 model, float32 in", 64, s2s("f32", np.float32)), ("s2s", "s2s f32 model, float64 in", 64, s2s("f32", np.float64)),
             ("s2s", "s2s bf16 model, float32 in", 64, s2s("bf16", np.float32)), ("s2s", "s2s bf16 model, float64 in", 64, s2s("bf16", np.float64)),
             ("mixing", "mixing 34 users, float64 in", 64, mixing),
             ("convlstm", "convlstm predict", 8, convlstm("predict")), ("convlstm", "convlstm predict_index", 8, convlstm("predict_index")),
             ("evaluate", "evaluate s2s", 64, evaluate), ("fit", "fit batch 32", 256, fit(32, 256)), ("fit", "fit batch 1024", 32, fit(1024, 32))]
    return [(name, chunks, make) for group, name, chunks, make in table if group in only]


def leg(args, emit):
    root = args.parent if args.leg == "parent" else ROOT
    sys.path.insert(0, root)
    import torch
    from longterm360fov_amd import models
    assert os.path.dirname(os.path.dirname(os.path.abspath(models.__file__))) == os.path.abspath(root)
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    for name, chunks, make in cases(models, args.scale, args.only):
        os.environ.pop("FOV_FIT_RESIDENT_BYTES", None)
        m, fn = make()
        m.host_pipeline = False
        wall_ms(torch, fn)                       # code objects, workspaces, the trainer
        m.host_pipeline = args.leg == "on"
        first = wall_ms(torch, fn)               # leg on: allocates the ring
        ms = wall_ms(torch, fn)
        emit({"leg": args.leg, "round": args.round, "case": name, "chunks": chunks, "ms": ms, "first_call_ms": first,
              "ms_per_chunk": ms / chunks})
        del m, fn
        gc.collect()


def parts(args, emit):
    """Per chunk, each alone: narrowing into pinned, upload, kernels on resident inputs, download."""
    sys.path.insert(0, ROOT)
    import torch
    from longterm360fov_amd import hostpipe, models
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    reps = 7

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def host(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def measure(name, run, chunk, out_of):
        """chunk: the host arrays of one chunk; run(*device inputs) -> result(s)."""
        pinned = [torch.empty(a.shape, dtype=torch.float32, pin_memory=True) for a in chunk]
        dev = [torch.empty(a.shape, dtype=torch.float32, device="cuda") for a in chunk]
        views = [p.numpy() for p in pinned]
        narrow = lambda: [hostpipe.narrow(v, a) for v, a in zip(views, chunk)]
        upload = lambda: [d.copy_(p, non_blocking=True) for d, p in zip(dev, pinned)]
        narrow(), upload(), run(*dev)
        o = out_of(run(*dev))
        back = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in o]
        download = lambda: [b.copy_(t, non_blocking=True) for b, t in zip(back, o)]
        row = {"leg": "parts", "case": name, "in_bytes_f32": sum(4 * a.size for a in chunk), "in_dtype": str(chunk[0].dtype),
               "out_bytes": sum(t.numel() * t.element_size() for t in o),
               "narrow_ms": stats([host(narrow) for _ in range(reps)]), "upload_ms": stats([events(upload) for _ in range(reps)]),
               "compute_ms": stats([events(lambda: run(*dev)) for _ in range(reps)]),
               "download_ms": stats([events(download) for _ in range(reps)]),
               "serial_upload_ms": stats([host(lambda: [torch.from_numpy(models._as_f32(a)).to("cuda") for a in chunk]) for _ in range(reps)]),
               "serial_download_ms": stats([host(lambda: [t.cpu().numpy() for t in o]) for _ in range(reps)])}
        row["largest_part_ms"] = max(row[k]["median_ms"] for k in ("narrow_ms", "upload_ms", "compute_ms", "download_ms"))
        if chunk[0].dtype == np.float64:      # the other narrowing: pinned float64, upload, tensor.to(float32) on the device
            p64 = [torch.empty(a.shape, dtype=torch.float64, pin_memory=True) for a in chunk]
            v64 = [p.numpy() for p in p64]
            d64 = [torch.empty(a.shape, dtype=torch.float64, device="cuda") for a in chunk]
            stage = lambda: [np.copyto(v, a) for v, a in zip(v64, chunk)]
            cast = lambda: [d.copy_(p, non_blocking=True).to(torch.float32) for d, p in zip(d64, p64)]
            stage(), cast()
            row["device_narrowing"] = {"host_copy_to_pinned_f64_ms": stats([host(stage) for _ in range(reps)]),
                                       "upload_f64_and_cast_ms": stats([events(cast) for _ in range(reps)])}
        emit(row)

    one = lambda o: [o]
    if "s2s" in args.only:
        for dtype in ("f32", "bf16"):
            m = models.Seq2SeqLSTM(num_encoder_tokens=90, latent_dim=256, seed=1, dtype=dtype)
            m._device_weights()
            for in_dtype in (np.float32, np.float64):
                measure("s2s %s model, %s in" % (dtype, np.dtype(in_dtype).name), m.predict_device,
                        [uniform(1, (1024, 30, 90), in_dtype), uniform(2, (1024, 30, 6), in_dtype)], one)
    if "mixing" in args.only:
        m = models.OthersMixingSeq2Seq(num_encoder_tokens=90, latent_dim=256, num_user=34, seed=2)
        m._device_weights()
        measure("mixing 34 users, float64 in", m.predict_device,
                [uniform(3, (512, 30, 90), np.float64), uniform(4, (512, 30, 33, 6), np.float64), uniform(5, (512, 1, 6), np.float64)], one)
    if "convlstm" in args.only:
        from oracle import fov_oracle as O
        m = models.ConvLSTMSeq2Seq(O.init_convlstm_seq2seq(1, C=30, latent_dim=16, head="conv2d"), head="conv2d")
        maps = np.zeros((32, 10, 36, 18, 30), np.float32)
        maps.reshape(320, 648, 30)[np.arange(320)[:, None], np.random.default_rng(6).integers(0, 648, (320, 30)), np.arange(30)] = 1
        measure("convlstm predict", lambda e, d: m.predict_device(e, d, 10), [maps, maps[:, -1:].copy()], one)
        measure("convlstm predict_index", lambda e, d: m.predict_index_device(e, d, 10), [maps, maps[:, -1:].copy()], one)


def drive(args):
    open(args.out, "w").close()

    def child(name, rnd):
        cmd = ["timeout", "-k", "10", str(LIMIT[name]), sys.executable, os.path.abspath(__file__), "--leg", name, "--round", str(rnd),
               "--scale", str(args.scale), "--only", ",".join(args.only), "--parent", args.parent, "--out", args.out]
        print("+ " + " ".join(cmd), flush=True)
        rc = subprocess.call(cmd, cwd=args.parent if name == "parent" else ROOT)
        if rc != 0:
            sys.exit("%s (round %d) ended with status %d: nothing more is started" % (name, rnd, rc))
    order = ("parent", "off", "on")
    for rnd in range(args.rounds):
        for name in order[rnd % 3:] + order[:rnd % 3]:      # no leg always runs first
            child(name, rnd)
    child("parts", 0)
    summarise(args)


def summarise(args):
    """Median / min / max per leg and the verdict per shape from the children's rows in --out, appended to it."""
    order = ("parent", "off", "on")
    with open(args.out) as f:
        rows = [r for r in map(json.loads, f) if "leg" in r]
    part = {r["case"]: r for r in rows if r["leg"] == "parts"}
    all_beat = True
    with open(args.out, "a") as f:
        for case in dict.fromkeys(r["case"] for r in rows if r["leg"] != "parts"):
            ms = {name: [r["ms"] for r in rows if r["leg"] == name and r["case"] == case] for name in order}
            chunks = next(r["chunks"] for r in rows if r.get("case") == case and r["leg"] == "on")
            row = {"summary": case, "chunks": chunks, **{name: stats(ms[name]) for name in order},
                   "first_pipelined_call_ms": stats([r["first_call_ms"] for r in rows if r["leg"] == "on" and r["case"] == case]),
                   "slowest_on_beats_fastest_parent": max(ms["on"]) < min(ms["parent"]),
                   "off_median_inside_parent_spread": min(ms["parent"]) <= float(np.median(ms["off"])) <= max(ms["parent"]),
                   "on_ms_per_chunk": float(np.median(ms["on"])) / chunks}
            if case in part:
                row["largest_part_ms"] = part[case]["largest_part_ms"]
                row["resident_ms_per_chunk"] = part[case]["compute_ms"]["median_ms"]
            all_beat = all_beat and row["slowest_on_beats_fastest_parent"]
            f.write(json.dumps(row) + "\n")
            print(json.dumps(row), flush=True)
        verdict = {"verdict": "host_pipeline = None means ON" if all_beat else "host_pipeline = None means OFF",
                   "rule": "on only if the slowest pipelined round beats the fastest parent round at every timed shape"}
        f.write(json.dumps(verdict) + "\n")
        print(json.dumps(verdict), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("parent", "off", "on", "parts"))
    ap.add_argument("--round", type=int, default=0)
    ap.add_argument("--summarise", action="store_true", help="only append the summary rows to the children's rows in --out")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--only", default=",".join(GROUPS))
    ap.add_argument("--parent", default=os.path.join(ROOT, "build", "parent"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "host_pipeline_time.jsonl"))
    args = ap.parse_args()
    args.only = [g for g in args.only.split(",") if g]
    args.parent, args.out = os.path.abspath(args.parent), os.path.abspath(args.out)
    if args.summarise:
        return summarise(args)
    if args.leg is None:
        if not os.path.isdir(os.path.join(args.parent, "longterm360fov_amd")):
            sys.exit("--parent %s holds no checkout of the parent commit" % args.parent)
        return drive(args)

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    (parts if args.leg == "parts" else leg)(args, emit)


if __name__ == "__main__":
    main()
