"""What the Keras 'accuracy' metric costs: the kernel against a device copy of the same bytes, and a fit step with the metric
against one without.

Without --phase this is the driver: it runs the phases below one after the other, each as a child process of its own under
`timeout -k 10`, chained so that the first failure ends the run, and leaves their JSON lines in --out (default
profiles/accuracy_metric_time.jsonl, written anew).  The driver itself never touches the GPU.  Inside a phase the legs
alternate in one process, --repeats times each, and a row reports median / min / max.

  kernel   fov_categorical_accuracy at the heat-map shape (2 560 maps x 648 rows x 30 channels, the prediction time-major,
           the target batch-major) and at 320 rows x 6, alternated with a torch device-to-device copy of the same number of
           bytes (what the kernel reads: both operands; the copy also writes them, its rate counts both directions); the
           ratio of the two rates and of the two times.
  step     trainer.train_step of config 1's model (Seq2SeqLSTM, H 128, batch 32, T 10 -> 10) and of the heat-map model at
           B 32 (36 x 18 x 30, T 10 -> 10, head 512 -> 1024 -> 30), compiled with metrics=None and with metrics=['accuracy'],
           alternated; the extra time per step.  --label names the commit the rows belong to: run the phase from a checkout of
           the parent commit with --label parent --cases off to get the third leg (the switch is off there: it must agree
           with this commit's metrics=None within the repeat spread).

    python tools/accuracy_metric_time.py [--repeats 5] [--out FILE] [--phase kernel|step] [--label this] [--cases off,on]
"""
import argparse
import gc
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = (("kernel", 240), ("step", 420))      # name, time limit of the child in seconds
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


def kernel(a):
    import torch
    from longterm360fov_amd import ops, utility
    out = torch.zeros(1, dtype=torch.int64, device="cuda")
    shapes = {"heat map: 2560 maps x 648 rows x 30, prediction time-major": (256, 10, 648, 30, 20),
              "LSTM models: 320 rows x 6": (32, 10, 1, 6, 200)}
    for name, (B, T, R, C, reps) in shapes.items():
        g = torch.Generator(device="cuda").manual_seed(1)
        pred = torch.rand((T, B, R, C), device="cuda", generator=g).transpose(0, 1)
        tgt = torch.rand((B, T, R, C), device="cuda", generator=g)
        tgt[:, :, ::2] = 2.0 * pred[:, :, ::2] + 1.0                     # half the rows agree
        nbytes = 2 * pred.numel() * 4
        src = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda").normal_()
        dst = torch.empty_like(src)
        legs = {"categorical_accuracy": lambda: ops.categorical_accuracy(pred, tgt, out=out, accumulate=True),
                "torch copy of the same number of bytes": lambda: dst.copy_(src)}
        traffic = {"categorical_accuracy": nbytes, "torch copy of the same number of bytes": 2 * nbytes}      # the copy writes too
        for fn in legs.values():
            fn()
            fn()
        torch.cuda.synchronize()
        want = utility.categorical_accuracy(pred.cpu().numpy(), tgt.cpu().numpy())
        got = int(ops.categorical_accuracy(pred, tgt).item())
        assert got == want[0], (got, want)
        times = {k: [] for k in legs}
        for _ in range(a.repeats):
            for k, fn in legs.items():
                times[k].append(event_ms(torch, fn, reps))
        rate = {}
        for k in legs:
            s = stats(times[k])
            rate[k] = traffic[k] / (s["median_ms"] * 1e-3) / 1e12
            emit({"phase": "kernel", "label": a.label, "shape": name, "call": k, "launches": reps, **s, "mbytes_moved": traffic[k] / 1e6,
                  "tbytes_per_s": rate[k]})
        k0, k1 = list(legs)
        emit({"phase": "kernel", "label": a.label, "shape": name, "matches": got, "rows": want[1], "mbytes_read_by_the_kernel": nbytes / 1e6,
              "kernel_rate_over_copy_rate": rate[k0] / rate[k1],
              "kernel_median_over_copy_median": float(np.median(times[k0]) / np.median(times[k1]))})


def step_models():
    from longterm360fov_amd import models as M
    from oracle import fov_oracle as O
    rng = np.random.default_rng(2)

    def config1():
        enc, dec0, tgt = O.synthetic_batch(1, 32, 10, 10)
        m = M.Seq2SeqLSTM(latent_dim=128, seed=1)
        return m, dict(optimizer="Adam", loss="mean_squared_error"), [enc, np.concatenate([dec0, tgt[:, :-1]], 1)], tgt

    def heatmap():
        w = O.init_convlstm_seq2seq(1, C=30, latent_dim=16, head="conv2d")
        enc = rng.random((32, 10, 36, 18, 30)).astype(np.float32)
        tgt = rng.random((32, 10, 36, 18, 30)).astype(np.float32)
        tgt /= tgt.sum(-1, keepdims=True)
        return M.ConvLSTMSeq2Seq(w, head="conv2d"), dict(optimizer="adam", loss="categorical_crossentropy"), [enc, enc[:, -1:]], tgt
    return {"config 1: Seq2SeqLSTM H 128, batch 32, T 10 -> 10": (config1, 200),
            "heat map: ConvLSTMSeq2Seq B 32, 36 x 18 x 30, T 10 -> 10": (heatmap, 3)}


def step(a):
    import torch
    cases = [c for c in a.cases.split(",") if c]
    for name, (make, calls) in step_models().items():
        legs = {}
        for case in cases:
            m, kw, x, y = make()
            m.compile(metrics=["accuracy"] if case == "on" else None, **kw)
            tr = m._get_trainer()
            batch = [m._to_device(v) for v in m._fit_inputs(x)] + [m._to_device(y)]
            legs[case] = (lambda tr=tr, batch=batch: tr.train_step(*batch))
        for fn in legs.values():
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(a.repeats):
            for k, fn in legs.items():
                times[k].append(event_ms(torch, fn, calls))
        for k in legs:
            emit({"phase": "step", "label": a.label, "model": name, "metrics": None if k == "off" else ["accuracy"], "steps": calls,
                  **stats(times[k])})
        if "on" in legs and "off" in legs:
            emit({"phase": "step", "label": a.label, "model": name,
                  "extra_ms_per_step_median": float(np.median(times["on"]) - np.median(times["off"])),
                  "off_spread_ms": float(np.max(times["off"]) - np.min(times["off"]))})
        del legs
        gc.collect()
        torch.cuda.empty_cache()


def drive(a):
    open(a.out, "w").close()
    for name, limit in PHASES:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--phase", name, "--repeats", str(a.repeats),
               "--out", a.out, "--label", a.label, "--cases", a.cases]
        print("+ " + " ".join(cmd), flush=True)
        code = subprocess.call(cmd, cwd=ROOT)
        if code != 0:       # a fault, an abort or a time limit: nothing more is started on the GPU
            print("phase %s ended with status %d: stopping" % (name, code), flush=True)
            return code
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "accuracy_metric_time.jsonl"))
    ap.add_argument("--phase", choices=[p for p, _ in PHASES], help="run one phase in this process (what the driver starts)")
    ap.add_argument("--label", default="this", help="the commit the rows belong to ('this' | 'parent')")
    ap.add_argument("--cases", default="off,on", help="step phase: 'off' = metrics=None, 'on' = metrics=['accuracy']")
    a = ap.parse_args()
    if a.phase is None:
        sys.exit(drive(a))
    global OUT
    OUT = a.out
    {"kernel": kernel, "step": step}[a.phase](a)


if __name__ == "__main__":
    main()
