"""What training and predicting the 2- and 3-layer seq2seq LSTM models in one launch per direction
(fov_stacked_seq2seq_train_fwd / _bwd, fov_lstm_seq_wgrad_layers) is worth against the per-layer path they replace - 2L forward
calls, the head, 2L BPTT calls with their own weight-gradient launches, the optimizer - which is the parent commit's code path,
unchanged.

One process, device-resident inputs and weights, HIP events around `--calls` back-to-back calls; the fused and the per-layer
path alternate, `--repeats` times each (StackedSeq2SeqTrainer.fused_stack True / False on two trainers built from the same
weights; StackedSeq2SeqLSTM.predict_device with fused=True / False; the library's knob is cached per process, so it is not what
switches here).  A row reports median / min / max; the verdict row of a shape says whether the fused path's SLOWEST repeat beats
the per-layer path's FASTEST one (the rule of DESIGN.md section 5) and how many library calls a step makes on either path
(counted by wrapping every ops function that launches, once, outside the timed region).

Shapes: the scripts' own (B 64, F 6, H 32, T 10 -> 10) and the metric's horizon at scale (B 1024 and 4096, F 90, H 64,
T 30 -> 30), L = 2 and 3; `train_step` and `predict` each.

    python tools/stacked_train_time.py [--repeats 5] [--calls 50] [--out profiles/stacked_train_time.jsonl]
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
LAUNCHING = ("lstm_seq", "lstm_seq_train", "lstm_seq_bwd", "lstm_seq_wgrad", "lstm_seq_wgrad_layers", "dense", "dense_bwd", "dense_mse_head",
             "mse_dense_grad", "adam_step", "scale_", "stacked_seq2seq_train_fwd", "stacked_seq2seq_train_bwd")


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


def count_calls(ops, fn):
    """Library calls (ops functions that launch) one fn() makes: every name in LAUNCHING wrapped for the one call."""
    n, saved = [0], {k: getattr(ops, k) for k in LAUNCHING}

    def wrap(f):
        def g(*a, **k):
            n[0] += 1
            return f(*a, **k)
        return g
    for k, f in saved.items():
        setattr(ops, k, wrap(f))
    try:
        fn()
    finally:
        for k, f in saved.items():
            setattr(ops, k, f)
    return n[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join("profiles", "stacked_train_time.jsonl"))
    a = ap.parse_args()
    import torch
    from longterm360fov_amd import ops
    from longterm360fov_amd.models import StackedSeq2SeqLSTM
    from longterm360fov_amd.training import StackedSeq2SeqTrainer
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for B, F, H, T_in, T_out in SHAPES:
        for L in (2, 3):
            m = StackedSeq2SeqLSTM(num_encoder_tokens=F, latent_dim=H, num_layers=L, recurrent_activation="sigmoid", seed=L)
            rng = np.random.default_rng(B + L)
            t = lambda *s: torch.from_numpy(rng.uniform(-0.9, 0.9, s).astype(np.float32)).cuda()
            e, d, y = t(B, T_in, F), t(B, T_out, 6), t(B, T_out, 6)
            trainers = {}
            for k, fused in (("fused", True), ("per layer", False)):
                trainers[k] = StackedSeq2SeqTrainer(m._w, L, act="sigmoid")
                trainers[k].fused_stack = fused
                trainers[k].fused_stack_max_batch = None      # what is measured here is what would set the bound
            shape = {"B": B, "F_enc": F, "H": H, "L": L, "T_in": T_in, "T_out": T_out}
            legs = {"train_step": {k: (lambda tr=tr: tr.train_step(e, d, y)) for k, tr in trainers.items()},
                    "predict": {"fused": lambda: m.predict_device(e, d, fused=True), "per layer": lambda: m.predict_device(e, d, fused=False)}}
            for what, pair in legs.items():
                outs = {k: fn() for k, fn in pair.items()}      # warm-up: buffers, LDS attribute, weights uploaded
                for fn in pair.values():
                    fn()
                torch.cuda.synchronize()
                calls = {k: count_calls(ops, fn) for k, fn in pair.items()}
                times = {k: [] for k in pair}
                for _ in range(a.repeats):
                    for k, fn in pair.items():
                        times[k].append(event_ms(torch, fn, a.calls))
                for tr in trainers.values():
                    tr.check()
                if what == "predict":
                    m._ws.check()
                for k in pair:
                    emit({**shape, "what": what, "path": k, "calls": a.calls, "library_calls": calls[k], **stats(times[k])})
                verdict = {**shape, "what": what, "tiles": (B + 15) // 16,
                           "speedup_median": float(np.median(times["per layer"]) / np.median(times["fused"])),
                           "slowest_fused_ms": float(np.max(times["fused"])), "fastest_per_layer_ms": float(np.min(times["per layer"])),
                           "slowest_fused_beats_fastest_per_layer": bool(np.max(times["fused"]) < np.min(times["per layer"]))}
                if what == "predict":
                    verdict["max_abs_fused_minus_per_layer"] = float((outs["fused"] - outs["per layer"]).abs().max().item())
                emit(verdict)
            del m, trainers, e, d, y, legs
            gc.collect()
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
