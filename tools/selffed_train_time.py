"""What training the self-fed one-layer decoder (SelfFedSeq2SeqTrainer, FoV_seq2seq_no_teac_forc.py:37-149) with its unroll as ONE
launch per direction (fov_selffed_decoder_fwd / _bwd) is worth against the step-by-step walk it replaces - about six launches
per predicted second - which is the parent commit's code path, unchanged (fused_unroll = fused_unroll_bwd = False).

One process, device-resident inputs and weights, HIP events around `--calls` back-to-back train_step calls; the fused trainer
and the loop trainer (same initial weights) alternate, `--repeats` times each.  A row reports median / min / max; the verdict
row of a shape says whether the fused step's SLOWEST repeat beats the loop's FASTEST one (the rule of DESIGN.md section 5).
At the script's shape the unroll's forward and backward are also timed alone (both forms, on the same tape), and the two
kernels at T 30 and T 2: the slope is a step without launch and weight prologue, printed beside the step's MFMA issue time
(32 cycles per v_mfma_f32_16x16x4_f32; forward 16 + H + H/4 of them per wave, backward 4 + H + 16).

Shapes: the script's (B 32, F 90, H 64, O 6, T 10 -> 10), the metric's horizon (T 30 -> 30), and B 256 / 1024 / 4096 at T 30 -> 30.

    python tools/selffed_train_time.py [--repeats 5] [--calls 20] [--out profiles/selffed_train_time.jsonl]
"""
import argparse
import gc
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(32, 10, 10), (32, 30, 30), (256, 30, 30), (1024, 30, 30), (4096, 30, 30)]      # B, T_in, T_out
F, H, O_ = 90, 64, 6
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


def alternate(torch, legs, repeats, calls):
    for fn in legs.values():      # warm-up: buffers, LDS attribute, workspaces
        fn(); fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            times[k].append(event_ms(torch, fn, calls))
    return times


def verdict(times):
    return {"speedup_median": float(np.median(times["loop"]) / np.median(times["fused"])),
            "slowest_fused_ms": float(np.max(times["fused"])), "fastest_loop_ms": float(np.min(times["loop"])),
            "slowest_fused_beats_fastest_loop": bool(np.max(times["fused"]) < np.min(times["loop"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "selffed_train_time.jsonl"))
    a = ap.parse_args()
    import torch
    from longterm360fov_amd import ops
    from longterm360fov_amd.models import glorot_uniform, init_lstm_weights
    from longterm360fov_amd.training import SelfFedSeq2SeqTrainer
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    rng = np.random.default_rng(7)
    w = {}
    w["enc_K"], w["enc_R"], w["enc_b"] = init_lstm_weights(rng, F, H)
    w["dec_K"], w["dec_R"], w["dec_b"] = init_lstm_weights(rng, O_, H)
    w["dense_W"], w["dense_b"] = glorot_uniform(rng, H, O_), np.zeros(O_, np.float32)
    cu = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()

    def trainers():
        fused, loop = SelfFedSeq2SeqTrainer(w), SelfFedSeq2SeqTrainer(w)
        loop.fused_unroll = loop.fused_unroll_bwd = False
        return fused, loop

    for B, T_in, T_out in SHAPES:
        enc, dec0, tgt = cu(rng.uniform(-1, 1, (B, T_in, F))), cu(rng.uniform(-1, 1, (B, 1, O_))), cu(rng.uniform(-1, 1, (B, T_out, O_)))
        fused, loop = trainers()
        shape = {"B": B, "F": F, "H": H, "O": O_, "T_in": T_in, "T_out": T_out}
        first = {k: float(t.train_step(enc, dec0, tgt).item()) for k, t in (("fused", fused), ("loop", loop))}
        times = alternate(torch, {"fused": lambda: fused.train_step(enc, dec0, tgt), "loop": lambda: loop.train_step(enc, dec0, tgt)},
                          a.repeats, a.calls)
        fused.ws.check(); loop.ws.check()
        for k in times:
            emit({**shape, "call": "train_step, " + k, "calls": a.calls, **stats(times[k])})
        emit({**shape, "call": "train_step", "tiles": (B + 15) // 16, "first_loss_fused": first["fused"], "first_loss_loop": first["loop"],
              **verdict(times)})
        if B == 32:     # the unroll alone, forward and backward apart, both forms on the same inputs / tape
            x0, dl = dec0.reshape(B, O_), cu(rng.standard_normal((T_out, B, O_)))
            fwd = alternate(torch, {"fused": lambda: fused._unroll_forward("dec", "dense", x0, None, None, T_out, "tanh"),
                                    "loop": lambda: loop._unroll_forward("dec", "dense", x0, None, None, T_out, "tanh")}, a.repeats, a.calls)
            tp = loop._unroll_forward("dec", "dense", x0, None, None, T_out, "tanh")
            bwd = alternate(torch, {"fused": lambda: fused._unroll_backward(tp, dl), "loop": lambda: loop._unroll_backward(tp, dl)},
                            a.repeats, a.calls)
            for name, t in (("unroll forward", fwd), ("unroll backward + weight-gradient products", bwd)):
                for k in t:
                    emit({**shape, "call": "%s, %s" % (name, k), "calls": a.calls, **stats(t[k])})
                emit({**shape, "call": name, **verdict(t)})
        del fused, loop
        gc.collect()
        torch.cuda.empty_cache()

    # the two kernels alone at T 30 and T 2: the slope is a step without launch and prologue
    B = 32
    dw = {k: cu(v) for k, v in w.items()}
    x0 = cu(rng.uniform(-1, 1, (B, O_)))
    args = (x0, dw["dec_K"], dw["dec_R"], dw["dec_b"], dw["dense_W"], dw["dense_b"])
    med = {}
    for T in (30, 2):
        dl = cu(rng.standard_normal((T, B, O_)))
        _, tp = ops.selffed_decoder_fwd(*args, T)
        legs = {"forward": lambda: ops.selffed_decoder_fwd(*args, T),
                "backward": lambda: ops.selffed_decoder_bwd(tp, dl, dw["dec_K"], dw["dec_R"], dw["dense_W"])}
        t = alternate(torch, legs, a.repeats, 5 * a.calls)
        for k in t:
            med[k, T] = float(np.median(t[k]))
            emit({"B": B, "H": H, "O": O_, "T": T, "call": "kernel + output allocation, " + k, "calls": 5 * a.calls, **stats(t[k])})
    for k, mfmas in (("forward", 16 + H + H // 4), ("backward", 4 + H + 16)):
        us = (med[k, 30] - med[k, 2]) * 1e3 / 28
        emit({"B": B, "H": H, "O": O_, "call": k + " kernel, per step (slope T 30 - T 2)", "us_per_step": us,
              "cycles_per_step_at_%.1f_GHz" % CLOCK_GHZ: us * CLOCK_GHZ * 1e3, "mfma_per_wave_per_step": mfmas,
              "mfma_issue_cycles_per_step": 32 * mfmas, "split_of_the_remainder": "not measured"})
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
