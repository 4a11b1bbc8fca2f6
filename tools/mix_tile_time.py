"""What running OthersMixingSeq2Seq (given_others_gt_mean_var_seq2seq.py:98-308, mlp_mixing) at its own width is worth: the
opt-in native_width=True - the encoder stack in one launch, the whole unrolled decoder in one launch each way on the
one-workgroup-per-tile kernels (mix_tile.hip), an unpadded trainer - against the default, which zero-pads every LSTM to H = 256
and runs the eight-workgroups-per-tile exchange kernels.  The default leg is the parent commit's path, unchanged: the baseline.

One process.  `train_step`: device-resident inputs and weights, HIP events around `--calls` back-to-back trainer steps.
`predict`: the model's own call on host arrays (one chunk), a host clock around `--calls` calls that ends in a synchronise.  The
native leg and the padded leg (the same weights) alternate, `--repeats` times each after a warm-up of both.  A row reports median
/ min / max; the verdict row of a shape says whether the native leg's SLOWEST repeat beats the padded leg's FASTEST one (the rule
of DESIGN.md section 5 for a later flip of the default), and carries the largest difference of the two legs' predictions on the
same inputs, which must stay within 2e-5.

Shapes (F 90, 34 users): the script's own (B 32, H 32, T 10 -> 10), T 30 -> 30 at B 32 / 256 / 1024, and H 64 at B 32.

    python tools/mix_tile_time.py [--repeats 20] [--calls 5] [--out profiles/mix_tile_time.jsonl]

Kernel-alone times are not this tool's: `--trace-leg native|padded` runs 20 training steps and 20 predictions of one leg at the
script's own shape and exits, to be run under `rocprofv3 --kernel-trace --stats -- python tools/mix_tile_time.py --trace-leg ...`.
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(32, 32, 10, 10), (32, 32, 30, 30), (32, 256, 30, 30), (32, 1024, 30, 30), (64, 32, 30, 30)]      # H, B, T_in, T_out
F, O_, USERS = 90, 6, 34
PREDICTION_BOUND = 2e-5


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


def host_ms(torch, fn, calls):
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def alternate(torch, clock, legs, repeats, calls):
    for fn in legs.values():      # warm-up: buffers, LDS attribute, workspaces, the side stream's first in-line step
        fn(); fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            times[k].append(clock(torch, fn, calls))
    return times


def verdict(times):
    return {"speedup_median": float(np.median(times["padded"]) / np.median(times["native"])),
            "slowest_native_ms": float(np.max(times["native"])), "fastest_padded_ms": float(np.min(times["padded"])),
            "slowest_native_beats_fastest_padded": bool(np.max(times["native"]) < np.min(times["padded"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "mix_tile_time.jsonl"))
    ap.add_argument("--trace-leg", choices=("native", "padded"), default=None)
    a = ap.parse_args()
    import torch
    from longterm360fov_amd.models import OthersMixingSeq2Seq
    from longterm360fov_amd.training import PaddedTrainer
    if not torch.cuda.is_available():
        raise SystemExit("mix_tile_time.py measures on the GPU: none found")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    rng = np.random.default_rng(7)
    cu = lambda x: torch.from_numpy(x).cuda()
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
    if a.trace_leg:
        H, B, T_in, T_out = SHAPES[0]
        m = OthersMixingSeq2Seq(num_encoder_tokens=F, latent_dim=H, num_user=USERS, seed=11, native_width=a.trace_leg == "native")
        enc, oth, dec0, tgt = u(B, T_in, F), u(B, T_out, USERS - 1, O_), u(B, 1, O_), u(B, T_out, O_)
        tr, d = m._make_trainer("adam"), [cu(x) for x in (enc, oth, dec0, tgt)]
        for _ in range(20):
            tr.train_step(*d)
        for _ in range(20):
            m.predict([enc, oth, dec0], batch_size=B)
        torch.cuda.synchronize()
        return
    for H, B, T_in, T_out in SHAPES:
        native = OthersMixingSeq2Seq(num_encoder_tokens=F, latent_dim=H, num_user=USERS, seed=11, native_width=True)
        padded = OthersMixingSeq2Seq(num_encoder_tokens=F, latent_dim=H, num_user=USERS, seed=11)
        padded.set_weights(native.get_weights())
        assert native._run_width() == H and padded._run_width() == 256
        enc, oth, dec0, tgt = u(B, T_in, F), u(B, T_out, USERS - 1, O_), u(B, 1, O_), u(B, T_out, O_)
        shape = {"B": B, "F": F, "H": H, "O": O_, "users": USERS, "T_in": T_in, "T_out": T_out}
        # ---- train_step ----
        tn, tp = native._make_trainer("adam"), padded._make_trainer("adam")
        assert tn.tile_decoder and not isinstance(tn, PaddedTrainer) and isinstance(tp, PaddedTrainer)
        d = [cu(x) for x in (enc, oth, dec0, tgt)]
        legs = {"native": lambda: tn.train_step(*d), "padded": lambda: tp.train_step(*d)}
        first = {k: float(fn().item()) for k, fn in legs.items()}
        times = alternate(torch, event_ms, legs, a.repeats, a.calls)
        for k in times:
            emit({**shape, "call": "train_step, " + k, "calls": a.calls, **stats(times[k])})
        emit({**shape, "call": "train_step", "tiles": (B + 15) // 16, "first_loss_native": first["native"], "first_loss_padded": first["padded"],
              **verdict(times)})
        del tn, tp
        # ---- predict ----
        xin = [enc, oth, dec0]
        legs = {"native": lambda: native.predict(xin, batch_size=B), "padded": lambda: padded.predict(xin, batch_size=B)}
        y = {k: fn() for k, fn in legs.items()}
        diff = float(np.abs(y["native"] - y["padded"]).max())
        assert diff <= PREDICTION_BOUND, "the two legs' predictions differ by %.3e at %r" % (diff, shape)
        times = alternate(torch, host_ms, legs, a.repeats, a.calls)
        for k in times:
            emit({**shape, "call": "predict, " + k, "calls": a.calls, **stats(times[k])})
        emit({**shape, "call": "predict", "tiles": (B + 15) // 16, "max_abs_native_minus_padded": diff, **verdict(times)})
        del native, padded
        gc.collect()
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
