"""What the two encoder layers' BPTT as ONE launch (fov_lstm_stack2_bwd at H = 32 / 64, stack2_tile_bwd_kernel) is worth to the
trainers that run at the model's own width: `fused_encoder_bwd` on against off.  The off leg makes exactly the parent commit's calls
(two ops.lstm_seq_bwd, which walk these widths from the host): the baseline.

One process.  Device-resident inputs and weights, HIP events around `--calls` back-to-back `train_step`s; the legs alternate,
`--repeats` times each after a warm-up of all.  A row reports median / min / max; the verdict row of a shape says whether the on
leg's SLOWEST repeat beats the off leg's FASTEST one (the rule of DESIGN.md section 5 for a default).

    mixing    OthersMixingTrainer(tile_decoder=True) through OthersMixingSeq2Seq(native_width=True), the shapes of
              tools/mix_tile_time.py: H 32 at B 32 / 256 / 1024 and T 10 -> 10, 30 -> 30; H 64 at B 32.  A third leg, `padded`, is the
              model's default (every LSTM zero-padded to 256): its verdict row says whether native_width=True with the fused encoder
              BPTT now meets the same rule against it.
    context   OthersContextTrainer in its three modes, the shapes of tools/selffed2_time.py (H 32).

    python tools/stack2_tile_bwd_time.py [--repeats 20] [--calls 5] [--out profiles/stack2_tile_bwd_time.jsonl]

Kernel-alone times are not this tool's: `--trace-leg on|off` runs 20 training steps of one mixing leg at the script's own shape and
exits, to be run under `rocprofv3 --kernel-trace --stats -- python tools/stack2_tile_bwd_time.py --trace-leg ...`."""
import argparse
import gc
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIX_SHAPES = [(32, 32, 10, 10), (32, 32, 30, 30), (32, 256, 30, 30), (32, 1024, 30, 30), (64, 32, 30, 30)]      # H, B, T_in, T_out
CTX_SHAPES = [(32, 10, 10), (32, 30, 30), (256, 30, 30), (1024, 30, 30)]                                        # B, T_in, T_out (H 32)
MODES = ("target_user_only", "others_mlp", "others_lstm")
F, O_, USERS = 90, 6, 34


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
    for fn in legs.values():      # warm-up: buffers, LDS attribute, workspaces, the side stream's first in-line step
        fn(); fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            times[k].append(event_ms(torch, fn, calls))
    return times


def verdict(times, new, base):
    return {"speedup_median": float(np.median(times[base]) / np.median(times[new])),
            "slowest_%s_ms" % new: float(np.max(times[new])), "fastest_%s_ms" % base: float(np.min(times[base])),
            "slowest_%s_beats_fastest_%s" % (new, base): bool(np.max(times[new]) < np.min(times[base]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "stack2_tile_bwd_time.jsonl"))
    ap.add_argument("--trace-leg", choices=("on", "off"), default=None)
    a = ap.parse_args()
    import torch
    from longterm360fov_amd.models import OthersContextSeq2Seq, OthersMixingSeq2Seq
    if not torch.cuda.is_available():
        raise SystemExit("stack2_tile_bwd_time.py measures on the GPU: none found")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    rng = np.random.default_rng(7)
    cu = lambda x: torch.from_numpy(x).cuda()
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)

    def pair(model):
        on, off = model._make_trainer("adam"), model._make_trainer("adam")
        on.fused_encoder_bwd, off.fused_encoder_bwd = True, False
        return on, off

    if a.trace_leg:
        H, B, T_in, T_out = MIX_SHAPES[0]
        m = OthersMixingSeq2Seq(num_encoder_tokens=F, latent_dim=H, num_user=USERS, seed=11, native_width=True)
        tr = pair(m)[0 if a.trace_leg == "on" else 1]
        d = [cu(x) for x in (u(B, T_in, F), u(B, T_out, USERS - 1, O_), u(B, 1, O_), u(B, T_out, O_))]
        for _ in range(20):
            tr.train_step(*d)
        torch.cuda.synchronize()
        return
    for H, B, T_in, T_out in MIX_SHAPES:
        native = OthersMixingSeq2Seq(num_encoder_tokens=F, latent_dim=H, num_user=USERS, seed=11, native_width=True)
        padded = OthersMixingSeq2Seq(num_encoder_tokens=F, latent_dim=H, num_user=USERS, seed=11)
        padded.set_weights(native.get_weights())
        d = [cu(x) for x in (u(B, T_in, F), u(B, T_out, USERS - 1, O_), u(B, 1, O_), u(B, T_out, O_))]
        shape = {"trainer": "mixing", "B": B, "F": F, "H": H, "O": O_, "users": USERS, "T_in": T_in, "T_out": T_out}
        on, off = pair(native)
        tp = padded._make_trainer("adam")
        assert on.tile_decoder and off.tile_decoder
        legs = {"on": lambda: on.train_step(*d), "off": lambda: off.train_step(*d), "padded": lambda: tp.train_step(*d)}
        first = {k: float(fn().item()) for k, fn in legs.items()}
        times = alternate(torch, legs, a.repeats, a.calls)
        for k in times:
            emit({**shape, "call": "train_step, " + k, "calls": a.calls, **stats(times[k])})
        emit({**shape, "call": "train_step", "tiles": (B + 15) // 16, **{"first_loss_" + k: v for k, v in first.items()}, **verdict(times, "on", "off")})
        emit({**shape, "call": "train_step, native width against padded", **verdict(times, "on", "padded")})
        del on, off, tp, native, padded
        gc.collect()
        torch.cuda.empty_cache()
    H = 32
    for mode in MODES:
        for B, T_in, T_out in CTX_SHAPES:
            m = OthersContextSeq2Seq(mode, num_encoder_tokens=F, latent_dim=H, num_user=USERS, seed=11, predict_step=T_out)
            d = [cu(x) for x in (u(B, T_in, F), u(B, T_out, USERS - 1, O_), u(B, 1, O_), u(B, T_out, O_))]
            shape = {"trainer": "context", "mode": mode, "B": B, "F": F, "H": H, "O": O_, "users": USERS, "T_in": T_in, "T_out": T_out}
            on, off = pair(m)
            legs = {"on": lambda: on.train_step(*d), "off": lambda: off.train_step(*d)}
            first = {k: float(fn().item()) for k, fn in legs.items()}
            times = alternate(torch, legs, a.repeats, a.calls)
            on.ws.check(); off.ws.check()
            for k in times:
                emit({**shape, "call": "train_step, " + k, "calls": a.calls, **stats(times[k])})
            emit({**shape, "call": "train_step", "tiles": (B + 15) // 16, **{"first_loss_" + k: v for k, v in first.items()}, **verdict(times, "on", "off")})
            del on, off, m
            gc.collect()
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
