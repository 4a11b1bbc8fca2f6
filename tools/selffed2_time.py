"""What the self-fed two-layer decoder as ONE launch per direction (fov_selffed2_decoder_fwd / _bwd, lstm_selffed2.hip) is worth to
OthersContextSeq2Seq (given_others_gt_mean_var_seq2seq.py:203-299, heads target_user_only / others_mlp / others_lstm) against
the step-by-step walk it replaces - three launches per predicted second forward, five backward - which stays in the code under
FOV_NO_SELFFED2_FUSED=1 and is the parent commit's path, unchanged: that leg is the baseline.

One process.  `train_step`: device-resident inputs and weights, HIP events around `--calls` back-to-back OthersContextTrainer
steps.  `predict`: the model's own call on host arrays (one chunk), a host clock around `--calls` calls, each of which ends in
the device-to-host copy of the prediction.  The fused leg and the walk leg (same weights; the knob is set around the walk leg
and the wrappers follow the environment) alternate, `--repeats` times each after a warm-up of both.  A row reports median /
min / max; the verdict row of a shape says whether the fused leg's SLOWEST repeat beats the walk's FASTEST one (the rule of
DESIGN.md section 5).

Shapes: the script's (B 32, F 90, H 32, 34 users, T 10 -> 10), T 30 -> 30, and B 256 / 1024 at T 30 -> 30.

    python tools/selffed2_time.py [--repeats 20] [--calls 5] [--out profiles/selffed2_time.jsonl]
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

SHAPES = [(32, 10, 10), (32, 30, 30), (256, 30, 30), (1024, 30, 30)]      # B, T_in, T_out
MODES = ("target_user_only", "others_mlp", "others_lstm")
F, H, O_, USERS = 90, 32, 6, 34
KNOB = "FOV_NO_SELFFED2_FUSED"


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


def walk_leg(fn):
    """fn under the knob: the parent commit's path."""
    def run():
        os.environ[KNOB] = "1"
        try:
            return fn()
        finally:
            del os.environ[KNOB]
    return run


def alternate(torch, clock, legs, repeats, calls):
    for fn in legs.values():      # warm-up: buffers, LDS attribute, workspaces
        fn(); fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            times[k].append(clock(torch, fn, calls))
    return times


def verdict(times):
    return {"speedup_median": float(np.median(times["walk"]) / np.median(times["fused"])),
            "slowest_fused_ms": float(np.max(times["fused"])), "fastest_walk_ms": float(np.min(times["walk"])),
            "slowest_fused_beats_fastest_walk": bool(np.max(times["fused"]) < np.min(times["walk"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "selffed2_time.jsonl"))
    a = ap.parse_args()
    assert KNOB not in os.environ, "the knob is this script's to set"
    import torch
    from longterm360fov_amd import ops
    from longterm360fov_amd.models import OthersContextSeq2Seq
    if not torch.cuda.is_available():
        raise SystemExit("selffed2_time.py measures on the GPU: none found")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    rng = np.random.default_rng(7)
    cu = lambda x: torch.from_numpy(x).cuda()
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
    for mode in MODES:
        for B, T_in, T_out in SHAPES:
            assert ops.selffed2_decoder_supported(B, T_out, O_, H) and ops.selffed2_decoder_supported(B, T_out, O_, H, backward=True)
            m = OthersContextSeq2Seq(mode, num_encoder_tokens=F, latent_dim=H, num_user=USERS, seed=11, predict_step=T_out)
            enc, oth, dec0, tgt = u(B, T_in, F), u(B, T_out, USERS - 1, O_), u(B, 1, O_), u(B, T_out, O_)
            shape = {"mode": mode, "B": B, "F": F, "H": H, "O": O_, "users": USERS, "T_in": T_in, "T_out": T_out}
            # ---- train_step ----
            fused, walk = m._make_trainer("adam"), m._make_trainer("adam")
            d = [cu(x) for x in (enc, oth, dec0, tgt)]
            legs = {"fused": lambda: fused.train_step(*d), "walk": walk_leg(lambda: walk.train_step(*d))}
            first = {k: float(fn().item()) for k, fn in legs.items()}
            times = alternate(torch, event_ms, legs, a.repeats, a.calls)
            fused.ws.check(); walk.ws.check()
            for k in times:
                emit({**shape, "call": "train_step, " + k, "calls": a.calls, **stats(times[k])})
            emit({**shape, "call": "train_step", "tiles": (B + 15) // 16, "first_loss_fused": first["fused"], "first_loss_walk": first["walk"],
                  **verdict(times)})
            del fused, walk
            # ---- predict ----
            xin = [enc, dec0] if mode == "target_user_only" else [enc, oth, dec0]
            legs = {"fused": lambda: m.predict(xin, batch_size=B), "walk": walk_leg(lambda: m.predict(xin, batch_size=B))}
            y = {k: fn() for k, fn in legs.items()}
            times = alternate(torch, host_ms, legs, a.repeats, a.calls)
            for k in times:
                emit({**shape, "call": "predict, " + k, "calls": a.calls, **stats(times[k])})
            emit({**shape, "call": "predict", "tiles": (B + 15) // 16, "max_abs_fused_minus_walk": float(np.abs(y["fused"] - y["walk"]).max()),
                  **verdict(times)})
            del m
            gc.collect()
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
