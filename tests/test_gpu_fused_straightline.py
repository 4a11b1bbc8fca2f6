"""The fused (one-launch) encode + decode kernel runs its middle steps through a steady-state copy of the step - same-XCD
exchange, six input k-blocks, every `t` condition a compile-time fact - and its first and last steps, the write-through
exchange and other input widths through the general copy.  These tests sit on the seams: phase
lengths at which the steady-state loop runs zero, one or two times, a padded grid, a ragged last tile, every hidden size,
both activations, the three input-width paths, and the header a launch leaves behind.

Bounds: fused against two launches, fast against write-through exchange and first against second call are the SAME
arithmetic in the same order - bit-equal.  Against the fp64 oracle the bound is the suite's 2e-5 (test_gpu_parity.py)."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

pytestmark = pytest.mark.gpu

TIGHT = 2e-5


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()   # (a copy: the cached inputs are read-only)


@functools.lru_cache(maxsize=None)
def weights(H, F_enc, F_dec):
    w = O.init_seq2seq(7000 + H + F_enc, F_enc, F_dec, H, bias_noise=0.05)
    for v in w.values():
        v.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def device_weights(H, F_enc, F_dec):
    return {k: dev(v) for k, v in weights(H, F_enc, F_dec).items()}


@functools.lru_cache(maxsize=None)
def inputs(B, T_in, F_enc, F_dec):
    rng = np.random.default_rng(7100 + 131 * B + 17 * T_in + F_enc)
    enc = rng.uniform(-1, 1, (B, T_in, F_enc)).astype(np.float32)
    dec0 = rng.uniform(-1, 1, (B, 1, F_dec)).astype(np.float32)
    enc.setflags(write=False)
    dec0.setflags(write=False)
    return enc, dec0


def run_all_forms(B, T_in, T_out, H, act, F_enc=90, F_dec=6):
    """fused call, its repeat on the same workspace, the two-launch form, the write-through exchange -> the fused output"""
    from longterm360fov_amd import ops
    w = weights(H, F_enc, F_dec)
    dw = device_weights(H, F_enc, F_dec)
    enc, dec0 = inputs(B, T_in, F_enc, F_dec)
    d_enc, d_dec0 = dev(enc), dev(dec0)
    ws = ops.Workspace()
    one = ops.seq2seq_decode(d_enc, d_dec0, dw, T_out, act=act, impl="cluster", workspace=ws).clone()
    ws.check()
    # header state: a second launch continues from the epoch / launch count the fused one left behind
    again = ops.seq2seq_decode(d_enc, d_dec0, dw, T_out, act=act, impl="cluster", workspace=ws).clone()
    ws.check()
    assert torch.equal(again, one), "second call on the same workspace differs"
    os.environ["FOV_TWO_LAUNCHES"] = "1"
    try:
        two = ops.seq2seq_decode(d_enc, d_dec0, dw, T_out, act=act, impl="cluster", workspace=ws).clone()
        ws.check()
    finally:
        del os.environ["FOV_TWO_LAUNCHES"]
    assert torch.equal(one, two), "fused call differs from encoder launch + decoder launch"
    os.environ["FOV_FORCE_SAFE_EXCHANGE"] = "1"
    try:
        safe = ops.seq2seq_decode(d_enc, d_dec0, dw, T_out, act=act, impl="cluster", workspace=ws).clone()
        ws.check()
        if H > 64:
            assert ws.exchange_mode() == 2
    finally:
        os.environ.pop("FOV_FORCE_SAFE_EXCHANGE", None)
    assert torch.equal(safe, one), "write-through exchange differs from the fast path"
    back = ops.seq2seq_decode(d_enc, d_dec0, dw, T_out, act=act, impl="cluster", workspace=ws)
    ws.check()
    assert torch.equal(back, one), "call after the write-through launch differs"
    ref = O.seq2seq_decode(enc.astype(np.float64), dec0.astype(np.float64), {k: v.astype(np.float64) for k, v in w.items()}, T_out, act=act)
    got = one.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    err = float(np.abs(got - ref).max())
    print("B=%d T=%d->%d H=%d F=%d %s: max abs err vs fp64 oracle %.3e" % (B, T_in, T_out, H, F_enc, act, err))
    assert err <= TIGHT, err
    return one


# B 48 at H 256 = three groups: the grid is padded to eight; B 20 = a ragged second tile
@pytest.mark.parametrize("B,H,act", [(48, 256, "sigmoid"), (48, 256, "hard_sigmoid"), (20, 256, "sigmoid"), (20, 128, "sigmoid"),
                                     (20, 128, "hard_sigmoid"), (20, 64, "sigmoid"), (20, 64, "hard_sigmoid")])
@pytest.mark.parametrize("T_out", [1, 2, 3])
@pytest.mark.parametrize("T_in", [1, 2, 3, 5])
def test_peeled_steps_at_short_phases(B, H, act, T_in, T_out):
    """Phase lengths around the peeling: the encoder phase's steady-state loop covers steps 1 .. T_in - 3 (none up to
    T_in = 3, two at T_in = 5), the decoder phase's 1 .. T_out - 2 (none up to T_out = 2, one at T_out = 3)."""
    run_all_forms(B, T_in, T_out, H, act)


@pytest.mark.parametrize("F_enc", [90, 33, 96])
@pytest.mark.parametrize("T_in,T_out", [(5, 3), (7, 5)])
def test_input_width_paths(F_enc, T_in, T_out):
    """F_enc 90 and 96 have six input k-blocks (the steady-state copy, all six staging columns written; at 96 no pad column
    is left), F_enc 33 has three (the general copy in every step)."""
    run_all_forms(48, T_in, T_out, 256, "sigmoid", F_enc=F_enc)


def test_longer_phases_and_batch_rows_are_independent():
    """More steady-state steps than first / last ones, and a sequence's output does not depend on its place in the batch."""
    from longterm360fov_amd import ops
    B, T_in, T_out, H = 40, 9, 7, 256
    one = run_all_forms(B, T_in, T_out, H, "sigmoid")
    enc, dec0 = inputs(B, T_in, 90, 6)
    perm = np.random.default_rng(5).permutation(B)
    outp = ops.seq2seq_decode(dev(enc[perm]), dev(dec0[perm]), device_weights(H, 90, 6), T_out, impl="cluster", workspace=ops.Workspace())
    assert torch.equal(outp, one[perm])
