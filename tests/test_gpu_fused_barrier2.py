"""The cluster LSTM step around its second barrier: the bias enters every step as the C operand of
the first MFMA on each accumulator instead of by copy, and the decoder checks the tags of the Dense partials once in front
of its spin loop.

Bias path: with all four weight matrices zero the output is a function of the biases alone, so a dropped or doubled bias
shows at 1e-1; and random weights with a bias as large as the pre-activations.  Both through every entry point that runs
the step: the fused call, the decoder alone, a layer with and without an initial state, a layer from a precomputed input
projection.  Seams: phase lengths at which the steady-state loop takes one to four turns and hands over to the general
tail steps at each of the three x-tile residues, padded grid and ragged tile, inputs that differ strongly from step to
step so that a stale x or h tile shows - what any change to the order of LDS reads around barrier 2 has to survive.

Bounds: the suite's 2e-5 against the fp64 oracle (test_gpu_parity.py); bit-equal where two forms are the same arithmetic.
The spin loops' turn and give-up paths are not tested: they cannot be reached without provoking a hang."""
import functools

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

pytestmark = pytest.mark.gpu

TIGHT = 2e-5
B_BIAS = 20   # a full tile and a ragged one


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()   # (a copy: the cached inputs are read-only)


def f64(w):
    return {k: v.astype(np.float64) for k, v in w.items()}


@functools.lru_cache(maxsize=None)
def bias_weights(H, kind, F_enc=90, F_dec=6):
    """'bias_only': zero K, R, dK, dR, biases uniform in +-2.  'noisy': the usual initialisation, bias noise 1.0."""
    w = O.init_seq2seq(8100 + H + F_enc, F_enc, F_dec, H, bias_noise=1.0)
    if kind == "bias_only":
        rng = np.random.default_rng(8200 + H)
        for k in ("enc_K", "enc_R", "dec_K", "dec_R"):
            w[k] = np.zeros_like(w[k])
        for k in ("enc_b", "dec_b", "dense_b"):
            w[k] = rng.uniform(-2, 2, w[k].shape).astype(np.float32)
    for v in w.values():
        v.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def bias_inputs(H, T, F_enc=90, F_dec=6):
    rng = np.random.default_rng(8300 + 7 * H + T + F_enc)
    d = dict(enc=rng.uniform(-1, 1, (B_BIAS, T, F_enc)), dec0=rng.uniform(-1, 1, (B_BIAS, 1, F_dec)),
             h0=rng.uniform(-1, 1, (B_BIAS, H)), c0=rng.uniform(-1, 1, (B_BIAS, H)))
    d = {k: v.astype(np.float32) for k, v in d.items()}
    for v in d.values():
        v.setflags(write=False)
    return d


def close(got, ref, what):
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    err = float(np.abs(got - ref).max())
    print("%s: max abs err vs fp64 oracle %.3e" % (what, err))
    assert err <= TIGHT, (what, err)


def decoder_ref(dec0, h, c, w, T_out, act):
    """O.seq2seq_decode's loop from a given state"""
    y, out = dec0[:, 0], []
    for _ in range(T_out):
        h, c = O.lstm_step(y, h, c, w["dec_K"], w["dec_R"], w["dec_b"], act)
        y = O.dense(h, w["dense_W"], w["dense_b"])
        out.append(y)
    return np.stack(out, axis=1)


@pytest.mark.parametrize("act", ["sigmoid", "hard_sigmoid"])
@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("kind", ["bias_only", "noisy"])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_bias_through_every_entry_point(H, kind, T, act):
    from longterm360fov_amd import ops
    w, x = bias_weights(H, kind), bias_inputs(H, T)
    w64, x64 = f64(w), f64(x)
    dw = {k: dev(v) for k, v in w.items()}
    tag = "H=%d %s T=%d %s " % (H, kind, T, act)

    out = ops.seq2seq_decode(dev(x["enc"]), dev(x["dec0"]), dw, T, act=act, impl="cluster", workspace=ops.Workspace())
    ref = O.seq2seq_decode(x64["enc"], x64["dec0"], w64, T, act=act)
    if kind == "bias_only":   # the premise of the case: the biases alone move the output, and by far more than the bound
        flipped = dict(w64, dec_b=-w64["dec_b"])
        assert np.abs(ref - O.seq2seq_decode(x64["enc"], x64["dec0"], flipped, T, act=act)).max() > 1e-1
    close(out, ref, tag + "fused call")

    out = ops.seq2seq_decoder(dev(x["dec0"]), dev(x["h0"]), dev(x["c0"]), dw, T, act=act, impl="cluster", workspace=ops.Workspace())
    close(out, decoder_ref(x64["dec0"], x64["h0"], x64["c0"], w64, T, act), tag + "decoder alone")

    for state in (False, True):
        h0, c0 = (x["h0"], x["c0"]) if state else (None, None)
        hs, hT, cT = ops.lstm_seq(dev(x["enc"]), dw["enc_K"], dw["enc_R"], dw["enc_b"], dev(h0) if state else None,
                                  dev(c0) if state else None, act=act, impl="cluster", workspace=ops.Workspace())
        r_hs, r_h, r_c = O.lstm_layer(x64["enc"], w64["enc_K"], w64["enc_R"], w64["enc_b"],
                                      x64["h0"] if state else None, x64["c0"] if state else None, act=act)
        what = tag + ("layer from a state" if state else "layer from zero")
        close(hs, r_hs, what + " hs")
        close(hT, r_h, what + " hT")
        close(cT, r_c, what + " cT")

    # the layer again from its input projection (rounded to fp32 once: 1e-7 of a pre-activation of a few units)
    zx = (x64["enc"] @ w64["enc_K"]).astype(np.float32)
    hs, hT, cT = ops.lstm_seq_zx(dev(zx), dw["enc_R"], dw["enc_b"], act=act, impl="cluster", workspace=ops.Workspace())
    r_hs, r_h, r_c = O.lstm_layer(x64["enc"], w64["enc_K"], w64["enc_R"], w64["enc_b"], act=act)
    close(hs, r_hs, tag + "zx layer hs")
    close(cT, r_c, tag + "zx layer cT")


@pytest.mark.parametrize("F", [10, 33])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("H", [64, 256])
def test_bias_with_other_input_widths(H, T, F):
    """One input k-block (the opening block is also the closing one) and three (opening block, loop, closing block): the
    run-time-length input projection, which the 90-wide input of the other cases never takes."""
    from longterm360fov_amd import ops
    for kind in ("bias_only", "noisy"):
        w, x = bias_weights(H, kind, F_enc=F), bias_inputs(H, T, F_enc=F)
        w64, x64 = f64(w), f64(x)
        for state in (False, True):
            hs, hT, cT = ops.lstm_seq(dev(x["enc"]), dev(w["enc_K"]), dev(w["enc_R"]), dev(w["enc_b"]), dev(x["h0"]) if state else None,
                                      dev(x["c0"]) if state else None, impl="cluster", workspace=ops.Workspace())
            r_hs, _, r_c = O.lstm_layer(x64["enc"], w64["enc_K"], w64["enc_R"], w64["enc_b"],
                                        x64["h0"] if state else None, x64["c0"] if state else None)
            close(hs, r_hs, "H=%d F=%d T=%d %s state=%s hs" % (H, F, T, kind, state))
            close(cT, r_c, "H=%d F=%d T=%d %s state=%s cT" % (H, F, T, kind, state))


# ---- seams of the steady-state loop: what is read behind barrier 2 of one step feeds the next ----
@functools.lru_cache(maxsize=None)
def seam_weights(F_enc):
    w = O.init_seq2seq(8400 + F_enc, F_enc, 6, 256, bias_noise=0.05)
    for v in w.values():
        v.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def seam_inputs(B, T_in, F_enc):
    """x_t scaled by (-1)^t (t + 1) / T: neighbouring steps differ in sign and size, a stale x or h tile shows"""
    rng = np.random.default_rng(8500 + 131 * B + 17 * T_in + F_enc)
    scale = np.array([(-1.0) ** t * (t + 1) / T_in for t in range(T_in)])
    enc = (rng.uniform(-1, 1, (B, T_in, F_enc)) * scale[None, :, None]).astype(np.float32)
    dec0 = rng.uniform(-1, 1, (B, 1, 6)).astype(np.float32)
    enc.setflags(write=False)
    dec0.setflags(write=False)
    return enc, dec0


def all_forms(B, T_in, T_out, F_enc):
    """as test_gpu_fused_straightline.run_all_forms, on this file's inputs: fused == its repeat on the same workspace ==
    two launches == write-through exchange, and the oracle within the bound"""
    import os
    from longterm360fov_amd import ops
    w = seam_weights(F_enc)
    dw = {k: dev(v) for k, v in w.items()}
    enc, dec0 = seam_inputs(B, T_in, F_enc)
    d_enc, d_dec0 = dev(enc), dev(dec0)
    ws = ops.Workspace()

    def call():
        out = ops.seq2seq_decode(d_enc, d_dec0, dw, T_out, impl="cluster", workspace=ws).clone()
        ws.check()
        return out

    one = call()
    assert torch.equal(call(), one), "second call on the same workspace differs"
    for knob, what in (("FOV_TWO_LAUNCHES", "encoder launch + decoder launch"), ("FOV_FORCE_SAFE_EXCHANGE", "write-through exchange")):
        os.environ[knob] = "1"
        try:
            other = call()
            if knob == "FOV_FORCE_SAFE_EXCHANGE":
                assert ws.exchange_mode() == 2
        finally:
            del os.environ[knob]
        assert torch.equal(other, one), "fused call differs from " + what
    assert torch.equal(call(), one), "call after the write-through launch differs"
    close(one, O.seq2seq_decode(enc.astype(np.float64), dec0.astype(np.float64), f64(w), T_out), "B=%d T=%d->%d F=%d" % (B, T_in, T_out, F_enc))


@pytest.mark.parametrize("T_out", [3, 4, 5])
@pytest.mark.parametrize("T_in", [4, 5, 6, 7])
@pytest.mark.parametrize("B,F_enc", [(48, 90), (20, 90), (48, 33), (20, 33)])
def test_steady_loop_seams_around_barrier_2(B, F_enc, T_in, T_out):
    """H 256.  B 48 = three groups on a grid padded to eight, B 20 = a ragged second tile.  F 90: the encoder's steady-state
    loop takes T_in - 3 = 1 .. 4 turns and hands over to the two general tail steps at every x-tile residue (T_in mod 3);
    F 33: the general copy in every encoder step.  The decoder's steady-state loop takes T_out - 2 = 1 .. 3 turns."""
    all_forms(B, T_in, T_out, F_enc)
