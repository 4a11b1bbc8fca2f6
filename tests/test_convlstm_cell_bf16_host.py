"""ConvLSTMSeq2Seq(cell_dtype='bf16') without a GPU: the constructor's and the training entry points' errors, and the yardsticks
tests/test_gpu_convlstm_cell_bf16.py measures the bf16 cell with, checked where it is cheap.

Operator level.  The reference of one step (cell_bf16_ref) is O.convlstm2d_step with O.round_bf16 (round-to-nearest-even) on
x, h, K and R - O.conv2d_same does not go through O._mm, so O.bf16_operands() does not reach it -, bias, gates and cell update
in the arrays' dtype.  The GPU file bounds |gpu - ref| by OP_TOL = 1e-5 of max|ref| per tensor.  Here, over every operator
shape of the GPU file and both activations: the reference on fp32 and on fp64 arrays (identical rounded operands, NumPy's two
accumulations) agrees within 1e-6 of max|ref| - a tenth of the bound -, and each operand mistake the bound has to catch
(weights left unrounded, inputs left unrounded, truncation instead of round-to-nearest-even) moves h and c by at least
10 x the bound.

Model level.  cells_bf16_forward is O.convlstm_seq2seq_forward with the cells' operands rounded, and the head's as well when
the model under test runs a bf16 head.  As tests/test_convlstm_bf16_host.py does for the head: on fp32 and on fp64 arrays it
agrees within HALF of TIGHT, and the fp32 run is within HALF of LOOSE of the full-precision fp64 oracle."""
import functools
import os
import sys

import numpy as np
import pytest

from oracle import fov_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_convlstm_bf16_host import (FULL, FULL_ROWS, LOOSE, SMALL_CASES, TIGHT, conv2d_bf16_ref, f64, full_inputs,  # noqa: E402
                                     full_weights, small_inputs, worst)

OP_TOL = 1e-5           # |gpu - ref| <= OP_TOL * max|ref| per tensor: the head's bound
ACTS = ("hard_sigmoid", "sigmoid")

# (B, H, W, C, F, k).  The patch-resident form: the model's first layer (two k-blocks); C + F = 48 (half-empty second k-block);
# one short k-block with the F = 8 unit split; B 1 with a partial last row group; the transposed map with k 3 and the x | h
# boundary inside a 16-byte bf16 slot; the Conv1D model's map.
PATCH_SHAPES = [(2, 36, 18, 32, 32, 5), (2, 36, 18, 32, 16, 5), (2, 36, 18, 16, 8, 5), (1, 20, 18, 32, 32, 5), (2, 18, 36, 12, 16, 3),
                (3, 1, 30, 4, 32, 5)]
# The plain form: ragged F and C; F no power of two; the dense head's 1 x 1 map; C + F = 72.
PLAIN_SHAPES = [(2, 4, 5, 3, 5, 3), (2, 9, 6, 10, 12, 3), (2, 1, 1, 6, 12, 5), (2, 9, 6, 40, 32, 3)]
MISTAKE_SHAPE = (2, 36, 18, 32, 32, 5)
REGIME_SHAPES = [(2, 12, 18, 32, 32, 5), (2, 9, 6, 12, 8, 3)]
# model-level cases of the GPU file: every small case under both head dtypes and both activations, the cells always bf16
MODEL_CASES = [case + (dtype, act) for case in SMALL_CASES for dtype in ("f32", "bf16") for act in ACTS]


def cell_inputs(seed, B, H, W, C, F, k, extra=0):
    """x N(0,1) (extra more channels for the views the GPU file cuts it from), h = 0.5 N(0,1) clipped to (-1, 1), c = 0.7 N(0,1),
    K Glorot-uniform, R orthogonal, b = 0.05 N(0,1) with the unit forget bias: the Keras initialisers of
    O.init_convlstm_seq2seq."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, H, W, C + extra)).astype(np.float32)
    h = np.clip(0.5 * rng.standard_normal((B, H, W, F)), -1, 1).astype(np.float32)
    c = (0.7 * rng.standard_normal((B, H, W, F))).astype(np.float32)
    lim = np.sqrt(6.0 / (k * k * C + k * k * 4 * F))
    K = rng.uniform(-lim, lim, (k, k, C, 4 * F)).astype(np.float32)
    R = O._orthogonal(rng, k * k * F, 4 * F, np.float32).reshape(k, k, F, 4 * F)
    b = (0.05 * rng.standard_normal(4 * F)).astype(np.float32)
    b[F:2 * F] += 1
    return {"x": x, "h": h, "c": c, "K": K, "R": R, "b": b}


def truncate_bf16(a):
    """Round-toward-zero to bfloat16, in the input's dtype: the rounding the kernels must NOT use."""
    a32 = np.ascontiguousarray(a, dtype=np.float32)
    return (a32.view(np.uint32) & 0xFFFF0000).view(np.float32).astype(np.asarray(a).dtype)


def cell_step(x, h, c, K, R, b, act, rx=O.round_bf16, rw=O.round_bf16):
    """One ConvLSTM2D step with rx on the inputs x, h and rw on the kernels K, R of the two convolutions (the arithmetic
    contract of fov_convlstm_cell_fwd_bf16 with the defaults), everything else in the arrays' dtype -> dict(h, c, gates
    (activated i, f, g, o)).  h None: zero state, K alone; c None: zero cell state; b None: no bias."""
    F = K.shape[3] // 4
    zero = np.zeros(x.shape[:3] + (F,), x.dtype)
    p = {"K": rw(K), "R": rw(R), "act": act}
    r = O.regime_convlstm_reference(p, x.dtype, x=rx(x), b=np.zeros(4 * F, x.dtype) if b is None else b,
                                    h=zero if h is None else rx(h), c=zero if c is None else c)
    return {"h": r["h"], "c": r["c"], "gates": r["gates"]}


def cell_bf16_ref(x, h, c, K, R, b, act):
    return cell_step(x, h, c, K, R, b, act)


def as64(p):
    return {k: v.astype(np.float64) for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def cached_inputs(shape, extra=0):
    return cell_inputs(sum(s * 10 ** i for i, s in enumerate(shape)), *shape, extra=extra)


def cells_bf16_forward(enc_in, dec_in0, w, T_out, head="conv2d", act="hard_sigmoid", head_bf16=True):
    """O.convlstm_seq2seq_forward (heads 'conv2d' / 'conv1d') with bf16-rounded operands in the convolutions of all six
    ConvLSTM2D layers and, with head_bf16, in the three head convolutions."""
    rb = O.round_bf16
    step = lambda x, h, c, n: O.convlstm2d_step(rb(x), rb(h), c, rb(w[n + "_K"]), rb(w[n + "_R"]), w[n + "_b"], act)
    conv = conv2d_bf16_ref if head_bf16 else O.conv2d_same
    B, T_in, H, W, _ = enc_in.shape
    seq = [enc_in[:, t] for t in range(T_in)]
    states = []
    for l in range(3):
        F = w["enc%d_R" % l].shape[2]
        h, c = np.zeros((B, H, W, F), enc_in.dtype), np.zeros((B, H, W, F), enc_in.dtype)
        nxt = []
        for t in range(T_in):
            h, c = step(seq[t], h, c, "enc%d" % l)
            nxt.append(h)
        seq = nxt
        states.append((h, c))
    inp = dec_in0[:, 0]
    outs = []
    for _ in range(T_out):
        feats = []
        cur = inp
        for l in range(3):
            h, c = step(cur, states[l][0], states[l][1], "dec%d" % l)
            states[l] = (h, c)
            feats.append(h)
            cur = h
        y = np.concatenate(feats, axis=-1)
        y = np.maximum(conv(y, w["head0_W"], w["head0_b"]), 0)
        y = np.maximum(conv(y, w["head1_W"], w["head1_b"]), 0)
        y = conv(y, w["head2_W"], w["head2_b"])
        y = O.softmax_last(np.maximum(y, 0) if head == "conv2d" else y)
        outs.append(y)
        inp = y
    return np.stack(outs, axis=1)


def _weights():
    return O.init_convlstm_seq2seq(3, C=10, latent_dim=8, head="conv2d", head_filters=(24, 40))


# ---------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------
def test_cell_dtype_defaults_to_f32_and_rejects_unknown_values():
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    w = _weights()
    assert ConvLSTMSeq2Seq(w).cell_dtype == "f32"
    assert ConvLSTMSeq2Seq(w, dtype="bf16").cell_dtype == "f32"          # dtype does not change the cells
    m = ConvLSTMSeq2Seq(w, cell_dtype="bf16")
    assert (m.dtype, m.cell_dtype) == ("f32", "bf16")                    # and cell_dtype does not change the head
    m = ConvLSTMSeq2Seq(w, dtype="bf16", cell_dtype="bf16")
    assert (m.dtype, m.cell_dtype) == ("bf16", "bf16")
    for bad in ("fp16", "float32", "bfloat16", None):
        with pytest.raises(ValueError, match="cell_dtype"):
            ConvLSTMSeq2Seq(w, cell_dtype=bad)


def test_every_head_accepts_bf16_cells():
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    wc = O.init_convlstm_seq2seq(3, C=3, latent_dim=16, head="conv1d", head_filters=(32, 48))
    assert ConvLSTMSeq2Seq(wc, head="conv1d", cell_dtype="bf16").cell_dtype == "bf16"
    wd = O.init_convlstm_seq2seq(3, C=6, latent_dim=8, head="dense", map_hw=(1, 1))
    assert ConvLSTMSeq2Seq(wd, head="dense", cell_dtype="bf16").cell_dtype == "bf16"
    with pytest.raises(ValueError, match="dense"):                       # the head's own rule is untouched
        ConvLSTMSeq2Seq(wd, head="dense", dtype="bf16", cell_dtype="bf16")


def test_bf16_cells_with_a_dilation_are_rejected():
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    w = _weights()
    assert ConvLSTMSeq2Seq(w, dilation_rate=2).dilation_rate == 2
    assert ConvLSTMSeq2Seq(w, dilation_rate=1, cell_dtype="bf16").dilation_rate == 1
    with pytest.raises(ValueError, match="dilation_rate"):
        ConvLSTMSeq2Seq(w, dilation_rate=2, cell_dtype="bf16")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bf16_cell_model_refuses_to_train_before_any_device_work(dtype):
    """fit, train_on_batch, fit_trajectories and train_on_trajectories of a model with bf16 cells raise NotImplementedError
    from _make_trainer - on a machine without a GPU, so nothing touched the device first - and say what to do instead."""
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    w = O.init_convlstm_seq2seq(3, C=30, latent_dim=8, k=3, head="conv2d", head_filters=(24, 40))
    m = ConvLSTMSeq2Seq(w, head="conv2d", dtype=dtype, cell_dtype="bf16")
    m.compile(optimizer="RMSprop", loss="mean_squared_error")
    maps = np.zeros((2, 2, 36, 18, 30), np.float32)
    xyz = np.zeros((2, 2, 30, 3), np.float32)
    xyz[..., 0] = 1
    calls = [lambda: m.fit([maps, maps[:, -1:]], maps, batch_size=2, epochs=1),
             lambda: m.train_on_batch([maps, maps[:, -1:]], maps),
             lambda: m.fit_trajectories(xyz, xyz[:, -1:], xyz, batch_size=2, epochs=1),
             lambda: m.train_on_trajectories(xyz, xyz[:, -1:], xyz)]
    for call in calls:
        with pytest.raises(NotImplementedError, match=r"f32.*get_weights\(\)"):
            call()
    with pytest.raises(NotImplementedError):
        m._make_trainer("rmsprop")
    got = m.get_weights()
    assert all(a.dtype == np.float32 for a in got)
    m.set_weights(got)


# ---------------------------------------------------------------------------------------
# the operator yardstick: NumPy only
# ---------------------------------------------------------------------------------------
def rel(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", PATCH_SHAPES + PLAIN_SHAPES)
def test_operator_reference_noise_and_the_mistakes_the_bound_must_catch(shape, act):
    p = cached_inputs(shape)
    q = as64(p)
    r64 = cell_bf16_ref(q["x"], q["h"], q["c"], q["K"], q["R"], q["b"], act)
    r32 = cell_bf16_ref(p["x"], p["h"], p["c"], p["K"], p["R"], p["b"], act)
    # the restatement is O.convlstm2d_step on rounded operands
    rb = O.round_bf16
    h_o, c_o = O.convlstm2d_step(rb(q["x"]), rb(q["h"]), q["c"], rb(q["K"]), rb(q["R"]), q["b"], act)
    np.testing.assert_array_equal(r64["h"], h_o)
    np.testing.assert_array_equal(r64["c"], c_o)
    for n in ("h", "c", "gates"):
        assert r32[n].dtype == np.float32 and r64[n].dtype == np.float64
        e = rel(r32[n], r64[n])
        print("%s %s %s: fp32 vs fp64 accumulation %.2e of max|ref|" % (shape, act, n, e))
        assert e <= 0.1 * OP_TOL, (shape, act, n)
    ident = lambda a: a
    wrong = {"weights unrounded": cell_step(q["x"], q["h"], q["c"], q["K"], q["R"], q["b"], act, rw=ident),
             "inputs unrounded": cell_step(q["x"], q["h"], q["c"], q["K"], q["R"], q["b"], act, rx=ident),
             "truncated": cell_step(q["x"], q["h"], q["c"], q["K"], q["R"], q["b"], act, rx=truncate_bf16, rw=truncate_bf16)}
    for name, w in wrong.items():
        for n in ("h", "c"):
            e = rel(w[n], r64[n])
            print("%s %s %s: %s moves it by %.2e of max|ref|" % (shape, act, n, name, e))
            assert e >= 10 * OP_TOL, (shape, act, n, name)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", REGIME_SHAPES)
def test_saturated_regime_reference_noise(shape, act):
    """O.regime_convlstm_cell (R3) on rounded operands: fp32 and fp64 arrays agree within a tenth of both bounds of the GPU test."""
    B, H, W, C, F, k = shape
    p = O.regime_convlstm_cell(40 + C, B, H, W, C, F, k, act)
    r64 = cell_bf16_ref(*[p[n].astype(np.float64) for n in ("x", "h", "c", "K", "R", "b")], act)
    r32 = cell_bf16_ref(*[p[n] for n in ("x", "h", "c", "K", "R", "b")], act)
    for n in ("h", "c", "gates"):
        e, w = rel(r32[n], r64[n]), O.regime_error(r32[n], r64[n], "f32")
        print("regime %s %s %s: %.2e of max|ref|, %.3f of the written bound" % (shape, act, n, e, w))
        assert e <= 0.1 * OP_TOL and w <= 0.1


# ---------------------------------------------------------------------------------------
# the model yardstick: NumPy only
# ---------------------------------------------------------------------------------------
def _check_yardstick(name, enc, dec0, w, T_out, head, act, head_bf16):
    e64, d64 = enc.astype(np.float64), dec0.astype(np.float64)
    r64 = cells_bf16_forward(e64, d64, f64(w), T_out, head, act, head_bf16)
    r32 = cells_bf16_forward(enc, dec0, w, T_out, head, act, head_bf16)
    assert r32.dtype == np.float32 and r64.dtype == np.float64
    full = O.convlstm_seq2seq_forward(e64, d64, f64(w), T_out, head, act)
    t, l = worst(r32, r64, TIGHT), worst(r32, full, LOOSE)
    moved = float(np.abs(r64 - full).max())
    print("%s: fp32 vs fp64 arrays %.3f of TIGHT, fp32 restatement vs fp64 oracle %.3f of LOOSE, rounding moves the output by %.2e"
          % (name, t, l, moved))
    assert t <= 0.5 and l <= 0.5
    assert moved > 0            # the restatement really rounds something


@pytest.mark.parametrize("name,head,B,T_in,T_out,H,W,C,L,hf,seed,dtype,act", MODEL_CASES)
def test_yardstick_small_models(name, head, B, T_in, T_out, H, W, C, L, hf, seed, dtype, act):
    w = O.init_convlstm_seq2seq(seed, C=C, latent_dim=L, head=head, head_filters=hf)
    enc, dec0 = small_inputs(head, B, T_in, H, W, C)
    _check_yardstick("%s, %s head, %s" % (name, dtype, act), enc, dec0, w, T_out, head, act, dtype == "bf16")


def test_yardstick_full_size_two_sequences():
    """configs[3] cut to two of the GPU test's sequences, T 10 -> 10, head 512 -> 1024 -> 30, cells and head in bf16."""
    enc, dec0 = full_inputs(FULL_ROWS[1:3])
    _check_yardstick("configs[3], two sequences, all bf16", enc, dec0, full_weights(), FULL["T"], "conv2d", "hard_sigmoid", True)
