"""The 2- and 3-layer seq2seq model's decode as ONE launch (fov_stacked_seq2seq_decode_fwd, lstm_stacked_s2s.hip) against the
fp64 NumPy oracle (oracle.fov_oracle.stacked_seq2seq_forward: Fov_seq2seq_2layers.py:360-430, batched).

Bounds - the project's written ones against the fp64 oracle, for outputs and for every layer's final state:
    |gpu - ref| <= 1e-3 |ref| + 1e-5 per element   AND   max |gpu - ref| <= 2e-5.
The oracle run on fp32 arrays stays within 1.2e-7 of its fp64 run at every shape below (T 64 -> 64 included), so fp32 arithmetic
sits two orders of magnitude inside the bound.  The fused call and the host loop are two kernels each within 2e-5 of the same
oracle: they agree within 4e-5.  Shapes: ragged and whole tiles, one sequence, one step, every input k-block count with a
partial last block, both run widths, both depths, padded model widths below 32 and between 32 and 64."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def f64(w):
    return {k: v.astype(np.float64) for k, v in w.items()}


def _weights(L, H, F_enc, F_dec=6, seed=None):
    """As tests/test_gpu_train.py::test_stacked_seq2seq_layers builds them."""
    rng = np.random.default_rng(L * 1000 + H + 7 * F_enc if seed is None else seed)
    w = {}
    for side, f0 in (("enc", F_enc), ("dec", F_dec)):
        for l in range(L):
            k_, r_, b_ = O.init_lstm(rng, f0 if l == 0 else H, H)
            w["%s%d_K" % (side, l)], w["%s%d_R" % (side, l)] = k_, r_
            w["%s%d_b" % (side, l)] = (b_ + 0.1 * rng.standard_normal(4 * H)).astype(np.float32)
    w["dense_W"] = rng.uniform(-0.3, 0.3, (H, F_dec)).astype(np.float32)
    w["dense_b"] = rng.uniform(-0.1, 0.1, F_dec).astype(np.float32)
    return w


def _inputs(F_enc, B, T_in, T_out):
    """enc (B,T_in,F_enc), dec0 (B,1,6) from O.synthetic_batch: F = 6 is the scripts' (mu, var) second, 90 the raw second,
    3 its first frame, 96 both side by side."""
    enc90, dec0, _ = O.synthetic_batch(31 + B, max(B, 1), max(T_in, 1), max(T_out, 1))
    enc90, dec0 = enc90[:B, :T_in], dec0[:B]
    mv = O.meanvar_xyz(enc90.astype(np.float64)).astype(np.float32) if T_in and B else np.zeros((B, T_in, 6), np.float32)
    enc = {6: mv, 90: enc90, 3: enc90[:, :, :3], 96: np.concatenate([enc90, mv], axis=-1)}[F_enc]
    return np.ascontiguousarray(enc, dtype=np.float32), np.ascontiguousarray(dec0, dtype=np.float32)


def _oracle(enc, dec0, w, L, act, T_out):
    """stacked_seq2seq_forward's autoregressive branch, keeping every layer's state -> (y (B,T_out,O), hT, cT (L,B,H)), fp64."""
    enc, dec0, w = enc.astype(np.float64), dec0.astype(np.float64), f64(w)
    states, inp = [], enc
    for l in range(L):
        inp, h, c = O.lstm_layer(inp, w["enc%d_K" % l], w["enc%d_R" % l], w["enc%d_b" % l], act=act)
        states.append([h, c])
    x, out = dec0[:, 0], []
    for _ in range(T_out):
        for l in range(L):
            states[l] = list(O.lstm_step(x, states[l][0], states[l][1], w["dec%d_K" % l], w["dec%d_R" % l], w["dec%d_b" % l], act))
            x = states[l][0]
        x = O.dense(x, w["dense_W"], w["dense_b"])
        out.append(x)
    y = np.stack(out, axis=1) if out else np.zeros((enc.shape[0], 0, dec0.shape[2]))
    if T_out:
        np.testing.assert_array_equal(y, O.stacked_seq2seq_forward(enc, dec0, w, L, act, T_out=T_out))
    return y, np.stack([s[0] for s in states]), np.stack([s[1] for s in states])


@functools.lru_cache(maxsize=None)
def _case(L, H, F_enc, B, T_in, T_out, act):
    """One case's weights, inputs and fp64 reference, computed once and shared (nobody writes into them)."""
    w = _weights(L, H, F_enc)
    enc, dec0 = _inputs(F_enc, B, T_in, T_out)
    ref = _oracle(enc, dec0, w, L, act, T_out)
    for a in list(w.values()) + [enc, dec0] + list(ref):
        a.setflags(write=False)
    return w, enc, dec0, ref


def _held(tag, got, ref):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float(err.max()) if err.size else 0.0
    print("%s: max |gpu - fp64 oracle| %.3e" % (tag, worst))
    assert (err <= 1e-3 * np.abs(ref) + 1e-5).all() and worst <= 2e-5, (tag, worst)


def _run(w, enc, dec0, L, T_out, act, states=False, **kw):
    from longterm360fov_amd import ops
    dw = {k: dev(v) for k, v in w.items()}
    B, H = enc.shape[0], w["enc0_R"].shape[0]
    hT = torch.full((L, B, H), 7.0, device="cuda") if states else None
    cT = torch.full((L, B, H), 7.0, device="cuda") if states else None
    y = ops.stacked_seq2seq_decode(dev(enc), dev(dec0), dw, L, T_out, act=act, hT=hT, cT=cT, **kw)
    torch.cuda.synchronize()
    return (y.cpu().numpy(), hT.cpu().numpy(), cT.cpu().numpy()) if states else y.cpu().numpy()


PARITY = [(2, 32, 6, 17, 5, 5, "sigmoid"),          # ragged second tile
          (3, 64, 90, 33, 4, 5, "hard_sigmoid"),    # three tiles, six input k-blocks (the last partial), K_0 resident in LDS
          (2, 64, 3, 16, 3, 2, "sigmoid"),          # F_enc not a multiple of 4, exactly one tile
          (3, 32, 96, 1, 2, 3, "sigmoid"),          # one sequence, the widest input
          (2, 32, 90, 64, 10, 10, "hard_sigmoid"),  # the scripts' batch and lengths
          (2, 64, 6, 5, 1, 1, "sigmoid")]           # one step each


@pytest.mark.parametrize("L,H,F_enc,B,T_in,T_out,act", PARITY)
def test_parity_through_the_c_abi(L, H, F_enc, B, T_in, T_out, act):
    w, enc, dec0, (y_ref, h_ref, c_ref) = _case(L, H, F_enc, B, T_in, T_out, act)
    y, hT, cT = _run(w, enc, dec0, L, T_out, act, states=True)
    tag = "L%d H%d F%d B%d T%d->%d %s" % (L, H, F_enc, B, T_in, T_out, act)
    _held(tag + " out", y, y_ref)
    _held(tag + " hT", hT, h_ref)
    _held(tag + " cT", cT, c_ref)
    np.testing.assert_array_equal(_run(w, enc, dec0, L, T_out, act), y)      # without the optional outputs: the same result


@pytest.mark.parametrize("H", [20, 40, 64])
@pytest.mark.parametrize("L", [2, 3])
def test_padded_widths_through_the_model(L, H):
    """latent_dim 20 runs at width 32, 40 at 64: decode_sequence against the oracle at the model's OWN width, and against the
    host loop (FOV_NO_STACKED_DECODE=1; the wrapper re-reads the library's knobs when the environment changed)."""
    from longterm360fov_amd.models import StackedSeq2SeqLSTM
    from longterm360fov_amd.training import stacked_weight_order
    B, T_in, T_out, act = 21, 3, 4, "sigmoid"
    w, enc, dec0, (y_ref, _, _) = _case(L, H, 6, B, T_in, T_out, act)
    m = StackedSeq2SeqLSTM(num_encoder_tokens=6, latent_dim=H, num_layers=L, recurrent_activation=act)
    m.set_weights([w[k] for k in stacked_weight_order(L)])
    assert "FOV_NO_STACKED_DECODE" not in os.environ
    fused = m.decode_sequence(enc, dec0, predict_step=T_out)
    os.environ["FOV_NO_STACKED_DECODE"] = "1"
    try:
        loop = m.decode_sequence(enc, dec0, predict_step=T_out)
    finally:
        del os.environ["FOV_NO_STACKED_DECODE"]
    _held("model L%d H%d fused" % (L, H), fused, y_ref)
    _held("model L%d H%d host loop" % (L, H), loop, y_ref)
    d = float(np.abs(fused - loop).max())
    print("model L%d H%d: fused vs host loop %.3e" % (L, H, d))
    assert d <= 4e-5
    np.testing.assert_array_equal(m.decode_sequence(enc, dec0, predict_step=T_out), fused)      # the knob is off again


def test_no_encoder_steps_start_the_decoder_from_zero_states():
    L, H, B, T_out = 3, 32, 17, 4
    w, enc, dec0, (y_ref, h_ref, c_ref) = _case(L, H, 6, B, 0, T_out, "sigmoid")
    assert enc.shape == (B, 0, 6)
    y, hT, cT = _run(w, enc, dec0, L, T_out, "sigmoid", states=True)
    _held("T_in 0 out", y, y_ref)
    _held("T_in 0 hT", hT, h_ref)
    _held("T_in 0 cT", cT, c_ref)


def test_no_decoder_steps_run_the_encoder_stack_alone():
    """T_out = 0: `out` is not written (a zero-length view inside a canary-filled buffer), hT / cT are the encoder stack's
    final states (O.lstm_layer, layer on layer)."""
    L, H, B, T_in = 2, 64, 17, 3
    w, enc, dec0, _ = _case(L, H, 6, B, T_in, 0, "hard_sigmoid")
    buf = torch.full((B * 2 * 6 + 64,), -3.0, device="cuda")
    out = buf[32:32].reshape(B, 0, 6)
    y, hT, cT = _run(w, enc, dec0, L, 0, "hard_sigmoid", states=True, out=out)
    assert y.shape == (B, 0, 6) and bool((buf == -3.0).all())
    inp, wd = enc.astype(np.float64), f64(w)
    for l in range(L):
        inp, h, c = O.lstm_layer(inp, wd["enc%d_K" % l], wd["enc%d_R" % l], wd["enc%d_b" % l], act="hard_sigmoid")
        _held("T_out 0 hT layer %d" % l, hT[l], h)
        _held("T_out 0 cT layer %d" % l, cT[l], c)


def test_empty_batch_launches_nothing():
    from longterm360fov_amd import ops
    from longterm360fov_amd.models import StackedSeq2SeqLSTM
    w = _case(2, 32, 6, 17, 5, 5, "sigmoid")[0]
    y = ops.stacked_seq2seq_decode(torch.empty((0, 5, 6), device="cuda"), torch.empty((0, 1, 6), device="cuda"),
                                   {k: dev(v) for k, v in w.items()}, 2, 7)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (0, 7, 6)
    m = StackedSeq2SeqLSTM(num_encoder_tokens=6, latent_dim=32, num_layers=2)
    got = m.decode_sequence(np.zeros((0, 5, 6), np.float32), np.zeros((0, 1, 6), np.float32), predict_step=7)
    assert got.shape == (0, 7, 6) and got.dtype == np.float32


def test_output_view_between_canaries_stays_inside():
    """B = 17: the second tile holds one live row; the 15 padded rows store nothing past the end of `out` (nor before it)."""
    L, H, F_enc, B, T_in, T_out, act = 2, 32, 6, 17, 5, 5, "sigmoid"
    w, enc, dec0, (y_ref, h_ref, _) = _case(L, H, F_enc, B, T_in, T_out, act)
    pad, n = 16 * T_out * 6 + 64, B * T_out * 6
    buf = torch.full((n + 2 * pad,), -3.0, device="cuda")
    sbuf = torch.full((2, L * B * H + 2 * 16 * H,), -3.0, device="cuda")
    views = [sbuf[i, 16 * H:16 * H + L * B * H].reshape(L, B, H) for i in range(2)]
    from longterm360fov_amd import ops
    y = ops.stacked_seq2seq_decode(dev(enc), dev(dec0), {k: dev(v) for k, v in w.items()}, L, T_out, act=act,
                                   out=buf[pad:pad + n].reshape(B, T_out, 6), hT=views[0], cT=views[1])
    torch.cuda.synchronize()
    assert y.data_ptr() == buf[pad:].data_ptr()
    _held("view out", y.cpu().numpy(), y_ref)
    _held("view hT", views[0].cpu().numpy(), h_ref)
    assert bool((buf[:pad] == -3.0).all()) and bool((buf[pad + n:] == -3.0).all())
    assert bool((sbuf[:, :16 * H] == -3.0).all()) and bool((sbuf[:, 16 * H + L * B * H:] == -3.0).all())


def test_exact_properties():
    """A row's result depends on nothing but its own sequence: repeatable, permutation-equivariant, independent of its
    tile-mates and of its place in the batch - all bit for bit."""
    L, H, F_enc, B, T_in, T_out, act = 3, 64, 90, 33, 4, 5, "hard_sigmoid"
    w, enc, dec0, _ = _case(L, H, F_enc, B, T_in, T_out, act)
    y, hT, cT = _run(w, enc, dec0, L, T_out, act, states=True)
    y2, hT2, cT2 = _run(w, enc, dec0, L, T_out, act, states=True)
    for a, b in ((y, y2), (hT, hT2), (cT, cT2)):
        np.testing.assert_array_equal(a, b)
    perm = np.random.default_rng(5).permutation(B)
    yp, hTp, _ = _run(w, enc[perm], dec0[perm], L, T_out, act, states=True)
    np.testing.assert_array_equal(yp, y[perm])
    np.testing.assert_array_equal(hTp, hT[:, perm])
    np.testing.assert_array_equal(_run(w, enc[:16], dec0[:16], L, T_out, act), y[:16])
    np.testing.assert_array_equal(_run(w, enc[32:33], dec0[32:33], L, T_out, act), y[32:33])


@pytest.mark.parametrize("L,H,F_enc,act", [(2, 64, 90, "sigmoid"), (3, 32, 6, "hard_sigmoid")])
def test_long_run(L, H, F_enc, act):
    """T 64 -> 64 (the oracle's own fp32-vs-fp64 distance here: 1.1e-7 / 4.5e-8): the same bounds, outputs inside (-1, 1),
    bitwise repeatable."""
    B, T = 16, 64
    w, enc, dec0, (y_ref, h_ref, c_ref) = _case(L, H, F_enc, B, T, T, act)
    y, hT, cT = _run(w, enc, dec0, L, T, act, states=True)
    _held("long L%d H%d out" % (L, H), y, y_ref)
    _held("long L%d H%d hT" % (L, H), hT, h_ref)
    _held("long L%d H%d cT" % (L, H), cT, c_ref)
    assert np.isfinite(y).all() and float(np.abs(y).max()) < 1.0
    np.testing.assert_array_equal(_run(w, enc, dec0, L, T, act), y)


def test_decode_sequence_is_one_launch(monkeypatch):
    """With the per-layer and Dense wrappers made to raise, the 32-wide two-layer model still decodes (the one-launch call
    needs neither); at latent_dim 128 the host loop is still the path, and the same patch raises."""
    from longterm360fov_amd import ops
    from longterm360fov_amd.models import StackedSeq2SeqLSTM
    from longterm360fov_amd.training import stacked_weight_order
    L, H, B, T_in, T_out, act = 2, 32, 17, 5, 5, "sigmoid"
    w, enc, dec0, (y_ref, _, _) = _case(L, H, 6, B, T_in, T_out, act)

    def boom(*a, **k):
        raise AssertionError("a per-step launch")
    monkeypatch.setattr(ops, "lstm_seq", boom)
    monkeypatch.setattr(ops, "dense", boom)
    m = StackedSeq2SeqLSTM(num_encoder_tokens=6, latent_dim=H, num_layers=L, recurrent_activation=act)
    m.set_weights([w[k] for k in stacked_weight_order(L)])
    _held("one launch", m.decode_sequence(enc, dec0, predict_step=T_out), y_ref)
    wide = StackedSeq2SeqLSTM(num_encoder_tokens=6, latent_dim=128, num_layers=L, recurrent_activation=act)
    with pytest.raises(AssertionError, match="a per-step launch"):
        wide.decode_sequence(enc, dec0, predict_step=T_out)


def test_weights_set_later_reach_the_padded_copy():
    """The padded weights are cached beside the device weights: set_weights must drop them."""
    from longterm360fov_amd.models import StackedSeq2SeqLSTM
    from longterm360fov_amd.training import stacked_weight_order
    L, H, B, T_in, T_out, act = 2, 20, 21, 3, 4, "sigmoid"
    w, enc, dec0, (y_ref, _, _) = _case(L, H, 6, B, T_in, T_out, act)
    m = StackedSeq2SeqLSTM(num_encoder_tokens=6, latent_dim=H, num_layers=L, recurrent_activation=act, seed=3)
    first = m.decode_sequence(enc, dec0, predict_step=T_out)
    m.set_weights([w[k] for k in stacked_weight_order(L)])
    got = m.decode_sequence(enc, dec0, predict_step=T_out)
    _held("after set_weights", got, y_ref)
    assert float(np.abs(got - first).max()) > 1e-3


def test_first_step_against_the_teacher_forced_graph():
    """decode_sequence(predict_step=1) and predict([enc, dec0]) are the same mathematics on two kernels, each within 2e-5 of
    the oracle."""
    from longterm360fov_amd.models import StackedSeq2SeqLSTM
    from longterm360fov_amd.training import stacked_weight_order
    for L, H in ((2, 32), (3, 64)):
        w, enc, dec0, _ = _case(L, H, 6, 21, 3, 4, "sigmoid")
        m = StackedSeq2SeqLSTM(num_encoder_tokens=6, latent_dim=H, num_layers=L, recurrent_activation="sigmoid")
        m.set_weights([w[k] for k in stacked_weight_order(L)])
        a, b = m.decode_sequence(enc, dec0, predict_step=1), m.predict([enc, dec0])
        assert a.shape == b.shape == (21, 1, 6)
        assert float(np.abs(a - b).max()) <= 4e-5


@pytest.mark.parametrize("L,H,F_enc,F_dec", [(2, 128, 6, 6), (1, 32, 6, 6), (4, 32, 6, 6), (2, 32, 6, 9), (2, 64, 97, 6)])
def test_unsupported_shapes_are_refused_before_any_launch(L, H, F_enc, F_dec):
    from longterm360fov_amd import _lib, ops
    w = {k: dev(v) for k, v in _weights(L, H, F_enc, F_dec, seed=1).items()}
    B, T_in, T_out = 5, 2, 2
    assert not ops.stacked_seq2seq_decode_supported(B, T_in, T_out, F_enc, F_dec, H, L)
    out = torch.full((B, T_out, F_dec), -3.0, device="cuda")
    with pytest.raises(ops.FovError) as e:
        ops.stacked_seq2seq_decode(torch.zeros((B, T_in, F_enc), device="cuda"), torch.zeros((B, 1, F_dec), device="cuda"), w, L, T_out, out=out)
    torch.cuda.synchronize()
    assert e.value.code == _lib.ERR_UNSUPPORTED and "fov_stacked_seq2seq_decode_fwd" in str(e.value)
    assert bool((out == -3.0).all())
