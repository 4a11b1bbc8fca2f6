"""The target-only seq2seq model with bf16 matrix-core operands (fov_seq2seq_decode_fwd_bf16, fov_dense_fwd_bf16, the bf16
Seq2SeqTrainer and Seq2SeqLSTM(dtype='bf16')), through the C ABI.

Tolerances are tests/test_gpu_bf16.py's: TIGHT against the bf16-operand restatement (oracle/fov_oracle.py under
bf16_operands(): the encoder gates, the decoder gates and the Dense head round both operands to bf16), LOOSE against the
full-precision one.  O.seq2seq_decode does not round the Dense head's operands, so the bf16-operand reference is composed
here from O.lstm_layer, O.lstm_step and O.dense(..., matrix_core=True).
"""
import os
import tempfile

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

pytestmark = pytest.mark.gpu

TIGHT = 1e-3     # vs the bf16-operand restatement
LOOSE = 5e-3     # vs the full-precision restatement
_W_ORDER = ("enc_K", "enc_R", "enc_b", "dec_K", "dec_R", "dec_b", "dense_W", "dense_b")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def devw(w):
    return {k: dev(v) for k, v in w.items()}


def f64(w):
    return {k: v.astype(np.float64) for k, v in w.items()}


def weights(seed, F_enc, F_dec, H=256):
    return O.init_seq2seq(seed, F_enc=F_enc, F_dec=F_dec, H=H, bias_noise=0.1)


def inputs(seed, B, T_in, F_enc, F_dec):
    rng = np.random.default_rng(seed)
    enc = rng.uniform(-1, 1, (B, T_in, F_enc)).astype(np.float32)
    dec0 = rng.uniform(-0.5, 0.5, (B, 1, F_dec)).astype(np.float32)
    return enc, dec0


def ref_decode_bf16(enc, dec0, w, T_out, act):
    """fp64 restatement of the bf16 fused call: every product with x or h on its left sees bf16 operands."""
    w = f64(w)
    with O.bf16_operands():
        _, h, c = O.lstm_layer(enc.astype(np.float64), w["enc_K"], w["enc_R"], w["enc_b"], act=act)
        y = dec0[:, 0].astype(np.float64)
        out = []
        for _ in range(T_out):
            h, c = O.lstm_step(y, h, c, w["dec_K"], w["dec_R"], w["dec_b"], act)
            y = O.dense(h, w["dense_W"], w["dense_b"], matrix_core=True)
            out.append(y)
    return np.stack(out, axis=1) if out else np.zeros((enc.shape[0], 0, dec0.shape[2])), h, c


def ref_decode_f64(enc, dec0, w, T_out, act):
    return O.seq2seq_decode(enc.astype(np.float64), dec0.astype(np.float64), f64(w), T_out, act)


@pytest.mark.parametrize("B,T_in,T_out,F_enc,F_dec,act", [
    (1, 1, 1, 90, 6, "sigmoid"),
    (37, 5, 4, 33, 3, "hard_sigmoid"),
    (16 * 32 + 9, 30, 30, 256, 6, "sigmoid"),       # two tile rounds on 256 CUs, ragged last tile
    (37, 30, 1, 256, 3, "sigmoid"),
    (16 * 32 + 9, 1, 4, 33, 6, "hard_sigmoid"),
    (1, 5, 30, 90, 3, "hard_sigmoid"),
    (37, 5, 30, 90, 6, "sigmoid"),
    (37, 5, 4, 130, 6, "hard_sigmoid"),              # F_enc > 96, not a multiple of 4: element-wise x staging
])
def test_fused_bf16_decode_matches_oracles(B, T_in, T_out, F_enc, F_dec, act):
    from longterm360fov_amd import ops
    w = weights(100 + F_enc + F_dec, F_enc, F_dec)
    enc, dec0 = inputs(B * 7 + T_in * 3 + T_out, B, T_in, F_enc, F_dec)
    ws = ops.Workspace()
    hT = torch.empty((B, 256), device="cuda")
    cT = torch.empty((B, 256), device="cuda")
    out = ops.seq2seq_decode(dev(enc), dev(dec0), devw(w), T_out, act=act, workspace=ws, hT=hT, cT=cT, dtype="bf16")
    ws.check()
    got = out.cpu().numpy()
    assert got.shape == (B, T_out, F_dec)
    ref_t, rh, rc = ref_decode_bf16(enc, dec0, w, T_out, act)
    ref_l = ref_decode_f64(enc, dec0, w, T_out, act)
    e_t = np.abs(got - ref_t).max()
    e_l = np.abs(got - ref_l).max()
    e_h = max(np.abs(hT.cpu().numpy() - rh).max(), np.abs(cT.cpu().numpy() - rc).max() / max(1.0, np.abs(rc).max()))
    print("bf16 fused B=%d T %d->%d F %d/%d %s: vs bf16-operand oracle %.2e (state %.2e), vs fp64 oracle %.2e"
          % (B, T_in, T_out, F_enc, F_dec, act, e_t, e_h, e_l))
    assert np.isfinite(got).all()
    assert e_t <= TIGHT and e_h <= TIGHT and e_l <= LOOSE


def test_fused_bf16_decode_at_config1_shape():
    """configs[1]: B 1024, T 30 -> 30, H 256.  64 sequences against both oracles; all 1024 repeatable bit for bit,
    equivariant under a batch permutation, finite, inside (-1, 1), and within LOOSE of the fp32 fused call."""
    from longterm360fov_amd import ops
    B, T_in, T_out, act = 1024, 30, 30, "sigmoid"
    w = O.init_seq2seq(11, H=256, bias_noise=0.05)
    enc, dec0, _ = O.synthetic_batch(12, B, T_in, T_out)
    dw = devw(w)
    ws = ops.Workspace()
    a = ops.seq2seq_decode(dev(enc), dev(dec0), dw, T_out, act=act, workspace=ws, dtype="bf16").cpu().numpy()
    b = ops.seq2seq_decode(dev(enc), dev(dec0), dw, T_out, act=act, workspace=ws, dtype="bf16").cpu().numpy()
    perm = np.random.default_rng(13).permutation(B)
    c = ops.seq2seq_decode(dev(enc[perm]), dev(dec0[perm]), dw, T_out, act=act, workspace=ws, dtype="bf16").cpu().numpy()
    f = ops.seq2seq_decode(dev(enc), dev(dec0), dw, T_out, act=act, workspace=ws).cpu().numpy()
    ws.check()
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a[perm], c)
    assert np.isfinite(a).all() and np.abs(a).max() < 1.0
    n = 64
    ref_t, _, _ = ref_decode_bf16(enc[:n], dec0[:n], w, T_out, act)
    ref_l = ref_decode_f64(enc[:n], dec0[:n], w, T_out, act)
    e_t, e_l, e_f = np.abs(a[:n] - ref_t).max(), np.abs(a[:n] - ref_l).max(), np.abs(a - f).max()
    print("bf16 fused configs[1]: vs bf16-operand oracle %.2e, vs fp64 oracle %.2e, vs fp32 fused call %.2e" % (e_t, e_l, e_f))
    assert e_t <= TIGHT and e_l <= LOOSE and e_f <= LOOSE


@pytest.mark.parametrize("B,T_in,F_enc", [(37, 5, 90), (16 * 32 + 9, 3, 256), (21, 1, 33)])
def test_encoder_only_state_equals_bf16_layer(B, T_in, F_enc):
    """T_out = 0: the fused call runs the encoder alone; its final state is fov_lstm_seq_fwd_bf16's bit for bit."""
    from longterm360fov_amd import ops
    w = weights(7, F_enc, 6)
    enc, dec0 = inputs(8 + B, B, T_in, F_enc, 6)
    dw = devw(w)
    ws = ops.Workspace()
    hT = torch.full((B, 256), 3.0, device="cuda")
    cT = torch.full((B, 256), 3.0, device="cuda")
    out = ops.seq2seq_decode(dev(enc), dev(dec0), dw, 0, workspace=ws, hT=hT, cT=cT, dtype="bf16")
    _, lh, lc, _ = ops.lstm_seq_bf16(dev(enc), dw["enc_K"], dw["enc_R"], dw["enc_b"], workspace=ws, reserve=False)
    ws.check()
    assert out.shape == (B, 0, 6)
    assert torch.equal(hT, lh) and torch.equal(cT, lc)


@pytest.mark.parametrize("act", ["sigmoid", "hard_sigmoid"])
def test_fused_bf16_decode_equals_host_stepped_composition(act):
    """The fused call equals lstm_seq_bf16 (one step per call, the state fed back) followed by dense_bf16, the output fed
    back as the next input - bit for bit, outputs and final state."""
    from longterm360fov_amd import ops
    B, T_in, T_out, F_enc, F_dec = 37, 5, 4, 90, 6
    w = weights(21, F_enc, F_dec)
    enc, dec0 = inputs(22, B, T_in, F_enc, F_dec)
    dw = devw(w)
    ws = ops.Workspace()
    hT = torch.empty((B, 256), device="cuda")
    cT = torch.empty((B, 256), device="cuda")
    fused = ops.seq2seq_decode(dev(enc), dev(dec0), dw, T_out, act=act, workspace=ws, hT=hT, cT=cT, dtype="bf16")
    _, h, c, _ = ops.lstm_seq_bf16(dev(enc), dw["enc_K"], dw["enc_R"], dw["enc_b"], act=act, workspace=ws, reserve=False)
    x = dev(dec0)
    outs = []
    for _ in range(T_out):
        hs, h, c, _ = ops.lstm_seq_bf16(x, dw["dec_K"], dw["dec_R"], dw["dec_b"], h, c, act=act, workspace=ws, reserve=False)
        y = ops.dense_bf16(hs, dw["dense_W"], dw["dense_b"], activation="tanh")     # (B,1,F_dec)
        outs.append(y)
        x = y.contiguous()
    ws.check()
    stepped = torch.cat(outs, dim=1)
    assert torch.equal(fused, stepped), float((fused - stepped).abs().max())
    assert torch.equal(hT, h) and torch.equal(cT, c)


def test_dense_bf16_matches_bf16_operand_oracle():
    from longterm360fov_amd import ops
    rng = np.random.default_rng(3)
    for N, In, Out, act in ((1, 256, 6, "tanh"), (37, 256, 3, None), (100, 90, 16, "tanh")):
        x = rng.uniform(-1, 1, (N, In)).astype(np.float32)
        W = (0.2 * rng.standard_normal((In, Out))).astype(np.float32)
        b = (0.1 * rng.standard_normal(Out)).astype(np.float32)
        y = ops.dense_bf16(dev(x), dev(W), dev(b), activation=act).cpu().numpy()
        with O.bf16_operands():
            r = O.dense(x.astype(np.float64), W.astype(np.float64), b.astype(np.float64), activation=act, matrix_core=True)
        assert np.abs(y - r).max() <= 1e-5 * max(1.0, np.abs(r).max()), (N, In, Out, np.abs(y - r).max())


def test_resident_limit_forces_more_rounds_without_changing_output():
    """FOV_DBG_RESIDENT_LIMIT: fewer CUs -> fewer groups of eight workgroups and more tile rounds; same output bit for bit.
    Fewer CUs than one group: refused as unsupported."""
    from longterm360fov_amd import _lib, ops
    B, T_in, T_out = 16 * 9 + 5, 4, 3
    w = weights(31, 90, 6)
    enc, dec0 = inputs(32, B, T_in, 90, 6)
    dw = devw(w)
    ws = ops.Workspace()
    full = ops.seq2seq_decode(dev(enc), dev(dec0), dw, T_out, workspace=ws, dtype="bf16")
    ws.check()
    try:
        os.environ["FOV_DBG_RESIDENT_LIMIT"] = "24"     # 3 groups for 10 tiles: four rounds
        lim = ops.seq2seq_decode(dev(enc), dev(dec0), dw, T_out, workspace=ws, dtype="bf16")
        ws.check()
        os.environ["FOV_DBG_RESIDENT_LIMIT"] = "4"      # < one group
        with pytest.raises(_lib.FovError) as ei:
            ops.seq2seq_decode(dev(enc), dev(dec0), dw, T_out, workspace=ws, dtype="bf16")
        assert ei.value.code == _lib.ERR_UNSUPPORTED
    finally:
        os.environ.pop("FOV_DBG_RESIDENT_LIMIT", None)
        ops._sync_env()
    assert torch.equal(full, lim)
    again = ops.seq2seq_decode(dev(enc), dev(dec0), dw, T_out, workspace=ws, dtype="bf16")
    ws.check()
    assert torch.equal(full, again)


def test_empty_batch_launches_nothing_and_empty_encoder_starts_from_zero_state():
    from longterm360fov_amd import ops
    w = weights(41, 90, 6)
    dw = devw(w)
    ws = ops.Workspace()
    enc, dec0 = inputs(42, 37, 4, 90, 6)
    ops.seq2seq_decode(dev(enc), dev(dec0), dw, 3, workspace=ws, dtype="bf16")
    ws.check()
    hdr0 = ws.buf[:16].cpu().numpy().view(np.uint32).copy()
    empty = ops.seq2seq_decode(dev(enc[:0]), dev(dec0[:0]), dw, 3, workspace=ws, dtype="bf16")
    torch.cuda.synchronize()
    assert empty.shape == (0, 3, 6)
    np.testing.assert_array_equal(ws.buf[:16].cpu().numpy().view(np.uint32), hdr0)   # no launch: epoch and launch count unchanged
    # T_in = 0: the decoder from a zero state
    for act in ("sigmoid", "hard_sigmoid"):
        e0 = enc[:, :0]
        out = ops.seq2seq_decode(dev(e0), dev(dec0), dw, 5, act=act, workspace=ws, dtype="bf16").cpu().numpy()
        ws.check()
        ref_t, _, _ = ref_decode_bf16(e0, dec0, w, 5, act)
        ref_l = ref_decode_f64(e0, dec0, w, 5, act)
        assert np.abs(out - ref_t).max() <= TIGHT and np.abs(out - ref_l).max() <= LOOSE


def test_unsupported_shapes_and_short_workspace():
    from longterm360fov_amd import _lib, ops
    enc, dec0 = inputs(51, 5, 3, 90, 6)
    ws = ops.Workspace()
    for H, F_enc, F_dec in ((128, 90, 6), (256, 300, 6), (256, 90, 9)):
        w = O.init_seq2seq(52, F_enc=F_enc, F_dec=F_dec, H=H)
        e, d = inputs(53, 5, 3, F_enc, F_dec)
        with pytest.raises(_lib.FovError) as ei:
            ops.seq2seq_decode(dev(e), dev(d), devw(w), 2, workspace=ws, dtype="bf16")
        assert ei.value.code == _lib.ERR_UNSUPPORTED, (H, F_enc, F_dec)
    with pytest.raises(_lib.FovError) as ei:
        ops.dense_bf16(dev(np.zeros((4, 300))), dev(np.zeros((300, 6))), dev(np.zeros(6)))
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        ops.seq2seq_decode(dev(enc), dev(dec0), devw(weights(54, 90, 6)), 2, workspace=ws, dtype="fp16")
    # a workspace shorter than header + granule area
    w = devw(weights(55, 90, 6))
    out = torch.empty((5, 2, 6), device="cuda")
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    L = _lib.lib()
    rc = L.fov_seq2seq_decode_fwd_bf16(dev(enc).data_ptr(), dev(dec0).data_ptr(), *[w[k].data_ptr() for k in _W_ORDER],
                                       out.data_ptr(), None, None, 5, 3, 2, 90, 6, 256, 0, buf.data_ptr(), buf.numel(),
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == _lib.ERR_WORKSPACE


def test_poisoned_workspace_is_fail_stop_and_sticky():
    """A set timeout word: the bf16 fused call skips its body (outputs untouched), check() reports ERR_TIMEOUT once and
    clears it, after which the workspace works again (the word is set by hand, as a give-up leaves it)."""
    from longterm360fov_amd import _lib, ops
    w = weights(61, 90, 6)
    enc, dec0 = inputs(62, 40, 5, 90, 6)
    dw = devw(w)
    ws = ops.Workspace()
    good = ops.seq2seq_decode(dev(enc), dev(dec0), dw, 4, workspace=ws, dtype="bf16").cpu().numpy()
    ws.check()
    ws.buf[:4] = torch.tensor([1, 0, 0, 0], dtype=torch.uint8, device="cuda")
    out = torch.full((40, 4, 6), 7.0, dtype=torch.float32, device="cuda")
    hT = torch.full((40, 256), 7.0, dtype=torch.float32, device="cuda")
    ops.seq2seq_decode(dev(enc), dev(dec0), dw, 4, workspace=ws, out=out, hT=hT, dtype="bf16")
    ops.seq2seq_decode(dev(enc), dev(dec0), dw, 4, workspace=ws, out=out, hT=hT, dtype="bf16")
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0
    assert float(hT.min()) == 7.0 and float(hT.max()) == 7.0
    with pytest.raises(_lib.FovError) as ei:
        ws.check()
    assert ei.value.code == _lib.ERR_TIMEOUT
    ws.check()
    again = ops.seq2seq_decode(dev(enc), dev(dec0), dw, 4, workspace=ws, dtype="bf16").cpu().numpy()
    ws.check()
    np.testing.assert_array_equal(again, good)


def _batch(seed, B, T_in, T_out):
    enc, dec0, tgt = O.synthetic_batch(seed, B, T_in, T_out)
    return enc, np.concatenate([dec0, tgt[:, :-1]], axis=1), tgt


@pytest.mark.parametrize("act", ["sigmoid", "hard_sigmoid"])
def test_bf16_trainer_matches_fp64_oracle(act):
    from longterm360fov_amd import ops
    from longterm360fov_amd.training import Seq2SeqTrainer
    B, T_in, T_out = 40, 6, 5
    w = O.init_seq2seq(71, H=256, bias_noise=0.1)
    enc, dec_in, tgt = _batch(72, B, T_in, T_out)
    loss_ref, g_ref, _ = O.seq2seq_loss_and_grads(enc.astype(np.float64), dec_in.astype(np.float64), tgt.astype(np.float64),
                                                  f64(w), act)
    tr = Seq2SeqTrainer(w, act=act, dtype="bf16")
    loss, y = tr.forward_backward(dev(enc), dev(dec_in), dev(tgt))
    tr.ws.check()
    loss = float(loss.item())
    print("bf16 trainer %s: loss %.6e vs fp64 %.6e" % (act, loss, loss_ref))
    assert abs(loss - loss_ref) <= 2e-3 * loss_ref
    for k in _W_ORDER:
        a = tr.g[k].detach().cpu().numpy().astype(np.float64).ravel()
        r = g_ref[k].ravel()
        scale = np.abs(r).max()
        err = np.abs(a - r).max()
        cos = float(a @ r / (np.linalg.norm(a) * np.linalg.norm(r)))
        print("  grad %-8s max|ref| %.3e  max err %.3e  cosine %.6f" % (k, scale, err, cos))
        assert np.isfinite(a).all() and err <= 3e-2 * scale and cos >= 0.999, (k, err, scale, cos)
    tf = ops.seq2seq_teacher_forced(dev(enc), dev(dec_in), tr.w, act=act, dtype="bf16")
    assert torch.equal(y, tf)


def test_bf16_adam_steps_lower_the_loss_like_fp32():
    from longterm360fov_amd.training import Seq2SeqTrainer
    B, T_in, T_out = 64, 10, 10
    w = O.init_seq2seq(81, H=256, bias_noise=0.05)
    enc, dec_in, tgt = _batch(82, B, T_in, T_out)
    losses = {}
    for dt in ("f32", "bf16"):
        tr = Seq2SeqTrainer(w, dtype=dt, optimizer="adam")
        ls = [float(tr.train_step(dev(enc), dev(dec_in), dev(tgt)).item()) for _ in range(3)]
        ls.append(float(tr.eval_loss(dev(enc), dev(dec_in), dev(tgt)).item()))
        tr.check()
        losses[dt] = ls
    print("adam losses f32 %s bf16 %s" % (losses["f32"], losses["bf16"]))
    b, f = losses["bf16"], losses["f32"]
    assert b[-1] < b[0]
    assert abs(b[-1] - f[-1]) <= 0.02 * f[-1]


def test_seq2seq_model_in_bf16():
    from longterm360fov_amd.models import Seq2SeqLSTM
    for bad in (dict(latent_dim=64, dtype="bf16"), dict(latent_dim=256, dtype="fp16")):
        with pytest.raises(ValueError):
            Seq2SeqLSTM(**bad)
    B, T_in, T_out = 48, 5, 4
    w = O.init_seq2seq(91, H=256, bias_noise=0.05)
    enc, dec_in, tgt = _batch(92, B, T_in, T_out)
    dec0 = dec_in[:, :1]
    m = Seq2SeqLSTM(latent_dim=256, seed=1, dtype="bf16")
    m.set_weights([w[k] for k in _W_ORDER])
    # inference: the fused call, the teacher-forced graph, and the reference's host loop over encoder_model / decoder_model
    dec = m.decode_sequence(enc, dec0, predict_step=T_out)
    ref_t, _, _ = ref_decode_bf16(enc, dec0, w, T_out, "sigmoid")
    assert np.abs(dec - ref_t).max() <= TIGHT and np.abs(dec - ref_decode_f64(enc, dec0, w, T_out, "sigmoid")).max() <= LOOSE
    pred = m.predict([enc, dec_in])
    w64 = f64(w)
    with O.bf16_operands():
        _, h, c = O.lstm_layer(enc.astype(np.float64), w64["enc_K"], w64["enc_R"], w64["enc_b"])
        hs, _, _ = O.lstm_layer(dec_in.astype(np.float64), w64["dec_K"], w64["dec_R"], w64["dec_b"], h, c)
        ref_p = O.dense(hs.reshape(-1, 256), w64["dense_W"], w64["dense_b"], matrix_core=True).reshape(B, T_out, -1)
    ref_pl = O.seq2seq_teacher_forced(enc.astype(np.float64), dec_in.astype(np.float64), w64)
    assert np.abs(pred - ref_p).max() <= TIGHT and np.abs(pred - ref_pl).max() <= LOOSE
    h, c = m.encoder_model.predict(enc)
    target, outs = dec0, []
    for _ in range(T_out):
        y, h, c = m.decoder_model.predict([target, h, c])
        outs.append(y)
        target = y
    np.testing.assert_array_equal(np.concatenate(outs, axis=1), dec)
    # training: one epoch lowers the loss; the .h5 file carries the fp32 master weights
    m.compile(optimizer="Adam", loss="mean_squared_error")
    mse = lambda: float(np.mean((m.predict([enc, dec_in]) - tgt) ** 2))
    before = mse()
    np.random.seed(0)
    m.fit([enc, dec_in], tgt, batch_size=16, epochs=1, shuffle=False)
    after = mse()
    print("bf16 model fit: loss %.6e -> %.6e" % (before, after))
    assert after < before
    assert all(a.dtype == np.float32 for a in m.get_weights())
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "s2s_bf16.h5")
        m.save_weights(p)
        m2 = Seq2SeqLSTM(latent_dim=256, seed=9, dtype="bf16")
        m2.load_weights(p)
        for a, b in zip(m2.get_weights(), m.get_weights()):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(m2.predict([enc, dec_in]), m.predict([enc, dec_in]))
        np.testing.assert_array_equal(m2.decode_sequence(enc, dec0, predict_step=T_out), m.decode_sequence(enc, dec0, predict_step=T_out))
