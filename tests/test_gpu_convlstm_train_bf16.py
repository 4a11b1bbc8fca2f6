"""ConvLSTMTrainer(head_dtype='bf16') and ConvLSTMSeq2Seq(dtype='bf16', train_dtype='bf16') on the GPU.

References and bounds are test_convlstm_train_bf16_host's: every gradient against the rounded-operand autograd within TRAINER
of the tensor's scale and against the full-precision fp64 graph within FULL_PRECISION, the loss within LOSS_REL; the CPU file
checks that the references' own noise takes at most half of each.  The full-size case is configs[3]'s shape class (36 x 18 x
30 maps, T 10 -> 10, head 56 -> 512 -> 1024 -> 30) at B = 32 instead of 256, which keeps it to a few seconds."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_convlstm_bf16_host as HB  # noqa: E402
from test_convlstm_train_bf16_host import (FULL_PRECISION, LOOSE, LOSS_REL, TRAIN_CASES, TRAINER, of_scale, train_inputs,  # noqa: E402
                                           train_references)

pytestmark = pytest.mark.gpu
TIGHT = HB.TIGHT


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def trainer(case, w, head_dtype, **kw):
    from longterm360fov_amd.training import ConvLSTMTrainer
    return ConvLSTMTrainer(w, head=case[1], act=case[13], dropout_rate=case[11], loss=case[12], head_dtype=head_dtype, **kw)


@pytest.mark.parametrize("idx", range(len(TRAIN_CASES)), ids=[c[0] for c in TRAIN_CASES])
def test_bf16_head_gradients_loss_and_training(idx):
    case = TRAIN_CASES[idx]
    w, enc, dec0, tgt, masks = train_inputs(case)
    (l64, g64, P64), (lf, gf, _) = train_references(idx)
    dmasks = None if masks is None else {k: dev(v) for k, v in masks.items()}
    tr = trainer(case, w, "bf16")
    loss, P = tr.forward_backward(dev(enc), dev(dec0), dev(tgt), masks=dmasks)
    loss = float(loss.item())
    worst = HB.worst(P.cpu().numpy().astype(np.float64), P64, TIGHT)
    print("%s: loss %.6e (rounded autograd %.6e, full precision %.6e); prediction %.3f of TIGHT" % (case[0], loss, l64, lf, worst))
    assert worst <= 1.0
    assert abs(loss - l64) <= LOSS_REL * abs(l64) and abs(loss - lf) <= LOSS_REL * abs(lf)
    for k in tr.order:
        got = tr.g[k].detach().cpu().numpy().astype(np.float64)
        et, ef = of_scale(got, g64[k]), of_scale(got, gf[k])
        print("  %-8s vs rounded autograd %.2e of scale, vs full precision %.2e" % (k, et, ef))
        assert et <= TRAINER, (k, et)
        assert ef <= FULL_PRECISION, (k, ef)
    tr.check()
    # the fp32 trainer on the same data: first-step loss within LOOSE
    tf = trainer(case, w, "f32")
    lf32, _ = tf.forward_backward(dev(enc), dev(dec0), dev(tgt), masks=dmasks)
    assert abs(loss - float(lf32.item())) <= LOOSE * abs(float(lf32.item()))
    # five RMSprop steps reduce the loss (evaluated without dropout)
    before = float(tr.eval_loss(dev(enc), dev(dec0), dev(tgt)).item())
    for _ in range(5):
        tr.train_step(dev(enc), dev(dec0), dev(tgt))
    after = float(tr.eval_loss(dev(enc), dev(dec0), dev(tgt)).item())
    tr.check()
    assert np.isfinite(after) and after < before


@pytest.mark.parametrize("idx", [0, 1], ids=[c[0] for c in TRAIN_CASES[:2]])
def test_trainer_forward_is_the_bf16_models_predict(idx):
    """The trainer's forward runs the launches ConvLSTMSeq2Seq(dtype='bf16').predict_device runs.  The cells of the two differ in
    how the first layer's input channels are padded; where the fp32 pair is bit-identical the bf16 pair must be too, elsewhere it
    is held to TIGHT."""
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    case = TRAIN_CASES[idx]
    w, enc, dec0, _, _ = train_inputs(case)
    T_out = case[4]
    pairs = {}
    for dt in ("f32", "bf16"):
        P = trainer(case, w, dt)._forward(dev(enc), dev(dec0), T_out)[0].transpose(0, 1)
        Q = ConvLSTMSeq2Seq(w, head=case[1], recurrent_activation=case[13], dtype=dt).predict_device(dev(enc), dev(dec0), T_out)
        pairs[dt] = (P.contiguous(), Q)
    same32 = torch.equal(*pairs["f32"])
    same16 = torch.equal(*pairs["bf16"])
    worst = HB.worst(pairs["bf16"][0].cpu().numpy().astype(np.float64), pairs["bf16"][1].cpu().numpy().astype(np.float64), TIGHT)
    print("%s: fp32 pair bit-identical %s, bf16 pair bit-identical %s (%.3f of TIGHT)" % (case[0], same32, same16, worst))
    if same32:
        assert same16
    assert worst <= 1.0


def test_model_trains_with_train_dtype_bf16():
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    rng = np.random.default_rng(3)
    w = O.init_convlstm_seq2seq(9, C=3, latent_dim=8, head="conv1d", head_filters=(16, 24))
    enc = rng.random((24, 3, 1, 30, 3)).astype(np.float32)
    tgt = rng.random((24, 2, 1, 30, 3)).astype(np.float32)
    tgt /= tgt.sum(-1, keepdims=True)
    m = ConvLSTMSeq2Seq(w, head="conv1d", dtype="bf16", train_dtype="bf16")
    m.compile(optimizer="RMSprop", loss="mean_squared_error")
    first = m.train_on_batch([enc[:8], enc[:8, -1:]], tgt[:8])
    assert np.isfinite(first)
    # the packs were rebuilt: predict = a fresh bf16 model on the trained weights, bit for bit
    got = m.predict([enc[:4], enc[:4, -1:]], predict_step=2)
    fresh = ConvLSTMSeq2Seq(dict(zip(m._order, m.get_weights())), head="conv1d", dtype="bf16")
    assert np.array_equal(got, fresh.predict([enc[:4], enc[:4, -1:]], predict_step=2))
    assert not np.array_equal(got, ConvLSTMSeq2Seq(w, head="conv1d", dtype="bf16").predict([enc[:4], enc[:4, -1:]], predict_step=2))
    val = ([enc[16:], enc[16:, -1:]], tgt[16:])
    h = m.fit([enc[:16], enc[:16, -1:]], tgt[:16], batch_size=8, epochs=3, shuffle=False, validation_data=val)
    assert len(h.history["loss"]) == 3 and h.history["loss"][-1] < h.history["loss"][0]
    tr = m._get_trainer()
    assert tr.head_dtype == "bf16"
    ev = float(tr.eval_loss(dev(enc[16:]), dev(enc[16:, -1:]), dev(tgt[16:])).item())
    assert abs(h.history["val_loss"][-1] - ev) <= 1e-6 * abs(ev)


def test_model_trains_on_trajectories_with_train_dtype_bf16():
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    w = O.init_convlstm_seq2seq(3, C=30, latent_dim=8, k=3, head="conv2d", head_filters=(24, 40))
    m = ConvLSTMSeq2Seq(w, head="conv2d", dtype="bf16", train_dtype="bf16")
    m.compile(optimizer="RMSprop", loss="mean_squared_error")
    xyz = O.synthetic_xyz(np.random.default_rng(2), 2, 3, 30).reshape(2, 3, 30, 3).astype(np.float32)
    l0 = m.train_on_trajectories(xyz[:, :2], xyz[:, 1:2], xyz[:, 1:])
    l1 = m.train_on_trajectories(xyz[:, :2], xyz[:, 1:2], xyz[:, 1:])
    assert np.isfinite(l0) and np.isfinite(l1) and l1 != l0
    assert m._get_trainer().head_dtype == "bf16"


def test_full_size_step_against_the_fp32_trainer(capfd):
    """configs[3]'s layers (head 56 -> 512 -> 1024 -> 30 on 36 x 18 maps, T 10 -> 10) at B = 32: the last layer's dy goes through
    the channel-padded buffer (30 -> 32), the 512 -> 1024 weight gradient through the tuned kernel with split slices."""
    B = 32
    w = HB.full_weights()
    enc, dec0 = HB.full_inputs(list(range(B)))
    tgt, _ = HB.full_inputs(list(range(B, 2 * B)))
    from longterm360fov_amd.training import ConvLSTMTrainer
    res = {}
    for dt in ("f32", "bf16"):
        tr = ConvLSTMTrainer(w, head="conv2d", head_dtype=dt)
        os.environ["FOV_DBG_TRACE"] = "1"
        capfd.readouterr()
        try:
            loss, _ = tr.forward_backward(dev(enc), dev(dec0), dev(tgt))
            tr.check()
        finally:
            del os.environ["FOV_DBG_TRACE"]
        plans = [ln for ln in capfd.readouterr().err.splitlines() if "conv2d_wgrad_bf16: " in ln]
        assert len(plans) == (3 if dt == "bf16" else 0) and all("tuned form" in ln for ln in plans), plans
        res[dt] = (float(loss.item()), {k: tr.g[k].detach().cpu().numpy().astype(np.float64) for k in tr.order if k.startswith("head") and k.endswith("_W")})
        del tr
        torch.cuda.empty_cache()
    l32, g32 = res["f32"]
    l16, g16 = res["bf16"]
    print("full size: loss fp32 %.6e bf16 %.6e" % (l32, l16))
    assert np.isfinite(l16) and abs(l16 - l32) <= LOOSE * abs(l32)
    errs = {k: of_scale(g16[k], g32[k]) for k in g32}
    for k, e in errs.items():
        print("  %s: %.2e of scale vs the fp32 trainer" % (k, e))
    for k, e in errs.items():
        assert np.isfinite(g16[k]).all() and e <= FULL_PRECISION, (k, e)
