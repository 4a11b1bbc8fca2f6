"""GPU parity of the training path (a6/a7): gradients of the teacher-forced graph, Keras Adam /
RMSprop steps and `fit` against the fp64 oracle (oracle/fov_oracle.py::seq2seq_loss_and_grads,
adam_step), through the C ABI.  Gradient tolerance: |gpu - ref| <= 1e-3*|ref| + 2e-4*max|ref| per
tensor (the 1e-3 relative bar of north_star with a floor for near-zero entries), plus a tight bound
1e-4 * max|ref| on the worst element."""
import os

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

pytestmark = pytest.mark.gpu

_W_ORDER = ("enc_K", "enc_R", "enc_b", "dec_K", "dec_R", "dec_b", "dense_W", "dense_b")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def f64(w):
    return {k: v.astype(np.float64) for k, v in w.items()}


def batch(seed, B, T_in, T_out):
    enc, dec0, tgt = O.synthetic_batch(seed, B, T_in, T_out)
    dec_in = np.concatenate([dec0, tgt[:, :-1]], axis=1)
    return enc, dec_in, tgt


def check_grads(got, ref, tag):
    for k in _W_ORDER:
        a = got[k].detach().cpu().numpy().astype(np.float64)
        r = ref[k]
        scale = np.abs(r).max()
        err = np.abs(a - r)
        print("%s grad %-8s max|ref| %.3e  max err %.3e" % (tag, k, scale, err.max()))
        assert np.isfinite(a).all()
        assert (err <= 1e-3 * np.abs(r) + 2e-4 * scale).all(), (tag, k, err.max(), scale)
        assert err.max() <= 1e-4 * scale + 1e-9, (tag, k, err.max(), scale)


@pytest.mark.parametrize("impl,H,B,T_in,T_out", [
    ("generic", 32, 9, 5, 4), ("cluster", 64, 21, 4, 3), ("cluster", 128, 32, 10, 10), ("cluster", 256, 40, 6, 5),
])
@pytest.mark.parametrize("act", ["sigmoid", "hard_sigmoid"])
def test_gradients_match_oracle(impl, H, B, T_in, T_out, act):
    from longterm360fov_amd.training import Seq2SeqTrainer
    w = O.init_seq2seq(50 + H, H=H, bias_noise=0.1)
    enc, dec_in, tgt = batch(51 + B, B, T_in, T_out)
    loss_ref, g_ref, y_ref = O.seq2seq_loss_and_grads(enc.astype(np.float64), dec_in.astype(np.float64),
                                                     tgt.astype(np.float64), f64(w), act)
    tr = Seq2SeqTrainer(w, act=act, impl=impl)
    loss, y = tr.forward_backward(dev(enc), dev(dec_in), dev(tgt))
    tr.ws.check()
    assert abs(float(loss.item()) - loss_ref) <= 1e-5 * max(loss_ref, 1e-6) + 1e-9
    np.testing.assert_allclose(y.cpu().numpy(), y_ref, atol=2e-5)
    check_grads(tr.g, g_ref, "%s H%d %s" % (impl, H, act))


def test_shard_weighted_gradients_equal_full_batch():
    """Data parallel rule: sum_r (n_r/n) grad_r == grad of the whole batch (what the single
    all-reduce of the flat buffer computes); unequal shard sizes included."""
    from longterm360fov_amd.training import Seq2SeqTrainer
    H, B = 64, 37
    w = O.init_seq2seq(77, H=H, bias_noise=0.1)
    enc, dec_in, tgt = batch(78, B, 5, 4)
    tr = Seq2SeqTrainer(w)
    tr.forward_backward(dev(enc), dev(dec_in), dev(tgt))
    full = tr.grad.clone()
    acc = torch.zeros_like(full)
    for lo, hi in ((0, 19), (19, 37)):
        tr.forward_backward(dev(enc[lo:hi]), dev(dec_in[lo:hi]), dev(tgt[lo:hi]), grad_weight=(hi - lo) / B)
        acc += tr.grad
    scale = float(full.abs().max())
    assert float((acc - full).abs().max()) <= 2e-6 * scale + 1e-10


@pytest.mark.parametrize("optimizer", ["adam", "rmsprop"])
def test_training_steps_match_oracle(optimizer):
    """k optimizer steps on one batch: per-step loss and final weights vs the fp64 oracle."""
    from longterm360fov_amd.training import Seq2SeqTrainer
    H, B, T_in, T_out, steps = 128, 32, 10, 10, 6
    w = O.init_seq2seq(91, H=H, bias_noise=0.05)
    enc, dec_in, tgt = batch(92, B, T_in, T_out)
    tr = Seq2SeqTrainer(w, optimizer=optimizer)
    w64 = f64(w)
    m = {k: np.zeros_like(v) for k, v in w64.items()}
    v = {k: np.zeros_like(v) for k, v in w64.items()}
    losses, ref_losses = [], []
    for t in range(1, steps + 1):
        losses.append(float(tr.train_step(dev(enc), dev(dec_in), dev(tgt)).item()))
        l, g, _ = O.seq2seq_loss_and_grads(enc.astype(np.float64), dec_in.astype(np.float64), tgt.astype(np.float64), w64)
        ref_losses.append(l)
        for k in w64:
            if optimizer == "adam":
                O.adam_step(w64[k], g[k], m[k], v[k], t)
            else:
                O.rmsprop_step(w64[k], g[k], m[k])
    print("losses gpu", losses, "\nlosses ref", ref_losses)
    assert ref_losses[-1] < ref_losses[0]
    np.testing.assert_allclose(losses, ref_losses, rtol=2e-4)
    got = tr.weights_numpy()
    for k in w64:
        d = np.abs(got[k] - w64[k])
        # the optimizers divide by sqrt(v): entries whose gradient is ~0 are ill-conditioned, so allow
        # a few of them to differ by up to one learning-rate step while the bulk agrees tightly
        assert d.max() <= 1.5e-3 * steps, (k, d.max())
        assert np.mean(d <= 2e-5) >= 0.995, (k, np.mean(d <= 2e-5))


def test_fit_surface_and_callbacks(tmp_path):
    from longterm360fov_amd.callbacks import EarlyStopping, ModelCheckpoint, ReduceLROnPlateau
    from longterm360fov_amd.models import Seq2SeqLSTM
    np.random.seed(0)
    enc, dec_in, tgt = batch(5, 200, 10, 10)
    m = Seq2SeqLSTM(latent_dim=64, seed=3, recurrent_activation="hard_sigmoid")
    with pytest.raises(RuntimeError):
        m.fit([enc, dec_in], tgt)
    m.compile(optimizer="Adam", loss="mean_squared_error")
    ck = ModelCheckpoint(str(tmp_path / "fov_s2s_epoch{epoch:02d}-{val_loss:.4f}.h5"), monitor="val_loss", save_best_only=True)
    rl = ReduceLROnPlateau(monitor="val_loss", factor=0.2, patience=3, min_lr=1e-6)
    es = EarlyStopping(monitor="val_loss", min_delta=0, patience=10)
    h = m.fit([enc, dec_in], tgt, batch_size=32, epochs=6, validation_split=0.2, shuffle=True, callbacks=[ck, rl, es])
    assert len(h.history["loss"]) == 6 and len(h.history["val_loss"]) == 6
    assert h.history["loss"][-1] < h.history["loss"][0]
    assert ck.saved and all(os.path.exists(p) and p.endswith(".h5") for p in ck.saved)   # Keras-layout HDF5 (keras_h5.py)
    # the checkpoint round-trips into a fresh model and reproduces predictions
    m2 = Seq2SeqLSTM(latent_dim=64, seed=9, recurrent_activation="hard_sigmoid")
    m2.load_weights(ck.saved[-1])
    p1 = m.predict([enc[:8], dec_in[:8]])
    assert p1.shape == (8, 10, 6)
    # train_on_batch keeps optimizer state and returns the loss of that batch
    l0 = m.train_on_batch([enc[:32], dec_in[:32]], tgt[:32])
    assert np.isfinite(l0)


def test_model_object_sampling_models_match_fused_decode():
    """decode_sequence (one fused call) == the reference's host loop over encoder_model /
    decoder_model (FoV_seq2seq.py:154-178), and both match the oracle."""
    from longterm360fov_amd.config import cfg
    from longterm360fov_amd.models import Seq2SeqLSTM
    m = Seq2SeqLSTM(latent_dim=128, seed=4)
    w = dict(zip(_W_ORDER, m.get_weights()))
    enc, dec0, _ = O.synthetic_batch(6, 5, 10, 10)
    fused = m.decode_sequence(enc)                      # first decoder input = mu/var of the last second
    h, c = m.encoder_model.predict(enc)
    from longterm360fov_amd.utility import get_gt_target_xyz
    target_seq = get_gt_target_xyz(enc[:, -1:, :].astype(np.float64)).astype(np.float32)
    steps = []
    for _ in range(cfg.predict_step):
        y, h, c = m.decoder_model.predict([target_seq, h, c])
        steps.append(y)
        target_seq = y
    loop = np.concatenate(steps, axis=1)
    np.testing.assert_allclose(fused, loop, atol=2e-6)
    ref = O.seq2seq_decode(enc.astype(np.float64), target_seq * 0 + get_gt_target_xyz(enc[:, -1:, :].astype(np.float64)),
                           f64(w), cfg.predict_step)
    np.testing.assert_allclose(fused, ref, atol=2e-5)


def _dp_worker(rank, world_size, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)   # one GPU on the box: gloo carries the CUDA buffers
    try:
        from longterm360fov_amd import parallel
        from longterm360fov_amd.training import Seq2SeqTrainer
        w = O.init_seq2seq(123, H=64, bias_noise=0.05)
        enc, dec_in, tgt = batch(124, 37, 6, 5)
        lo, hi = parallel.shard_range(37)
        tr = Seq2SeqTrainer(w)
        losses = [float(tr.train_step(dev(enc[lo:hi]), dev(dec_in[lo:hi]), dev(tgt[lo:hi]), n_global=37).item())
                  for _ in range(3)]
        q.put((rank, losses, tr.flat.detach().cpu().numpy()))
    finally:
        dist.destroy_process_group()


def test_data_parallel_two_ranks_equal_single_process():
    """2 ranks (gloo, both on the one GPU of the box), unequal shards 19/18, three Adam steps:
    losses and parameters equal the single-process run on the whole batch."""
    import socket
    import torch.multiprocessing as mp
    from longterm360fov_amd.training import Seq2SeqTrainer
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    w = O.init_seq2seq(123, H=64, bias_noise=0.05)
    enc, dec_in, tgt = batch(124, 37, 6, 5)
    tr = Seq2SeqTrainer(w)
    ref_losses = [float(tr.train_step(dev(enc), dev(dec_in), dev(tgt)).item()) for _ in range(3)]
    ref_flat = tr.flat.detach().cpu().numpy()
    for rank, losses, flat in res:
        np.testing.assert_allclose(losses, ref_losses, rtol=1e-5)
        d = np.abs(flat - ref_flat)
        assert d.max() <= 3e-3 and np.mean(d <= 2e-5) >= 0.995, (rank, d.max(), np.mean(d <= 2e-5))
    np.testing.assert_array_equal(res[0][2], res[1][2])     # replicas stay bit-identical


def _dp_mixing_worker(rank, world_size, port, q, dtype):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        from longterm360fov_amd import parallel
        from longterm360fov_amd.training import OthersMixingTrainer
        w = O.init_others_mixing(223, H=256, num_user=5, bias_noise=0.05)
        enc, dec0, tgt, oth = O.synthetic_batch(224, 41, 3, 4, num_others=4)
        lo, hi = parallel.shard_range(41)
        tr = OthersMixingTrainer(w, dtype=dtype)
        tr.overlap_allreduce = True   # the opt-in order: the decoder's gradients go out under the encoder's BPTT (the default - one all-reduce at the end - is what _dp_worker above runs)
        losses = [float(tr.train_step(dev(enc[lo:hi]), dev(oth[lo:hi]), dev(dec0[lo:hi]), dev(tgt[lo:hi]), n_global=41).item())
                  for _ in range(3)]
        tr.check()
        q.put((rank, losses, tr.flat.detach().cpu().numpy()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_data_parallel_mixing_trainer_two_ranks(dtype):
    """The others-mixing trainer under data parallelism (2 ranks over gloo on the box's one GPU, shards 21 / 20): the shard
    weight rides on the loss gradient, the decoder / head part of the flat buffer - written by the fused weight-gradient
    products - is all-reduced while the encoder's BPTT runs, the rest at the end of the step; three Adam steps give the losses
    and parameters of the single-process run on the whole batch, and the replicas stay bit-identical."""
    import socket
    import torch.multiprocessing as mp
    from longterm360fov_amd.training import OthersMixingTrainer
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_mixing_worker, args=(r, 2, port, q, dtype)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    w = O.init_others_mixing(223, H=256, num_user=5, bias_noise=0.05)
    enc, dec0, tgt, oth = O.synthetic_batch(224, 41, 3, 4, num_others=4)
    tr = OthersMixingTrainer(w, dtype=dtype)
    ref_losses = [float(tr.train_step(dev(enc), dev(oth), dev(dec0), dev(tgt)).item()) for _ in range(3)]
    ref_flat = tr.flat.detach().cpu().numpy()
    tol = 1e-5 if dtype == "f32" else 2e-3      # bf16: the two shards round different partial sums
    for rank, losses, flat in res:
        np.testing.assert_allclose(losses, ref_losses, rtol=tol)
        d = np.abs(flat - ref_flat)
        assert d.max() <= 4e-3 and np.mean(d <= (2e-5 if dtype == "f32" else 2e-3)) >= 0.99, (rank, d.max())
    np.testing.assert_array_equal(res[0][2], res[1][2])     # replicas stay bit-identical


def _fit_worker(rank, world_size, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        q.put((rank, _fit_shuffled(seed=5 if rank == 0 else 991)))   # rank 1's own np.random state must not matter
    finally:
        dist.destroy_process_group()


def _fit_shuffled(seed):
    from longterm360fov_amd.models import Seq2SeqLSTM
    enc, dec_in, tgt = batch(31, 45, 5, 4)
    m = Seq2SeqLSTM(latent_dim=64, seed=8)
    m.compile(optimizer="Adam", loss="mean_squared_error")
    np.random.seed(seed)
    h = m.fit([enc, dec_in], tgt, batch_size=16, epochs=2, validation_split=0.2, shuffle=True)
    return h.history["loss"], h.history["val_loss"], np.concatenate([a.ravel() for a in m.get_weights()])


def test_fit_shuffle_two_ranks_equal_single_process():
    """fit(shuffle=True) under data parallelism: rank 0's permutation is broadcast every epoch, each rank takes its
    contiguous shard of every global batch - losses and weights equal the single-process fit with rank 0's seed
    (the ranks' own np.random states differ on purpose)."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_fit_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ref_loss, ref_val, ref_w = _fit_shuffled(seed=5)
    for rank, (loss, val, wts) in res:
        np.testing.assert_allclose(loss, ref_loss, rtol=2e-5)
        np.testing.assert_allclose(val, ref_val, rtol=2e-5)
        d = np.abs(wts - ref_w)
        assert d.max() <= 3e-3 and np.mean(d <= 2e-5) >= 0.99, (rank, d.max(), np.mean(d <= 2e-5))
    np.testing.assert_array_equal(res[0][1][2], res[1][1][2])     # replicas stay bit-identical


def test_poisoned_workspace_is_fail_stop_and_sticky():
    """A set timeout word is never cleared by a launch: later persistent-kernel calls on that workspace skip their
    bodies (outputs untouched), the guarded optimizer leaves the parameters alone, check() reports the failure ONCE
    and clears it, after which the workspace works again."""
    from longterm360fov_amd import ops, _lib
    w = O.init_seq2seq(3, H=256, bias_noise=0.05)
    enc, dec0, _ = O.synthetic_batch(4, 40, 5, 4)
    dw = {k: dev(v) for k, v in w.items()}
    ws = ops.Workspace()
    good = ops.seq2seq_decode(dev(enc), dev(dec0), dw, 4, workspace=ws).cpu().numpy()
    ws.check()
    ws.buf[:4] = torch.tensor([1, 0, 0, 0], dtype=torch.uint8, device="cuda")     # what a give-up leaves behind
    out = torch.full((40, 4, 6), 7.0, dtype=torch.float32, device="cuda")
    ops.seq2seq_decode(dev(enc), dev(dec0), dw, 4, workspace=ws, out=out)
    ops.seq2seq_decode(dev(enc), dev(dec0), dw, 4, workspace=ws, out=out)          # still poisoned: nothing clears it
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0
    p = torch.ones(1000, device="cuda"); g = torch.ones(1000, device="cuda")
    m = torch.zeros(1000, device="cuda"); v = torch.zeros(1000, device="cuda")
    ops.adam_step(p, g, m, v, 1, guards=[ws.buf])
    assert float(p.min()) == 1.0 and float(m.abs().max()) == 0.0                   # update skipped on the device
    with pytest.raises(_lib.FovError) as ei:
        ws.check()
    assert ei.value.code == _lib.ERR_TIMEOUT
    ws.check()                                                                     # reported once, then clean
    again = ops.seq2seq_decode(dev(enc), dev(dec0), dw, 4, workspace=ws).cpu().numpy()
    ws.check()
    np.testing.assert_array_equal(again, good)
    ops.adam_step(p, g, m, v, 1, guards=[ws.buf])
    assert float(p.max()) < 1.0


def test_persistent_bptt_matches_stepped_and_oracle():
    """The one-launch cluster BPTT kernel vs the host-stepped recurrence (FOV_BWD_STEPPED=1) and the
    fp64 oracle: ragged multi-tile batch (more tiles than groups), given initial state, dhs + dhT/dcT."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(7)
    for H, B, T in ((256, 16 * 64 + 16 * 3 + 5, 3), (128, 37, 6), (64, 21, 4), (512, 16 * 16 + 16 * 2 + 5, 3), (512, 32, 10), (512, 100, 4),
                    (256, 100, 5), (128, 16 * 9, 3), (128, 32, 10)):
        F = 11      # width 512: lstm_bwd16.hip - sixteen workgroups per tile (293 sequences = 19 tiles on 16 groups), thirty-two up to
        # eight tiles (32 sequences = lstm.py's batch; 100 = seven tiles, the last one ragged).  Widths 128 / 256 take the same
        # kernel (sixteen units per workgroup) up to eight tiles: (128, 37), (256, 100), (128, 32); (128, 144) = nine tiles does not
        K, R, b = O.init_lstm(rng, F, H, np.float32)
        b = (b + 0.1 * rng.standard_normal(b.shape)).astype(np.float32)
        x = rng.uniform(-1, 1, (B, T, F)).astype(np.float32)
        h0 = (0.3 * rng.standard_normal((B, H))).astype(np.float32)
        c0 = (0.3 * rng.standard_normal((B, H))).astype(np.float32)
        dhs = (0.1 * rng.standard_normal((B, T, H))).astype(np.float32)
        dhT = (0.1 * rng.standard_normal((B, H))).astype(np.float32)
        dcT = (0.1 * rng.standard_normal((B, H))).astype(np.float32)
        d64 = lambda a: a.astype(np.float64)
        hs64, _, _, res64 = O.lstm_layer_train(d64(x), d64(K), d64(R), d64(b), d64(h0), d64(c0))
        ref = O.lstm_layer_backward(d64(x), d64(K), d64(R), d64(h0), d64(c0), hs64, res64, d64(dhs), d64(dhT), d64(dcT))
        hs, hT, cT, res = ops.lstm_seq_train(dev(x), dev(K), dev(R), dev(b), dev(h0), dev(c0))
        outs = {}
        try:
            for mode in ("persistent", "stepped") + (("groups32",) if (H == 512 and B <= 128) else ()):
                if mode == "stepped":
                    os.environ["FOV_BWD_STEPPED"] = "1"
                if mode == "groups32":      # the thirty-two-workgroup form of the width-512 kernel (one cell per lane)
                    os.environ.pop("FOV_BWD_STEPPED", None)
                    os.environ["FOV_BWD16_GROUPS"] = "32"
                sc = ops.Scratch()
                outs[mode] = ops.lstm_seq_bwd(dev(x), dev(K), dev(R), hs, res, h0=dev(h0), c0=dev(c0), dhs=dev(dhs),
                                              dhT=dev(dhT), dcT=dev(dcT), need_dx=True, need_state_grads=True, scratch=sc)
                sc.check()
        finally:
            os.environ.pop("FOV_BWD_STEPPED", None)
            os.environ.pop("FOV_BWD16_GROUPS", None)
        if "groups32" in outs:
            for k in ("dz", "dx", "dK", "dR", "db", "dh0", "dc0"):
                g32, ref_k = outs["groups32"][k].cpu().numpy().astype(np.float64), ref[k]
                assert np.abs(g32 - ref_k).max() <= 1e-4 * np.abs(ref_k).max() + 1e-9, (H, k, "groups32")
        for k in ("dz", "dx", "dK", "dR", "db", "dh0", "dc0"):
            a = outs["persistent"][k].cpu().numpy().astype(np.float64)
            s_ = outs["stepped"][k].cpu().numpy().astype(np.float64)
            r = ref[k]
            scale = np.abs(r).max()
            print("H%d %-4s max|ref| %.3e  persistent err %.3e  stepped err %.3e" % (H, k, scale, np.abs(a - r).max(), np.abs(s_ - r).max()))
            assert np.abs(a - r).max() <= 1e-4 * scale + 1e-9, (H, k)
            assert np.abs(s_ - r).max() <= 1e-4 * scale + 1e-9, (H, k)


def test_stepped_bptt_hard_sigmoid_matches_oracle(capfd):
    """The host-stepped recurrence (FOV_BWD_STEPPED=1) with hard_sigmoid gates against the fp64 oracle: H = 64, B = 21 (one full
    tile and a ragged one), T = 4, F = 11, given initial state, dhs + dhT / dcT; the bound of the sigmoid twin above.
    The case is the clamped regime of the oracle's generator (47 % of the i / f / o pre-activations beyond +-2.5, so both
    values of the derivative occur); seed 155 is the first but one whose fp64 pre-activations all keep 1e-3 from the kinks
    (1.6e-3, asserted below), so the fp32 forward and the oracle take the same branch at every element.  On the CPU the oracle run
    on fp32 arrays differs from the fp64 one by at most 0.003 of the bound on this case; the GPU's own error is printed per tensor."""
    from longterm360fov_amd import ops
    H, B, T, F = 64, 21, 4, 11
    p = O.regime_lstm(155, F, H, "R1", B, T)
    assert p["act"] == "hard_sigmoid"
    dhs, dhT, dcT = O.regime_upstream(156, B, T, H)
    d64 = lambda a: a.astype(np.float64)
    x, K, R, b, h0, c0 = (p[k] for k in ("x", "K", "R", "b", "h0", "c0"))
    hs64, _, _, res64 = O.lstm_layer_train(d64(x), d64(K), d64(R), d64(b), d64(h0), d64(c0), act="hard_sigmoid")
    z = O.regime_preactivations(d64(x), d64(K), d64(R), d64(b), hs64, d64(h0))
    gates = np.concatenate([z[..., :2 * H], z[..., 3 * H:]], axis=-1)
    assert np.abs(np.abs(gates) - 2.5).min() >= 1e-3
    assert 0.3 < (np.abs(gates) > 2.5).mean() < 0.7
    ref = O.lstm_layer_backward(d64(x), d64(K), d64(R), d64(h0), d64(c0), hs64, res64, d64(dhs), d64(dhT), d64(dcT), act="hard_sigmoid")
    hs, _, _, res = ops.lstm_seq_train(dev(x), dev(K), dev(R), dev(b), dev(h0), dev(c0), act="hard_sigmoid")
    capfd.readouterr()
    before = {k: os.environ.get(k) for k in ("FOV_BWD_STEPPED", "FOV_DBG_TRACE")}
    os.environ.update({k: "1" for k in before})
    try:
        sc = ops.Scratch()
        got = ops.lstm_seq_bwd(dev(x), dev(K), dev(R), hs, res, h0=dev(h0), c0=dev(c0), dhs=dev(dhs), dhT=dev(dhT), dcT=dev(dcT),
                               need_dx=True, need_state_grads=True, act="hard_sigmoid", scratch=sc)
        sc.check()
    finally:
        for k, v in before.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    assert capfd.readouterr().err.count("launched: lstm_bwd_pointwise") == T       # the stepped form ran, one launch per step
    for k in ("dz", "dx", "dK", "dR", "db", "dh0", "dc0"):
        a, r = got[k].cpu().numpy().astype(np.float64), ref[k]
        print("%-4s max|ref| %.3e  stepped hard_sigmoid err %.3e" % (k, np.abs(r).max(), np.abs(a - r).max()))
        assert np.abs(a - r).max() <= 1e-4 * np.abs(r).max() + 1e-9, k


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("N,In1,In2,Out", [(5120, 256, 256, 1024), (5120, 256, 0, 1024), (40, 128, 64, 256), (1000, 90, 256, 1024),
                                           (777, 256, 128, 512), (33, 256, 0, 64)])
def test_fused_weight_gradient_product(N, In1, In2, Out, dtype):
    """fov_wgrad_fused: [dK ; dR ; db] = [x1 | x2 | 1]^T dz as ONE product + one reduce, written where the three lie adjacent
    in a flat gradient buffer - against the fp64 products, against the three separate launches (same operand rounding),
    overwrite and accumulate, split and single-slice shapes, and the shapes that fall back to the separate products."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(N + In1)
    x1 = rng.standard_normal((N, In1)).astype(np.float32)
    x2 = rng.standard_normal((N, In2)).astype(np.float32) if In2 else None
    dz = rng.standard_normal((N, Out)).astype(np.float32)
    rows = In1 + In2 + 1
    r = (lambda a: O.round_bf16(a.astype(np.float64))) if dtype == "bf16" else (lambda a: a.astype(np.float64))
    ref = np.concatenate([r(x1).T @ r(dz)] + ([r(x2).T @ r(dz)] if In2 else []) + [dz.astype(np.float64).sum(0, keepdims=True)], 0)
    out = torch.full((rows * Out + 7,), 3.0, device="cuda")              # the tail must stay untouched
    view = out[:rows * Out]
    ops.wgrad_fused(dev(x1), None if x2 is None else dev(x2), dev(dz), view, dtype=dtype)
    got = view.view(rows, Out).cpu().numpy().astype(np.float64)
    scale = np.abs(ref[:-1]).max()
    assert np.abs(got[:-1] - ref[:-1]).max() <= 2e-5 * scale, np.abs(got[:-1] - ref[:-1]).max() / scale
    assert np.abs(got[-1] - ref[-1]).max() <= 2e-5 * np.abs(ref[-1]).max() + 1e-4      # the bias row is an fp32 sum in both modes
    assert float(out[rows * Out:].min()) == 3.0 and float(out[rows * Out:].max()) == 3.0
    # the separate launches
    sep = torch.empty(rows, Out, device="cuda")
    ops.dense_bwd(dev(x1), torch.empty(In1, Out, device="cuda"), dev(dz), dW=sep[:In1], db=sep[rows - 1], need_dx=False, dtype=dtype)
    if In2:
        ops.dense_bwd(dev(x2), torch.empty(In2, Out, device="cuda"), dev(dz), dW=sep[In1:In1 + In2], need_db=False, need_dx=False,
                      dtype=dtype)
    assert (view.view(rows, Out) - sep).abs().max().item() <= 2e-5 * scale
    # accumulate: twice the product on top of the first result
    ops.wgrad_fused(dev(x1), None if x2 is None else dev(x2), dev(dz), view, accumulate=True, dtype=dtype)
    got2 = view.view(rows, Out).cpu().numpy().astype(np.float64)
    assert np.abs(got2 - 2 * got).max() <= 4e-5 * scale + 2e-4
    # no bias row
    nb = torch.empty((rows - 1) * Out, device="cuda")
    ops.wgrad_fused(dev(x1), None if x2 is None else dev(x2), dev(dz), nb, bias=False, dtype=dtype)
    assert (nb.view(rows - 1, Out) - torch.from_numpy(got[:-1].astype(np.float32)).cuda()).abs().max().item() <= 1e-6 * scale + 1e-6


@pytest.mark.parametrize("B,T,H,O,U", [(512, 10, 256, 6, 34), (37, 3, 64, 6, 5), (8, 2, 32, 3, 1), (130, 7, 128, 8, 3)])
def test_mixing_head_weight_gradients_one_launch(B, T, H, O, U):
    """fov_mix_head_wgrad: [dense_W ; dense_b] = [h2 | 1]^T dpre_p and [mix_W ; mix_b] = [others | p | 1]^T dpre_m over all
    steps, one launch + one reduce, `others` read in its (B,T,...) layout - against fp64 products; accumulate; untouched tail."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(B + H)
    n_oth = (U - 1) * O
    h2 = rng.standard_normal((T, B, H)).astype(np.float32)
    dp = rng.standard_normal((T, B, O)).astype(np.float32)
    dm = rng.standard_normal((T, B, O)).astype(np.float32)
    p = rng.standard_normal((T, B, O)).astype(np.float32)
    oth = rng.standard_normal((B, T, max(U - 1, 0), O)).astype(np.float32)
    d = lambda a: a.astype(np.float64)
    fl = lambda a: d(a).reshape(T * B, -1)
    oth_tb = d(oth).transpose(1, 0, 2, 3).reshape(T * B, n_oth)
    ref = np.concatenate([fl(h2).T @ fl(dp), fl(dp).sum(0, keepdims=True), oth_tb.T @ fl(dm), fl(p).T @ fl(dm),
                          fl(dm).sum(0, keepdims=True)], 0)
    n = ref.size
    out = torch.full((n + 5,), 7.0, device="cuda")
    ops.mix_head_wgrad(dev(h2), dev(dp), dev(oth), dev(p), dev(dm), out[:n])
    got = out[:n].view(-1, O).cpu().numpy().astype(np.float64)
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() <= 2e-5 * scale, np.abs(got - ref).max() / scale
    assert float(out[n:].min()) == 7.0 and float(out[n:].max()) == 7.0
    ops.mix_head_wgrad(dev(h2), dev(dp), dev(oth), dev(p), dev(dm), out[:n], accumulate=True)
    assert np.abs(out[:n].view(-1, O).cpu().numpy() - 2 * got).max() <= 4e-5 * scale


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("state", [False, True])
@pytest.mark.parametrize("B,T,F,H", [(64, 6, 256, 256), (40, 5, 90, 256), (33, 2, 256, 256), (48, 4, 128, 128)])
def test_layer_backward_adjacent_gradients_take_the_fused_product(B, T, F, H, dtype, state):
    """fov_lstm_seq_bwd handed dK, dR, db that lie adjacent (a trainer's flat buffer) forms them as ONE product
    [x | h_{t-1} | 1]^T dz - h_{t-1} read from the h_t tape shifted by a step, zero at t = 0 - or, when F is no multiple of the
    row tile, dR and db as [h_{t-1} | 1]^T dz: same gradients as with three separate buffers (three products + column sums)."""
    from longterm360fov_amd import ops
    if dtype == "bf16" and H != 256:
        pytest.skip("the bf16 path is built for H = 256")
    rng = np.random.default_rng(B + F)
    K, R, b = O.init_lstm(rng, F, H)
    x = rng.standard_normal((B, T, F)).astype(np.float32)
    dhs = rng.standard_normal((B, T, H)).astype(np.float32)
    # a given initial state (a decoder layer seeded by the encoder) adds h0^T dz_0 to dR behind the fused product
    h0 = dev((0.5 * rng.standard_normal((B, H))).astype(np.float32)) if state else None
    c0 = dev((0.5 * rng.standard_normal((B, H))).astype(np.float32)) if state else None
    hs, hT, cT, res = ops.lstm_seq_train(dev(x), dev(K), dev(R), dev(b), h0, c0, act="sigmoid", dtype=dtype)
    sep = ops.lstm_seq_bwd(dev(x), dev(K), dev(R), hs, res, h0=h0, c0=c0, dhs=dev(dhs), act="sigmoid", dtype=dtype)
    flat = torch.zeros((F + H + 1) * 4 * H, device="cuda")
    dK, dR, db = flat[:F * 4 * H].view(F, 4 * H), flat[F * 4 * H:(F + H) * 4 * H].view(H, 4 * H), flat[(F + H) * 4 * H:]
    fused = ops.lstm_seq_bwd(dev(x), dev(K), dev(R), hs, res, h0=h0, c0=c0, dhs=dev(dhs), dK=dK, dR=dR, db=db, act="sigmoid", dtype=dtype)
    assert torch.equal(fused["dz"], sep["dz"])
    for k in ("dK", "dR", "db"):
        scale = sep[k].abs().max().item()
        err = (fused[k] - sep[k]).abs().max().item()
        print("adjacent-gradient backward %s %s: max|ref| %.3e err %.3e" % (dtype, k, scale, err))
        assert err <= 2e-5 * scale + 1e-6, (k, err, scale)
    # accumulate on top
    ops.lstm_seq_bwd(dev(x), dev(K), dev(R), hs, res, h0=h0, c0=c0, dhs=dev(dhs), dK=dK, dR=dR, db=db, act="sigmoid", accumulate=True,
                     dtype=dtype)
    for k in ("dK", "dR", "db"):
        assert (fused[k] - 2 * sep[k]).abs().max().item() <= 4e-5 * sep[k].abs().max().item() + 2e-6, k


def _torch_mixing_graph(enc, oth, dec0, tgt, w, act, mixing="mlp"):
    """Independent fp64 reference of the a4 training graph (given_others...py:203-308) on torch.autograd."""
    t = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in w.items()}
    H = w["enc1_R"].shape[0]
    s = torch.sigmoid if act == "sigmoid" else (lambda z: torch.clamp(0.2 * z + 0.5, 0, 1))

    def step(x, h, c, K, R, b):
        z = x @ K + b + h @ R
        i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
        c = f * c + i * g
        return o * torch.tanh(c), c

    e, o_, d0, tg = (torch.tensor(a.astype(np.float64)) for a in (enc, oth, dec0, tgt))
    B = e.shape[0]
    z0 = torch.zeros(B, H, dtype=torch.float64)
    h1, c1, h2, c2 = z0, z0, z0, z0
    for tt in range(e.shape[1]):
        h1, c1 = step(e[:, tt], h1, c1, t["enc1_K"], t["enc1_R"], t["enc1_b"])
        h2, c2 = step(h1, h2, c2, t["enc2_K"], t["enc2_R"], t["enc2_b"])
    x = d0[:, 0]
    outs = []
    for tt in range(o_.shape[1]):
        h1, c1 = step(x, h1, c1, t["dec1_K"], t["dec1_R"], t["dec1_b"])
        h2, c2 = step(h1, h2, c2, t["dec2_K"], t["dec2_R"], t["dec2_b"])
        p = torch.tanh(h2 @ t["dense_W"] + t["dense_b"])
        cat = torch.cat([o_[:, tt], p[:, None, :]], dim=1)
        if mixing == "conv":      # conv_mixing (:188-197,284-290): users = channels of a 1 x 6 map, three Conv2D(1x3, same, relu)
            a = cat[:, :, None, :]                                       # NCHW (B,U,1,6)
            for i in range(3):
                a = torch.relu(torch.nn.functional.conv2d(a, t["mixc%d_W" % i].permute(3, 2, 0, 1), t["mixc%d_b" % i], padding=(0, 1)))
            x = a[:, 0, 0, :]
        else:
            x = torch.tanh(cat.reshape(B, -1) @ t["mix_W"] + t["mix_b"])
        outs.append(x)
    y = torch.stack(outs, 1)
    loss = torch.mean((y - tg) ** 2)
    loss.backward()
    return float(loss), {k: v.grad.numpy() for k, v in t.items()}, y.detach().numpy()


@pytest.mark.parametrize("H,B,U,T_in,T_out,act", [(64, 20, 5, 4, 3, "sigmoid"), (128, 33, 34, 5, 4, "hard_sigmoid"),
                                                  (256, 16, 34, 3, 3, "sigmoid"), (256, 37, 5, 2, 4, "hard_sigmoid"),
                                                  (256, 530, 3, 2, 2, "sigmoid"), (256, 512, 34, 10, 10, "sigmoid"),
                                                  (256, 48, 34, 30, 30, "sigmoid"), (256, 512, 34, 30, 30, "sigmoid")])   # the metric's horizon
def test_others_mixing_gradients_and_training(H, B, U, T_in, T_out, act):
    """a4 training: gradients of the unrolled no-teacher-forcing graph (feedback path included) against
    torch.autograd in fp64, then three Adam steps reduce the loss."""
    from longterm360fov_amd.training import OthersMixingTrainer, _MIX_ORDER
    w = O.init_others_mixing(70 + H, H=H, num_user=U, bias_noise=0.1)
    enc, dec0, tgt, oth = O.synthetic_batch(71 + B, B, T_in, T_out, num_others=U - 1)
    loss_ref, g_ref, y_ref = _torch_mixing_graph(enc, oth, dec0, tgt, w, act)
    tr = OthersMixingTrainer(w, act=act)
    loss, y = tr.forward_backward(dev(enc), dev(oth), dev(dec0), dev(tgt))
    tr.ws.check(); tr.bwd_scratch.check()
    assert abs(float(loss.item()) - loss_ref) <= 1e-5 * loss_ref + 1e-9
    np.testing.assert_allclose(y.cpu().numpy(), y_ref, atol=2e-5)
    for k in _MIX_ORDER:
        a = tr.g[k].detach().cpu().numpy().astype(np.float64)
        scale = np.abs(g_ref[k]).max()
        err = np.abs(a - g_ref[k]).max()
        print("mixing H%d grad %-8s max|ref| %.3e  max err %.3e" % (H, k, scale, err))
        assert err <= 1e-4 * scale + 1e-9, (k, err, scale)
    if H == 256:   # the fused forward / backward launches and the step-wise path give the same gradients
        tr.ws_bwd.check()
        tr2 = OthersMixingTrainer(w, act=act)
        tr2.fused_decoder = False
        tr2.fused_decoder_bwd = False
        loss2, y2 = tr2.forward_backward(dev(enc), dev(oth), dev(dec0), dev(tgt))
        assert abs(float(loss2.item()) - float(loss.item())) <= 1e-6 * abs(float(loss.item())) + 1e-9
        for k in _MIX_ORDER:
            d = (tr.g[k] - tr2.g[k]).abs().max().item()
            assert d <= 2e-5 * tr2.g[k].abs().max().item() + 1e-9, (k, d)
    losses = [float(tr.train_step(dev(enc), dev(oth), dev(dec0), dev(tgt)).item()) for _ in range(4)]
    assert losses[-1] < losses[0]


@pytest.mark.parametrize("H,B,U,T_in,T_out,act", [(64, 20, 5, 4, 3, "sigmoid"), (128, 33, 34, 5, 4, "hard_sigmoid"),
                                                  (256, 48, 34, 3, 5, "sigmoid")])
def test_others_conv_mixing_gradients_and_training(H, B, U, T_in, T_out, act):
    """conv_mixing (given_others_gt_mean_var_seq2seq.py:56,188-197,284-290): forward against the NumPy oracle, gradients of the
    unrolled graph (three 1x3 convolutions over the users-as-channels map, feedback path included) against torch.autograd
    fp64, the model object's predict / fit surface and an HDF5 round trip."""
    from longterm360fov_amd.models import OthersConvMixingSeq2Seq
    from longterm360fov_amd.training import OthersConvMixingTrainer, _CONV_MIX_ORDER
    w = {k: v for k, v in O.init_others_mixing(170 + H, H=H, num_user=U, bias_noise=0.1).items() if not k.startswith("mix_")}
    rng = np.random.default_rng(H + U)
    for i, (c, n) in enumerate(((U, 8), (8, 8), (8, 1))):
        w["mixc%d_W" % i] = (rng.standard_normal((1, 3, c, n)) / np.sqrt(3 * c)).astype(np.float32)
        w["mixc%d_b" % i] = rng.uniform(0.05, 0.3, n).astype(np.float32)       # keeps most relu units alive
    w["mixc2_W"] = np.abs(w["mixc2_W"])     # the single output channel stays positive: the feedback path carries gradient
    enc, dec0, tgt, oth = O.synthetic_batch(171 + B, B, T_in, T_out, num_others=U - 1)
    tgt = np.abs(tgt)
    y_np = O.others_mixing_forward(enc.astype(np.float64), oth.astype(np.float64), dec0.astype(np.float64), f64(w), act=act, mixing="conv")
    loss_ref, g_ref, y_ref = _torch_mixing_graph(enc, oth, dec0, tgt, w, act, mixing="conv")
    np.testing.assert_allclose(y_np, y_ref, atol=1e-12)
    assert (y_ref > 0).mean() > 0.5
    tr = OthersConvMixingTrainer(w, act=act)
    loss, y = tr.forward_backward(dev(enc), dev(oth), dev(dec0), dev(tgt))
    tr.check()
    assert abs(float(loss.item()) - loss_ref) <= 1e-5 * loss_ref + 1e-9
    np.testing.assert_allclose(y.cpu().numpy(), y_ref, atol=2e-5)
    for k in _CONV_MIX_ORDER:
        a = tr.g[k].detach().cpu().numpy().astype(np.float64)
        scale = np.abs(g_ref[k]).max()
        err = np.abs(a - g_ref[k]).max()
        print("conv mixing H%d grad %-8s max|ref| %.3e  max err %.3e" % (H, k, scale, err))
        assert scale > 0 and err <= 1e-4 * scale + 1e-9, (k, err, scale)
    m = OthersConvMixingSeq2Seq(latent_dim=H, num_user=U, recurrent_activation=act, seed=1)
    m.set_weights([w[k] for k in _CONV_MIX_ORDER])
    got = m.predict([enc, oth, dec0])
    np.testing.assert_allclose(got, y_ref, atol=2e-5)
    m.compile(optimizer="Adam", loss="mean_squared_error")
    losses = [m.train_on_batch([enc, oth, dec0], tgt) for _ in range(5)]
    assert abs(losses[0] - loss_ref) <= 1e-5 * loss_ref + 1e-9 and losses[-1] < losses[0]
    h = m.fit([enc, oth, dec0], tgt, batch_size=16, epochs=2, validation_split=0.2)
    assert len(h.history["loss"]) == 2 and "val_loss" in h.history
    import os, tempfile
    with tempfile.TemporaryDirectory() as d:
        m.save_weights(os.path.join(d, "conv_mixing.h5"))
        m2 = OthersConvMixingSeq2Seq(latent_dim=H, num_user=U, recurrent_activation=act, seed=9)
        m2.load_weights(os.path.join(d, "conv_mixing.h5"))
        np.testing.assert_array_equal(m2.predict([enc, oth, dec0]), m.predict([enc, oth, dec0]))


def test_others_mixing_fit_surface():
    from longterm360fov_amd.models import OthersMixingSeq2Seq
    np.random.seed(1)
    enc, dec0, tgt, oth = O.synthetic_batch(3, 96, 6, 5, num_others=33)
    m = OthersMixingSeq2Seq(latent_dim=64, num_user=34, seed=2)
    m.compile(optimizer="Adam", loss="mean_squared_error", metrics=["accuracy"])
    h = m.fit([enc, oth, dec0], tgt, batch_size=32, epochs=3, validation_split=0.1, shuffle=True, initial_epoch=0)
    assert len(h.history["loss"]) == 3 and h.history["loss"][-1] < h.history["loss"][0] and "val_loss" in h.history
    assert m.predict([enc[:4], oth[:4], dec0[:4]]).shape == (4, 5, 6)

    def gen():
        while True:
            for lo in range(0, 96, 32):
                yield [enc[lo:lo + 32], oth[lo:lo + 32], dec0[lo:lo + 32]], tgt[lo:lo + 32]
    h2 = m.fit_generator(gen(), steps_per_epoch=3, epochs=2, validation_data=gen(), validation_steps=1)
    assert len(h2.history["loss"]) == 2 and "val_loss" in h2.history


@pytest.mark.parametrize("N,In,Out", [(5000, 64, 6), (9001, 40, 12), (300, 256, 6), (4096, 16, 1)])
def test_dense_bwd_tall_narrow(N, In, Out):
    """Dense backward on the (B*T, 6)-shaped operands of the training graph (FoV_seq2seq.py:96-97 under
    model.fit): every colsum variant (narrow rows-per-thread, column-per-thread) and GEMM staging path."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(N + Out)
    x = rng.standard_normal((N, In)).astype(np.float32)
    W = rng.standard_normal((In, Out)).astype(np.float32)
    d = rng.standard_normal((N, Out)).astype(np.float32)
    dx, dW, db = ops.dense_bwd(dev(x), dev(W), dev(d))
    x64, W64, d64 = x.astype(np.float64), W.astype(np.float64), d.astype(np.float64)
    for got, ref, name in ((dx, d64 @ W64.T, "dx"), (dW, x64.T @ d64, "dW"), (db, d64.sum(0), "db")):
        err = np.abs(got.cpu().numpy() - ref).max()
        assert err <= 2e-5 * np.abs(ref).max() + 1e-6, (name, err)
    # accumulate adds to what is there
    dW0, db0 = dW.clone(), db.clone()
    ops.dense_bwd(dev(x), dev(W), dev(d), dW=dW, db=db, need_dx=False, accumulate=True)
    assert torch.allclose(dW, 2 * dW0, rtol=1e-5, atol=1e-5) and torch.allclose(db, 2 * db0, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("N,H,O", [(37, 64, 6), (512, 256, 6), (5, 128, 3)])
def test_mix_head_forward_backward(N, H, O):
    """One decoder step of the mixing head (given_others...py:127-130,168,257-265) as single launches, against
    torch.autograd fp64; `add` is a strided row view like others_proj[:, t]."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(N + H)
    h = rng.standard_normal((N, H)).astype(np.float32)
    Wd = (rng.standard_normal((H, O)) / np.sqrt(H)).astype(np.float32)
    bd = rng.standard_normal(O).astype(np.float32) * 0.1
    Wp = (rng.standard_normal((O, O)) * 0.5).astype(np.float32)
    add = rng.standard_normal((N, 3, O)).astype(np.float32)
    dml = rng.standard_normal((N, O)).astype(np.float32)
    dfb = rng.standard_normal((N, O)).astype(np.float32)
    t = lambda a: torch.tensor(a.astype(np.float64), requires_grad=True)
    th, tWd, tbd, tWp = t(h), t(Wd), t(bd), t(Wp)
    p_ref = torch.tanh(th @ tWd + tbd)
    zm = p_ref @ tWp + torch.tensor(add[:, 1].astype(np.float64))
    m_ref = torch.tanh(zm)
    # loss gradient arrives w.r.t. the pre-tanh of m, the feedback gradient w.r.t. m itself
    ((zm * torch.tensor(dml.astype(np.float64))).sum() + (m_ref * torch.tensor(dfb.astype(np.float64))).sum()).backward()
    p_out = torch.empty((N, O), device="cuda"); m_out = torch.empty((N, O), device="cuda")
    ops.mix_head_fwd(dev(h), dev(Wd), dev(bd), dev(Wp), dev(add)[:, 1], p_out, m_out)
    assert np.abs(p_out.cpu().numpy() - p_ref.detach().numpy()).max() < 2e-6
    assert np.abs(m_out.cpu().numpy() - m_ref.detach().numpy()).max() < 2e-6
    dpm = torch.empty((N, O), device="cuda"); dpp = torch.empty((N, O), device="cuda")
    dh = ops.mix_head_bwd(dev(dml), dev(dfb), m_out, p_out, dev(Wp), dev(Wd), dpm, dpp)
    assert np.abs(dh.cpu().numpy() - th.grad.numpy()).max() <= 2e-5 * np.abs(th.grad.numpy()).max() + 1e-7
    # the pre-activation gradients reproduce the weight gradients: dWp = p^T dpre_m, dWd = h^T dpre_p
    dWp = p_out.double().T @ dpm.double()
    dWd = dev(h).double().T @ dpp.double()
    assert np.abs(dWp.cpu().numpy() - tWp.grad.numpy()).max() <= 2e-5 * np.abs(tWp.grad.numpy()).max() + 1e-7
    assert np.abs(dWd.cpu().numpy() - tWd.grad.numpy()).max() <= 2e-5 * np.abs(tWd.grad.numpy()).max() + 1e-7
    dh0 = ops.mix_head_bwd(dev(dml), None, m_out, p_out, dev(Wp), dev(Wd), dpm, dpp)   # last step: no feedback
    assert np.isfinite(dh0.cpu().numpy()).all()


def _torch_tf_lstm_graph(x, y, cells, head, init, fps, running_length, forget_bias=1.0, masks=None):
    """Independent fp64 restatement of the lstm.py training graph (tf.contrib LSTMCell: fused [x,h].W, gates
    i, j, f, o, forget_bias inside the cell; heads of _pred_mean_var_xyz2_new; likelihood_loss_tf)."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    cw = [(t(W), t(b)) for W, b in cells]
    hw = {k: t(v) for k, v in head.items()}
    inp = torch.tensor(x.astype(np.float64))
    st = torch.tensor(init.astype(np.float64))
    finals = []
    for l, (W, b) in enumerate(cw):
        c, h = st[l, 0], st[l, 1]
        H = h.shape[1]
        outs = []
        for tt in range(inp.shape[1]):
            z = torch.cat([inp[:, tt], h], 1) @ W + b
            i, j, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
            c = torch.sigmoid(f + forget_bias) * c + torch.sigmoid(i) * torch.tanh(j)
            h = torch.sigmoid(o) * torch.tanh(c)
            outs.append(h)
        hs = torch.stack(outs, 1)
        finals.append((c, h))
        inp = hs if (masks is None or l == len(cw) - 1) else hs * torch.tensor(masks[l].astype(np.float64))
    hT = finals[-1][1]
    mu = torch.tanh(torch.relu(hT @ hw["mu_W1"] + hw["mu_b1"]) @ hw["mu_W2"] + hw["mu_b2"])
    var = torch.exp(torch.relu(hT @ hw["var_W1"] + hw["var_b1"]) @ hw["var_W2"] + hw["var_b2"])
    yy = torch.tensor(y.astype(np.float64)).reshape(y.shape[0], y.shape[1], fps, 3)
    eps = 1e-20
    l = torch.log(var + eps)[:, None, None, :] + (yy - mu[:, None, None, :]) ** 2 / (var + eps)[:, None, None, :]
    loss = torch.clamp(l, -10, 10).sum((1, 2, 3)).mean() / running_length / fps
    loss.backward()
    return float(loss.detach()), [(W.grad.numpy(), b.grad.numpy()) for W, b in cw], {k: v.grad.numpy() for k, v in hw.items()}, \
        mu.detach().numpy(), var.detach().numpy()


@pytest.mark.parametrize("H,B,T,with_masks", [(40, 9, 4, False), (400, 12, 3, True), (400, 32, 10, False), (400, 20, 2, False)])
def test_tf_stacked_lstm_training_graph(H, B, T, with_masks):
    """a10 training: mycode/lstm.py (2 x LSTMCell(H) with a fed state, mean / variance heads, Gaussian NLL, TF
    RMSProp with clipping) against torch.autograd fp64; gradients are compared in tf.contrib layout."""
    from longterm360fov_amd.training import TFLSTMTrainer
    from longterm360fov_amd.models import convert_tf_lstmcell
    rng = np.random.default_rng(H + B)
    F, fps = 90, 30
    cells = []
    for l in range(2):
        Fin = F if l == 0 else H
        cells.append(((rng.standard_normal((Fin + H, 4 * H)) / np.sqrt(Fin + H)).astype(np.float32),
                      (0.1 * rng.standard_normal(4 * H)).astype(np.float32)))
    head = {}
    for br in ("mu", "var"):
        head[br + "_W1"] = (rng.standard_normal((H, 32)) / np.sqrt(H)).astype(np.float32)
        head[br + "_b1"] = (0.1 * rng.standard_normal(32)).astype(np.float32)
        head[br + "_W2"] = (rng.standard_normal((32, 3)) / np.sqrt(32)).astype(np.float32)
        head[br + "_b2"] = (0.1 * rng.standard_normal(3)).astype(np.float32)
    x = rng.uniform(-1, 1, (B, T, F)).astype(np.float32)
    y = rng.uniform(-1, 1, (B, 1, 3 * fps)).astype(np.float32)
    init = (0.2 * rng.standard_normal((2, 2, B, H))).astype(np.float32)
    masks = None
    if with_masks:   # DropoutWrapper(output_keep_prob=0.9) on what layer 0 hands up
        masks = [((rng.random((B, T, H)) < 0.9) / 0.9).astype(np.float32), None]
    loss_ref, cg, hg, mu_ref, var_ref = _torch_tf_lstm_graph(x, y, cells, head, init, fps, 10, masks=masks)
    tr = TFLSTMTrainer(cells, head, lr=1e-3, clip_value=1.0, fps=fps, running_length=10)
    dm = None if masks is None else [dev(masks[0]), None]
    loss, mu, var, state = tr.forward_backward(dev(x), dev(y), dev(init), masks=dm)
    assert np.abs(mu.cpu().numpy() - mu_ref).max() < 1e-5 and np.abs(var.cpu().numpy() - var_ref).max() < 1e-4 * np.abs(var_ref).max()
    assert abs(float(loss.item()) - loss_ref) <= 1e-5 * abs(loss_ref) + 1e-7
    # H = 400 runs zero-padded at width 512 (lstm_wide16.hip forward with the tape, lstm_bwd16.hip BPTT), H = 40 at 64
    assert tr.Hp == (512 if H == 400 else 64) and tr.w["R0"].shape == (tr.Hp, 4 * tr.Hp) and state.shape == (2, 2, B, H)
    assert tr.padded_slices_are_zero()
    tg = tr.grads_numpy()
    for k in TFLSTMTrainer.HEAD:
        a = tg[k]
        assert np.abs(a - hg[k]).max() <= 2e-4 * np.abs(hg[k]).max() + 1e-9, k
    for l in range(2):   # gradients in tf.contrib layout: columns i, j, f, o of the fused kernel
        K, R, b = (tg["%s%d" % (n, l)] for n in ("K", "R", "b"))
        perm = np.concatenate([np.arange(0, H), np.arange(2 * H, 3 * H), np.arange(H, 2 * H), np.arange(3 * H, 4 * H)])
        Wg = np.empty_like(cg[l][0]); Wg[:, perm] = np.concatenate([K, R], 0)
        bg = np.empty_like(cg[l][1]); bg[perm] = b
        assert np.abs(Wg - cg[l][0]).max() <= 2e-4 * np.abs(cg[l][0]).max() + 1e-9, ("W", l)
        assert np.abs(bg - cg[l][1]).max() <= 2e-4 * np.abs(cg[l][1]).max() + 1e-9, ("b", l)
    # the fused two-head launches (tf_head.hip) against the generic Dense / activation entry points
    os.environ["FOV_NO_TF_HEAD"] = "1"
    try:
        loss_u, mu_u, var_u, _ = tr.forward_backward(dev(x), dev(y), dev(init), masks=dm)
        tg_u = tr.grads_numpy()
    finally:
        os.environ.pop("FOV_NO_TF_HEAD", None)
    assert np.abs(mu_u.cpu().numpy() - mu.cpu().numpy()).max() < 2e-6 and abs(float(loss_u.item()) - float(loss.item())) < 1e-6
    for k in tr.order:
        assert np.abs(tg_u[k] - tg[k]).max() <= 2e-5 * np.abs(tg[k]).max() + 1e-9, k
    # round trip of the layout conversion, then a few optimizer steps reduce the loss
    for (W0, b0), (W1, b1) in zip(cells, tr.cells_tf()):
        assert np.abs(W0 - W1).max() < 1e-7 and np.abs(b0 - b1).max() < 1e-6
    l0 = float(tr.train_step(dev(x), dev(y), dev(init))[0].item())
    for _ in range(5):
        l1 = float(tr.train_step(dev(x), dev(y), dev(init))[0].item())
    assert l1 < l0
    assert tr.padded_slices_are_zero()
    # the unpadded trainer (step-wise / generic kernels) takes the same steps
    tu = TFLSTMTrainer(cells, head, lr=1e-3, clip_value=1.0, fps=fps, running_length=10, pad=False)
    assert tu.Hp == H
    for _ in range(6):
        tu.train_step(dev(x), dev(y), dev(init))
    for (W0, b0), (W1, b1) in zip(tu.cells_tf(), tr.cells_tf()):
        assert np.abs(W0 - W1).max() < 2e-5 and np.abs(b0 - b1).max() < 2e-5
    # TF RMSProp semantics: ms starts at one, eps inside the root, clipped gradient
    p = torch.zeros(3, device="cuda"); gg = torch.tensor([0.5, -3.0, 0.0], device="cuda"); ms = torch.ones(3, device="cuda")
    from longterm360fov_amd import ops
    ops.rmsprop_tf_step(p, gg, ms, lr=0.1, decay=0.9, eps=1e-10, clip_value=1.0)
    gc = np.array([0.5, -1.0, 0.0]); ms_ref = 0.9 + 0.1 * gc ** 2
    assert np.allclose(ms.cpu().numpy(), ms_ref, atol=1e-6) and np.allclose(p.cpu().numpy(), -0.1 * gc / np.sqrt(ms_ref + 1e-10), atol=1e-6)


def _torch_self_fed_graph(enc, dec0, tgt, w, act, no_init, residual, enc_as_in, dact, embed=False, tgt_rec=None):
    """Independent fp64 reference of FoV_seq2seq_no_teac_forc.py:37-149 (onelayer_tar_seq2seq) on torch.autograd."""
    t = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in w.items()}
    H = w["enc_R"].shape[0]
    s = torch.sigmoid if act == "sigmoid" else (lambda z: torch.clamp(0.2 * z + 0.5, 0, 1))
    fa = torch.tanh if dact == "tanh" else torch.relu

    def step(x, h, c, K, R, b):
        z = x @ K + b + h @ R
        i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
        c = f * c + i * g
        return o * torch.tanh(c), c

    e, d0, tg = (torch.tensor(a.astype(np.float64)) for a in (enc, dec0, tgt))
    B = e.shape[0]
    h = c = torch.zeros(B, H, dtype=torch.float64)
    for tt in range(e.shape[1]):
        h, c = step(e[:, tt], h, c, t["enc_K"], t["enc_R"], t["enc_b"])
    h_enc, sh, sc = h, h, c
    if embed:
        sh, sc = torch.tanh(h @ t["emb1_W"] + t["emb1_b"]), torch.tanh(c @ t["emb2_W"] + t["emb2_b"])
    x0 = fa(h_enc @ t["dense_W"] + t["dense_b"]) if enc_as_in else d0[:, 0]
    h, c = (torch.zeros(B, H, dtype=torch.float64),) * 2 if no_init else (sh, sc)
    r = fa(x0 @ t["res_W"] + t["res_b"]) if residual else 0.0
    x, outs = x0, []
    for _ in range(tg.shape[1]):
        h, c = step(x, h, c, t["dec_K"], t["dec_R"], t["dec_b"])
        x = fa(h @ t["dense_W"] + t["dense_b"]) + r
        outs.append(x)
    y = torch.stack(outs, 1)
    loss = torch.mean((y - tg) ** 2)
    rec = None
    if tgt_rec is not None:     # reconstruction decoder: its own LSTM + Dense(F, tanh), seeded with the same states
        x, h, c, outs = torch.tanh(h_enc @ t["recd_W"] + t["recd_b"]), sh, sc, []
        for _ in range(tg.shape[1]):
            h, c = step(x, h, c, t["rec_K"], t["rec_R"], t["rec_b"])
            x = torch.tanh(h @ t["recd_W"] + t["recd_b"])
            outs.append(x)
        rec = torch.stack(outs, 1)
        loss = loss + torch.mean((rec - torch.tensor(tgt_rec.astype(np.float64))) ** 2)
    loss.backward()
    grads = {k: (np.zeros_like(w[k], dtype=np.float64) if v.grad is None else v.grad.numpy()) for k, v in t.items()}
    if rec is not None:
        return float(loss), grads, y.detach().numpy(), rec.detach().numpy()
    return float(loss), grads, y.detach().numpy()


@pytest.mark.parametrize("H,B,T_in,T_out,act,no_init,residual,enc_as_in,dact", [
    (64, 21, 4, 5, "sigmoid", True, False, False, "tanh"),          # the script as committed (:29, cfg defaults)
    (128, 33, 5, 4, "hard_sigmoid", False, False, False, "tanh"),   # decoder seeded with the encoder state
    (256, 40, 3, 6, "sigmoid", False, True, False, "tanh"),         # cfg.add_residual_link
    (64, 17, 4, 3, "hard_sigmoid", True, False, True, "tanh"),      # cfg.enc_last_out_as_dec_in
    (32, 9, 3, 4, "sigmoid", False, True, True, "relu"),            # all of them + cfg.rescale_input
])
def test_no_teacher_forcing_one_layer_gradients_and_training(H, B, T_in, T_out, act, no_init, residual, enc_as_in, dact):
    """§8(f) rank 3 sibling topology: forward against the NumPy oracle, gradients of the self-fed unrolled graph
    against torch.autograd fp64, the model object's predict against the oracle, and Adam steps reduce the loss."""
    from longterm360fov_amd.models import NoTeacherForcingSeq2Seq
    from longterm360fov_amd.training import SelfFedSeq2SeqTrainer
    w = O.init_seq2seq(90 + H, H=H, bias_noise=0.1)
    rng = np.random.default_rng(H + B)
    if residual:
        w["res_W"] = rng.uniform(-0.5, 0.5, (6, 6)).astype(np.float32)
        w["res_b"] = rng.uniform(-0.1, 0.1, 6).astype(np.float32)
    enc, dec0, tgt = O.synthetic_batch(91 + B, B, T_in, T_out)
    if dact == "relu":
        tgt = np.abs(tgt)
    kw = dict(decoder_no_init_state=no_init, add_residual_link=residual, enc_last_out_as_dec_in=enc_as_in)
    y_np = O.onelayer_tar_seq2seq_forward(enc.astype(np.float64), dec0.astype(np.float64), f64(w), T_out, act=act,
                                          dense_activation=dact, **kw)
    loss_ref, g_ref, y_ref = _torch_self_fed_graph(enc, dec0, tgt, w, act, no_init, residual, enc_as_in, dact)
    np.testing.assert_allclose(y_np, y_ref, atol=1e-12)
    tr = SelfFedSeq2SeqTrainer(w, act=act, dense_activation=dact, **kw)
    loss, y = tr.forward_backward(dev(enc), dev(dec0), dev(tgt))
    tr.ws.check(); tr.bwd_scratch.check()
    assert abs(float(loss.item()) - loss_ref) <= 1e-5 * loss_ref + 1e-9
    np.testing.assert_allclose(y.cpu().numpy(), y_ref, atol=2e-5)
    for k in tr.g:
        a = tr.g[k].detach().cpu().numpy().astype(np.float64)
        scale = max(np.abs(g_ref[k]).max(), 1e-30)
        err = np.abs(a - g_ref[k]).max()
        print("self-fed H%d grad %-8s max|ref| %.3e  max err %.3e" % (H, k, scale, err))
        assert err <= 1e-4 * scale + 1e-9, (k, err, scale)
    if no_init and not enc_as_in:       # reference quirk: the encoder does not reach the loss
        assert float(tr.g["enc_K"].abs().max()) == 0.0
    m = NoTeacherForcingSeq2Seq(latent_dim=H, recurrent_activation=act, predict_step=T_out, rescale_input=(dact == "relu"), **kw)
    order = list(_W_ORDER) + (["res_W", "res_b"] if residual else [])
    m.set_weights([w[k] for k in order])
    got = m.predict(enc if enc_as_in else [enc, dec0])
    assert got.shape == (B, T_out, 6)
    np.testing.assert_allclose(got, y_ref, atol=2e-5)
    assert (np.abs(got - y_ref) <= 1e-3 * np.abs(y_ref) + 1e-5).all()
    m.compile(optimizer="Adam", loss="mean_squared_error")
    losses = [m.train_on_batch(enc if enc_as_in else [enc, dec0], tgt) for _ in range(4)]
    assert losses[-1] < losses[0]
    h = m.fit(enc if enc_as_in else [enc, dec0], tgt, batch_size=16, epochs=2, validation_split=0.2)
    assert len(h.history["loss"]) == 2 and "val_loss" in h.history


@pytest.mark.parametrize("H,B,T,act,no_init,residual,enc_as_in,embed,recons", [
    (64, 19, 4, "sigmoid", False, False, False, True, False),       # cfg.embed_frame_state_enc2dec alone
    (64, 21, 5, "sigmoid", True, False, True, False, True),         # cfg.has_reconstruct_loss as the script wires it (:135, :267)
    (128, 33, 4, "hard_sigmoid", False, True, True, True, True),    # both, + residual link, decoder seeded with the embedded state
    (256, 24, 3, "sigmoid", True, False, False, True, True),        # zero-state decoder: the encoder is reached only through the reconstruction
    (32, 17, 3, "sigmoid", False, True, True, True, True),          # the scripts' latent_dim: predict runs zero-padded to 64 units, embeddings / reconstruction layers included
])
def test_no_teacher_forcing_embedded_state_and_reconstruction_decoder(H, B, T, act, no_init, residual, enc_as_in, embed, recons):
    """cfg.embed_frame_state_enc2dec (FoV_seq2seq_no_teac_forc.py:47-52: Dense(latent_dim, tanh) on the encoder's h and c) and
    cfg.has_reconstruct_loss (:56-59,90-95,120-139: second self-fed LSTM + Dense(num_encoder_tokens, tanh), two outputs,
    MSE + MSE, target encoder_input[:, ::-1] :267): forward against the NumPy oracle, all gradients against torch.autograd
    fp64, the model object's two-output predict / fit surface."""
    from longterm360fov_amd.models import NoTeacherForcingSeq2Seq
    from longterm360fov_amd.training import SelfFedSeq2SeqTrainer, self_fed_weight_order
    F = 90
    w = O.init_seq2seq(190 + H, H=H, bias_noise=0.1)
    rng = np.random.default_rng(H + B)
    u = lambda *shape: rng.uniform(-0.3, 0.3, shape).astype(np.float32)
    if residual:
        w["res_W"], w["res_b"] = u(6, 6), u(6)
    if embed:
        w["emb1_W"], w["emb1_b"], w["emb2_W"], w["emb2_b"] = u(H, H) / 4, u(H), u(H, H) / 4, u(H)
    if recons:
        w["rec_K"], w["rec_R"], w["rec_b"] = O.init_lstm(rng, F, H)
        w["recd_W"], w["recd_b"] = u(H, F), u(F)
    enc, dec0, tgt = O.synthetic_batch(291 + B, B, T, T)
    tgt_rec = np.ascontiguousarray(enc[:, ::-1, :]) if recons else None
    kw = dict(decoder_no_init_state=no_init, add_residual_link=residual, enc_last_out_as_dec_in=enc_as_in,
              embed_frame_state_enc2dec=embed, has_reconstruct_loss=recons)
    ref = _torch_self_fed_graph(enc, dec0, tgt, w, act, no_init, residual, enc_as_in, "tanh", embed=embed, tgt_rec=tgt_rec)
    loss_ref, g_ref, y_ref = ref[:3]
    y_np = O.onelayer_tar_seq2seq_forward(enc.astype(np.float64), dec0.astype(np.float64), f64(w), T, act=act, **kw)
    if recons:
        np.testing.assert_allclose(y_np[0], y_ref, atol=1e-12)
        np.testing.assert_allclose(y_np[1], ref[3], atol=1e-12)
    else:
        np.testing.assert_allclose(y_np, y_ref, atol=1e-12)
    tr = SelfFedSeq2SeqTrainer(w, act=act, **kw)
    packed = np.concatenate([tgt, tgt_rec], -1) if recons else tgt
    loss, y = tr.forward_backward(dev(enc), dev(dec0), dev(packed))
    tr.check()
    assert abs(float(loss.item()) - loss_ref) <= 1e-5 * loss_ref + 1e-9
    np.testing.assert_allclose(y.cpu().numpy()[..., :6], y_ref, atol=2e-5)
    if recons:
        np.testing.assert_allclose(y.cpu().numpy()[..., 6:], ref[3], atol=2e-5)
    assert set(tr.g) == set(self_fed_weight_order(residual, embed, recons))
    for k in tr.g:
        a = tr.g[k].detach().cpu().numpy().astype(np.float64)
        scale = max(np.abs(g_ref[k]).max(), 1e-30)
        err = np.abs(a - g_ref[k]).max()
        print("self-fed+ H%d grad %-8s max|ref| %.3e  max err %.3e" % (H, k, scale, err))
        assert err <= 1e-4 * scale + 1e-9, (k, err, scale)
    if embed and no_init and not recons:
        assert float(tr.g["emb1_W"].abs().max()) == 0.0       # zero-state decoder: the embedding is not reached
    assert float(tr.g["enc_K"].abs().max()) > 0.0 or (no_init and not enc_as_in and not recons)
    m = NoTeacherForcingSeq2Seq(latent_dim=H, recurrent_activation=act, predict_step=T, **kw)
    m.set_weights([w[k] for k in self_fed_weight_order(residual, embed, recons)])
    x = [enc, np.zeros((B, T, 6), np.float32)] if enc_as_in else [enc, dec0]     # [encoder_inputs, time_ind_input] (:135) / [enc, dec0]
    got = m.predict(x)
    if recons:
        assert isinstance(got, list) and got[0].shape == (B, T, 6) and got[1].shape == (B, T, F)
        np.testing.assert_allclose(got[0], y_ref, atol=2e-5)
        np.testing.assert_allclose(got[1], ref[3], atol=2e-5)
    else:
        np.testing.assert_allclose(got, y_ref, atol=2e-5)
    m.compile(optimizer="Adam", loss="mean_squared_error")
    yt = [tgt, tgt_rec] if recons else tgt
    l0 = m.train_on_batch(x, yt)
    assert abs(l0 - loss_ref) <= 1e-5 * loss_ref + 1e-9
    losses = [l0] + [m.train_on_batch(x, yt) for _ in range(4)]
    assert losses[-1] < losses[0]
    h = m.fit(x, yt, batch_size=8, epochs=2, validation_split=0.25)
    assert len(h.history["loss"]) == 2 and "val_loss" in h.history
    if recons:
        with pytest.raises(ValueError):
            m.train_on_batch(x, tgt)
    # Keras HDF5 round trip with the extra layers
    import os, tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "self_fed.h5")
        m.save_weights(path)
        m2 = NoTeacherForcingSeq2Seq(latent_dim=H, recurrent_activation=act, predict_step=T, seed=3, **kw)
        m2.load_weights(path)
        for a, b in zip(m.get_weights(), m2.get_weights()):
            assert np.array_equal(a, b)


def _torch_tf_lstm_refeed_graph(x, y, cells, head, init, fps, running_length, noise, forget_bias=1.0, masks=None):
    """fp64 restatement of the predict_len > 1 training graph of lstm.py:446-468: the window is shifted by one second,
    its last slot is tf.random_normal(mean=mu, stddev=sqrt(var)) = mu + sqrt(var) * noise (utility.py:83-89, frames
    interleaved x,y,z by tf.stack axis=-1), the whole stack re-runs from the same fed state and the losses add up."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    cw = [(t(W), t(b)) for W, b in cells]
    hw = {k: t(v) for k, v in head.items()}
    st = torch.tensor(init.astype(np.float64))

    def run(inp, mk):
        for l, (W, b) in enumerate(cw):
            c, h = st[l, 0], st[l, 1]
            H = h.shape[1]
            outs = []
            for tt in range(inp.shape[1]):
                z = torch.cat([inp[:, tt], h], 1) @ W + b
                i, j, f, o = z[:, :H], z[:, H:2 * H], z[:, 2 * H:3 * H], z[:, 3 * H:]
                c = torch.sigmoid(f + forget_bias) * c + torch.sigmoid(i) * torch.tanh(j)
                h = torch.sigmoid(o) * torch.tanh(c)
                outs.append(h)
            hs = torch.stack(outs, 1)
            inp = hs if (mk is None or l == len(cw) - 1) else hs * torch.tensor(mk[l].astype(np.float64))
        mu = torch.tanh(torch.relu(h @ hw["mu_W1"] + hw["mu_b1"]) @ hw["mu_W2"] + hw["mu_b2"])
        var = torch.exp(torch.relu(h @ hw["var_W1"] + hw["var_b1"]) @ hw["var_W2"] + hw["var_b2"])
        return mu, var

    def nll(mu, var, yk):
        yy = yk.reshape(yk.shape[0], 1, fps, 3)
        l = torch.log(var + 1e-20)[:, None, None, :] + (yy - mu[:, None, None, :]) ** 2 / (var + 1e-20)[:, None, None, :]
        return torch.clamp(l, -10, 10).sum((1, 2, 3)).mean() / running_length / fps

    win = torch.tensor(x.astype(np.float64))
    yt = torch.tensor(y.astype(np.float64))
    nz = torch.tensor(noise.astype(np.float64))
    B = win.shape[0]
    loss = 0.0
    for k in range(y.shape[1]):
        if k > 0:
            smp = (mu[:, None, :] + torch.sqrt(var)[:, None, :] * nz[k - 1].reshape(B, fps, 3)).reshape(B, 1, 3 * fps)
            win = torch.cat([win[:, 1:], smp], 1)
        mu, var = run(win, None if masks is None else masks[k])
        loss = loss + nll(mu, var, yt[:, k])
    loss.backward()
    return float(loss.detach()), [(W.grad.numpy(), b.grad.numpy()) for W, b in cw], {k: v.grad.numpy() for k, v in hw.items()}, \
        mu.detach().numpy(), var.detach().numpy()


@pytest.mark.parametrize("H,B,T,P,with_masks", [(40, 9, 3, 5, False), (400, 12, 4, 3, True)])
def test_tf_stacked_lstm_sampled_refeed_training_graph(H, B, T, P, with_masks):
    """a10, the predict_len > 1 form mycode/config.py:21 ships: sampled re-feed through fov_sample_refeed_fwd / _bwd with the
    noise given explicitly, P windows (P > T: early samples shift out of the window), against torch.autograd fp64."""
    from longterm360fov_amd.training import TFLSTMTrainer
    rng = np.random.default_rng(7 * H + B)
    F, fps = 90, 30
    cells = []
    for l in range(2):
        Fin = F if l == 0 else H
        cells.append(((rng.standard_normal((Fin + H, 4 * H)) / np.sqrt(Fin + H)).astype(np.float32),
                      (0.1 * rng.standard_normal(4 * H)).astype(np.float32)))
    head = {}
    for br in ("mu", "var"):
        head[br + "_W1"] = (rng.standard_normal((H, 32)) / np.sqrt(H)).astype(np.float32)
        head[br + "_b1"] = (0.1 * rng.standard_normal(32)).astype(np.float32)
        head[br + "_W2"] = (rng.standard_normal((32, 3)) / np.sqrt(32)).astype(np.float32)
        head[br + "_b2"] = (0.1 * rng.standard_normal(3)).astype(np.float32)
    x = rng.uniform(-1, 1, (B, T, F)).astype(np.float32)
    y = rng.uniform(-1, 1, (B, P, 3 * fps)).astype(np.float32)
    init = (0.2 * rng.standard_normal((2, 2, B, H))).astype(np.float32)
    noise = rng.standard_normal((P - 1, B, F)).astype(np.float32)
    masks = None
    if with_masks:   # a fresh DropoutWrapper mask per dynamic_rnn call
        masks = [[((rng.random((B, T, H)) < 0.9) / 0.9).astype(np.float32), None] for _ in range(P)]
    loss_ref, cg, hg, mu_ref, var_ref = _torch_tf_lstm_refeed_graph(x, y, cells, head, init, fps, 10, noise, masks=masks)
    tr = TFLSTMTrainer(cells, head, lr=1e-3, clip_value=1.0, fps=fps, running_length=10)
    dm = None if masks is None else [[dev(m[0]), None] for m in masks]
    loss, mu, var, state = tr.forward_backward(dev(x), dev(y), dev(init), masks=dm, noise=dev(noise))
    assert state.shape == (2, 2, B, H)
    assert np.abs(mu.cpu().numpy() - mu_ref).max() < 2e-5 and np.abs(var.cpu().numpy() - var_ref).max() < 1e-4 * np.abs(var_ref).max()
    assert abs(float(loss.item()) - loss_ref) <= 1e-5 * abs(loss_ref) + 1e-7
    tg = tr.grads_numpy()
    assert tr.padded_slices_are_zero()
    for k in TFLSTMTrainer.HEAD:
        a = tg[k]
        print("refeed head grad %-7s max|ref| %.3e err %.3e" % (k, np.abs(hg[k]).max(), np.abs(a - hg[k]).max()))
        assert np.abs(a - hg[k]).max() <= 2e-4 * np.abs(hg[k]).max() + 1e-9, k
    for l in range(2):
        K, R, b = (tg["%s%d" % (n, l)] for n in ("K", "R", "b"))
        perm = np.concatenate([np.arange(0, H), np.arange(2 * H, 3 * H), np.arange(H, 2 * H), np.arange(3 * H, 4 * H)])
        Wg = np.empty_like(cg[l][0]); Wg[:, perm] = np.concatenate([K, R], 0)
        bg = np.empty_like(cg[l][1]); bg[perm] = b
        assert np.abs(Wg - cg[l][0]).max() <= 2e-4 * np.abs(cg[l][0]).max() + 1e-9, ("W", l)
        assert np.abs(bg - cg[l][1]).max() <= 2e-4 * np.abs(cg[l][1]).max() + 1e-9, ("b", l)
    losses = [float(tr.train_step(dev(x), dev(y), dev(init), masks=dm, noise=dev(noise))[0].item()) for _ in range(6)]
    assert losses[-1] < losses[0]


@pytest.mark.parametrize("std,planar", [("sqrt", False), ("var", True)])
def test_sample_refeed_kernels(std, planar):
    """fov_sample_refeed_fwd / _bwd: both stddev conventions (lstm.py sqrt(var); lstm_keras.py:39-44 var) and both layouts,
    writing into / reading from a slot of a (B,T,90) window; backward against torch.autograd."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(3)
    B, fps, T = 37, 30, 4
    mu = torch.tensor(rng.uniform(-1, 1, (B, 3)), requires_grad=True)
    var = torch.tensor(rng.uniform(0.05, 1.0, (B, 3)), requires_grad=True)
    nz = torch.tensor(rng.standard_normal((B, 3 * fps)))
    sd = torch.sqrt(var) if std == "sqrt" else var
    if planar:
        xr = (mu[:, :, None] + sd[:, :, None] * nz.reshape(B, 3, fps)).reshape(B, 3 * fps)
    else:
        xr = (mu[:, None, :] + sd[:, None, :] * nz.reshape(B, fps, 3)).reshape(B, 3 * fps)
    dxr = torch.tensor(rng.standard_normal((B, 3 * fps)))
    (xr * dxr).sum().backward()
    win = torch.zeros((B, T, 3 * fps), dtype=torch.float32, device="cuda")
    mu_d, var_d, nz_d = dev(mu.detach().numpy()), dev(var.detach().numpy()), dev(nz.numpy())
    ops.sample_refeed(mu_d, var_d, nz_d, out=win[:, 2], std=std, planar=planar)
    np.testing.assert_allclose(win[:, 2].cpu().numpy(), xr.detach().numpy(), atol=1e-6)
    assert float(win[:, [0, 1, 3]].abs().max()) == 0.0
    dwin = torch.zeros((B, T, 3 * fps), dtype=torch.float32, device="cuda")
    dwin[:, 1] = dev(dxr.numpy())
    dmu = torch.full((B, 3), 0.5, dtype=torch.float32, device="cuda")
    dvar = torch.full((B, 3), -0.25, dtype=torch.float32, device="cuda")
    ops.sample_refeed_bwd(dwin[:, 1], var_d, nz_d, dmu, dvar, std=std, planar=planar, accumulate=True)
    np.testing.assert_allclose(dmu.cpu().numpy() - 0.5, mu.grad.numpy(), atol=2e-5)
    np.testing.assert_allclose(dvar.cpu().numpy() + 0.25, var.grad.numpy(), rtol=1e-4, atol=5e-5)
    ops.sample_refeed_bwd(dwin[:, 1], var_d, nz_d, dmu, dvar, std=std, planar=planar, accumulate=False)
    np.testing.assert_allclose(dmu.cpu().numpy(), mu.grad.numpy(), atol=2e-5)


def test_tf_stacked_lstm_sampled_rollout():
    """lstm.py:714-740 test-time loop (state carried from run to run, one sampled second shifted in per step) against the
    NumPy oracle with the same noise."""
    from longterm360fov_amd.training import TFLSTMTrainer
    rng = np.random.default_rng(11)
    H, B, T, P, F, fps = 48, 10, 4, 6, 90, 30
    cells = []
    for l in range(2):
        Fin = F if l == 0 else H
        cells.append(((rng.standard_normal((Fin + H, 4 * H)) / np.sqrt(Fin + H)).astype(np.float32),
                      (0.1 * rng.standard_normal(4 * H)).astype(np.float32)))
    head = {}
    for br in ("mu", "var"):
        head[br + "_W1"] = (rng.standard_normal((H, 32)) / np.sqrt(H)).astype(np.float32)
        head[br + "_b1"] = (0.1 * rng.standard_normal(32)).astype(np.float32)
        head[br + "_W2"] = (rng.standard_normal((32, 3)) / np.sqrt(32)).astype(np.float32)
        head[br + "_b2"] = (0.1 * rng.standard_normal(3)).astype(np.float32)
    x = rng.uniform(-1, 1, (B, T, F)).astype(np.float32)
    init = (0.2 * rng.standard_normal((2, 2, B, H))).astype(np.float32)
    noise = rng.standard_normal((P, B, F)).astype(np.float32)
    c64 = [(W.astype(np.float64), b.astype(np.float64)) for W, b in cells]
    mu_ref, var_ref, st_ref = O.tf_lstm_sampled_rollout(x.astype(np.float64), c64, {k: v.astype(np.float64) for k, v in head.items()},
                                                         init.astype(np.float64), noise.astype(np.float64))
    tr = TFLSTMTrainer(cells, head, fps=fps, running_length=10)
    mus, vs, st = tr.rollout(dev(x), dev(init), dev(noise))
    np.testing.assert_allclose(mus.cpu().numpy(), mu_ref, atol=2e-5)
    np.testing.assert_allclose(vs.cpu().numpy(), var_ref, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(st.cpu().numpy(), st_ref, atol=2e-5)


def _torch_single_lstm_graph(x, tgt, w, act, unrolled, noise):
    """fp64 torch.autograd restatement of lstm_keras.py (see oracle single_lstm_keras_forward)."""
    t = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in w.items()}
    H = w["R"].shape[0]
    s = torch.sigmoid if act == "sigmoid" else (lambda z: torch.clamp(0.2 * z + 0.5, 0, 1))
    xs, tg = torch.tensor(x.astype(np.float64)), torch.tensor(tgt.astype(np.float64))
    B, F = xs.shape[0], xs.shape[2]
    h = c = torch.zeros(B, H, dtype=torch.float64)
    outs = []
    xin = xs[:, 0]
    for tt in range(tg.shape[1]):
        if not unrolled:
            xin = xs[:, tt]
        z = xin @ t["K"] + t["b"] + h @ t["R"]
        i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
        c = f * c + i * g
        h = o * torch.tanh(c)
        y = torch.tanh(h @ t["dense_W"] + t["dense_b"])
        outs.append(y)
        if unrolled and noise is not None and tt < tg.shape[1] - 1:
            nz = torch.tensor(noise[tt].astype(np.float64)).reshape(B, 3, F // 3)
            xin = (y[:, :3, None] + y[:, 3:6, None] * nz).reshape(B, F)
    y = torch.stack(outs, 1)
    loss = torch.mean((y - tg) ** 2)
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in t.items()}, y.detach().numpy()


@pytest.mark.parametrize("H,B,T,act,unrolled,refeed", [(64, 21, 5, "sigmoid", False, False), (128, 33, 4, "hard_sigmoid", True, False),
                                                       (64, 19, 5, "sigmoid", True, True), (256, 40, 4, "hard_sigmoid", True, True)])
def test_single_lstm_keras_unrollings(H, B, T, act, unrolled, refeed):
    """mycode/lstm_keras.py: the three unrollings (per-step, one-second input repeated, sampled re-feed with the variance as
    stddev in planar layout) - forward vs the NumPy oracle, gradients vs torch.autograd fp64, model-object surface."""
    from longterm360fov_amd.models import KerasSingleLSTM
    from longterm360fov_amd.training import SingleLSTMTrainer, _SINGLE_ORDER
    rng = np.random.default_rng(H + B)
    w0 = O.init_seq2seq(40 + H, H=H, bias_noise=0.1)
    w = {"K": w0["enc_K"], "R": w0["enc_R"], "b": w0["enc_b"], "dense_W": w0["dense_W"], "dense_b": w0["dense_b"]}
    enc, _, tgt = O.synthetic_batch(41 + B, B, T, T)
    x = enc if not unrolled else enc[:, -1:]
    noise = rng.standard_normal((T - 1, B, 90)).astype(np.float32) if refeed else None
    y_np = O.single_lstm_keras_forward(x.astype(np.float64), f64(w), T, unrolled, None if noise is None else noise.astype(np.float64), act)
    loss_ref, g_ref, y_ref = _torch_single_lstm_graph(x, tgt, w, act, unrolled, noise)
    np.testing.assert_allclose(y_np, y_ref, atol=1e-12)
    tr = SingleLSTMTrainer(w, act=act, unrolled=unrolled, sample_and_refeed=refeed)
    loss, y = tr.forward_backward(dev(x), dev(tgt), noise=None if noise is None else dev(noise))
    tr.ws.check(); tr.bwd_scratch.check()
    assert abs(float(loss.item()) - loss_ref) <= 1e-5 * loss_ref + 1e-9
    np.testing.assert_allclose(y.cpu().numpy(), y_ref, atol=3e-5)
    for k in _SINGLE_ORDER:
        a = tr.g[k].detach().cpu().numpy().astype(np.float64)
        scale = np.abs(g_ref[k]).max()
        err = np.abs(a - g_ref[k]).max()
        print("single-lstm H%d grad %-8s max|ref| %.3e  max err %.3e" % (H, k, scale, err))
        assert err <= 1e-4 * scale + 1e-9, (k, err, scale)
    m = KerasSingleLSTM(latent_dim=H, recurrent_activation=act, unrolled=unrolled, sample_and_refeed=refeed, predict_step=T)
    m.set_weights([w[k] for k in _SINGLE_ORDER])
    got = m.predict(x, noise=noise)
    np.testing.assert_allclose(got, y_ref, atol=3e-5)
    m.compile(optimizer="Adam", loss="mean_squared_error", metrics=["accuracy"])
    losses = [m.train_on_batch(x, tgt, noise=noise) for _ in range(4)]
    assert losses[-1] < losses[0]
    h = m.fit(x, tgt, batch_size=16, epochs=2, validation_split=0.1, shuffle=False)
    assert len(h.history["loss"]) == 2 and "val_loss" in h.history


def _torch_stacked_graph(enc, dec_in, tgt, w, L, act):
    t = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in w.items()}
    H = w["enc0_R"].shape[0]
    s = torch.sigmoid if act == "sigmoid" else (lambda z: torch.clamp(0.2 * z + 0.5, 0, 1))

    def layer(x, K, R, b, h, c):
        outs = []
        for tt in range(x.shape[1]):
            z = x[:, tt] @ K + b + h @ R
            i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
            c = f * c + i * g
            h = o * torch.tanh(c)
            outs.append(h)
        return torch.stack(outs, 1), h, c

    e, d, tg = (torch.tensor(a.astype(np.float64)) for a in (enc, dec_in, tgt))
    z0 = torch.zeros(e.shape[0], H, dtype=torch.float64)
    st, inp = [], e
    for l in range(L):
        inp, h, c = layer(inp, t["enc%d_K" % l], t["enc%d_R" % l], t["enc%d_b" % l], z0, z0)
        st.append((h, c))
    inp = d
    for l in range(L):
        inp, _, _ = layer(inp, t["dec%d_K" % l], t["dec%d_R" % l], t["dec%d_b" % l], st[l][0], st[l][1])
    y = torch.tanh(inp @ t["dense_W"] + t["dense_b"])
    loss = torch.mean((y - tg) ** 2)
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in t.items()}, y.detach().numpy()


@pytest.mark.parametrize("L,H,B,T_in,T_out,act", [(2, 32, 21, 5, 4, "sigmoid"), (3, 64, 33, 4, 5, "hard_sigmoid"),
                                                  (2, 256, 40, 6, 5, "sigmoid"), (2, 128, 130, 10, 10, "hard_sigmoid")])
def test_stacked_seq2seq_layers(L, H, B, T_in, T_out, act):
    """Fov_seq2seq_2layers.py / 3layers.py: L-layer teacher-forced graph (gradients vs torch.autograd fp64), the autoregressive
    decode loop vs the NumPy oracle, and the fit surface."""
    from longterm360fov_amd.models import StackedSeq2SeqLSTM
    from longterm360fov_amd.training import StackedSeq2SeqTrainer, stacked_weight_order
    rng = np.random.default_rng(L * 1000 + H)
    w = {}
    for side, f0 in (("enc", 6), ("dec", 6)):
        for l in range(L):
            k_, r_, b_ = O.init_lstm(rng, 6 if l == 0 else H, H)
            w["%s%d_K" % (side, l)], w["%s%d_R" % (side, l)] = k_, r_
            w["%s%d_b" % (side, l)] = (b_ + 0.1 * rng.standard_normal(4 * H)).astype(np.float32)
    w["dense_W"] = rng.uniform(-0.3, 0.3, (H, 6)).astype(np.float32)
    w["dense_b"] = rng.uniform(-0.1, 0.1, 6).astype(np.float32)
    enc90, dec0, tgt = O.synthetic_batch(31 + B, B, T_in, T_out)
    enc = O.meanvar_xyz(enc90.astype(np.float64)).astype(np.float32)       # the scripts feed (mu, var) seconds: Input(shape=(None, 6))
    dec_in = np.concatenate([dec0, tgt[:, :-1]], axis=1)
    order = stacked_weight_order(L)
    loss_ref, g_ref, y_ref = _torch_stacked_graph(enc, dec_in, tgt, w, L, act)
    y_np = O.stacked_seq2seq_forward(enc.astype(np.float64), dec_in.astype(np.float64), f64(w), L, act)
    np.testing.assert_allclose(y_np, y_ref, atol=1e-12)
    tr = StackedSeq2SeqTrainer(w, L, act=act)
    loss, y = tr.forward_backward(dev(enc), dev(dec_in), dev(tgt))
    tr.ws.check(); tr.bwd_scratch.check()
    assert abs(float(loss.item()) - loss_ref) <= 1e-5 * loss_ref + 1e-9
    np.testing.assert_allclose(y.cpu().numpy(), y_ref, atol=2e-5)
    for k in order:
        a = tr.g[k].detach().cpu().numpy().astype(np.float64)
        scale = np.abs(g_ref[k]).max()
        err = np.abs(a - g_ref[k]).max()
        print("stacked L%d H%d grad %-8s max|ref| %.3e  max err %.3e" % (L, H, k, scale, err))
        assert err <= 1e-4 * scale + 1e-9, (k, err, scale)
    m = StackedSeq2SeqLSTM(num_encoder_tokens=6, latent_dim=H, num_layers=L, recurrent_activation=act)
    m.set_weights([w[k] for k in order])
    np.testing.assert_allclose(m.predict([enc, dec_in]), y_ref, atol=2e-5)
    ar_ref = O.stacked_seq2seq_forward(enc.astype(np.float64), dec0.astype(np.float64), f64(w), L, act, T_out=T_out)
    ar = m.decode_sequence(enc, dec0, predict_step=T_out)
    assert (np.abs(ar - ar_ref) <= 1e-3 * np.abs(ar_ref) + 1e-5).all() and np.abs(ar - ar_ref).max() <= 2e-5
    m.compile(optimizer="Adam", loss="mean_squared_error", metrics=["accuracy"])
    losses = [m.train_on_batch([enc, dec_in], tgt) for _ in range(4)]
    assert losses[-1] < losses[0]
    h = m.fit([enc, dec_in], tgt, batch_size=16, epochs=2, validation_split=0.1)
    assert len(h.history["loss"]) == 2 and "val_loss" in h.history


def _torch_others_context_graph(enc, oth, dec0, tgt, w, mode, act):
    """fp64 torch.autograd restatement of given_others...py with target_user_only / others_mlp / others_lstm (see the oracle's
    others_context_forward for the line references)."""
    t = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in w.items()}
    H = w["enc1_R"].shape[0]
    s = torch.sigmoid if act == "sigmoid" else (lambda z: torch.clamp(0.2 * z + 0.5, 0, 1))

    def step(x, h, c, n):
        z = x @ t[n + "_K"] + t[n + "_b"] + h @ t[n + "_R"]
        i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
        c = f * c + i * g
        return o * torch.tanh(c), c

    def layer(x, n, h, c):
        outs = []
        for tt in range(x.shape[1]):
            h, c = step(x[:, tt], h, c, n)
            outs.append(h)
        return torch.stack(outs, 1), h, c

    e, o_, d0, tg = (torch.tensor(a.astype(np.float64)) for a in (enc, oth, dec0, tgt))
    B, T_out = e.shape[0], tg.shape[1]
    z0 = torch.zeros(B, H, dtype=torch.float64)
    hs1, h1, c1 = layer(e, "enc1", z0, z0)
    _, h2, c2 = layer(hs1, "enc2", z0, z0)
    ctx = None
    if mode == "others_mlp":
        ctx = torch.relu(torch.relu(o_.reshape(B, T_out, -1) @ t["oth_W1"] + t["oth_b1"]) @ t["oth_W2"] + t["oth_b2"])
    elif mode == "others_lstm":
        seq, init = o_.reshape(B, T_out, -1), {"f": (z0, z0), "b": (z0, z0)}
        for j in (1, 2):
            fs, fh, fc = layer(seq, "ol%df" % j, *init["f"])
            bs, bh, bc = layer(torch.flip(seq, (1,)), "ol%db" % j, *init["b"])
            seq, init = torch.cat([fs, torch.flip(bs, (1,))], 2), {"f": (fh, fc), "b": (bh, bc)}
        ctx = seq
    x, outs = d0[:, 0], []
    for tt in range(T_out):
        h1, c1 = step(x, h1, c1, "dec1")
        h2, c2 = step(h1, h2, c2, "dec2")
        x = torch.tanh((h2 if ctx is None else torch.cat([ctx[:, tt], h2], 1)) @ t["dense_W"] + t["dense_b"])
        outs.append(x)
    y = torch.stack(outs, 1)
    loss = torch.mean((y - tg) ** 2)
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in t.items()}, y.detach().numpy()


@pytest.mark.parametrize("mode,H,B,U,T_in,T_out,act", [("target_user_only", 64, 21, 5, 4, 5, "sigmoid"),
                                                       ("others_mlp", 32, 33, 34, 3, 4, "hard_sigmoid"),
                                                       ("others_lstm", 32, 19, 6, 3, 5, "sigmoid"),
                                                       ("others_lstm", 256, 24, 34, 2, 3, "hard_sigmoid")])
def test_others_context_heads(mode, H, B, U, T_in, T_out, act):
    """given_others...py with its other module flags (target_user_only, others_mlp, others_lstm = two Bidirectional LSTMs whose
    second is seeded with the first's final states): forward vs the NumPy oracle, gradients vs torch.autograd fp64."""
    from longterm360fov_amd.models import OthersContextSeq2Seq
    from longterm360fov_amd.training import OthersContextTrainer, others_context_order
    m = OthersContextSeq2Seq(mode, latent_dim=H, num_user=U, recurrent_activation=act, seed=H + B, predict_step=T_out)
    rng = np.random.default_rng(B)
    w = {k: (v + (0.1 * rng.standard_normal(v.shape).astype(np.float32) if k.endswith("_b") or k.endswith("b1") or k.endswith("b2") else 0))
         for k, v in zip(others_context_order(mode), m.get_weights())}
    m.set_weights([w[k] for k in others_context_order(mode)])
    enc, dec0, tgt, oth = O.synthetic_batch(71 + B, B, T_in, T_out, num_others=U - 1)
    loss_ref, g_ref, y_ref = _torch_others_context_graph(enc, oth, dec0, tgt, w, mode, act)
    y_np = O.others_context_forward(enc.astype(np.float64), oth.astype(np.float64), dec0.astype(np.float64), f64(w), T_out, mode, act)
    np.testing.assert_allclose(y_np, y_ref, atol=1e-12)
    tr = OthersContextTrainer(w, mode, act=act)
    loss, y = tr.forward_backward(dev(enc), dev(oth), dev(dec0), dev(tgt))
    tr.ws.check(); tr.bwd_scratch.check()
    assert abs(float(loss.item()) - loss_ref) <= 1e-5 * loss_ref + 1e-9
    np.testing.assert_allclose(y.cpu().numpy(), y_ref, atol=2e-5)
    for k in others_context_order(mode):
        a = tr.g[k].detach().cpu().numpy().astype(np.float64)
        scale = np.abs(g_ref[k]).max()
        err = np.abs(a - g_ref[k]).max()
        print("%s H%d grad %-8s max|ref| %.3e  max err %.3e" % (mode, H, k, scale, err))
        assert err <= 1e-4 * scale + 1e-9, (k, err, scale)
    xin = [enc, dec0] if mode == "target_user_only" else [enc, oth, dec0]
    got = m.predict(xin)
    np.testing.assert_allclose(got, y_ref, atol=2e-5)
    assert (np.abs(got - y_ref) <= 1e-3 * np.abs(y_ref) + 1e-5).all()
    m.compile(optimizer="Adam", loss="mean_squared_error")
    losses = [m.train_on_batch(xin, tgt) for _ in range(4)]
    assert losses[-1] < losses[0]
    h = m.fit(xin, tgt, batch_size=16, epochs=2, validation_split=0.2)
    assert len(h.history["loss"]) == 2 and "val_loss" in h.history


def test_config2_full_size_training_gradients():
    """configs[1] shape at full size (B = 1024, T 30 -> 30, H = 256): loss, prediction and every gradient of the teacher-forced
    training step against the fp64 oracle (BPTT through 30 + 30 steps)."""
    from longterm360fov_amd.training import Seq2SeqTrainer
    B, T_in, T_out, H = 1024, 30, 30, 256
    w = O.init_seq2seq(1234, H=H, bias_noise=0.05)
    enc, dec_in, tgt = batch(1234, B, T_in, T_out)
    loss_ref, g_ref, y_ref = O.seq2seq_loss_and_grads(enc.astype(np.float64), dec_in.astype(np.float64), tgt.astype(np.float64),
                                                     f64(w), "sigmoid")
    tr = Seq2SeqTrainer(w, act="sigmoid")
    loss, y = tr.forward_backward(dev(enc), dev(dec_in), dev(tgt))
    tr.ws.check(); tr.bwd_scratch.check()
    assert abs(float(loss.item()) - loss_ref) <= 1e-5 * loss_ref + 1e-9
    np.testing.assert_allclose(y.cpu().numpy(), y_ref, atol=2e-5)
    check_grads(tr.g, g_ref, "config2 full size")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_training_step_same_xcd_and_safe_exchange_agree_bitwise(dtype):
    """The eight-workgroup kernels of the configs[2] step (wide-input layers, fused decoder forward / backward, BPTT) take
    the same-XCD granule exchange (sc0 stores) only when their run-time handshake shows the whole group on one XCD;
    FOV_FORCE_SAFE_EXCHANGE=1 (-> fov_workspace_force_safe) keeps them on the placement-independent write-through
    exchange.  Three optimizer steps must give bit-identical parameters either way."""
    from longterm360fov_amd.training import OthersMixingTrainer
    w = O.init_others_mixing(323, H=256, num_user=6, bias_noise=0.05)
    enc, dec0, tgt, oth = O.synthetic_batch(324, 512, 4, 3, num_others=5)
    flats, modes = {}, {}
    try:
        for forced in ("0", "1"):
            os.environ["FOV_FORCE_SAFE_EXCHANGE"] = forced
            tr = OthersMixingTrainer(w, dtype=dtype)
            for _ in range(3):
                tr.train_step(dev(enc), dev(oth), dev(dec0), dev(tgt))
            tr.check()
            flats[forced] = tr.flat.clone()
            modes[forced] = tr.ws.exchange_mode()
            print("FOV_FORCE_SAFE_EXCHANGE=%s: exchange mode of the last launch on the forward workspace: %d" % (forced, modes[forced]))
    finally:
        os.environ.pop("FOV_FORCE_SAFE_EXCHANGE", None)
    assert modes["1"] == 2
    assert torch.equal(flats["0"], flats["1"])


@pytest.mark.parametrize("kind", ["seq2seq", "mixing"])
def test_fit_at_the_reference_widths_runs_padded_on_the_matrix_core_kernels(kind):
    """latent_dim = 32 (given_others_gt_mean_var_seq2seq.py:38; FoV_seq2seq.py ships 64) is not a width of the persistent
    kernels: the trainers pad to the next one (training.PaddedTrainer - 64 for the target-only model, 256 for the fused
    others-mixing path).  Exactness: padded slices of parameters and gradients stay EXACTLY zero, and parameters after
    four optimizer steps equal the unpadded run on the generic kernels (impl='generic'); the generic kernel is not
    launched at all by the padded run."""
    from longterm360fov_amd import _lib
    from longterm360fov_amd.models import OthersMixingSeq2Seq, Seq2SeqLSTM, _MIX_ORDER
    from longterm360fov_amd.training import PaddedTrainer
    H, B, T = 32, 24, 4
    if kind == "seq2seq":
        w = O.init_seq2seq(501, H=H, bias_noise=0.1)
        enc, dec0, tgt = O.synthetic_batch(502, B, T, T)
        x = [enc, np.concatenate([dec0, tgt[:, :-1]], axis=1)]
        make = lambda impl: Seq2SeqLSTM(latent_dim=H, impl=impl, seed=0)
        order = list(w)
    else:
        w = O.init_others_mixing(503, H=H, num_user=5, bias_noise=0.1)
        enc, dec0, tgt, oth = O.synthetic_batch(504, B, T, T, num_others=4)
        x = [enc, oth, dec0]
        make = lambda impl: OthersMixingSeq2Seq(latent_dim=H, num_user=5, impl=impl, seed=0)
        order = list(_MIX_ORDER)
    res = {}
    for impl in ("generic", "auto"):
        m = make(impl)
        m.set_weights([w[k] for k in order])
        m.compile(optimizer="Adam", loss="mean_squared_error")
        n0 = _lib.lib().fov_debug_generic_launches()
        losses = [m.train_on_batch(x, tgt) for _ in range(4)]
        n1 = _lib.lib().fov_debug_generic_launches()
        tr = m._get_trainer()
        if impl == "auto":
            assert isinstance(tr, PaddedTrainer) and tr.Hp == (64 if kind == "seq2seq" else 256)
            assert n1 == n0, "the padded run launched the generic kernel %d times" % (n1 - n0)
            assert tr.padded_slices_are_zero()
        else:
            assert not isinstance(tr, PaddedTrainer) and n1 > n0
        res[impl] = (losses, m.get_weights())
    np.testing.assert_allclose(res["auto"][0], res["generic"][0], rtol=2e-5)
    for a, b in zip(res["auto"][1], res["generic"][1]):
        assert a.shape == b.shape
        np.testing.assert_allclose(a, b, atol=2e-6, rtol=1e-5)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_deferred_split_reductions_equal_immediate(dtype):
    """fov_reduce_defer_begin / _flush / _end (model.fit's backward: the split weight-gradient products of a step summed by ONE
    launch): same gradients bit for bit as one reduce per product - several products into adjacent ranges of a flat buffer, an
    ACCUMULATING product over a range a pending record covers (flushes first: in-stream order), a product whose output lies
    outside the registered buffer (reduced at once), an arena too small for one of the products (reduced at once) and more
    products than the record table holds."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(3)
    N, H, O = 5120, 256, 6
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).cuda()
    x1, x2, dz, xs, dp = t(N, H), t(N, H), t(N, 4 * H), t(N, O), t(N, O)
    nfused = (2 * H + 1) * 4 * H
    nsk = O * 4 * H
    nhead = (H + 1) * O

    def run(arena_mb):
        flat = torch.zeros(nfused + nsk + nhead + 64, dtype=torch.float32, device="cuda")
        outside = torch.zeros((H + 1) * 4 * H, dtype=torch.float32, device="cuda")
        sc = ops.Scratch()
        arena = torch.empty(max(arena_mb, 0) << 18, dtype=torch.float32, device="cuda") if arena_mb else None
        if arena is not None:
            ops.reduce_defer_begin(flat, arena)
        a, b, c = flat[:nfused], flat[nfused:nfused + nsk], flat[nfused + nsk:nfused + nsk + nhead]
        ops.wgrad_fused(x1, x2, dz, a, scratch=sc, dtype=dtype)                                    # [x1 | x2 | 1]^T dz
        ops.dense_bwd(xs, torch.zeros((O, 4 * H), device="cuda"), dz, dW=b.view(O, 4 * H), need_db=False, need_dx=False, scratch=sc)   # skinny
        ops.wgrad_fused(x1, None, dp, c, scratch=sc)                                               # [x1 | 1]^T dp
        ops.wgrad_fused(x2, x1, dz, a, accumulate=True, scratch=sc, dtype=dtype)                   # overlaps the first record
        ops.wgrad_fused(x1, None, dz, outside, scratch=sc, dtype=dtype)                            # not in the flat buffer
        for _ in range(20):                                                                        # more records than the table holds
            ops.wgrad_fused(x1, None, dp, c, accumulate=True, scratch=sc)
        if arena is not None:
            ops.reduce_defer_end(flat)
        torch.cuda.synchronize()
        return flat.clone(), outside.clone()

    f0, o0 = run(0)
    for mb in (256, 8):          # 8 MiB: the large products do not fit and are reduced at once, the small ones are deferred
        f1, o1 = run(mb)
        assert torch.equal(f0, f1) and torch.equal(o0, o1)
    ref = torch.cat([x1, x2, torch.ones(N, 1, device="cuda")], 1).double().T @ dz.double() + \
        torch.cat([x2, x1, torch.ones(N, 1, device="cuda")], 1).double().T @ dz.double()
    tol = 2e-3 if dtype == "f32" else 0.5
    assert (f0[:nfused].view(2 * H + 1, 4 * H).double() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item() / 100)


def _poison(ws):
    """What a give-up leaves in a workspace: the sticky timeout word (header word 0)."""
    ws.buf[:4] = torch.tensor([1, 0, 0, 0], dtype=torch.uint8, device="cuda")


def test_failed_steps_are_not_counted_and_earlier_ones_are():
    """Round-3 advisor finding: check() set Adam's step counter back by EVERY step since the last check, including the ones
    whose updates had been applied.  The guarded optimizer now counts on the device the updates that ran (fov_adam_step_guarded's
    `applied`): two good steps, a give-up before the third, two skipped steps -> check() raises once and step_count == 2; the
    next step is Adam's t = 3 on the parameters of step 2, exactly what an undisturbed third step gives."""
    from longterm360fov_amd import _lib
    from longterm360fov_amd.training import Seq2SeqTrainer
    w = O.init_seq2seq(71, H=64, bias_noise=0.05)
    enc, dec_in, tgt = batch(72, 24, 5, 4)
    args = (dev(enc), dev(dec_in), dev(tgt))
    ref = Seq2SeqTrainer(w)
    for _ in range(3):
        ref.train_step(*args)
    ref.check()
    tr = Seq2SeqTrainer(w)
    tr.train_step(*args); tr.train_step(*args)
    after2 = tr.flat.clone()
    _poison(tr.ws)
    tr.train_step(*args); tr.train_step(*args)            # skipped on the device, no host synchronisation
    assert tr.step_count == 4 and torch.equal(tr.flat, after2)
    with pytest.raises(_lib.FovError) as ei:
        tr.check()
    assert ei.value.code == _lib.ERR_TIMEOUT
    assert tr.step_count == 2 and int(tr.applied.item()) == 2
    tr.train_step(*args)
    tr.check()
    assert tr.step_count == 3 and torch.equal(tr.flat, ref.flat)


def _dp_poison_worker(rank, world_size, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        from longterm360fov_amd import _lib, parallel
        from longterm360fov_amd.training import Seq2SeqTrainer
        w = O.init_seq2seq(123, H=64, bias_noise=0.05)
        enc, dec_in, tgt = batch(124, 37, 6, 5)
        lo, hi = parallel.shard_range(37)
        a = (dev(enc[lo:hi]), dev(dec_in[lo:hi]), dev(tgt[lo:hi]))
        tr = Seq2SeqTrainer(w)
        tr.train_step(*a, n_global=37)
        after1 = tr.flat.detach().cpu().numpy().copy()
        if rank == 1:
            _poison(tr.ws)                                # only rank 1's persistent kernels "gave up"
        tr.train_step(*a, n_global=37)
        tr.train_step(*a, n_global=37)
        raised = None
        try:
            tr.check()                                    # every rank must leave here the same way
        except _lib.FovError as e:
            raised = e.code
        skipped = bool(np.array_equal(tr.flat.detach().cpu().numpy(), after1))
        count = tr.step_count
        # the group is still in step: the next collectives complete (they would hang if one rank had left alone)
        tr.train_step(*a, n_global=37)
        tr.check()
        q.put((rank, raised, skipped, count, tr.step_count, tr.flat.detach().cpu().numpy()))
    finally:
        dist.destroy_process_group()


def test_data_parallel_failed_step_is_skipped_and_reported_on_every_rank():
    """Round-3 advisor finding (medium): a give-up on ONE rank made every rank skip its updates - but only that rank's check()
    raised; the others sailed on into the next collective and hung.  Two ranks (gloo, one GPU), rank 1 poisoned after step 1:
    both skip steps 2 and 3, BOTH raise ERR_TIMEOUT from check(), both set step_count back to 1, and the following step (a
    collective) completes with bit-identical replicas."""
    import socket
    import torch.multiprocessing as mp
    from longterm360fov_amd import _lib
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_poison_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, raised, skipped, count, count_after, flat in res:
        assert raised == _lib.ERR_TIMEOUT, (rank, raised)
        assert skipped, rank
        assert count == 1 and count_after == 2, (rank, count, count_after)
    np.testing.assert_array_equal(res[0][5], res[1][5])


def test_epoch_rezero_keeps_the_timeout_word():
    """Round-3 advisor finding: the launch path's re-zero of header and granule area (host epoch past 0x70000000) also cleared a
    sticky timeout word set since the last fov_check_status.  It now leaves header word 0 alone: the launch that crosses the
    threshold on a poisoned workspace still skips its body, and the check still reports the give-up."""
    from longterm360fov_amd import ops, _lib
    w = O.init_seq2seq(3, H=256, bias_noise=0.05)
    enc, dec0, _ = O.synthetic_batch(4, 40, 5, 4)
    dw = {k: dev(v) for k, v in w.items()}
    ws = ops.Workspace()
    good = ops.seq2seq_decode(dev(enc), dev(dec0), dw, 4, impl="cluster", workspace=ws).clone()
    ws.check()
    L = _lib.lib()
    _lib.check(L.fov_debug_set_epoch(ws.buf.data_ptr(), ws.buf.numel(), 0x70000000 - 5, torch.cuda.current_stream().cuda_stream))
    _poison(ws)
    out = torch.full((40, 4, 6), 7.0, dtype=torch.float32, device="cuda")
    for _ in range(3):      # the first crosses the threshold
        ops.seq2seq_decode(dev(enc), dev(dec0), dw, 4, impl="cluster", workspace=ws, out=out)
    torch.cuda.synchronize()
    hdr = ws.buf[:32].cpu().numpy().view(np.uint32)
    assert hdr[0] != 0, "the re-zero erased the timeout word"
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0
    with pytest.raises(_lib.FovError):
        ws.check()
    again = ops.seq2seq_decode(dev(enc), dev(dec0), dw, 4, impl="cluster", workspace=ws)
    ws.check()
    assert torch.equal(again, good)


def test_padded_trainer_forwards_attribute_writes():
    """Round-3 advisor finding: PaddedTrainer forwarded attribute READS to the trainer it wraps but kept WRITES (except lr) to
    itself, so tr.overlap_allreduce = True on a latent_dim 32 / 64 model silently did nothing."""
    import copy
    from longterm360fov_amd.training import PaddedTrainer, Seq2SeqTrainer
    w = O.init_seq2seq(9, H=32, bias_noise=0.05)
    tr = PaddedTrainer(lambda wp: Seq2SeqTrainer(wp), w, 32, 64)
    tr.overlap_allreduce = True
    tr.defer_reduces = True
    tr.lr = 5e-4
    assert tr.inner.overlap_allreduce is True and tr.inner.defer_reduces is True and tr.inner.lr == 5e-4
    assert "overlap_allreduce" not in tr.__dict__
    with pytest.raises(AttributeError):
        PaddedTrainer.__new__(PaddedTrainer).anything      # before `inner` exists: AttributeError, not KeyError (copy / pickle probe this)
    assert copy.copy(tr).inner is tr.inner


def test_workspace_init_forgets_a_prepacked_weight_copy():
    """Round-3 advisor finding: fov_mix_decoder_prepack's mark survived fov_workspace_init / the reset in fov_check_status, which
    zero the packed copy: the next fov_mix_decoder_fwd on that workspace skipped its own pack and ran on zeros (a C-ABI caller's
    problem: the Python trainer packs at every step).  Through the entry points directly: pack, re-initialise, launch."""
    from longterm360fov_amd import _lib, ops
    H, U, NO, B, T_in, T_out = 256, 6, 6, 48, 3, 4
    w = O.init_others_mixing(41, H=H, num_user=U, bias_noise=0.1)
    enc, dec0, tgt, oth = O.synthetic_batch(42, B, T_in, T_out, num_others=U - 1)
    dw = {k: dev(v) for k, v in w.items()}
    n_oth = (U - 1) * NO
    Wm_o, Wm_p = dw["mix_W"][:n_oth].contiguous(), dw["mix_W"][n_oth:].contiguous()
    hs1, h1, c1 = ops.lstm_seq(dev(enc), dw["enc1_K"], dw["enc1_R"], dw["enc1_b"])
    zx = ops.matmul(hs1.reshape(B * T_in, H), dw["enc2_K"]).reshape(B, T_in, 4 * H)
    _, h2, c2 = ops.lstm_seq_zx(zx, dw["enc2_R"], dw["enc2_b"], return_sequences=False)
    oth_proj = ops.dense(dev(oth).reshape(B * T_out, n_oth), Wm_o, dw["mix_b"], activation=None).reshape(B, T_out, NO)
    ws = ops.Workspace()
    good = ops.mix_decoder(dev(dec0), h1, c1, h2, c2, oth_proj, dw, Wm_p, T_out, workspace=ws).clone()
    ws.check()
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    ops.mix_decoder_prepack(dw["dec2_K"], B, H, ws)                               # packed copy + mark ...
    _lib.check(L.fov_workspace_init(ws.buf.data_ptr(), ws.buf.numel(), stream))   # ... zeroed by the caller: the mark must go too
    again = ops.mix_decoder(dev(dec0), h1, c1, h2, c2, oth_proj, dw, Wm_p, T_out, workspace=ws)
    ws.check()
    assert torch.equal(again, good)
    # the same through the reset inside fov_check_status (a reported give-up zero-fills the workspace)
    ops.mix_decoder_prepack(dw["dec2_K"], B, H, ws)
    _poison(ws)
    with pytest.raises(_lib.FovError):
        ws.check()
    third = ops.mix_decoder(dev(dec0), h1, c1, h2, c2, oth_proj, dw, Wm_p, T_out, workspace=ws)
    ws.check()
    assert torch.equal(third, good)


def _torch_others_future_graph(enc, oth, dec0, tgt, w, act, conv_act="hard_sigmoid"):
    """Independent fp64 torch.autograd restatement of FoV_seq2seq_no_teac_forc.py:420-486 (torch's own conv2d for the ConvLSTM2D)."""
    import torch.nn.functional as Fn
    t = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in w.items()}
    H = w["enc_R"].shape[0]
    s = torch.sigmoid if act == "sigmoid" else (lambda z: torch.clamp(0.2 * z + 0.5, 0, 1))
    sc = torch.sigmoid if conv_act == "sigmoid" else (lambda z: torch.clamp(0.2 * z + 0.5, 0, 1))

    def step(x, h, c, K, R, b):
        z = x @ K + b + h @ R
        i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
        c = f * c + i * g
        return o * torch.tanh(c), c

    def conv(x, k):      # x (B,Hh,Ww,C) NHWC, k (kh,kw,C,N): 'same', cross-correlation
        kh, kw = k.shape[:2]
        y = Fn.conv2d(x.permute(0, 3, 1, 2), k.permute(3, 2, 0, 1), padding=(kh // 2, kw // 2))
        return y.permute(0, 2, 3, 1)

    e, o_, d0, tg = (torch.tensor(a.astype(np.float64)) for a in (enc, oth, dec0, tgt))
    B, T = o_.shape[0], o_.shape[1]
    h = c = torch.zeros(B, H, dtype=torch.float64)
    for tt in range(e.shape[1]):
        h, c = step(e[:, tt], h, c, t["enc_K"], t["enc_R"], t["enc_b"])
    hc = cc = torch.zeros(B, o_.shape[2], o_.shape[3], H, dtype=torch.float64)
    S = []
    for tt in range(T):
        z = conv(o_[:, tt], t["oth_K"]) + t["oth_b"] + conv(hc, t["oth_R"])
        i, f, g, oo = sc(z[..., :H]), sc(z[..., H:2 * H]), torch.tanh(z[..., 2 * H:3 * H]), sc(z[..., 3 * H:])
        cc = f * cc + i * g
        hc = oo * torch.tanh(cc)
        S.append(hc.reshape(B, -1) @ t["flat_W"] + t["flat_b"])
    x, ys = d0[:, 0], []
    for tt in range(T):
        h, c = step(x, h, c, t["dec_K"], t["dec_R"], t["dec_b"])
        x = torch.tanh(torch.cat([h, S[tt]], 1) @ t["dense_W"] + t["dense_b"])
        ys.append(x)
    y = torch.stack(ys, 1)
    loss = ((y - tg) ** 2).mean()
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in t.items()}, y.detach().numpy()


@pytest.mark.parametrize("H,B,U,fps,T_in,T_out,act", [(64, 5, 6, 7, 4, 3, "sigmoid"), (64, 9, 34, 30, 3, 2, "hard_sigmoid"), (32, 4, 8, 6, 2, 4, "sigmoid")])
def test_others_future_convlstm_model_gradients_and_fit(H, B, U, fps, T_in, T_out, act):
    """The second model of FoV_seq2seq_no_teac_forc.py (:420-486; VERDICT r03 missing #3): ConvLSTM2D(latent_dim, kernel
    (num_user-1, 3)) over the others' future, Flatten -> Dense(latent_dim), concatenated with the decoder output in front of
    the Dense(6, tanh) head, output fed back.  Forward vs the NumPy oracle, loss and every gradient vs torch.autograd fp64 (the
    script's own num_user = 34, fps = 30 among the cases), then the Keras surface: fit reduces the loss, predict = trainer."""
    from longterm360fov_amd.training import OthersFutureConvLSTMTrainer, OTHERS_FUTURE_ORDER
    from longterm360fov_amd.models import NoTeacherForcingOthersConvLSTM
    assert tuple(OTHERS_FUTURE_ORDER) == tuple(O.OTHERS_FUTURE_ORDER)
    w = O.init_others_future_convlstm(700 + H + U, H=H, num_user=U, fps=fps, bias_noise=0.05)
    rng = np.random.default_rng(701 + B)
    enc = rng.uniform(-1, 1, (B, T_in, 90)).astype(np.float32)
    oth = rng.uniform(-1, 1, (B, T_out, U - 1, fps, 3)).astype(np.float32)
    dec0 = rng.uniform(-1, 1, (B, 1, 6)).astype(np.float32)
    tgt = rng.uniform(-1, 1, (B, T_out, 6)).astype(np.float32)
    ref = O.others_future_convlstm_forward(enc.astype(np.float64), oth.astype(np.float64), dec0.astype(np.float64), f64(w), act=act)
    loss_ref, g_ref, y_t = _torch_others_future_graph(enc, oth, dec0, tgt, w, act)
    np.testing.assert_allclose(y_t, ref, atol=1e-10)                 # the two independent restatements agree
    tr = OthersFutureConvLSTMTrainer(w, act=act)
    loss, y = tr.forward_backward(dev(enc), dev(oth), dev(dec0), dev(tgt))
    tr.check()
    got = y.cpu().numpy()
    assert (np.abs(got - ref) <= 1e-3 * np.abs(ref) + 2e-5).all(), np.abs(got - ref).max()
    assert abs(float(loss.item()) - loss_ref) <= 1e-5 * loss_ref + 1e-9
    for k in OTHERS_FUTURE_ORDER:
        a = tr.g[k].detach().cpu().numpy().astype(np.float64)
        r = g_ref[k]
        scale = np.abs(r).max()
        err = np.abs(a - r)
        print("others-future grad %-8s max|ref| %.3e  max err %.3e" % (k, scale, err.max()))
        assert (err <= 1e-3 * np.abs(r) + 2e-4 * scale).all(), (k, err.max(), scale)
    # Keras surface
    m = NoTeacherForcingOthersConvLSTM(latent_dim=H, num_user=U, fps=fps, recurrent_activation=act, seed=3)
    m.set_weights([w[k] for k in OTHERS_FUTURE_ORDER])
    m.compile(optimizer="Adam", loss="mean_squared_error")
    p0 = m.predict([enc, oth, dec0])
    assert (np.abs(p0 - ref) <= 1e-3 * np.abs(ref) + 2e-5).all()
    l0 = float(((p0 - tgt) ** 2).mean())
    h = m.fit([enc, oth, dec0], tgt, batch_size=B, epochs=6, shuffle=False)
    assert abs(h.history["loss"][0] - l0) <= 1e-4 * l0 + 1e-7 and h.history["loss"][-1] < h.history["loss"][0]
    p1 = m.predict([enc, oth, dec0], batch_size=max(1, B // 2))       # batched predict on the trained weights
    assert float(((p1 - tgt) ** 2).mean()) < l0


@pytest.mark.parametrize("B,T,F,state,upstream", [(32, 10, 90, True, False), (12, 3, 90, False, True), (17, 1, 6, True, True), (48, 5, 30, False, False),
                                                  (1, 2, 90, False, False), (32, 12, 33, True, True)])
def test_two_layer_bptt_one_launch_equals_two_calls(B, T, F, state, upstream):
    """fov_lstm_stack2_bwd (both recurrences and dx = dz2 . K2^T between them as three roles of one launch, lstm.py:218-240 under
    its train_op) against two fov_lstm_seq_bwd calls: dz of both layers, state gradients, every weight gradient.  The only
    arithmetic difference is the summation order of dx (sixteen slice partials vs a split GEMM): 2e-5 of each tensor's scale;
    the second launch on the same workspace repeats the first bit for bit."""
    from longterm360fov_amd import ops
    H = 512
    if not ops.lstm_stack2_bwd_supported(B, T, F, H):
        pytest.skip("needs 3 x 16 workgroups per tile resident")
    rng = np.random.default_rng(B * 100 + T)
    K1, R1, b1 = O.init_lstm(rng, F, H, np.float32)
    K2, R2, b2 = O.init_lstm(rng, H, H, np.float32)
    x = dev(rng.uniform(-1, 1, (B, T, F)).astype(np.float32))
    st = lambda: dev((0.3 * rng.standard_normal((B, H))).astype(np.float32)) if state else None
    h01, c01, h02, c02 = st(), st(), st(), st()
    dK1, dR1, db1, dK2, dR2, db2 = (dev(a) for a in (K1, R1, b1, K2, R2, b2))
    hs1, _, _, res1 = ops.lstm_seq_train(x, dK1, dR1, db1, h01, c01, act="sigmoid")
    hs2, _, _, res2 = ops.lstm_seq_train(hs1, dK2, dR2, db2, h02, c02, act="sigmoid")
    dhT2 = dev((0.1 * rng.standard_normal((B, H))).astype(np.float32))
    dcT2 = dev((0.1 * rng.standard_normal((B, H))).astype(np.float32)) if upstream else None
    dhs2 = dev((0.05 * rng.standard_normal((B, T, H))).astype(np.float32)) if upstream else None
    dhT1 = dev((0.1 * rng.standard_normal((B, H))).astype(np.float32)) if upstream else None
    sc = ops.Scratch()
    # reference: two calls
    g = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    ga = {"K1": g(F, 4 * H), "R1": g(H, 4 * H), "b1": g(4 * H), "K2": g(H, 4 * H), "R2": g(H, 4 * H), "b2": g(4 * H)}
    e2 = ops.lstm_seq_bwd(hs1, dK2, dR2, hs2, res2, h0=h02, c0=c02, dhs=dhs2, dhT=dhT2, dcT=dcT2, dK=ga["K2"], dR=ga["R2"], db=ga["b2"],
                          need_dx=True, need_state_grads=True, act="sigmoid", scratch=sc)
    e1 = ops.lstm_seq_bwd(x, dK1, dR1, hs1, res1, h0=h01, c0=c01, dhs=e2["dx"], dhT=dhT1, dK=ga["K1"], dR=ga["R1"], db=ga["b1"],
                          need_state_grads=True, act="sigmoid", scratch=sc)
    sc.check()
    gb = {k: torch.zeros_like(v) for k, v in ga.items()}
    sc2 = ops.Scratch()
    one = ops.lstm_stack2_bwd(x, (dK1, dR1), (dK2, dR2), (hs1, res1, h01, c01), (hs2, res2, h02, c02), dhs2=dhs2, dhT2=dhT2, dcT2=dcT2,
                              dhT1=dhT1, grads1=(gb["K1"], gb["R1"], gb["b1"]), grads2=(gb["K2"], gb["R2"], gb["b2"]),
                              need_state_grads=True, act="sigmoid", scratch=sc2)
    sc2.check()
    def near(a, r, tag):
        scale = float(r.abs().max())
        err = float((a - r).abs().max())
        print("one-launch two-layer BPTT B=%d T=%d %-6s max|ref| %.3e err %.3e" % (B, T, tag, scale, err))
        assert err <= 2e-5 * scale + 1e-9, tag
    near(one["dz2"], e2["dz"], "dz2")        # (the roles are separate instantiations of the body: the compiler may contract
    near(one["dh0_2"], e2["dh0"], "dh0_2")    # the gates' arithmetic differently - not bit-identical by construction)
    near(one["dc0_2"], e2["dc0"], "dc0_2")
    near(one["dz1"], e1["dz"], "dz1")
    near(one["dh0_1"], e1["dh0"], "dh0_1")
    near(one["dc0_1"], e1["dc0"], "dc0_1")
    for k in ga:
        near(gb[k], ga[k], "d" + k)
    assert float(ga["K1"].abs().max()) > 0 and float(ga["R2"].abs().max()) > 0 or T == 1
    # a second launch on the same workspace (epoch tags continue), data path only: same dz
    two = ops.lstm_stack2_bwd(x, (dK1, dR1), (dK2, dR2), (hs1, res1, h01, c01), (hs2, res2, h02, c02), dhs2=dhs2, dhT2=dhT2, dcT2=dcT2,
                              dhT1=dhT1, act="sigmoid", scratch=sc2)
    sc2.check()
    assert torch.equal(two["dz1"], one["dz1"]) and torch.equal(two["dz2"], one["dz2"])


@pytest.mark.parametrize("B,T,F,H", [(2, 3, 90, 256), (1, 1, 6, 128), (5, 3, 90, 256), (16, 1, 90, 256), (3, 5, 6, 64)])
def test_layer_bptt_with_sixteen_rows_or_fewer(B, T, F, H):
    """fov_lstm_seq_bwd at batch x time <= 16 with dK | dR | db adjacent (a trainer's flat buffer; the partial last batch of a
    model.fit epoch): the fused [h_{t-1} | 1]^T dz product then has ONE 16-row k-tile starting at k = 0.  Round 4 found its
    final (unused) re-fetch reading the row BEFORE the hs tape - a memory access fault whenever the tape begins a mapped region
    (order-dependent in the full suite); the values were always right, which is all a test can assert portably."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(B * 10 + T)
    K, R, b = O.init_lstm(rng, F, H, np.float32)
    x = rng.uniform(-1, 1, (B, T, F)).astype(np.float32)
    dhT = (0.1 * rng.standard_normal((B, H))).astype(np.float32)
    d64 = lambda a: a.astype(np.float64)
    hs64, _, _, res64 = O.lstm_layer_train(d64(x), d64(K), d64(R), d64(b), None, None, act="sigmoid")
    ref = O.lstm_layer_backward(d64(x), d64(K), d64(R), None, None, hs64, res64, None, d64(dhT), None, act="sigmoid")
    hs, _, _, res = ops.lstm_seq_train(dev(x), dev(K), dev(R), dev(b), act="sigmoid")
    flat = torch.zeros((F + H + 1) * 4 * H, dtype=torch.float32, device="cuda")
    dK, dR, db = flat[:F * 4 * H].view(F, 4 * H), flat[F * 4 * H:(F + H) * 4 * H].view(H, 4 * H), flat[(F + H) * 4 * H:]
    sc = ops.Scratch()
    for rep in range(2):      # accumulate = True on zeros, then once more: twice the gradient
        ops.lstm_seq_bwd(dev(x), dev(K), dev(R), hs, res, dhT=dev(dhT), dK=dK, dR=dR, db=db, act="sigmoid", accumulate=True, scratch=sc)
        sc.check()
        for name, got, r in (("dK", dK, ref["dK"]), ("dR", dR, ref["dR"]), ("db", db, ref["db"])):
            err = np.abs(got.cpu().numpy().astype(np.float64) - (rep + 1) * r).max()
            assert err <= 2e-5 * (np.abs(r).max() + 1e-12) * (rep + 1) + 1e-9, (name, rep, err)


@pytest.mark.parametrize("rows,O,act", [(320, 3, "tanh"), (30720, 3, "tanh"), (1000, 6, None), (257, 8, "tanh"), (512, 1, "tanh"), (100, 12, "tanh"), (1, 3, "tanh")])
def test_dense_bias_gradient_from_the_loss_launch(rows, O, act):
    """fov_mse_dense_grad_db: dpre, the loss AND the Dense head's bias gradient (column sums of dpre) from one launch -
    block boundaries that are no multiple of the width, widths up to 8 in the kernel (12: the column-sum launches), a weight;
    against fp64 column sums of the dpre the same call returns, and dpre / loss against the call without db."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(rows + O)
    y = dev(np.tanh(rng.standard_normal((rows, O))))
    t = dev(rng.uniform(-1, 1, (rows, O)))
    db = torch.full((O,), 7.0, device="cuda")
    sc = ops.Scratch()
    for _ in range(3):   # the ticket ring: repeated launches
        dpre, loss = ops.mse_dense_grad(y, t, act, scratch=sc, weight=0.5, db=db)
    dpre0, loss0 = ops.mse_dense_grad(y, t, act, scratch=sc, weight=0.5)
    assert torch.equal(dpre, dpre0) and torch.equal(loss, loss0)
    ref = dpre.cpu().numpy().astype(np.float64).sum(axis=0)
    got = db.cpu().numpy().astype(np.float64)
    assert np.abs(got - ref).max() <= 1e-6 * max(1.0, np.abs(dpre.cpu().numpy()).sum(axis=0).max()), (got, ref)
    # the same bits every time (fixed summation order)
    db2 = torch.zeros((O,), device="cuda")
    ops.mse_dense_grad(y, t, act, scratch=sc, weight=0.5, db=db2)
    assert torch.equal(db, db2)


@pytest.mark.parametrize("N,H,O,act,weight", [(320, 128, 6, "tanh", 1.0), (320, 64, 6, "tanh", 0.37), (37, 256, 3, "tanh", 1.0), (4096, 256, 6, "tanh", 1.0),
                                              (30720, 256, 6, "tanh", 1.0), (4161, 128, 3, "tanh", 0.5), (50001, 512, 8, None, 1.0),
                                              (65, 512, 8, None, 1.0), (1, 32, 1, "tanh", 1.0), (1000, 100, 6, "tanh", 0.5)])
def test_dense_mse_head_one_launch(N, H, O, act, weight):
    """fov_dense_mse_head (round 5): Dense(O, tanh) + mean_squared_error of FoV_seq2seq.py:96-103, forward and backward in ONE launch
    (the reference's batch: 320 rows) - y, loss, dX, dW, db against fp64 NumPy and against the three separate entry points it
    replaces (fov_dense_fwd, fov_mse_dense_grad_db, fov_dense_bwd); gradients land in place in a flat buffer; deterministic."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(N + H)
    hs = rng.uniform(-1, 1, (N, H)).astype(np.float32)
    W = (rng.standard_normal((H, O)) / np.sqrt(H)).astype(np.float32)
    b = (0.1 * rng.standard_normal(O)).astype(np.float32)
    tg = rng.uniform(-1, 1, (N, O)).astype(np.float32)
    assert ops.dense_mse_head_supported(N, H, O) and not ops.dense_mse_head_supported((1 << 20) + 1, H, O) and not ops.dense_mse_head_supported(N, H, 9)
    pre = hs.astype(np.float64) @ W.astype(np.float64) + b
    y_ref = np.tanh(pre) if act else pre
    d = y_ref - tg
    loss_ref = weight * np.mean(d ** 2)
    dpre = 2.0 * d * weight / (N * O) * ((1 - y_ref ** 2) if act else 1.0)
    dX_ref, dW_ref, db_ref = dpre @ W.astype(np.float64).T, hs.astype(np.float64).T @ dpre, dpre.sum(0)
    flat = torch.zeros(H * O + O + 1 + 3, device="cuda")
    dW, db, loss = flat[:H * O].view(H, O), flat[H * O:H * O + O], flat[H * O + O:H * O + O + 1]
    y, dX, l = ops.dense_mse_head(dev(hs), dev(W), dev(b), dev(tg), act, dW=dW, db=db, loss=loss, weight=weight, scratch=ops.Scratch())
    torch.cuda.synchronize()
    assert l.data_ptr() == loss.data_ptr() and float(flat[-3:].abs().max().item()) == 0.0
    assert np.abs(y.cpu().numpy() - y_ref).max() <= 2e-6
    assert abs(float(loss.item()) - loss_ref) <= 1e-5 * abs(loss_ref) + 1e-9
    for got, ref, tag in ((dX, dX_ref, "dX"), (dW, dW_ref, "dW"), (db, db_ref, "db")):
        err = np.abs(got.cpu().numpy() - ref).max()
        assert err <= 2e-5 * np.abs(ref).max() + 1e-9, (tag, err, np.abs(ref).max())
    # the separate launches it replaces
    sc = ops.Scratch()
    y2 = ops.dense(dev(hs), dev(W), dev(b), activation=act)
    db2 = torch.zeros(O, device="cuda")
    dpre2, loss2 = ops.mse_dense_grad(y2, dev(tg), act, scratch=sc, weight=weight, db=db2)
    dW2 = torch.zeros((H, O), device="cuda")
    dX2, _, _ = ops.dense_bwd(dev(hs), dev(W), dpre2, dW=dW2, need_db=False, scratch=sc)
    assert (y - y2).abs().max().item() <= 1e-6 and abs(float(loss.item()) - float(loss2.item())) <= 1e-6 * abs(loss_ref) + 1e-9
    assert (dX - dX2).abs().max().item() <= 2e-5 * np.abs(dX_ref).max() + 1e-9 and (dW - dW2).abs().max().item() <= 2e-5 * np.abs(dW_ref).max() + 1e-9
    assert (db - db2).abs().max().item() <= 2e-5 * np.abs(db_ref).max() + 1e-9
    # bit for bit the same on a second call (fixed summation orders, the ticket is back at zero)
    flat2 = torch.zeros_like(flat)
    y3, dX3, _ = ops.dense_mse_head(dev(hs), dev(W), dev(b), dev(tg), act, dW=flat2[:H * O].view(H, O), db=flat2[H * O:H * O + O],
                                    loss=flat2[H * O + O:H * O + O + 1], weight=weight, scratch=ops.Scratch())
    assert torch.equal(flat2, flat) and torch.equal(y3, y) and torch.equal(dX3, dX)


@pytest.mark.parametrize("B,T1,T2,F1,F2,H,with_h0", [(32, 10, 10, 90, 6, 128, True), (32, 5, 4, 90, 6, 64, True), (7, 3, 9, 5, 6, 32, False),
                                                     (40, 16, 1, 90, 6, 256, True), (32, 10, 10, 90, 6, 16, True), (1, 1, 1, 3, 3, 16, True),
                                                     (20, 32, 30, 90, 6, 128, True), (32, 10, 10, 90, 512, 512, True), (9, 7, 2, 30, 6, 512, False),
                                                     (32, 30, 30, 90, 6, 256, True)])
def test_encoder_decoder_weight_gradients_one_launch(B, T1, T2, F1, F2, H, with_h0):
    """fov_lstm_seq_wgrad_pair (round 5): dK = x^T dz, dR = h_{t-1}^T dz (h_{-1} = h0 or 0), db = column sums of dz for the encoder
    and the decoder of FoV_seq2seq.py:68-93 from their dz tapes - at few rows ONE launch (16 x 64 tiles, 64 x 64 at H = 512 - lstm.py's two
    stacked layers -, rows split over a workgroup's waves) - against fp64 NumPy, against the per-layer entry point with the few-row kernels switched off, with
    accumulate, into a flat gradient buffer, and bit for bit the same twice.  The last case has too many rows for one launch and
    must equal two fov_lstm_seq_wgrad calls bit for bit."""
    import os
    from longterm360fov_amd import ops
    rng = np.random.default_rng(B * 1000 + T1 * 10 + H)
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
    x1, hs1, dz1 = u(B, T1, F1), u(B, T1, H), u(B, T1, 4 * H)
    x2, hs2, dz2 = u(B, T2, F2), u(B, T2, H), u(B, T2, 4 * H)
    h0_2 = u(B, H) if with_h0 else None
    one = ops.lstm_seq_wgrad_pair_one_launch(B, T1, T2, H)
    assert one == (B * max(T1, T2) <= 640 and H <= 512)

    def ref(x, hs, h0, dz):
        x, hs, dz = x.astype(np.float64), hs.astype(np.float64), dz.astype(np.float64)
        hp = np.concatenate([(h0.astype(np.float64) if h0 is not None else np.zeros((x.shape[0], H)))[:, None], hs[:, :-1]], axis=1)
        return (np.einsum("btf,btn->fn", x, dz), np.einsum("bth,btn->hn", hp, dz), dz.sum((0, 1)))

    refs = ref(x1, hs1, None, dz1) + ref(x2, hs2, h0_2, dz2)
    sizes = [F1 * 4 * H, H * 4 * H, 4 * H, F2 * 4 * H, H * 4 * H, 4 * H]
    offs = np.concatenate([[4], 4 + np.cumsum(sizes)])

    def views(flat):
        shp = [(F1, 4 * H), (H, 4 * H), (4 * H,), (F2, 4 * H), (H, 4 * H), (4 * H,)]
        return [flat[int(offs[i]):int(offs[i + 1])].view(*shp[i]) for i in range(6)]

    d = lambda a: None if a is None else dev(a)
    args1 = (d(x1), d(hs1), None, d(dz1))
    args2 = (d(x2), d(hs2), d(h0_2), d(dz2))
    flat = torch.full((int(offs[-1]) + 8,), 7.0, device="cuda")
    v = views(flat)
    ops.lstm_seq_wgrad_pair(args1 + tuple(v[:3]), args2 + tuple(v[3:]), scratch=ops.Scratch())
    torch.cuda.synchronize()
    assert float((flat[:4] - 7).abs().max().item()) == 0.0 and float((flat[int(offs[-1]):] - 7).abs().max().item()) == 0.0
    for got, r, tag in zip(v, refs, ("dK1", "dR1", "db1", "dK2", "dR2", "db2")):
        err = np.abs(got.cpu().numpy() - r).max()
        assert err <= 2e-5 * np.abs(r).max() + 1e-5, (tag, err, np.abs(r).max())
    # the per-layer entry point without the few-row kernels (split products + reduces)
    os.environ["FOV_NO_WGRAD_GROUP"] = "1"
    try:
        flat_s = torch.zeros_like(flat)
        s = views(flat_s)
        sc = ops.Scratch()
        ops.lstm_seq_wgrad(args1[0], args1[1], args1[3], dK=s[0], dR=s[1], db=s[2], scratch=sc)
        ops.lstm_seq_wgrad(args2[0], args2[1], args2[3], dK=s[3], dR=s[4], db=s[5], h0=args2[2], scratch=sc)
        torch.cuda.synchronize()
    finally:
        del os.environ["FOV_NO_WGRAD_GROUP"]
    ops.Scratch().get(256, flat.device)      # (the library re-reads its knobs)
    for got, sp, r in zip(v, s, refs):
        assert (got - sp).abs().max().item() <= 2e-5 * np.abs(r).max() + 1e-6
    if not one:
        flat_t = torch.zeros_like(flat)
        t = views(flat_t)
        sc = ops.Scratch()
        ops.lstm_seq_wgrad(args1[0], args1[1], args1[3], dK=t[0], dR=t[1], db=t[2], scratch=sc)
        ops.lstm_seq_wgrad(args2[0], args2[1], args2[3], dK=t[3], dR=t[4], db=t[5], h0=args2[2], scratch=sc)
        for got, tw in zip(v, t):
            assert torch.equal(got, tw)
    # accumulate on top, and the same bits on a second call
    flat2 = torch.full_like(flat, 7.0)
    v2 = views(flat2)
    ops.lstm_seq_wgrad_pair(args1 + tuple(v2[:3]), args2 + tuple(v2[3:]), scratch=ops.Scratch())
    assert torch.equal(flat2, flat)
    ops.lstm_seq_wgrad_pair(args1 + tuple(v2[:3]), args2 + tuple(v2[3:]), accumulate=True, scratch=ops.Scratch())
    torch.cuda.synchronize()
    for got, once in zip(v2, v):      # (one launch: C + tile in one rounding; the split products add their slices to C in another order)
        assert torch.equal(got, once + once) if one else (got - 2 * once).abs().max().item() <= 1e-5 * once.abs().max().item()
    # only some gradients asked for (the bias rides on dR, or on dK when dR is absent)
    dK_only = torch.zeros((F2, 4 * H), device="cuda")
    db_only = torch.zeros(4 * H, device="cuda")
    ops.lstm_seq_wgrad_pair(args1 + (None, v2[1], None), args2 + (dK_only, None, db_only), scratch=ops.Scratch())
    torch.cuda.synchronize()
    same = (lambda a, b: torch.equal(a, b)) if one else (lambda a, b: (a - b).abs().max().item() <= 1e-5 * b.abs().max().item())
    assert same(dK_only, v[3]) and same(db_only, v[5]) and same(v2[1], v[1])
