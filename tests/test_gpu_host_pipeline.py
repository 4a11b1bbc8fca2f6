"""predict / evaluate / fit on host arrays through the staging ring (longterm360fov_amd/hostpipe.py) against the same model
with host_pipeline = False.  The kernels and the chunk boundaries are the same, so every comparison is bit for bit: a
difference is a pipeline bug (a slot reused too early, an ordering rule missed), never rounding.

29 rows at batch 4: 8 chunks, the last of one row, three slots wrapped twice.  Every row's inputs are distinct, so a slot
that is rewritten before it was read, or read before it was written, shows as a wrong row."""
import functools
import time

import numpy as np
import pytest

from oracle import fov_oracle as O

pytestmark = pytest.mark.gpu

N, BS, T_IN, T_OUT = 29, 4, 3, 2


def u(seed, *shape):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)


def seq2seq(dtype="f32"):
    from longterm360fov_amd.models import Seq2SeqLSTM
    F, H = (90, 256) if dtype == "bf16" else (6, 64)
    m = Seq2SeqLSTM(num_encoder_tokens=F, latent_dim=H, seed=1, dtype=dtype)
    return m, [u(1, N, T_IN, F), u(2, N, T_OUT, 6)], {}


def self_fed():
    from longterm360fov_amd.models import NoTeacherForcingSeq2Seq
    m = NoTeacherForcingSeq2Seq(num_encoder_tokens=6, latent_dim=32, seed=2, predict_step=T_OUT)
    return m, [u(3, N, T_IN, 6), u(4, N, 1, 6)], {}


def stacked():
    from longterm360fov_amd.models import StackedSeq2SeqLSTM
    return StackedSeq2SeqLSTM(latent_dim=32, seed=3), [u(5, N, T_IN, 6), u(6, N, T_OUT, 6)], {}


def others_mlp():
    from longterm360fov_amd.models import OthersContextSeq2Seq
    m = OthersContextSeq2Seq("others_mlp", num_encoder_tokens=6, latent_dim=32, num_user=3, seed=4, predict_step=T_OUT)
    return m, [u(7, N, T_IN, 6), u(8, N, T_OUT, 2, 6), u(9, N, 1, 6)], {}


def mixing(conv=False):
    from longterm360fov_amd import models
    cls = models.OthersConvMixingSeq2Seq if conv else models.OthersMixingSeq2Seq
    m = cls(num_encoder_tokens=6, latent_dim=32, num_user=3, seed=7)
    return m, [u(15, N, T_IN, 6), u(16, N, T_OUT, 2, 6), u(17, N, 1, 6)], {}


def single_refeed():
    from longterm360fov_amd.models import KerasSingleLSTM
    m = KerasSingleLSTM(num_encoder_tokens=6, latent_dim=32, seed=6, unrolled=True, sample_and_refeed=True, predict_step=T_OUT)
    noise = np.random.default_rng(14).standard_normal((T_OUT - 1, N, 6)).astype(np.float32)
    return m, u(13, N, 1, 6), {"noise": noise}      # the closure's `lo` walks the noise: the chunks must come in order


def others_future():
    from longterm360fov_amd.models import NoTeacherForcingOthersConvLSTM
    m = NoTeacherForcingOthersConvLSTM(num_encoder_tokens=6, latent_dim=32, num_user=8, fps=6, seed=5)
    return m, [u(10, N, T_IN, 6), u(11, N, T_OUT, 7, 6, 3), u(12, N, 1, 6)], {}


def convlstm(method):
    from longterm360fov_amd import utility
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    w = O.init_convlstm_seq2seq(1234, C=30, latent_dim=8, k=3, head="conv2d", head_filters=(24, 40))
    v = np.random.default_rng(18).standard_normal((N, T_IN, 30, 3))
    ti, pi = utility.theta_phi_index_for_onehot((v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32))
    maps = utility.create_one_hot(ti, pi).transpose(0, 1, 3, 4, 2).astype(np.float32)
    return ConvLSTMSeq2Seq(w, head="conv2d"), [maps, maps[:, -1:]], {"predict_step": T_OUT, "_method": method}


FAMILIES = {
    "Seq2SeqLSTM[H64-f32]": seq2seq,
    "Seq2SeqLSTM[H256-bf16]": functools.partial(seq2seq, "bf16"),
    "NoTeacherForcingSeq2Seq": self_fed,
    "StackedSeq2SeqLSTM": stacked,
    "OthersContextSeq2Seq[others_mlp]": others_mlp,
    "OthersMixingSeq2Seq": mixing,
    "OthersConvMixingSeq2Seq": functools.partial(mixing, True),
    "KerasSingleLSTM[sample_and_refeed]": single_refeed,
    "NoTeacherForcingOthersConvLSTM": others_future,
    "ConvLSTMSeq2Seq.predict": functools.partial(convlstm, "predict"),
    "ConvLSTMSeq2Seq.predict_index": functools.partial(convlstm, "predict_index"),
}


def check_status(m):
    """Clean status: no persistent kernel gave up a wait in the pipelined run."""
    if getattr(m, "_ws", None) is not None:
        m._ws.check()
    if getattr(m, "_trainer", None) is not None:
        m._trainer.check()


def both(m, x, kw, batch_size=BS):
    """(serial, pipelined, the ring the pipelined call used or None) of the model's predict."""
    kw = dict(kw)
    call = getattr(m, kw.pop("_method", "predict"))
    m.host_pipeline = False
    want = call(x, batch_size=batch_size, **kw)
    m.host_pipeline = True
    m._pipe_rings.pop("predict", None)
    got = call(x, batch_size=batch_size, **kw)
    check_status(m)
    return want, got, m._pipe_rings.get("predict", (None, None))[1]


def same(got, want):
    assert type(got) is type(want)
    for g, w in zip(*(v if isinstance(v, list) else [v] for v in (got, want))):
        assert g.dtype == w.dtype and g.shape == w.shape
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_every_model_family_predicts_what_the_serial_loop_predicts(name):
    m, x, kw = FAMILIES[name]()
    want, got, ring = both(m, x, kw)
    assert ring is not None and ring.S == 3, "the pipelined call did not go through a three-slot ring"
    same(got, want)
    assert want.shape[0] == N and np.abs(want.astype(np.float64)).max() > 0
    assert len({want[i].tobytes() for i in range(N)}) > 1      # rows differ: a wrong row would show
    same(getattr(m, kw.get("_method", "predict"))(x, batch_size=BS, **{k: v for k, v in kw.items() if k != "_method"}), want)


@functools.lru_cache(maxsize=None)
def the_model():
    """One Seq2SeqLSTM for the input forms and the ordering cases, and its serial prediction."""
    m, x, _ = seq2seq()
    m.host_pipeline = False
    return m, x, m.predict(x, batch_size=BS)


def test_float64_and_strided_inputs():
    m, x, want = the_model()
    rng = np.random.default_rng(40)
    enc64, dec64 = rng.uniform(-1, 1, (N, T_IN, 6)), rng.uniform(-1, 1, (N, T_OUT, 6))      # float64, and they do round
    assert (enc64.astype(np.float32).astype(np.float64) != enc64).any()
    wide = np.zeros((2 * N, T_IN, 12))
    wide[::2, :, ::2] = enc64
    fortran = np.asfortranarray(dec64)
    for xs in ([enc64, dec64], [wide[::2, :, ::2], fortran], [enc64[::-1], dec64[::-1]], [x[0].transpose(1, 0, 2).copy().transpose(1, 0, 2), x[1]]):
        assert not all(a.flags.c_contiguous and a.dtype == np.float32 for a in xs)
        w, g, ring = both(m, xs, {})
        assert ring is not None
        same(g, w)
    same(m.predict([enc64[::-1], dec64[::-1]], batch_size=BS)[::-1], m.predict([enc64, dec64], batch_size=BS))


@pytest.mark.parametrize("n", [0, 1, BS, BS + 1])
def test_row_counts_around_one_chunk(n):
    m, x, want = the_model()
    w, g, ring = both(m, [a[:n] for a in x], {})
    same(g, w)
    same(g, want[:n])
    assert (ring is not None) == (n > BS)      # one chunk, or none, keeps the serial loop


def test_a_device_tensor_input_takes_the_old_path_and_a_mixed_call_stages_the_rest(monkeypatch):
    import torch
    m, x, want = the_model()
    dev = [torch.from_numpy(a).cuda() for a in x]
    m.host_pipeline = True
    m._device_weights()
    m._pipe_rings.pop("predict", None)
    got = m._predict_chunks(dev, BS, m.predict_device, (T_OUT, 6))
    assert "predict" not in m._pipe_rings      # nothing to stage: the serial loop
    same(got, want)
    got = m._predict_chunks([x[0], dev[1]], BS, m.predict_device, (T_OUT, 6))
    assert m._pipe_rings["predict"][1] is not None and len(m._pipe_rings["predict"][1].slots[0].dev_in) == 1
    same(got, want)
    check_status(m)


def test_late_consumer_uploads_finish_long_before_their_slot_is_read():
    """A few milliseconds of unrelated device work on the compute stream in front of every chunk: the uploads of the
    following chunks are done long before their kernels start, and must still find their own slot untouched."""
    import torch
    m, x, want = the_model()
    a = torch.randn(4096, 4096, device="cuda")
    m.host_pipeline = True
    run = m.predict_device

    def slow(e, d):
        torch.matmul(a, a)
        return run(e, d)
    m._device_weights()
    same(m._predict_chunks(x, BS, slow, (T_OUT, 6)), want)
    check_status(m)


def test_late_producer_the_device_drains_between_chunks(monkeypatch):
    from longterm360fov_amd import hostpipe
    m, x, want = the_model()
    narrow = hostpipe.narrow

    def slow(dst, src):
        time.sleep(0.005)
        narrow(dst, src)
    monkeypatch.setattr(hostpipe, "narrow", slow)
    m.host_pipeline = True
    same(m.predict(x, batch_size=BS), want)
    check_status(m)


def test_the_host_blocks_in_event_waits_only(monkeypatch):
    import torch
    m, x, want = the_model()
    m.host_pipeline = True
    m.predict(x, batch_size=BS)      # the ring exists
    counts = {"to_device": 0, "synchronize": 0, "cpu": 0, "event_wait": 0}

    def counted(name, fn):
        def wrapper(*a, **k):
            counts[name] += 1
            return fn(*a, **k)
        return wrapper
    monkeypatch.setattr(type(m), "_to_device", counted("to_device", type(m)._to_device))
    monkeypatch.setattr(torch.cuda, "synchronize", counted("synchronize", torch.cuda.synchronize))
    monkeypatch.setattr(torch.Tensor, "cpu", counted("cpu", torch.Tensor.cpu))
    monkeypatch.setattr(torch.cuda.Event, "synchronize", counted("event_wait", torch.cuda.Event.synchronize))
    got = m.predict(x, batch_size=BS)
    monkeypatch.undo()
    same(got, want)
    chunks = -(-N // BS)
    assert counts["to_device"] == counts["synchronize"] == counts["cpu"] == 0, counts
    assert chunks <= counts["event_wait"] <= chunks + 3, counts
    m.host_pipeline = False      # ... and the serial loop is still the serial loop
    monkeypatch.setattr(type(m), "_to_device", counted("to_device", type(m)._to_device))
    m.predict(x, batch_size=BS)
    assert counts["to_device"] == 2 * chunks


def test_a_python_exception_from_run_propagates_and_the_next_predict_is_whole():
    m, x, want = the_model()
    m.host_pipeline = True
    m._device_weights()
    calls = []

    def failing(e, d):
        calls.append(e.shape[0])
        if len(calls) == 4:      # chunk 3
            raise KeyError("chunk 3")
        return m.predict_device(e, d)
    with pytest.raises(KeyError, match="chunk 3"):
        m._predict_chunks(x, BS, failing, (T_OUT, 6))
    assert "predict" not in m._pipe_rings and not m._pipe_lock.locked()
    same(m.predict(x, batch_size=BS), want)
    check_status(m)


def training_data(n=40):
    enc, dec0, tgt = O.synthetic_batch(55, n, 5, 4)
    return enc, np.concatenate([dec0, tgt[:, :-1]], axis=1), tgt


def trained_model(metrics):
    from longterm360fov_amd.models import Seq2SeqLSTM
    m = Seq2SeqLSTM(latent_dim=64)
    m.compile(optimizer="Adam", loss="mean_squared_error", metrics=metrics)
    w0 = O.init_seq2seq(56, H=64, bias_noise=0.05)
    m.set_weights([w0[k] for k in ("enc_K", "enc_R", "enc_b", "dec_K", "dec_R", "dec_b", "dense_W", "dense_b")])
    return m


@pytest.mark.parametrize("metrics", [None, ["accuracy"]])
def test_evaluate_equals_the_serial_evaluate(metrics):
    enc, dec_in, tgt = training_data(29)
    m = trained_model(metrics)
    m.host_pipeline = False
    want = m.evaluate([enc, dec_in], tgt, batch_size=BS)
    m.host_pipeline = True
    got = m.evaluate([enc.astype(np.float64)[::-1][::-1], dec_in], tgt, batch_size=BS)
    ring = m._pipe_rings["evaluate"][1]
    assert ring is not None and ring.S == 3 and ring.held is None and not m._pipe_lock.locked()
    assert isinstance(want, list) == bool(metrics) and got == want
    assert m.evaluate([enc, dec_in], tgt, batch_size=BS) == want      # the kept ring again
    assert m.evaluate([enc, dec_in], tgt, batch_size=64) == m.test_on_batch([enc, dec_in], tgt)      # one chunk: serial
    check_status(m)


def test_an_exception_in_a_streamed_fit_leaves_the_next_fit_whole(monkeypatch):
    from longterm360fov_amd.callbacks import Callback
    enc, dec_in, tgt = training_data(40)
    monkeypatch.setenv("FOV_FIT_RESIDENT_BYTES", "0")

    class Failing(Callback):
        def on_epoch_end(self, epoch, logs=None):
            raise KeyError("epoch %d" % epoch)

    def run(pipeline):
        m = trained_model(None)
        m.host_pipeline = pipeline
        np.random.seed(7)
        with pytest.raises(KeyError, match="epoch 0"):
            m.fit([enc, dec_in], tgt, batch_size=BS, epochs=2, validation_split=0.2, callbacks=[Failing()])
        h = m.fit([enc, dec_in], tgt, batch_size=BS, epochs=1, validation_split=0.2)
        check_status(m)
        return h.history, m.get_weights()
    want, got = run(False), run(True)
    assert got[0] == want[0]
    for a, b in zip(got[1], want[1]):
        np.testing.assert_array_equal(a, b)


def test_fit_streamed_from_the_host_equals_the_serial_fit(monkeypatch):
    """FOV_FIT_RESIDENT_BYTES=0, 2 epochs, seeded shuffle, validation_split 0.2: 32 training rows in 8 steps of 4 and 8
    held-out rows in 2 batches an epoch, each batch gathered into pinned memory and uploaded under the step before it."""
    from longterm360fov_amd import models
    enc, dec_in, tgt = training_data(40)
    planned = []
    plan = models._ArrayFeed._plan_epoch
    monkeypatch.setattr(models._ArrayFeed, "_plan_epoch", lambda self, *a: (planned.append(len(a[0])), plan(self, *a))[1])

    def run(pipeline, metrics=None):
        m = trained_model(metrics)
        m.host_pipeline = pipeline
        np.random.seed(7)
        h = m.fit([enc, dec_in], tgt, batch_size=BS, epochs=2, validation_split=0.2, shuffle=True, verbose=0)
        check_status(m)
        return h.history, m.get_weights()

    run(True)
    assert planned == []      # the resident path never reaches the feed's new method
    monkeypatch.setenv("FOV_FIT_RESIDENT_BYTES", "0")
    for metrics in (None, ["accuracy"]):
        del planned[:]
        want = run(False, metrics)
        assert planned == []
        got = run(True, metrics)
        assert planned == [8, 8]
        assert sorted(got[0]) == sorted(want[0]) and "val_loss" in got[0] and ("val_acc" in got[0]) == bool(metrics)
        for key in want[0]:
            assert got[0][key] == want[0][key], key
        for a, b in zip(got[1], want[1]):
            np.testing.assert_array_equal(a, b)
