"""The chunked prediction of every model (KerasModelSurface._predict_chunks): `batch_size` rows per device call, the
outputs copied to the host and concatenated.

Each of the twelve sites at the smallest shapes its model takes, N = 5 rows with batch_size = 2 (chunks of 2, 2 and a
ragged 1): the chunked result equals, bit for bit, the concatenation of three un-chunked calls on rows [0:2], [2:4], [4:5]
(a row's result does not depend on the rows it shares a launch with), and for N = 0 every site returns an empty float32
array per output whose shape after the leading 0 is that of a non-empty call."""
import functools

import numpy as np
import pytest

from oracle import fov_oracle as O

pytestmark = pytest.mark.gpu

N, BS, T_IN, T_OUT, H = 5, 2, 3, 2, 32
PARTS = (slice(0, 2), slice(2, 4), slice(4, 5))


def u(seed, *shape):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)


def seq2seq(method, dtype="f32"):
    from longterm360fov_amd.models import Seq2SeqLSTM
    F, width = (90, 256) if dtype == "bf16" else (6, H)      # the bf16 kernels are built for latent_dim = 256
    m = Seq2SeqLSTM(num_encoder_tokens=F, latent_dim=width, seed=1, dtype=dtype)
    enc, dec_in = u(1, N, T_IN, F), u(2, N, T_OUT, 6)
    if method == "predict":
        return lambda r, bs: m.predict([enc[r], dec_in[r]], batch_size=bs)
    return lambda r, bs: m.decode_sequence(enc[r], dec_in[r, :1], predict_step=T_OUT, batch_size=bs)


def self_fed(**kw):
    from longterm360fov_amd.models import NoTeacherForcingSeq2Seq
    m = NoTeacherForcingSeq2Seq(num_encoder_tokens=6, latent_dim=H, seed=2, predict_step=T_OUT, **kw)
    enc, dec0 = u(3, N, T_IN, 6), u(4, N, 1, 6)
    return lambda r, bs: m.predict([enc[r], dec0[r]], batch_size=bs)


def stacked(method):
    from longterm360fov_amd.models import StackedSeq2SeqLSTM
    m = StackedSeq2SeqLSTM(latent_dim=H, seed=3)
    enc, dec_in = u(5, N, T_IN, 6), u(6, N, T_OUT, 6)
    if method == "predict":
        return lambda r, bs: m.predict([enc[r], dec_in[r]], batch_size=bs)
    return lambda r, bs: m.decode_sequence(enc[r], dec_in[r, :1], predict_step=T_OUT, batch_size=bs)


def others_context(mode):
    from longterm360fov_amd.models import OthersContextSeq2Seq
    m = OthersContextSeq2Seq(mode, num_encoder_tokens=6, latent_dim=H, num_user=3, seed=4, predict_step=T_OUT)
    enc, oth, dec0 = u(7, N, T_IN, 6), u(8, N, T_OUT, 2, 6), u(9, N, 1, 6)
    if mode == "target_user_only":
        return lambda r, bs: m.predict([enc[r], dec0[r]], batch_size=bs)
    return lambda r, bs: m.predict([enc[r], oth[r], dec0[r]], batch_size=bs)


def others_future():
    from longterm360fov_amd.models import NoTeacherForcingOthersConvLSTM
    m = NoTeacherForcingOthersConvLSTM(num_encoder_tokens=6, latent_dim=H, num_user=8, fps=6, seed=5)
    enc, oth, dec0 = u(10, N, T_IN, 6), u(11, N, T_OUT, 7, 6, 3), u(12, N, 1, 6)
    return lambda r, bs: m.predict([enc[r], oth[r], dec0[r]], batch_size=bs)


def single(refeed):
    from longterm360fov_amd.models import KerasSingleLSTM
    m = KerasSingleLSTM(num_encoder_tokens=6, latent_dim=H, seed=6, unrolled=refeed, sample_and_refeed=refeed, predict_step=T_OUT)
    x, noise = u(13, N, 1 if refeed else T_IN, 6), np.random.default_rng(14).standard_normal((T_OUT - 1, N, 6)).astype(np.float32)
    return lambda r, bs: m.predict(x[r], batch_size=bs, noise=noise[:, r] if refeed else None)


def mixing():
    from longterm360fov_amd.models import OthersMixingSeq2Seq
    m = OthersMixingSeq2Seq(num_encoder_tokens=6, latent_dim=H, num_user=3, seed=7)
    enc, oth, dec0 = u(15, N, T_IN, 6), u(16, N, T_OUT, 2, 6), u(17, N, 1, 6)
    return lambda r, bs: m.predict([enc[r], oth[r], dec0[r]], batch_size=bs)


def convlstm(method):
    from longterm360fov_amd import utility
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    w = O.init_convlstm_seq2seq(1234, C=30, latent_dim=8, k=3, head="conv2d", head_filters=(24, 40))
    v = np.random.default_rng(18).standard_normal((N, T_IN, 30, 3))
    xyz = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    m = ConvLSTMSeq2Seq(w, head="conv2d")
    if method == "predict_trajectories":
        return lambda r, bs: m.predict_trajectories(xyz[r], xyz[r, -1:], batch_size=bs, predict_step=T_OUT)
    ti, pi = utility.theta_phi_index_for_onehot(xyz)
    maps = utility.create_one_hot(ti, pi).transpose(0, 1, 3, 4, 2).astype(np.float32)
    return lambda r, bs: m.predict([maps[r], maps[r, -1:]], batch_size=bs, predict_step=T_OUT)


def convlstm_dense():
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    m = ConvLSTMSeq2Seq(O.init_convlstm_seq2seq(77, C=6, latent_dim=8, k=3, head="dense", map_hw=(1, 1)), head="dense")
    enc = u(19, N, T_IN, 1, 1, 6)
    return lambda r, bs: m.predict([enc[r], enc[r, -1:]], batch_size=bs, predict_step=T_OUT)


CASES = {
    "Seq2SeqLSTM.predict": functools.partial(seq2seq, "predict"),
    "Seq2SeqLSTM.predict[bf16]": functools.partial(seq2seq, "predict", "bf16"),
    "Seq2SeqLSTM.decode_sequence": functools.partial(seq2seq, "decode_sequence"),
    "NoTeacherForcingSeq2Seq.predict": self_fed,
    "NoTeacherForcingSeq2Seq.predict[unrolled]": functools.partial(self_fed, add_residual_link=True),
    "NoTeacherForcingSeq2Seq.predict[has_reconstruct_loss]": functools.partial(self_fed, has_reconstruct_loss=True),
    "StackedSeq2SeqLSTM.predict": functools.partial(stacked, "predict"),
    "StackedSeq2SeqLSTM.decode_sequence": functools.partial(stacked, "decode_sequence"),
    "OthersContextSeq2Seq.predict[others_mlp]": functools.partial(others_context, "others_mlp"),
    "OthersContextSeq2Seq.predict[target_user_only]": functools.partial(others_context, "target_user_only"),
    "NoTeacherForcingOthersConvLSTM.predict": others_future,
    "KerasSingleLSTM.predict": functools.partial(single, False),
    "KerasSingleLSTM.predict[sample_and_refeed]": functools.partial(single, True),
    "OthersMixingSeq2Seq.predict": mixing,
    "ConvLSTMSeq2Seq.predict": functools.partial(convlstm, "predict"),
    "ConvLSTMSeq2Seq.predict[dense]": convlstm_dense,
    "ConvLSTMSeq2Seq.predict_trajectories": functools.partial(convlstm, "predict_trajectories"),
}


@functools.lru_cache(maxsize=None)
def chunked(name):
    """(run, the outputs of run on all N rows with batch_size = BS), once per site."""
    run = CASES[name]()
    return run, outputs(run(slice(0, N), BS))


def outputs(y):
    return list(y) if isinstance(y, list) else [y]


@pytest.mark.parametrize("name", sorted(CASES))
def test_chunked_predict_equals_the_separate_calls(name):
    run, got = chunked(name)
    parts = [outputs(run(r, None)) for r in PARTS]
    assert len(got) == (2 if "has_reconstruct_loss" in name else 1)
    for i, g in enumerate(got):
        assert g.shape[0] == N and g.dtype == np.float32
        np.testing.assert_array_equal(g, np.concatenate([p[i] for p in parts], axis=0))
        assert np.abs(g).max() > 0 and np.isfinite(g).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_predict_of_no_rows_keeps_the_trailing_shape(name):
    run, full = chunked(name)
    for bs in (BS, None):
        empty = outputs(run(slice(0, 0), bs))
        assert len(empty) == len(full)
        for e, g in zip(empty, full):
            assert e.shape == (0,) + g.shape[1:] and e.dtype == np.float32
