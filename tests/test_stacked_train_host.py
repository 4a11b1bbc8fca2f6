"""The stacked seq2seq model's one-launch training entries without a GPU: fov_stacked_seq2seq_train_supported is arithmetic
(H = 32 or 64, L = 2 or 3, 1 <= F_enc <= 96, 1 <= F_dec <= 8, non-negative sizes) plus the FOV_NO_STACKED_TRAIN knob;
fov_stacked_seq2seq_train_fwd / _bwd refuse every other shape before they look at a pointer; fov_lstm_seq_wgrad_layers refuses a
layer count it does not take.  PaddedTrainer's padding of the stacked weight names, and the dataset methods' errors, are host
code too.  tests/test_abi.py holds the prototypes against the ctypes table."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from longterm360fov_amd import _lib

N_FWD_PTRS, N_BWD_PTRS = 15, 10


def _supported(B, T_in, T_out, F_enc, F_dec, H, L):
    return _lib.lib().fov_stacked_seq2seq_train_supported(B, T_in, T_out, F_enc, F_dec, H, L)


def _fwd(ptrs, B, T_in, T_out, F_enc, F_dec, H, L, act=_lib.ACT_SIGMOID):
    return _lib.lib().fov_stacked_seq2seq_train_fwd(*ptrs, B, T_in, T_out, F_enc, F_dec, H, L, act, None)


def _bwd(ptrs, B, T_in, T_out, H, L, act=_lib.ACT_SIGMOID):
    return _lib.lib().fov_stacked_seq2seq_train_bwd(*ptrs, B, T_in, T_out, H, L, act, None, 0, None)


def test_supported_truth_table():
    for H, L, F_enc, F_dec in itertools.product((32, 64), (2, 3), (1, 6, 16, 17, 90, 96), (1, 6, 8)):
        for B, T_in, T_out in ((0, 0, 0), (1, 1, 1), (17, 0, 3), (33, 3, 0), (100000, 30, 30)):
            assert _supported(B, T_in, T_out, F_enc, F_dec, H, L) == 1, (B, T_in, T_out, F_enc, F_dec, H, L)
    for H in (0, 16, 20, 48, 128, 256, -64):
        assert _supported(32, 10, 10, 6, 6, H, 2) == 0, H
    for L in (0, 1, 4, -2):
        assert _supported(32, 10, 10, 6, 6, 64, L) == 0, L
    for F_enc in (0, 97, 512, -1):
        assert _supported(32, 10, 10, F_enc, 6, 64, 2) == 0, F_enc
    for F_dec in (0, 9, 90, -1):
        assert _supported(32, 10, 10, 6, F_dec, 32, 3) == 0, F_dec
    assert _supported(-1, 10, 10, 6, 6, 64, 2) == 0 and _supported(32, -1, 10, 6, 6, 64, 2) == 0 and _supported(32, 10, -1, 6, 6, 64, 2) == 0


def test_scratch_bytes_is_the_dx_tape():
    f = _lib.lib().fov_stacked_seq2seq_train_bwd_scratch_bytes
    assert f(64, 10, 10, 32) == 4 * 64 * 10 * 32 and f(17, 3, 30, 64) == 4 * 17 * 30 * 64 and f(17, 30, 3, 64) == 4 * 17 * 30 * 64
    assert f(0, 10, 10, 32) == 0 and f(5, 0, 0, 64) == 0


@pytest.mark.parametrize("B,T_in,T_out,F_enc,F_dec,H,L", [(5, 2, 2, 6, 6, 16, 2), (5, 2, 2, 6, 6, 48, 2), (5, 2, 2, 6, 6, 128, 3),
                                                         (5, 2, 2, 6, 6, 64, 1), (5, 2, 2, 6, 6, 64, 4), (5, 2, 2, 97, 6, 64, 2),
                                                         (5, 2, 2, 6, 9, 32, 2), (5, 2, 2, 0, 6, 32, 2), (-1, 2, 2, 6, 6, 64, 2),
                                                         (5, -1, 2, 6, 6, 32, 3), (5, 2, -1, 6, 6, 32, 3)])
def test_unsupported_shapes_are_refused_before_any_pointer_is_looked_at(B, T_in, T_out, F_enc, F_dec, H, L):
    assert _supported(B, T_in, T_out, F_enc, F_dec, H, L) == 0
    wild = ctypes.c_void_p(0x10)      # would fault if an entry of a weight array were read
    assert _fwd([wild] * N_FWD_PTRS, B, T_in, T_out, F_enc, F_dec, H, L) == _lib.ERR_UNSUPPORTED
    msg = _lib.lib().fov_last_error().decode()
    assert "fov_stacked_seq2seq_train_fwd" in msg and "H=%d" % H in msg and "L=%d" % L in msg and "F_enc=%d" % F_enc in msg, msg
    if not (1 <= F_enc <= 96 and 1 <= F_dec <= 8):      # the backward does not take the input widths
        return
    assert _bwd([wild] * N_BWD_PTRS, B, T_in, T_out, H, L) == _lib.ERR_UNSUPPORTED
    msg = _lib.lib().fov_last_error().decode()
    assert "fov_stacked_seq2seq_train_bwd" in msg and "H=%d" % H in msg and "L=%d" % L in msg, msg


def _arr(n_set, value=0x1000):
    """An array of three pointers, the first n_set of them non-NULL (never dereferenced on the device here)."""
    a = (ctypes.c_void_p * 3)(*([value] * n_set + [None] * (3 - n_set)))
    return ctypes.cast(a, ctypes.c_void_p), a      # (keep `a` alive)


def test_missing_pointers_and_unknown_activations_are_invalid_and_an_empty_batch_is_a_no_op():
    some = ctypes.c_void_p(0x1000)
    assert _fwd([None] * N_FWD_PTRS, 4, 2, 2, 6, 6, 64, 2) == _lib.ERR_INVALID
    assert _bwd([None] * N_BWD_PTRS, 4, 2, 2, 64, 2) == _lib.ERR_INVALID
    two, keep2 = _arr(2)
    three, keep3 = _arr(3)
    # enc_in, dec_in | enc K, R, b, dec K, R, b | enc_hs, enc_res, dec_hs, dec_res, dec_top, hT, cT
    fwd = [some, some] + [two] * 6 + [None] * 7
    assert _fwd(fwd, 0, 3, 3, 6, 6, 64, 2) == _lib.OK and _fwd(fwd, 0, 0, 0, 1, 8, 32, 2, _lib.ACT_HARD_SIGMOID) == _lib.OK
    assert _fwd(fwd, 0, 3, 3, 6, 6, 64, 3) == _lib.ERR_INVALID                    # the third layer's weights are missing
    assert _fwd([some, some] + [three] * 6 + [None] * 7, 0, 3, 3, 6, 6, 64, 3) == _lib.OK
    assert _fwd(fwd, 0, 3, 3, 6, 6, 64, 2, 5) == _lib.ERR_INVALID                 # no such recurrent activation
    assert _fwd(fwd[:3] + [None] + fwd[4:], 0, 3, 3, 6, 6, 64, 2) == _lib.ERR_INVALID      # enc_R missing
    assert _fwd([None, some] + fwd[2:], 4, 3, 3, 6, 6, 64, 2) == _lib.ERR_INVALID           # an encoder step without enc_in
    # enc_res, dec_res, cT, dhs_top | enc R, K, dec R, K | enc_dz, dec_dz
    bwd = [some] * 4 + [two] * 4 + [some, some]
    assert _bwd(bwd, 0, 3, 3, 64, 2) == _lib.OK and _bwd(bwd, 0, 0, 0, 32, 2, _lib.ACT_HARD_SIGMOID) == _lib.OK
    assert _bwd(bwd, 5, 0, 0, 64, 2) == _lib.OK                                   # no step on either side: nothing to do
    assert _bwd(bwd, 0, 3, 3, 64, 2, 7) == _lib.ERR_INVALID
    assert _bwd(bwd, 0, 3, 3, 64, 3) == _lib.ERR_INVALID                          # the third layer's R and K are missing
    only_first, keep1 = _arr(1)
    assert _bwd(bwd[:5] + [only_first] + bwd[6:], 0, 3, 3, 64, 2) == _lib.ERR_INVALID     # K of layer 1 is needed ...
    upper = (ctypes.c_void_p * 3)(None, 0x1000, None)
    assert _bwd(bwd[:5] + [ctypes.cast(upper, ctypes.c_void_p)] + bwd[6:], 0, 3, 3, 64, 2) == _lib.OK   # ... K of layer 0 is not
    assert _bwd([None] + bwd[1:], 4, 3, 3, 64, 2) == _lib.ERR_INVALID             # encoder steps without their reserve
    assert _bwd(bwd, 4, 3, 3, 64, 2) == _lib.ERR_WORKSPACE                        # work to do and no scratch
    del keep1, keep2, keep3


def test_wgrad_layers_refuses_other_layer_counts_and_missing_arrays():
    f = _lib.lib().fov_lstm_seq_wgrad_layers
    for L in (0, 5, -1):
        assert f(L, *([None] * 9), 4, 32, 0, None, 0, None) == _lib.ERR_UNSUPPORTED
        assert "fov_lstm_seq_wgrad_layers" in _lib.lib().fov_last_error().decode()
    assert f(2, *([None] * 9), 4, 32, 0, None, 0, None) == _lib.ERR_INVALID


def test_knob_flips_supported():
    L_ = _lib.lib()
    assert "FOV_NO_STACKED_TRAIN" not in os.environ
    assert _supported(64, 10, 10, 6, 6, 32, 2) == 1
    os.environ["FOV_NO_STACKED_TRAIN"] = "1"
    try:
        L_.fov_reload_env()
        assert _supported(64, 10, 10, 6, 6, 32, 2) == 0 and _supported(4096, 30, 30, 90, 6, 64, 3) == 0
        assert L_.fov_stacked_seq2seq_decode_supported(64, 10, 10, 6, 6, 32, 2) == 1      # the decode has its own knob
        assert _fwd([None] * N_FWD_PTRS, 4, 2, 2, 6, 6, 64, 2) == _lib.ERR_INVALID        # the entries themselves do not read the knob
    finally:
        del os.environ["FOV_NO_STACKED_TRAIN"]
        L_.fov_reload_env()
    assert _supported(64, 10, 10, 6, 6, 32, 2) == 1


def test_ops_wrapper_follows_the_knob_when_the_environment_changes():
    from longterm360fov_amd import ops
    assert "FOV_NO_STACKED_TRAIN" in ops._ENV_KNOBS
    assert ops.stacked_seq2seq_train_supported(64, 10, 10, 6, 6, 32, 2) and not ops.stacked_seq2seq_train_supported(64, 10, 10, 6, 6, 20, 2)
    os.environ["FOV_NO_STACKED_TRAIN"] = "1"
    try:
        assert not ops.stacked_seq2seq_train_supported(64, 10, 10, 6, 6, 32, 2)
    finally:
        del os.environ["FOV_NO_STACKED_TRAIN"]
    assert ops.stacked_seq2seq_train_supported(64, 10, 10, 6, 6, 32, 2)


@pytest.mark.parametrize("H,L", [(20, 2), (20, 3), (40, 2), (40, 3)])
def test_padded_trainer_round_trips_the_stacked_weight_names(H, L):
    """pad -> unpad is the identity on every stacked weight, the padded tensors have the run width's shapes, and every padded
    slice - gate columns from H on, rows from H on of R, of the K of layers >= 1 and of dense_W - is zero."""
    from longterm360fov_amd.models import StackedSeq2SeqLSTM, padded_width
    from longterm360fov_amd.training import PaddedTrainer, stacked_weight_order
    rng = np.random.default_rng(100 * H + L)
    F, O = 6, 6
    w = {}
    for side, f0 in (("enc", F), ("dec", O)):
        for l in range(L):
            w["%s%d_K" % (side, l)] = rng.standard_normal((f0 if l == 0 else H, 4 * H)).astype(np.float32)
            w["%s%d_R" % (side, l)] = rng.standard_normal((H, 4 * H)).astype(np.float32)
            w["%s%d_b" % (side, l)] = rng.standard_normal(4 * H).astype(np.float32)
    w["dense_W"] = rng.standard_normal((H, O)).astype(np.float32)
    w["dense_b"] = rng.standard_normal(O).astype(np.float32)
    w = {k: w[k] for k in stacked_weight_order(L)}
    Hp = padded_width(H, StackedSeq2SeqLSTM.FUSED_WIDTHS)
    assert Hp == (32 if H == 20 else 64)
    hidden = tuple("%s%d_K" % (side, l) for side in ("enc", "dec") for l in range(1, L))
    seen = {}
    pt = PaddedTrainer(lambda wp: seen.setdefault("w", wp), w, H, Hp, hidden_inputs=hidden)
    wp = seen["w"]
    assert list(wp) == list(w)
    for k, v in wp.items():
        if k.endswith("_R") or k in hidden:
            assert v.shape == (Hp, 4 * Hp), k
            assert not v[H:].any(), k
        elif k.endswith("_K"):
            assert v.shape == (w[k].shape[0], 4 * Hp), k
        elif k.endswith("_b") and k != "dense_b":
            assert v.shape == (4 * Hp,), k
        if k == "dense_W":
            assert v.shape == (Hp, O) and not v[H:].any()
        elif k == "dense_b":
            np.testing.assert_array_equal(v, w[k])
        else:
            g4 = v.reshape(v.shape[:-1] + (4, Hp))
            assert not g4[..., H:].any(), k
            assert g4[..., :H].any(), k
    back = pt.unpad(wp)
    for k in w:
        np.testing.assert_array_equal(back[k], w[k])
    # a nonzero in a padded slice does not survive the round trip: that is what padded_slices_are_zero compares
    dirty = {k: v.copy() for k, v in wp.items()}
    dirty["enc1_K"][H, 0] = 1.0
    assert not np.array_equal(pt.pad(pt.unpad(dirty))["enc1_K"], dirty["enc1_K"])


def test_model_wraps_other_widths_up_to_64_and_leaves_the_rest(monkeypatch):
    from longterm360fov_amd import training
    from longterm360fov_amd.models import StackedSeq2SeqLSTM
    made = []

    class Probe:
        def __init__(self, w, L, **kw):
            made.append({k: v.shape for k, v in w.items()})
            self.lr = kw["lr"]
    monkeypatch.setattr(training, "StackedSeq2SeqTrainer", Probe)
    for H, Hp, wrapped in ((20, 32, True), (32, 32, False), (40, 64, True), (64, 64, False), (100, 100, False)):
        m = StackedSeq2SeqLSTM(num_encoder_tokens=6, latent_dim=H, num_layers=3, seed=1, device="cpu")
        tr = m._make_trainer("adam")
        assert isinstance(tr, training.PaddedTrainer) == wrapped, H
        shapes = made[-1]
        assert shapes["enc0_K"] == (6, 4 * Hp) and shapes["dec2_K"] == (Hp, 4 * Hp) and shapes["enc1_R"] == (Hp, 4 * Hp), (H, shapes)
        assert shapes["dense_W"] == (Hp, 6)


def test_dataset_method_errors_are_value_errors():
    """The model reads what Seq2SeqLSTM reads from a TrajectoryDataset: a dataset that does not fit is a ValueError (the right
    kind, with its reason), not the NotImplementedError of a model without dataset methods."""
    from longterm360fov_amd.models import StackedSeq2SeqLSTM

    class FakeDs:
        _dev, pick_user, num_user, fps, T_out = {}, False, 34, 30, 2

    m = StackedSeq2SeqLSTM(num_encoder_tokens=6, latent_dim=32, num_layers=2, seed=1, device="cpu")
    assert m.num_encoder_tokens == 6 and m.num_decoder_tokens == 6 and m._dataset_pick_user is False
    assert m._dataset_check(FakeDs()) == "mean_var"
    assert StackedSeq2SeqLSTM(num_encoder_tokens=90, latent_dim=32, seed=1, device="cpu")._dataset_check(FakeDs()) == "raw"
    picked = FakeDs()
    picked.pick_user = True
    with pytest.raises(ValueError, match="pick_user=False"):
        m.predict_dataset(picked)
    with pytest.raises(ValueError, match="encoder width 17"):
        StackedSeq2SeqLSTM(num_encoder_tokens=17, latent_dim=32, seed=1, device="cpu").predict_dataset(FakeDs())
    with pytest.raises(ValueError, match="the model predicts 3"):
        StackedSeq2SeqLSTM(num_encoder_tokens=6, num_decoder_tokens=3, latent_dim=32, seed=1, device="cpu").predict_dataset(FakeDs())
    host_only = FakeDs()
    host_only._dev = None
    with pytest.raises(RuntimeError, match="host tables only"):
        m.predict_dataset(host_only)
