"""The seq2seq LSTM models fed from FoV tracks held on the device: fov_window_inputs (one gather launch per batch),
TrajectoryDataset.batch, and predict_dataset / evaluate_dataset / fit_dataset against the same calls on host arrays.

The gather moves bits, so every comparison with the reference's windows (utility.get_data, float32) is for equality; the
mean / variance entries are equal to ops.meanvar_xyz of the materialised windows (that kernel's arithmetic for a row does not
depend on where the row lies) and within its own bound, 2e-6 (test_gpu_parity.test_meanvar_against_reference_fixture), of the
float64 helpers get_gt_target_xyz[_oth]."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_traj_dataset import NUM_USER, make_datadb, make_tiny_datadb  # noqa: E402

from longterm360fov_amd import _lib, utility  # noqa: E402
from longterm360fov_amd.config import cfg  # noqa: E402
from longterm360fov_amd.trajectories import TrajectoryDataset  # noqa: E402
from oracle import fov_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

MEANVAR_BOUND = 2e-6        # test_meanvar_against_reference_fixture's `tight`
HIT_RATE_BOUND = 2e-5       # test_fov_hit_rate_against_oracle's
T = 10


def _ops():
    from longterm360fov_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(stride, pick_user, tiny=False):
    """(dataset, get_data's arrays) of one setting; computed once, never written to."""
    keep = cfg.running_length, cfg.data_chunk_stride
    try:
        if tiny:
            cfg.running_length = 3
        cfg.data_chunk_stride = stride
        db, num_user = (make_tiny_datadb(), 3) if tiny else (make_datadb(), NUM_USER)
        np.random.seed(stride)
        ref = utility.get_data(db, pick_user=pick_user, num_user=num_user)
        np.random.seed(stride)
        ds = TrajectoryDataset(db, pick_user, num_user=num_user)
    finally:
        cfg.running_length, cfg.data_chunk_stride = keep
    for a in ref:
        a.setflags(write=False)
    return ds, ref


def check_batch(b, ref, index, enc_form, pick_user, fps=30):
    """Every entry of a batch dict against the reference's windows `ref` (get_data's tuple) at rows `index`."""
    ops = _ops()
    enc, fut = ref[0][index], ref[1][index]
    n, t = enc.shape[:2]
    mv = lambda a: host(ops.meanvar_xyz(dev(a), fps))
    within = lambda got, ref64: float(np.abs(got.astype(np.float64) - ref64).max()) if got.size else 0.0
    if enc_form == "raw":
        assert b["enc"].shape == (n, t, 3 * fps) and np.array_equal(host(b["enc"]), f32(enc))
    else:
        assert b["enc"].shape == (n, t, 6) and np.array_equal(host(b["enc"]), mv(enc))
        e = within(host(b["enc"]), utility.get_gt_target_xyz(enc))
        print("enc mean_var vs float64 helper: %.3e" % e)
        assert e <= MEANVAR_BOUND
    if "future_raw" in b:
        assert np.array_equal(host(b["future_raw"]), f32(fut))
    assert b["dec_in"].shape == (n, 1, 6) and b["target"].shape == (n, t, 6)
    assert np.array_equal(host(b["dec_in"]), mv(enc[:, -1:]))
    assert np.array_equal(host(b["target"]), mv(fut))
    e_dec = within(host(b["dec_in"]), utility.get_gt_target_xyz(enc[:, -1:]))
    e_tgt = within(host(b["target"]), utility.get_gt_target_xyz(fut))
    print("dec_in %.3e, target %.3e vs float64 helpers" % (e_dec, e_tgt))
    assert e_dec <= MEANVAR_BOUND and e_tgt <= MEANVAR_BOUND
    assert ("others" in b) == bool(pick_user)
    if pick_user:
        oth = utility.reshape_others_data(ref[4][:, index])                     # (n, T, U-1, 30, 3)
        assert b["others"].shape == oth.shape[:3] + (6,)
        assert np.array_equal(host(b["others"]), mv(oth))
        e_oth = within(host(b["others"]), utility.get_gt_target_xyz_oth(oth))
        print("others vs float64 helper: %.3e" % e_oth)
        assert e_oth <= MEANVAR_BOUND


# ---------------------------------------------------------------------------------------------------------------------------
# ds.batch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pick_user", [False, True])
@pytest.mark.parametrize("stride", [1, 3])
def test_whole_dataset_batch(stride, pick_user):
    ds, ref = case(stride, pick_user)
    n = len(ds)
    assert n == ref[0].shape[0] and n % 256 and (n * T * 45) % 256          # no output ends on a workgroup's edge
    index = np.arange(n)
    check_batch(ds.batch(index, enc="raw", future_raw=True), ref, index, "raw", pick_user)
    b = ds.batch(index, enc="mean_var")
    assert "future_raw" not in b
    check_batch(b, ref, index, "mean_var", pick_user)
    r = ds.batch_range(3, n - 2, enc="mean_var")
    for k in b:
        assert torch.equal(r[k], b[k][3:n - 2])


@pytest.mark.parametrize("pick_user", [False, True])
def test_tiny_running_length(pick_user):
    ds, ref = case(2, pick_user, tiny=True)
    assert ds.T_in == 3 and ds.fut_offset == 2 and len(ds) == ref[0].shape[0] > 0
    index = np.arange(len(ds))
    check_batch(ds.batch(index, future_raw=True), ref, index, "raw", pick_user)
    check_batch(ds.batch(index, enc="mean_var"), ref, index, "mean_var", pick_user)


@pytest.mark.parametrize("pick_user", [False, True])
def test_selections(pick_user):
    ds, ref = case(1, pick_user)
    n = len(ds)
    perm = np.random.default_rng(4).permutation(n)
    for index in (perm, perm[:1], np.array([n - 1]), np.array([5, 5, 0, 5]), np.arange(0)):
        check_batch(ds.batch(index, future_raw=True), ref, index, "raw", pick_user)
        check_batch(ds.batch(list(index), enc="mean_var"), ref, index, "mean_var", pick_user)
    for bad in ([n], [-1], [0, n + 3]):
        with pytest.raises(IndexError):
            ds.batch(bad)
    with pytest.raises(TypeError):
        ds.batch(np.array([0.5]))
    with pytest.raises(ValueError):
        ds.batch([0], enc="onehot")
    lead, tail = ds.split(0.75)
    k = len(lead)
    assert k == int(n * 0.75)
    check_batch(lead.batch(np.arange(k)), ref, np.arange(k), "raw", pick_user)
    check_batch(tail.batch(np.arange(n - k), enc="mean_var"), ref, np.arange(k, n), "mean_var", pick_user)
    with pytest.raises(IndexError):
        tail.batch([n - k])


def _tables(ds):
    d = ds._dev
    return d["secs"], d["feat"], d["sample"], d["others_base"]


def test_each_output_alone_and_no_others():
    """Every output NULL but one, in turn; n = 0; n_others = 0."""
    ops = _ops()
    ds, _ = case(3, True)
    secs, feat, sample, ob = _tables(ds)
    names = ops.WINDOW_INPUT_NAMES
    for width in (90, 6):
        full = ops.window_inputs(secs, feat, sample, ob, T, T, ds.fut_offset, enc_width=width, outputs=names)
        assert sorted(full) == sorted(names)
        for k in names:
            one = ops.window_inputs(secs, feat, sample, ob, T, T, ds.fut_offset, enc_width=width, outputs=(k,))
            assert list(one) == [k] and torch.equal(one[k], full[k])
    none = ops.window_inputs(secs, feat, sample, ob, T, T, ds.fut_offset, outputs=())
    assert none == {}
    empty = ops.window_inputs(secs, feat, sample[:0], ob, T, T, ds.fut_offset, outputs=names)
    assert [tuple(empty[k].shape) for k in names] == [(0, T, 90), (0, 6), (0, T, 6), (0, T, NUM_USER - 1, 6), (0, T, 90)]
    solo = ops.window_inputs(secs, feat, sample, None, T, T, ds.fut_offset, outputs=names)       # n_others = 0
    assert solo["others"].shape == (len(ds), T, 0, 6)
    for k in ("enc", "dec_in", "target", "future_raw"):
        assert torch.equal(solo[k], full[k] if k != "enc" else ops.window_inputs(secs, feat, sample, ob, T, T, ds.fut_offset,
                                                                                 outputs=("enc",))["enc"])
    with pytest.raises(ValueError):
        ops.window_inputs(secs, feat, sample, ob, T, T, ds.fut_offset, outputs=("enc", "dec"))
    with pytest.raises(TypeError):
        ops.window_inputs(secs, feat, sample.long(), ob, T, T, ds.fut_offset)


def test_unaligned_bases_take_the_scalar_form():
    """A base 4 bytes off an 8-byte boundary: the 4-byte form, same bits."""
    ops = _ops()
    ds, _ = case(3, True)
    secs, feat, sample, ob = _tables(ds)
    names = ops.WINDOW_INPUT_NAMES
    full = ops.window_inputs(secs, feat, sample, ob, T, T, ds.fut_offset, outputs=names)
    shifted = torch.empty(feat.numel() + 1, dtype=torch.float32, device=feat.device)[1:].view(feat.shape)
    shifted.copy_(feat)
    assert shifted.data_ptr() % 8 == 4 and shifted.is_contiguous()
    got = ops.window_inputs(secs, shifted, sample, ob, T, T, ds.fut_offset, outputs=names)
    for k in names:
        assert torch.equal(got[k], full[k])


# ---------------------------------------------------------------------------------------------------------------------------
# through the C ABI: samples that point outside the tables, a bad encoder width
# ---------------------------------------------------------------------------------------------------------------------------
def test_out_of_range_samples_write_zeros():
    ops = _ops()
    ds, _ = case(3, True)
    secs, feat, sample, ob = _tables(ds)
    rows, n = secs.shape[0], len(ds)
    names = ops.WINDOW_INPUT_NAMES
    good = ops.window_inputs(secs, feat, sample, ob, T, T, ds.fut_offset, outputs=names)
    bad = sample.clone()
    last = ds.fut_offset + T                                                  # seconds of its track a sample names
    whole = {1: (rows + 5, 0, 0), 4: (rows - last + 1, 0, 0), 7: (-1, 0, 3), 9: (0, 0, -2), 12: (0, 0, 2 ** 31 - 1),
             n - 1: (2 ** 31 - 1, 0, 2 ** 31 - 1)}
    for i, row in whole.items():
        bad[i] = torch.tensor(row, dtype=torch.int32)
    bad[14, 1] = ob.shape[0]                                                  # no such row of others_base: its others only
    bad[15, 1] = -1
    ob2 = torch.cat((ob, torch.tensor([[0, rows - last + 1, rows, -3]], dtype=torch.int32, device=ob.device)))
    bad[16, 1] = ob.shape[0]                                                  # ... with ob2 a row whose slots 1-3 lie outside
    bad[16, 2] = 0
    for table, oth_zero in ((ob, {14: slice(None), 15: slice(None), 16: slice(None)}),
                            (ob2, {15: slice(None), 16: slice(1, None)})):
        got = ops.window_inputs(secs, feat, bad, table, T, T, ds.fut_offset, outputs=names)
        torch.cuda.synchronize()
        keep = np.array([i for i in range(n) if i not in whole and i not in (14, 15, 16)])
        for k in names:
            g = host(got[k])
            assert not g[list(whole)].any(), k
            assert np.array_equal(g[keep], host(good[k])[keep]), k
            if k != "others":
                for i in (14, 15):
                    assert np.array_equal(g[i], host(good[k])[i]), k
        oth = host(got["others"])
        for i, slots in oth_zero.items():
            assert not oth[i][:, slots].any()
        if table is ob2:
            assert np.array_equal(oth[14], host(ops.window_inputs(secs, feat, bad[14:15], ob2, T, T, ds.fut_offset,
                                                                  outputs=("others",))["others"])[0])
            first = host(feat)[ds.fut_offset:ds.fut_offset + T]               # track 0 from second 0
            assert np.array_equal(oth[16][:, 0], first)


def test_bad_encoder_width_is_invalid():
    ds, _ = case(3, True)
    secs, feat, sample, ob = _tables(ds)
    L = _lib.lib()
    enc = torch.full((len(ds), T, 7), 3.0, dtype=torch.float32, device="cuda")
    args = lambda width, n: (secs.data_ptr(), feat.data_ptr(), secs.shape[0], 30, sample.data_ptr(), n, ob.data_ptr(), ob.shape[0],
                             ob.shape[1], T, T, ds.fut_offset, enc.data_ptr(), width, None, None, None, None, None)
    assert L.fov_window_inputs(*args(7, len(ds))) == _lib.ERR_INVALID
    assert b"enc_width" in L.fov_last_error()
    assert L.fov_window_inputs(*args(7, 0)) == _lib.ERR_INVALID
    assert L.fov_window_inputs(*args(6, 0)) == _lib.OK                        # n = 0: nothing launched
    torch.cuda.synchronize()
    assert bool((enc == 3.0).all())
    with pytest.raises(_lib.FovError):
        _ops().window_inputs(secs, feat, sample, ob, T, T, ds.fut_offset, enc_width=7)


# ---------------------------------------------------------------------------------------------------------------------------
# the models
# ---------------------------------------------------------------------------------------------------------------------------
# bf16 exists at latent_dim = 256 only (the models raise for any other width); fp32 runs at 128
MODELS = [("s2s", 128, "f32"), ("s2s", 256, "bf16"), ("mix", 128, "f32"), ("mix", 256, "bf16")]


def make_model(kind, H, dtype, enc_width=90, seed=3):
    from longterm360fov_amd.models import OthersMixingSeq2Seq, Seq2SeqLSTM
    if kind == "s2s":
        return Seq2SeqLSTM(num_encoder_tokens=enc_width, latent_dim=H, dtype=dtype, seed=seed)
    return OthersMixingSeq2Seq(num_encoder_tokens=enc_width, latent_dim=H, num_user=NUM_USER, dtype=dtype, seed=seed)


def host_arrays(m, ds, enc_form):
    """(x, y) for predict / evaluate / fit: what ds.batch hands out, copied to the host."""
    b = ds.batch(np.arange(len(ds)), enc=enc_form)
    return [host(a) for a in m._dataset_inputs(b)], host(b["target"])


@pytest.mark.parametrize("kind,H,dtype", MODELS)
def test_predict_and_evaluate_dataset(kind, H, dtype):
    enc_width = 6 if dtype == "f32" else 90                                   # both encoder forms get a turn
    ds, _ = case(1, kind == "mix")
    n = len(ds)
    m = make_model(kind, H, dtype, enc_width)
    m.compile(optimizer="Adam")
    x, y = host_arrays(m, ds, "mean_var" if enc_width == 6 else "raw")
    assert x[0].shape == (n, T, enc_width) and x[-1].shape == ((n, T, 6) if kind == "s2s" else (n, 1, 6))
    for bs in (None, 7):
        pred = m.predict_dataset(ds, batch_size=bs)
        assert pred.shape == (n, T, 6) and pred.dtype == np.float32
        assert np.array_equal(pred, m.predict(x, batch_size=bs))
        ev = m.evaluate_dataset(ds, batch_size=bs)
        assert sorted(ev) == ["hit_rate", "hit_rate_per_sequence", "loss"]
        assert ev["loss"] == m.evaluate(x, y, batch_size=bs)
        per = ev["hit_rate_per_sequence"]
        assert per.shape == (n, T) and per.dtype == np.float32
        ref = O.fov_hit_rate(pred[..., :3].astype(np.float64), y[..., :3].astype(np.float64))
        err = float(np.abs(per - ref).max())
        print("%s %s batch %s: loss %.6f, hit rate vs oracle %.3e" % (kind, dtype, bs, ev["loss"], err))
        assert err < HIT_RATE_BOUND
        # the mean over the sequences: an fp64 sum on the device against NumPy's fp64 one, of n values in [0, 1]
        assert ev["hit_rate"].shape == (T,) and np.abs(ev["hit_rate"] - per.mean(axis=0, dtype=np.float64)).max() <= n * 2.0 ** -52
    narrow = m.evaluate_dataset(ds, span_deg=90.0, gt_span_deg=100.0)["hit_rate_per_sequence"]
    assert np.abs(narrow - O.fov_hit_rate(pred[..., :3].astype(np.float64), y[..., :3].astype(np.float64), 90.0, 100.0)).max() < HIT_RATE_BOUND


def test_empty_dataset_through_the_models():
    ds = TrajectoryDataset({"short": make_datadb()["short"]}, False)
    m = make_model("s2s", 128, "f32")
    m.compile()
    assert m.predict_dataset(ds).shape == (0, T, 6)
    ev = m.evaluate_dataset(ds, batch_size=4)
    assert ev["hit_rate_per_sequence"].shape == (0, T) and ev["hit_rate"].shape == (T,)
    assert ds.batch(np.arange(0))["enc"].shape == (0, T, 90)


@pytest.mark.parametrize("kind", ["s2s", "mix"])
@pytest.mark.parametrize("shuffle", [False, True])
def test_fit_dataset_equals_fit_on_the_arrays(kind, shuffle, tmp_path):
    from longterm360fov_amd.callbacks import ModelCheckpoint
    ds, _ = case(1, kind == "mix")
    kw = dict(batch_size=8, epochs=2, validation_split=0.25, shuffle=shuffle)
    a, b = make_model(kind, 128, "f32"), make_model(kind, 128, "f32")
    a.compile(optimizer="Adam")
    b.compile(optimizer="Adam")
    x, y = host_arrays(a, ds, "raw")
    np.random.seed(21)
    ha = a.fit(x, y, **kw)
    ck = ModelCheckpoint(str(tmp_path / "traj{epoch:02d}.h5"), monitor="val_loss")
    np.random.seed(21)
    hb = b.fit_dataset(ds, callbacks=[ck], **kw)
    assert sorted(hb.history) == ["loss", "lr", "val_loss"] and len(hb.history["loss"]) == 2
    assert hb.history == ha.history
    for wa, wb in zip(a.get_weights(), b.get_weights()):
        assert np.array_equal(wa, wb)
    assert not np.array_equal(b.get_weights()[0], make_model(kind, 128, "f32").get_weights()[0])      # it did train
    assert len(ck.saved) == 2 and all(os.path.exists(p) for p in ck.saved)
    # held-out windows given as a dataset of their own: the same numbers
    c = make_model(kind, 128, "f32")
    c.compile(optimizer="Adam")
    lead, tail = ds.split(0.75)
    np.random.seed(21)
    hc = c.fit_dataset(lead, validation_data=tail, batch_size=8, epochs=2, shuffle=shuffle)
    assert hc.history == ha.history


def test_wrong_dataset_for_the_model():
    solo, _ = case(1, False)
    picked, _ = case(1, True)
    s2s, mix = make_model("s2s", 128, "f32"), make_model("mix", 128, "f32")
    for m, ds in ((s2s, picked), (mix, solo)):
        m.compile()
        for call in (m.predict_dataset, m.evaluate_dataset, m.fit_dataset):
            with pytest.raises(ValueError):
                call(ds)
    with pytest.raises(ValueError):
        make_model("s2s", 128, "f32", enc_width=12).predict_dataset(solo)
    with pytest.raises(RuntimeError):
        make_model("s2s", 128, "f32").fit_dataset(solo)                      # not compiled
