"""TrajectoryDataset's host tables against utility.get_data, row for row: the device pipeline of the seq2seq LSTM models
(longterm360fov_amd/trajectories.py) reads its windows through three ints each, and those ints must name exactly the seconds
the reference's windowing copies.  No GPU and no library: device=None builds the tables only."""
import numpy as np
import pytest

from longterm360fov_amd import utility
from longterm360fov_amd.config import cfg
from longterm360fov_amd.trajectories import TrajectoryDataset, gather_host

NUM_USER = 5
STRIDES = (1, 3, 5, 10)            # 3 does not divide running_length = 10: the future lies 9 seconds ahead


def _video(rng, users, frames):
    v = rng.standard_normal((users, frames, 3))
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    return {"x": v[..., 0].copy(), "y": v[..., 1].copy(), "z": v[..., 2].copy()}


def make_datadb(seed=7):
    """Three usable videos - fewer users than num_user (others padded by np.random draws) with a partial trailing second,
    exactly num_user, more (others cut) - and one of 19 seconds, which get_data skips, between them."""
    rng = np.random.default_rng(seed)
    return {"v1": _video(rng, 3, 21 * 30 + 7), "short": _video(rng, 4, 19 * 30), "v2": _video(rng, 5, 25 * 30),
            "v3": _video(rng, 7, 20 * 30)}


def make_tiny_datadb(seed=11):
    """For cfg.running_length = 3 and num_user = 3: 7 and 6 seconds, 2 users (one other, padded) and 4 (cut)."""
    rng = np.random.default_rng(seed)
    return {"a": _video(rng, 2, 7 * 30), "b": _video(rng, 4, 6 * 30 + 11)}


@pytest.fixture
def stride_cfg():
    keep = cfg.data_chunk_stride
    yield
    cfg.data_chunk_stride = keep


@pytest.mark.parametrize("pick_user", [False, True])
@pytest.mark.parametrize("stride", STRIDES)
def test_tables_name_get_datas_windows(stride, pick_user, stride_cfg):
    db = make_datadb()
    cfg.data_chunk_stride = stride
    np.random.seed(stride)
    ref = utility.get_data(db, pick_user=pick_user, num_user=NUM_USER)
    np.random.seed(stride)
    ds = TrajectoryDataset(db, pick_user, num_user=NUM_USER, stride=stride, device=None)
    assert ds.fut_offset == (10 // stride) * stride == ds.tables()["fut_offset"]
    assert ds.fut_offset == {1: 10, 3: 9, 5: 10, 10: 10}[stride]
    assert len(ds) == ref[0].shape[0] > 0
    got = gather_host(ds.tables(), np.arange(len(ds)))
    assert len(got) == len(ref) == (6 if pick_user else 3)
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype == np.float64 and g.shape == r.shape
        assert np.array_equal(g, r)
    # the default stride is cfg's
    np.random.seed(stride)
    assert np.array_equal(TrajectoryDataset(db, pick_user, num_user=NUM_USER, device=None).tables()["sample"], ds.tables()["sample"])


def test_pick_user_layout_and_padding():
    """Targets in user order inside a video, windows inside a target; a padded slot repeats one of the real others, a cut
    list keeps the first num_user - 1 in np.delete's order."""
    db = make_datadb()
    np.random.seed(3)
    ds = TrajectoryDataset(db, True, num_user=NUM_USER, stride=10, device=None)
    t = ds.tables()
    sample, ob = t["sample"], t["others_base"]
    assert ob.shape == (3 + 5 + 7, NUM_USER - 1) and sample.dtype == ob.dtype == np.int32
    assert (np.diff(sample[:, 1]) >= 0).all() and sample[:, 1].max() == len(ob) - 1
    assert sorted(set(ob[0][:2])) == [21, 42] and set(ob[0][2:]) <= {21, 42}      # v1: 21 seconds a track, target 0
    v3 = 3 * 21 + 5 * 25                                                           # first row of v3 (the short video holds none)
    assert ob[3 + 5 + 2].tolist() == [v3 + 20 * u for u in (0, 1, 3, 4)]           # target 2 of 7 users: 0, 1, 3, 4 kept
    assert t["secs"].shape == (3 * 21 + 5 * 25 + 7 * 20, 90)


def test_video_keys_select_and_order():
    db = make_datadb()
    ds = TrajectoryDataset(db, False, video_keys=["v3", "v1"], device=None)
    ref = utility.get_data({k: db[k] for k in ("v3", "v1")}, pick_user=False)
    assert len(ds) == ref[0].shape[0]
    for g, r in zip(gather_host(ds.tables(), np.arange(len(ds))), ref):
        assert np.array_equal(g, r)


@pytest.mark.parametrize("knob", ["time_shift", "purelly_testing"])
def test_unbuilt_settings_are_refused(knob):
    keep = cfg[knob]
    try:
        cfg[knob] = True
        with pytest.raises(ValueError):
            TrajectoryDataset(make_datadb(), False, device=None)
    finally:
        cfg[knob] = keep
    with pytest.raises(ValueError):
        TrajectoryDataset(make_datadb(), False, stride=11, device=None)
    with pytest.raises(ValueError):
        TrajectoryDataset(make_datadb(), False, stride=0, device=None)


def test_split_is_kerass_held_out_tail():
    db = make_datadb()
    np.random.seed(1)
    ds = TrajectoryDataset(db, True, num_user=NUM_USER, stride=5, device=None)
    n = len(ds)
    lead, tail = ds.split(0.75)
    assert len(lead) == int(n * 0.75) and len(lead) + len(tail) == n
    full = gather_host(ds.tables(), np.arange(n))
    for part, sl in ((lead, slice(0, len(lead))), (tail, slice(len(lead), n))):
        assert part.tables()["secs"] is ds.tables()["secs"]                        # views: the seconds are shared
        got = gather_host(part.tables(), np.arange(len(part)))
        for g, f in zip(got[:3], full[:3]):
            assert np.array_equal(g, f[sl])
        for g, f in zip(got[3:], full[3:]):
            assert np.array_equal(g, f[:, sl])
    assert len(ds.split(0.0)[0]) == 0 and len(ds.split(1.0)[1]) == 0
    with pytest.raises(ValueError):
        ds.split(1.5)


@pytest.mark.parametrize("pick_user", [False, True])
def test_empty_dataset(pick_user):
    db = {"short": make_datadb()["short"]}
    ds = TrajectoryDataset(db, pick_user, num_user=NUM_USER, device=None)
    ref = utility.get_data(db, pick_user=pick_user, num_user=NUM_USER)
    assert len(ds) == 0
    got = gather_host(ds.tables(), np.arange(0))
    assert [g.shape for g in got] == [r.shape for r in ref]
    assert len(TrajectoryDataset({}, pick_user, num_user=NUM_USER, device=None)) == 0
    with pytest.raises(RuntimeError):
        ds.batch(np.arange(0))                                                     # host tables only


def test_tiny_running_length():
    keep = cfg.running_length, cfg.data_chunk_stride
    try:
        cfg.running_length, cfg.data_chunk_stride = 3, 2
        db = make_tiny_datadb()
        for pick_user in (False, True):
            np.random.seed(5)
            ref = utility.get_data(db, pick_user=pick_user, num_user=3)
            np.random.seed(5)
            ds = TrajectoryDataset(db, pick_user, num_user=3, device=None)
            assert ds.fut_offset == 2 and len(ds) == ref[0].shape[0] > 0
            for g, r in zip(gather_host(ds.tables(), np.arange(len(ds))), ref):
                assert np.array_equal(g, r)
    finally:
        cfg.running_length, cfg.data_chunk_stride = keep
