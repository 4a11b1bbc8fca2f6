"""Host mirrors of the heat-map decode (utility.heatmap_argmax, utility.bin_centre_xyz) and the argument checks of
ConvLSTMSeq2Seq's decode entry points that run before any device work."""
import numpy as np
import pytest

from longterm360fov_amd import utility
from oracle import fov_oracle as O


def reference_line(decoded, fps=30):
    """mycode/convlstm_seq2seq.py:537-542 with batch_size / cfg.predict_step read off the array."""
    return np.argmax(decoded.reshape(decoded.shape[0], decoded.shape[1], -1, fps), axis=-2)


def test_heatmap_argmax_is_the_reference_line():
    rng = np.random.default_rng(0)
    d = rng.standard_normal((2, 3, 36, 18, 30)).astype(np.float32)
    got = utility.heatmap_argmax(d)
    assert got.shape == (2, 3, 30) and got.dtype == np.int64
    np.testing.assert_array_equal(got, reference_line(d))
    tied = rng.integers(0, 4, (2, 3, 36, 18, 30)).astype(np.float32)     # four levels: every maximum is taken many times
    flat = tied.reshape(2, 3, -1, 30)
    assert ((flat == flat.max(axis=-2, keepdims=True)).sum(axis=-2) > 1).all()
    np.testing.assert_array_equal(utility.heatmap_argmax(tied), reference_line(tied))


def test_bin_centres_round_trip_and_are_unit_vectors():
    index = np.arange(648)
    xyz = utility.bin_centre_xyz(index)
    assert xyz.shape == (648, 3) and xyz.dtype == np.float64
    assert np.abs(np.linalg.norm(xyz, axis=-1) - 1.0).max() <= 1e-7
    for centres in (xyz, xyz.astype(np.float32)):      # as float32 too: what the device form hands back
        assert np.abs(np.linalg.norm(centres.astype(np.float64), axis=-1) - 1.0).max() <= 1e-7
        ti, pi = utility.theta_phi_index_for_onehot(centres.reshape(1, 1, 648, 3))
        np.testing.assert_array_equal(ti.reshape(-1), index // 18)
        np.testing.assert_array_equal(pi.reshape(-1), index % 18)
    assert utility.bin_centre_xyz(np.arange(648).reshape(4, 162)).shape == (4, 162, 3)
    for bad in (-1, 648):
        with pytest.raises(ValueError):
            utility.bin_centre_xyz(np.array([0, bad]))


def test_decode_argument_errors_come_before_device_work():
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    m = ConvLSTMSeq2Seq(O.init_convlstm_seq2seq(3, C=30, latent_dim=8, k=3, head="conv2d", head_filters=(16, 16)))
    xyz = np.zeros((1, 2, 30, 3), np.float32)
    with pytest.raises(ValueError, match="output"):
        m.predict_trajectories(xyz, xyz[:, -1:], output="bogus")
    d = ConvLSTMSeq2Seq(O.init_convlstm_seq2seq(3, C=6, latent_dim=8, k=3, head="dense", map_hw=(1, 1)), head="dense")
    x = np.zeros((1, 2, 1, 1, 6), np.float32)
    with pytest.raises(ValueError, match="dense"):
        d.predict_index([x, x[:, -1:]])
    with pytest.raises(ValueError, match="dense"):
        d.predict_index_device(x, x[:, -1:])
    with pytest.raises(ValueError):
        d.predict_trajectories(xyz, xyz[:, -1:], output="index")
    with pytest.raises(ValueError):
        d.evaluate_trajectories(xyz, xyz[:, -1:], xyz)
