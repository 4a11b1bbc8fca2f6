"""CPU checks of the ConvLSTM heat-map input helpers: utility.theta_phi_index_for_onehot / create_one_hot against
tests/golden/onehot.npz (produced by the reference's xyz2thetaphi and _create_one_hot, tests/golden/make_onehot_fixtures.py)."""
import os

import numpy as np
import pytest

from longterm360fov_amd import utility

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "onehot.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_theta_phi_index_matches_reference(gold):
    ti, pi = utility.theta_phi_index_for_onehot(gold["xyz"])
    assert ti.dtype == np.float64 and ti.shape == gold["theta_index"].shape
    np.testing.assert_array_equal(ti, gold["theta_index"])
    np.testing.assert_array_equal(pi, gold["phi_index"])
    # the (N, T, 1, 30, 3) form of reshape2second_stacks' output
    ti5, pi5 = utility.theta_phi_index_for_onehot(gold["xyz"][:, :, None])
    np.testing.assert_array_equal(ti5, gold["theta_index"])
    np.testing.assert_array_equal(pi5, gold["phi_index"])


def test_reference_quirks_pinned(gold):
    """Both poles map to phi = 0; +0 vector -> (0, 9); y = +-0.0 with x < 0 -> theta bin 18."""
    v = np.array([[[[0, 0, 1], [0, 0, -1], [0, 0, 0], [-1, 0.0, 0], [-1, -0.0, 0]] + [[1, 0, 0]] * 25]], np.float32)
    ti, pi = utility.theta_phi_index_for_onehot(v)
    assert list(pi[0, 0, :3]) == [0, 0, 9]
    assert list(ti[0, 0, 2:5]) == [0, 18, 18]


def test_create_one_hot_matches_reference(gold):
    maps = utility.create_one_hot(gold["theta_index"], gold["phi_index"])
    assert maps.shape == gold["maps"].shape and maps.dtype == np.float64
    np.testing.assert_array_equal(maps, gold["maps"])
    # indices as the reference keeps them (integral float64)
    maps_f = utility.create_one_hot(gold["theta_index"].astype(np.float64), gold["phi_index"].astype(np.float64))
    np.testing.assert_array_equal(maps_f, gold["maps"])
    vec = utility.create_one_hot(gold["theta_index"], gold["phi_index"], vector=True)
    np.testing.assert_array_equal(vec, gold["maps"].reshape(vec.shape))
    assert vec.shape[-1] == 36 * 18


def test_create_one_hot_rejects_bad_indices(gold):
    ti, pi = gold["theta_index"].astype(np.float64), gold["phi_index"].astype(np.float64)
    bad = ti.copy()
    bad[0, 0, 0] = np.nan
    with pytest.raises(ValueError):
        utility.create_one_hot(bad, pi)
    bad = ti.copy()
    bad[1, 2, 3] = -1        # NumPy would wrap this to the last row silently
    with pytest.raises(ValueError):
        utility.create_one_hot(bad, pi)
    bad = pi.copy()
    bad[0, 0, 0] = 18
    with pytest.raises(ValueError):
        utility.create_one_hot(ti, bad)
