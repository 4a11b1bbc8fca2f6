#!/usr/bin/env python3
"""Generate tests/golden/onehot.npz: golden vectors of the ConvLSTM heat-map inputs, from the reference itself.

Runs ONLY in the authoring container (needs the reference checkout); the test-suite and the GPU box only read the .npz.
Nothing from the reference is copied: its modules are imported in place, with the same placeholder modules for
TensorFlow / Keras / h5py as make_data_fixtures.py, and called on seeded inputs.

What is pinned (reference file:line):
  * mycode/dataIO.py:77-82     xyz2thetaphi, called in place on the frame centres widened to float64
  * mycode/utility.py:536-542  theta / phi bin indices.  These lines sit inside _save_theta_phi_index's nested function,
    which reads undefined globals and calls xyz2thetaphi without importing it, so it cannot be called: the five lines are
    restated inline below (BIN_EDGES_536_542).
  * mycode/utility.py:557-571  _create_one_hot, called in place.  It sizes its array with `360/bin_size` (Python 2 integer
    division); bin_size is passed as an int subclass whose reflected division floors, so the call runs unchanged under
    Python 3.

Inputs (float32 frame centres, (N, T, 30, 3)): random unit vectors; the six axis directions, both poles among them;
y = +0.0 and -0.0 with x < 0; the zero vector; points 1 and 2 float32 ULPs either side of every theta and phi bin edge.
Stored: xyz, the reference's fp64 theta / phi, the bin indices (int32; the reference keeps them as integral float64) and the
maps as uint8 in the reference's (N, T, 30, 36, 18) layout.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_data_fixtures import REF, install_placeholders  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "onehot.npz")
N, T, F = 8, 10, 30


class Py2Int(int):
    """An int whose reflected true division floors: `360/bin_size` as Python 2 evaluated it."""

    def __rtruediv__(self, other):
        return int(other) // int(self)


def bin_indices_536_542(theta_list, phi_list, bin_size):
    # mycode/utility.py:536-542, restated (see the module docstring)
    theta_list2 = theta_list + np.pi
    theta_index = np.floor(theta_list2 / np.pi * 180 / bin_size)
    theta_index[theta_index == 360 / bin_size] -= 1
    phi_index = np.floor(phi_list / np.pi * 180 / bin_size)
    phi_index[phi_index == 180 / bin_size] -= 1
    return theta_index, phi_index


def _nudged(v, axis, steps=(-2, -1, 1, 2)):
    """v (3,) float32 and its copies with component `axis` moved by each number of float32 ULPs in `steps`."""
    out = [v.copy()]
    for s in steps:
        w = v.copy()
        for _ in range(abs(s)):
            w[axis] = np.nextafter(w[axis], np.float32(np.inf if s > 0 else -np.inf))
        out.append(w)
    return out


def frame_centres(rng):
    special = []
    # the six axis directions (both poles), y = +-0.0 with x < 0, the zero vector
    for v in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [-1, 0.0, 0], [-1, -0.0, 0],
              [-0.6, -0.0, 0.8], [-0.6, 0.0, -0.8], [-0.0, -0.0, 1], [0, 0, 0], [-0.0, -0.0, -0.0]):
        special.append(np.array(v, np.float32))
    # theta edges: azimuth k * 10 degrees (atan2 space), nudged in y and in x
    for k in range(36):
        a = np.deg2rad(10.0 * k)
        v = np.array([np.cos(a), np.sin(a), rng.uniform(-0.3, 0.3)], np.float32)
        special += _nudged(v, 1) + _nudged(v, 0)[1:]
    # phi edges: elevation k * 10 - 90 degrees at a random azimuth, nudged in z
    for k in range(19):
        e = np.deg2rad(10.0 * k - 90.0)
        a = rng.uniform(-np.pi, np.pi)
        v = np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], np.float32)
        special += _nudged(v, 2)
    special = np.stack(special)
    n_rand = N * T * F - len(special)
    assert n_rand > 0
    r = rng.standard_normal((n_rand, 3))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    allv = np.concatenate([special, r.astype(np.float32)])
    allv = allv[rng.permutation(len(allv))]            # spread the special frames over sequences and seconds
    return allv.reshape(N, T, F, 3)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference not present; fixtures can only be regenerated in the authoring container")
    install_placeholders()
    sys.path.insert(0, REF)
    from mycode import dataIO
    from mycode import utility as util

    rng = np.random.default_rng(2024)
    xyz = frame_centres(rng)
    x, y, z = (xyz[..., a].astype(np.float64) for a in range(3))
    theta, phi = dataIO.xyz2thetaphi(x, y, z)
    bin_size = Py2Int(10)
    ti, pi = bin_indices_536_542(theta, phi, bin_size)
    maps = util._create_one_hot(ti, pi, bin_size=bin_size)
    assert maps.shape == (N, T, F, 36, 18) and (maps.sum(axis=(3, 4)) == 1).all()
    out = {"xyz": xyz, "theta": theta, "phi": phi, "theta_index": ti.astype(np.int32), "phi_index": pi.astype(np.int32),
           "maps": maps.astype(np.uint8)}
    assert (out["theta_index"] == ti).all() and (out["phi_index"] == pi).all()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
