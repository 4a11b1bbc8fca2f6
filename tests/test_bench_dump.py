"""bench.py --dump-outputs: what the timed path returned in its last step, as .npy files under a size cap."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("fov_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float_arrays_and_samples_rows_past_the_cap(tmp_path):
    bench = _bench_module()
    small = np.arange(12, dtype=np.float64).reshape(3, 4)
    big = np.random.default_rng(5).standard_normal((1000, 6)).astype(np.float32)
    bench.dump_outputs(str(tmp_path / "a"), {"small": small, "ints": np.arange(4, dtype=np.int32)})
    assert np.array_equal(np.load(str(tmp_path / "a" / "small.npy")), small)
    ints = np.load(str(tmp_path / "a" / "ints.npy"))
    assert ints.dtype == np.float32 and np.array_equal(ints, np.arange(4))

    limit = 8000
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"big": big}, limit=limit)
    got = np.load(str(tmp_path / "b" / "big.npy"))
    rows = np.load(str(tmp_path / "b" / "big.rows.npy"))
    assert got.nbytes + rows.nbytes <= limit and 0 < got.shape[0] < big.shape[0]
    assert rows.dtype == np.float64 and (np.diff(rows) > 0).all()
    assert np.array_equal(got, big[rows.astype(np.int64)])
    assert np.array_equal(got, np.load(str(tmp_path / "c" / "big.npy")))      # the sample is fixed


def test_dump_outputs_is_refused_where_it_is_not_implemented():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--mode", "convlstm", "--dump-outputs", "x"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    """The headline run with --steps 3: three timed steps, and the dumped output is the fused call's result on the seeded
    inputs (first 16 sequences against the C oracle).  Without --full the line carries nothing that takes work of its own."""
    sys.path.insert(0, ROOT)
    from oracle import c_oracle as C
    from oracle import fov_oracle as O
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", d], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert res["steps"] == 3
    assert not {"kernels", "parity", "large_batch", "cpu_baseline", "extra"} & set(res), sorted(res)
    out = np.load(os.path.join(d, "seq2seq_decode.npy"))
    assert out.shape == (1024, 30, 6) and out.dtype == np.float32
    w = O.init_seq2seq(1234, 90, 6, 256, bias_noise=0.05)
    enc, dec0, _ = O.synthetic_batch(1234, 1024, 30, 30)
    ref = C.seq2seq_decode(enc[:16], dec0[:16], w, 30, 0)
    assert np.abs(out[:16] - ref).max() <= 1e-3 * np.abs(ref).max() + 1e-5
