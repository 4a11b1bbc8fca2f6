"""The host-array pipeline (longterm360fov_amd/hostpipe.py) on a machine without a GPU: the ring runs on NumpyBackend
(plain arrays, copies done where they are queued, every operation logged), so the chunk plan, the narrowing, the budget,
the switches and the error path are those of the GPU run; only the streams are missing."""
import os
import re

import numpy as np
import pytest

from longterm360fov_amd import hostpipe, ops
from longterm360fov_amd.models import KerasModelSurface, _as_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class HostModel(KerasModelSurface):
    """The model surface with its ring on NumpyBackend; run() sees NumPy 'device' inputs."""

    def __init__(self):
        self._w = {}
        self._init_surface((), None, "cpu")
        self.backends = []

    def _pipe_backend(self):
        self.backends.append(hostpipe.NumpyBackend())
        return self.backends[-1]

    def _to_device(self, a):      # the serial loop's upload: a CPU tensor, which has the .cpu().numpy() that loop ends in
        import torch
        return torch.from_numpy(_as_f32(a).copy())


def serial(arrays, batch_size, run):
    """What _predict_chunks returns, written out: run on float32 chunks, concatenated."""
    n = arrays[0].shape[0]
    bs = n if not batch_size else batch_size
    outs = [run(*[_as_f32(a[lo:lo + bs]) for a in arrays]) for lo in range(0, n, max(bs, 1))]
    return np.concatenate(outs, axis=0) if outs else np.zeros((0, 2), np.float32)


def rows(n, seed=0):
    return np.random.default_rng(seed).standard_normal((n, 3)) + np.arange(n)[:, None]      # every row distinct


def twice(x):
    return x[:, :2] * 2 + 1


@pytest.mark.parametrize("n,batch,chunks", [(0, 4, 0), (1, 4, 1), (4, 4, 1), (5, 4, 2), (29, 4, 8), (7, None, 1), (7, 0, 1)])
def test_chunk_plan_is_the_serial_loops(n, batch, chunks):
    plan = hostpipe.chunk_plan(n, batch)
    bs = n if not batch else batch
    assert plan == [(lo, min(lo + bs, n)) for lo in range(0, n, max(bs, 1))]
    assert len(plan) == chunks
    if n == 29:
        assert plan[-1] == (28, 29)


@pytest.mark.parametrize("n", [0, 1, 4, 5, 29])
def test_pipelined_predict_equals_the_serial_loop(n):
    m = HostModel()
    m.host_pipeline = True
    x = rows(n)
    got = m._predict_chunks([x], 4, twice, (2,))
    want = serial([x], 4, twice)
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    if n > 4:      # two chunks or more went through the ring: three slots, one host wait per chunk
        (b,) = m.backends
        ring = m._pipe_rings["predict"][1]
        assert ring.S == 3
        waits = sum(1 for what, _ in b.log if what == "host_wait")
        assert waits == len(hostpipe.chunk_plan(n, 4))
        assert not m._pipe_lock.locked()
    else:          # one chunk, or none: the serial loop
        assert m.backends == []


def test_29_rows_at_batch_4_wrap_three_slots_twice_in_order():
    m = HostModel()
    m.host_pipeline = True
    x = rows(29)
    seen = []

    def run(xd):
        seen.append(xd.copy())
        return twice(xd)
    got = m._predict_chunks([x], 4, run, (2,))
    np.testing.assert_array_equal(got, serial([x], 4, twice))
    assert [len(s) for s in seen] == [4] * 7 + [1]
    np.testing.assert_array_equal(np.concatenate(seen), _as_f32(x))
    # a second call of the same shapes reuses the ring; other shapes replace it
    m._predict_chunks([x], 4, twice, (2,))
    assert len(m.backends) == 1
    m._predict_chunks([x], 5, twice, (2,))
    assert len(m.backends) == 2 and len(m._pipe_rings) == 1


def test_several_outputs_none_and_two_host_inputs():
    m = HostModel()
    m.host_pipeline = True
    a, b = rows(9, 1), rows(9, 2).astype(np.float32)

    def run(x, nothing, y):
        assert nothing is None
        return x + y, (x - y)[:, :1]
    got = m._predict_chunks([a, None, b], 2, run, [(3,), (1,)])
    assert isinstance(got, list) and len(got) == 2
    np.testing.assert_array_equal(got[0], _as_f32(a) + b)
    np.testing.assert_array_equal(got[1], (_as_f32(a) - b)[:, :1])


def rounding_values():
    tiny = np.float64(np.finfo(np.float32).tiny)
    return np.array([2.0 ** 24 + 1, 2.0 ** 24 + 3, 1e40, -1e40, tiny / 3, -tiny / 7, 1e-46, 5e-324, 0.0, -0.0, np.nan, np.inf, -np.inf,
                     0.1, 1 + 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50, 3.4028235677973366e38], np.float64)


def narrowing_cases():
    v = rounding_values()
    base = np.random.default_rng(3).standard_normal((6, 5, 4)) * 1e3
    big = np.random.default_rng(4).standard_normal((64, 300, 90))      # 13.8 MB: split over the threads
    return {
        "rounding": np.tile(v, (3, 1)),
        "float16": base.astype(np.float16),
        "int32": (base * 1e5).astype(np.int32),
        "int64_past_2^24": np.array([[2 ** 24 + 1, -(2 ** 53) - 1, 2 ** 62]], np.int64),
        "bool": base > 0,
        "every_other_row": base[::2],
        "transposed": base.transpose(2, 0, 1),
        "fortran": np.asfortranarray(base),
        "reversed": base[::-1],
        "reversed_inner": base[:, ::-1, ::-2],
        "threads": big,
        "threads_strided": big[::-1, ::2],
        "float32": base.astype(np.float32),
    }


@pytest.mark.parametrize("name", sorted(narrowing_cases()))
def test_narrowing_equals_as_f32_bit_for_bit(name):
    src = narrowing_cases()[name]
    with np.errstate(over="ignore", invalid="ignore"):
        want = _as_f32(src)
    dst = np.full(src.shape, 7, np.float32)
    hostpipe.narrow(dst, src)
    assert dst.tobytes() == want.tobytes()
    if name == "rounding":
        assert np.isinf(want[0, 2]) and want[0, 0] == 2.0 ** 24 and np.signbit(want[0, 9]) and np.isnan(want[0, 10])


def test_narrowing_threads_are_capped():
    assert hostpipe.MAX_THREADS == 16
    hostpipe.narrow(np.empty((64, 300, 90), np.float32), np.zeros((64, 300, 90)))
    assert hostpipe._threads()._max_workers == 16
    assert "cpu_count" not in open(hostpipe.__file__).read()


def test_gather_equals_the_fancy_index():
    a = np.random.default_rng(5).standard_normal((11, 3, 2)).astype(np.float32)
    idx = np.random.default_rng(6).permutation(11)[:4]
    dst = np.empty((4, 3, 2), np.float32)
    hostpipe.gather(dst, a, idx)
    np.testing.assert_array_equal(dst, a[idx])
    hostpipe.gather(dst[:3], a, slice(8, 11))
    np.testing.assert_array_equal(dst[:3], a[8:11])


def test_budget_three_slots_then_two_then_the_serial_loop(monkeypatch):
    per = hostpipe.slot_bytes([(3,)], [(2,)], 4)
    assert per == 4 * (4 * 3 + 8 * 2)      # float32 inputs; a result is budgeted at 8 bytes an element
    assert hostpipe.slots_for(per, 3 * per) == 3
    assert hostpipe.slots_for(per, 3 * per - 1) == 2
    assert hostpipe.slots_for(per, 2 * per) == 2
    assert hostpipe.slots_for(per, 2 * per - 1) == 0
    monkeypatch.delenv("FOV_HOST_PIPELINE_BYTES", raising=False)
    assert hostpipe.budget_bytes() == 1 << 30
    x = rows(29)
    for budget, slots in ((3 * per, 3), (3 * per - 1, 2), (2 * per - 1, 0)):
        monkeypatch.setenv("FOV_HOST_PIPELINE_BYTES", str(budget))
        m = HostModel()
        m.host_pipeline = True
        np.testing.assert_array_equal(m._predict_chunks([x], 4, twice, (2,)), serial([x], 4, twice))
        ring = m._pipe_rings["predict"][1]
        if slots:
            assert ring.S == slots and m.backends[0].bytes <= budget
        else:
            assert ring is None and m.backends == []
        assert not m._pipe_lock.locked()


def test_the_attribute_wins_over_the_environment(monkeypatch):
    monkeypatch.delenv("FOV_HOST_PIPELINE", raising=False)
    assert hostpipe.enabled(None) is hostpipe.DEFAULT_ON
    assert hostpipe.enabled(True) is True and hostpipe.enabled(False) is False
    for env, on in (("1", True), ("0", False)):
        monkeypatch.setenv("FOV_HOST_PIPELINE", env)
        assert hostpipe.enabled(None) is on
        assert hostpipe.enabled(True) is True and hostpipe.enabled(False) is False
        m = HostModel()
        assert m.host_pipeline is None and m._pipelined() is on
        m.host_pipeline = not on
        m._predict_chunks([rows(9)], 2, twice, (2,))
        assert bool(m.backends) is (not on)


def test_with_the_pipeline_off_inputs_are_narrowed_up_front(monkeypatch):
    monkeypatch.delenv("FOV_HOST_PIPELINE", raising=False)
    m = HostModel()
    x = rows(5)
    m.host_pipeline = False
    assert m._host_in(x).dtype == np.float32
    m.host_pipeline = True
    assert m._host_in(x) is x and m._host_in(x[::2]).dtype == np.float64
    assert m._host_in([[1, 2], [3, 4]]).dtype == np.float32 and m._host_in(3).dtype == np.float32      # lists, scalars: as ever


def test_the_new_knobs_are_documented_and_not_among_the_librarys():
    doc = open(os.path.join(ROOT, "KNOBS.md")).read()
    for knob in ("FOV_HOST_PIPELINE", "FOV_HOST_PIPELINE_BYTES"):
        assert re.search(r"`%s(=[^`]*)?`" % knob, doc), knob
        assert knob not in ops._ENV_KNOBS
    assert doc.index("FOV_FIT_RESIDENT_BYTES") < doc.index("FOV_HOST_PIPELINE") < doc.index("FOV_FIT_RESIDENT_BYTES") + 2000


def test_an_exception_from_run_propagates_and_the_next_call_is_complete():
    m = HostModel()
    m.host_pipeline = True
    x = rows(23)      # 6 chunks of 4
    calls = []

    def failing(xd):
        calls.append(len(xd))
        if len(calls) == 4:      # chunk 3 of 6
            raise KeyError("chunk 3")
        return twice(xd)
    with pytest.raises(KeyError, match="chunk 3"):
        m._predict_chunks([x], 4, failing, (2,))
    assert len(calls) == 4
    assert m.backends[0].log[-1] == ("drain", None)      # the streams were waited for
    assert "predict" not in m._pipe_rings and not m._pipe_lock.locked()      # the ring is gone, the lock free
    np.testing.assert_array_equal(m._predict_chunks([x], 4, twice, (2,)), serial([x], 4, twice))
    assert len(m.backends) == 2


def test_a_second_thread_on_the_same_model_takes_the_serial_loop():
    m = HostModel()
    m.host_pipeline = True
    x = rows(9)
    inner = []

    def run(xd):
        if not inner:      # while the first call holds the ring, a call from "another thread" finds the lock taken
            inner.append(None)
            inner[0] = m._predict_chunks([x], 2, twice, (2,))
        return twice(xd)
    outer = m._predict_chunks([x], 2, run, (2,))
    np.testing.assert_array_equal(outer, serial([x], 2, twice))
    np.testing.assert_array_equal(inner[0], outer)
    assert len(m.backends) == 1


def test_a_wrong_result_shape_is_an_error_not_a_wrong_row():
    m = HostModel()
    m.host_pipeline = True
    with pytest.raises(ValueError, match="rows returned"):
        m._predict_chunks([rows(9)], 2, lambda xd: twice(xd)[:1], (2,))
    assert not m._pipe_lock.locked()


def test_uploader_keeps_the_slot_rules():
    """No download: the pinned inputs wait for the slot's previous upload (host), the device inputs for its previous
    reader (upload stream), and a batch staged ahead never lands in the slot that is being read."""
    b = hostpipe.NumpyBackend()
    ring = hostpipe.make_ring(lambda: b, [(3,)], [], 4, 1 << 20)
    assert ring.S == 3
    up = hostpipe.Uploader(ring)
    data = _as_f32(rows(24))
    fill = lambda k: (lambda views: hostpipe.narrow(views[0], data[4 * k:4 * k + 4]))
    for k in range(6):
        dev = up.next(fill(k), 4)
        if k < 5:
            up.ahead(fill(k + 1), 4)
        np.testing.assert_array_equal(dev[0], data[4 * k:4 * k + 4])      # staging k + 1 did not touch batch k
    ring.finish()
    assert ring.held is None
    assert sum(1 for what, _ in b.log if what == "host_wait") == 3      # batches 3, 4, 5 reuse a slot
    assert sum(1 for what, s in b.log if what == "wait" and s == "up") == 3
    assert sum(1 for what, s in b.log if what == "record" and s == "compute") == 6
