"""The bytes every forward workspace-size function and the two of a layer's backward answer, pinned for a grid that holds every
edge of every dispatch predicate.

ops.Workspace grows on these numbers, so a change reallocates in user code; and the launch side checks its workspace against
the same plan that the size functions answer from, so a size that moves means a kernel choice that moved.  The size functions
are arithmetic only: without a device the library counts 256 CUs and FOV_DBG_RESIDENT_LIMIT lowers that, so the table holds on
any machine.  fov_lstm_seq_bwd_workspace_bytes and fov_lstm_stack2_bwd_workspace_bytes answer from the carve that lstm_seq_bwd
and lstm_stack2_bwd cut their workspace by (lstm_train.hip).

The expected values are a recording, never a computation of the library under test:

    FOV_LIB_PATH=<libfov360_hip.so of the commit to pin> python tests/test_dispatch_host.py --record

writes dispatch_sizes.json beside this file (per function and environment the answers in grid order, run-length coded over the
list of distinct values).  Equality is exact.  The table here was recorded from the library of the commit before the backward
plan; the answers of the functions it already held came out as they were recorded on an MI355X before the forward plan."""
import contextlib
import itertools
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from longterm360fov_amd import _lib  # noqa: E402

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dispatch_sizes.json")

BS = (0, 1, 16, 128, 129, 512, 513)
TS = (0, 1, 50)
FS = (1, 96, 97, 100, 128, 256, 512)
FDECS = (1, 8, 9)
HS = (32, 64, 128, 256, 512, 1024)
IMPLS = (_lib.IMPL_AUTO, _lib.IMPL_GENERIC, _lib.IMPL_CLUSTER)
T_PAIRS = ((0, 0), (1, 1), (50, 50), (0, 50), (50, 1))      # (T_in, T_out): each length at each of its values, equal and unequal
ENVS = {"default": {}, "no_wide16": {"FOV_NO_WIDE16": "1"}, "resident8": {"FOV_DBG_RESIDENT_LIMIT": "8"},
        "resident3": {"FOV_DBG_RESIDENT_LIMIT": "3"}}

# function -> its argument tuples in a fixed order (the slowest-moving argument first)
GRIDS = {
    "fov_lstm_seq_workspace_bytes": [(B, T, F, H, impl) for impl, H, B, T, F in itertools.product(IMPLS, HS, BS, TS, FS)],
    "fov_seq2seq_decode_workspace_bytes": [(B, T_in, T_out, F, Fd, H, impl)
                                           for impl, H, B, (T_in, T_out), Fd, F in itertools.product(IMPLS, HS, BS, T_PAIRS[:2], FDECS, FS)],
    "fov_seq2seq_tf_workspace_bytes": [(B, T_in, T_out, F, Fd, H, impl)
                                       for impl, H, B, (T_in, T_out), Fd, F in itertools.product(IMPLS, HS, BS, T_PAIRS, FDECS, FS)],
    "fov_lstm_seq_bwd_workspace_bytes": [(B, T, F, H) for H, B, T, F in itertools.product(HS, BS, TS, FS)],
    "fov_lstm_stack2_bwd_workspace_bytes": [(B, T, F, H) for H, B, T, F in itertools.product(HS, BS, TS, FS)],
}


@contextlib.contextmanager
def environment(env):
    """The library caches its knobs: re-read them under `env`, and again once the caller's environment is back."""
    before = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    _lib.lib().fov_reload_env()
    try:
        yield
    finally:
        for k, v in before.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        _lib.lib().fov_reload_env()


def sweep(name):
    fn = getattr(_lib.lib(), name)
    return [int(fn(*args)) for args in GRIDS[name]]


def encode(answers, values):
    """[v, v, w, ...] -> [index of v, run length, index of w, run length, ...]"""
    index = {v: i for i, v in enumerate(values)}
    runs = []
    for v, group in itertools.groupby(answers):
        runs += [index[v], len(list(group))]
    return runs


def decode(runs, values):
    return [values[i] for i, n in zip(runs[0::2], runs[1::2]) for _ in range(n)]


def record():
    answers = {}
    for env_name, env in ENVS.items():
        with environment(env):
            for name in GRIDS:
                answers[name, env_name] = sweep(name)
    values = sorted(set(v for a in answers.values() for v in a))
    table = {"values": values, "runs": {name: {env_name: encode(answers[name, env_name], values) for env_name in ENVS} for name in GRIDS}}
    with open(TABLE, "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d answers, %d distinct, %d bytes" % (TABLE, sum(map(len, answers.values())), len(values), os.path.getsize(TABLE)))


@pytest.fixture(scope="module")
def table():
    assert os.path.getsize(TABLE) < 64 * 1024
    with open(TABLE) as f:
        return json.load(f)


def test_the_grid_holds_every_edge_the_predicates_have():
    """The edges are part of the check: B at the wide16 (128) and narrow-wide (512) limits and one past each, F at the narrow
    (96), vector (a multiple of four: 97 against 100) and F = H limits, F_dec at the head's eight, every width with a kernel of
    its own and one above and below them, every impl."""
    assert {0, 1, 16, 128, 129, 512, 513} <= set(BS) and {0, 1, 50} <= set(TS) and {1, 96, 97, 100, 128, 256, 512} <= set(FS)
    assert {1, 8, 9} <= set(FDECS) and {32, 64, 128, 256, 512, 1024} <= set(HS) and len(set(IMPLS)) == 3
    for name, grid in GRIDS.items():
        assert len(set(grid)) == len(grid), name


@pytest.mark.parametrize("env_name", list(ENVS))
@pytest.mark.parametrize("name", list(GRIDS))
def test_workspace_bytes_are_the_recorded_ones(table, name, env_name):
    want = decode(table["runs"][name][env_name], table["values"])
    assert len(want) == len(GRIDS[name])
    with environment(ENVS[env_name]):
        got = sweep(name)
    wrong = [(args, g, w) for args, g, w in zip(GRIDS[name], got, want) if g != w]
    assert not wrong, "%s under %s: %d of %d answers moved, first (arguments, now, recorded): %s" % (
        name, env_name, len(wrong), len(got), wrong[:5])


def test_the_environments_change_answers(table):
    """A sweep that never reached the library's knobs would pin four copies of one table."""
    runs = table["runs"]["fov_lstm_seq_workspace_bytes"]
    assert runs["no_wide16"] != runs["default"] and runs["resident8"] != runs["default"] and runs["resident3"] != runs["resident8"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: FOV_LIB_PATH=<library to pin> python tests/test_dispatch_host.py --record")
    record()
