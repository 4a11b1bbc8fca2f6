"""fov_stacked_seq2seq_decode_supported without a GPU: the rule is arithmetic (run width 32 or 64, 2 or 3 layers, F_enc <= 96,
F_dec <= 8, any non-negative batch and lengths) plus the FOV_NO_STACKED_DECODE knob; the _fwd entry refuses every other shape
before its first HIP call, so that runs here too.  tests/test_abi.py holds the prototypes against the ctypes table."""
import ctypes
import itertools
import os

import pytest

from longterm360fov_amd import _lib


def _supported(B, T_in, T_out, F_enc, F_dec, H, L):
    return _lib.lib().fov_stacked_seq2seq_decode_supported(B, T_in, T_out, F_enc, F_dec, H, L)


def test_supported_corners():
    for H, L, F_enc, B in itertools.product((32, 64), (2, 3), (1, 96), (0, 1, 100000)):
        assert _supported(B, 10, 10, F_enc, 6, H, L) == 1, (H, L, F_enc, B)
    for T_in, T_out, F_dec in ((0, 10, 1), (10, 0, 8), (0, 0, 6), (64, 64, 6)):
        assert _supported(64, T_in, T_out, 6, F_dec, 32, 2) == 1, (T_in, T_out, F_dec)


@pytest.mark.parametrize("B,T_in,T_out,F_enc,F_dec,H,L", [
    (5, 2, 2, 6, 6, 128, 2),     # wider than one workgroup's tile
    (5, 2, 2, 6, 6, 32, 1), (5, 2, 2, 6, 6, 32, 4),
    (5, 2, 2, 6, 9, 32, 2), (5, 2, 2, 97, 6, 64, 2),
    (5, 2, 2, 6, 6, 48, 2), (5, 2, 2, 6, 6, 16, 3),     # widths the caller has to pad
    (5, 2, 2, 0, 6, 32, 2), (5, 2, 2, 6, 0, 32, 2),
    (-1, 2, 2, 6, 6, 32, 2), (5, -1, 2, 6, 6, 32, 2), (5, 2, -1, 6, 6, 32, 2)])
def test_unsupported_shapes(B, T_in, T_out, F_enc, F_dec, H, L):
    L_ = _lib.lib()
    assert _supported(B, T_in, T_out, F_enc, F_dec, H, L) == 0
    # refused before any HIP call and before any pointer is looked at
    rc = L_.fov_stacked_seq2seq_decode_fwd(*([None] * 25), B, T_in, T_out, F_enc, F_dec, H, L, _lib.ACT_SIGMOID, None)
    assert rc == _lib.ERR_UNSUPPORTED
    msg = L_.fov_last_error().decode()
    assert "fov_stacked_seq2seq_decode_fwd" in msg and "H=%d" % H in msg and "L=%d" % L in msg


def test_missing_pointers_are_invalid_arguments_and_an_empty_batch_is_a_no_op():
    L_ = _lib.lib()
    assert L_.fov_stacked_seq2seq_decode_fwd(*([None] * 25), 4, 2, 2, 6, 6, 32, 2, _lib.ACT_SIGMOID, None) == _lib.ERR_INVALID
    some = ctypes.c_void_p(0x1000)      # never dereferenced: B = 0 returns before a launch
    ptrs = [None, None] + [some] * 6 + [None] * 3 + [some] * 6 + [None] * 3 + [some, some] + [None] * 3
    assert L_.fov_stacked_seq2seq_decode_fwd(*ptrs, 0, 2, 2, 6, 6, 32, 2, _lib.ACT_SIGMOID, None) == _lib.OK
    assert L_.fov_stacked_seq2seq_decode_fwd(*ptrs, 0, 2, 2, 6, 6, 32, 3, _lib.ACT_SIGMOID, None) == _lib.ERR_INVALID   # layer 3 missing
    assert L_.fov_stacked_seq2seq_decode_fwd(*ptrs, 0, 2, 2, 6, 6, 32, 2, 5, None) == _lib.ERR_INVALID                # no such activation


def test_knob_flips_supported():
    L_ = _lib.lib()
    assert "FOV_NO_STACKED_DECODE" not in os.environ
    assert _supported(64, 10, 10, 6, 6, 32, 2) == 1
    os.environ["FOV_NO_STACKED_DECODE"] = "1"
    try:
        L_.fov_reload_env()
        assert _supported(64, 10, 10, 6, 6, 32, 2) == 0 and _supported(1024, 30, 30, 90, 6, 64, 3) == 0
    finally:
        del os.environ["FOV_NO_STACKED_DECODE"]
        L_.fov_reload_env()
    assert _supported(64, 10, 10, 6, 6, 32, 2) == 1
