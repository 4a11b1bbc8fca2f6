"""fov_selffed_decoder_supported without a GPU: the rule is arithmetic (H = 32 or 64, 1 <= O <= 8, any non-negative batch and
length) plus the FOV_NO_SELFFED_FUSED knob; fov_selffed_decoder_fwd / _bwd refuse every other shape before their first HIP call,
so that runs here too.  tests/test_abi.py holds the prototypes against the ctypes table."""
import ctypes
import itertools
import os

import pytest

from longterm360fov_amd import _lib

N_FWD_PTRS, N_BWD_PTRS = 15, 14


def _supported(B, T, O, H):
    return _lib.lib().fov_selffed_decoder_supported(B, T, O, H)


def _fwd(ptrs, B, T, O, H, act=_lib.ACT_SIGMOID, dact=1):
    return _lib.lib().fov_selffed_decoder_fwd(*ptrs, B, T, O, H, act, dact, None)


def _bwd(ptrs, B, T, O, H, act=_lib.ACT_SIGMOID, dact=1, a_from_A=0):
    return _lib.lib().fov_selffed_decoder_bwd(*ptrs, B, T, O, H, act, dact, a_from_A, None)


def test_supported_truth_table():
    for H, O, B, T in itertools.product((32, 64), (1, 3, 6, 8), (0, 1, 17, 100000), (0, 1, 30, 64)):
        assert _supported(B, T, O, H) == 1, (B, T, O, H)
    for H in (0, 16, 48, 128, 256, -64):
        assert _supported(32, 10, 6, H) == 0, H
    for O in (0, 9, 90, -1):
        assert _supported(32, 10, O, 64) == 0, O
    assert _supported(-1, 10, 6, 64) == 0 and _supported(32, -1, 6, 64) == 0


@pytest.mark.parametrize("B,T,O,H", [(5, 2, 6, 16), (5, 2, 6, 48), (5, 2, 6, 128), (5, 2, 0, 64), (5, 2, 9, 32),
                                     (-1, 2, 6, 64), (5, -1, 6, 32)])
def test_unsupported_shapes_are_refused_before_any_pointer_is_looked_at(B, T, O, H):
    assert _supported(B, T, O, H) == 0
    for name, call, n in (("fov_selffed_decoder_fwd", _fwd, N_FWD_PTRS), ("fov_selffed_decoder_bwd", _bwd, N_BWD_PTRS)):
        assert call([None] * n, B, T, O, H) == _lib.ERR_UNSUPPORTED
        msg = _lib.lib().fov_last_error().decode()
        assert name in msg and "H=%d" % H in msg and "O=%d" % O in msg, msg


def test_missing_pointers_and_unknown_activations_are_invalid_and_an_empty_batch_is_a_no_op():
    some = ctypes.c_void_p(0x1000)      # never dereferenced: B = 0 and T = 0 return before a launch
    assert _fwd([None] * N_FWD_PTRS, 4, 2, 6, 64) == _lib.ERR_INVALID
    assert _bwd([None] * N_BWD_PTRS, 4, 2, 6, 64) == _lib.ERR_INVALID
    # x0, h0, c0 | K, R, b, W, bd | r | Hs, Cs, XA, A, RES, y
    fwd = [some, None, None] + [some] * 5 + [None] * 7
    assert _fwd(fwd, 0, 3, 6, 64) == _lib.OK and _fwd(fwd, 0, 3, 1, 32, _lib.ACT_HARD_SIGMOID, 2) == _lib.OK
    assert _fwd(fwd, 5, 0, 6, 64) == _lib.OK                      # no step: nothing is written
    assert _fwd(fwd, 0, 3, 6, 64, 5, 1) == _lib.ERR_INVALID       # no such recurrent activation
    for dact in (0, 3, 4):                                        # the head is tanh (1) or relu (2)
        assert _fwd(fwd, 0, 3, 6, 64, _lib.ACT_SIGMOID, dact) == _lib.ERR_INVALID
    assert _fwd([some, some, None] + fwd[3:], 0, 3, 6, 64) == _lib.ERR_INVALID    # h0 without c0
    assert _fwd(fwd[:4] + [None] + fwd[5:], 0, 3, 6, 64) == _lib.ERR_INVALID      # R missing
    # Cs, XA, A, RES, dloss | K, R, W | DY, DPRE, DZ, dx0, dh0, dc0
    bwd = [some, some, None, some, some] + [some] * 3 + [some] * 4 + [None, None]
    assert _bwd(bwd, 0, 3, 6, 64) == _lib.OK and _bwd(bwd, 0, 0, 8, 32, _lib.ACT_HARD_SIGMOID, 2, 1) == _lib.OK
    assert _bwd(bwd, 0, 3, 6, 64, 2, 1) == _lib.ERR_INVALID and _bwd(bwd, 0, 3, 6, 64, 0, 0) == _lib.ERR_INVALID
    assert _bwd(bwd[:7] + [None] + bwd[8:], 0, 3, 6, 64) == _lib.ERR_INVALID      # W missing


def test_knob_flips_supported():
    L_ = _lib.lib()
    assert "FOV_NO_SELFFED_FUSED" not in os.environ
    assert _supported(32, 10, 6, 64) == 1
    os.environ["FOV_NO_SELFFED_FUSED"] = "1"
    try:
        L_.fov_reload_env()
        assert _supported(32, 10, 6, 64) == 0 and _supported(4096, 30, 1, 32) == 0
        assert _fwd([None] * N_FWD_PTRS, 4, 2, 6, 64) == _lib.ERR_INVALID     # the entries themselves do not read the knob
    finally:
        del os.environ["FOV_NO_SELFFED_FUSED"]
        L_.fov_reload_env()
    assert _supported(32, 10, 6, 64) == 1


def test_ops_wrapper_follows_the_knob_when_the_environment_changes():
    from longterm360fov_amd import ops
    assert "FOV_NO_SELFFED_FUSED" in ops._ENV_KNOBS
    assert ops.selffed_decoder_supported(32, 10, 6, 64) and not ops.selffed_decoder_supported(32, 10, 90, 64)
    os.environ["FOV_NO_SELFFED_FUSED"] = "1"
    try:
        assert not ops.selffed_decoder_supported(32, 10, 6, 64)
    finally:
        del os.environ["FOV_NO_SELFFED_FUSED"]
    assert ops.selffed_decoder_supported(32, 10, 6, 64)
