"""fov_selffed2_decoder_supported without a GPU: the rule is arithmetic (1 <= O <= 8, any non-negative batch and length; H = 32
or 64 for the forward, H = 32 alone for the backward) plus the FOV_NO_SELFFED2_FUSED knob; fov_selffed2_decoder_fwd / _bwd
refuse every other shape before they look at a pointer and before their first HIP call, so that runs here too.
tests/test_abi.py holds the prototypes against the ctypes table."""
import ctypes
import itertools
import os

import pytest

from longterm360fov_amd import _lib

N_FWD_PTRS, N_BWD_PTRS = 24, 19


def _supported(B, T, O, H, backward):
    return _lib.lib().fov_selffed2_decoder_supported(B, T, O, H, backward)


def _fwd(ptrs, B, T, O, H, act=_lib.ACT_SIGMOID):
    return _lib.lib().fov_selffed2_decoder_fwd(*ptrs, B, T, O, H, act, None)


def _bwd(ptrs, B, T, O, H, act=_lib.ACT_SIGMOID):
    return _lib.lib().fov_selffed2_decoder_bwd(*ptrs, B, T, O, H, act, None)


def _rule(B, T, O, H, backward):
    return int(B >= 0 and T >= 0 and 1 <= O <= 8 and (H == 32 or (H == 64 and not backward)))


def test_supported_truth_table():
    for H, O, backward in itertools.product((16, 32, 48, 64, 128), (0, 1, 8, 9), (0, 1)):
        for B, T in ((0, 0), (1, 1), (17, 30), (100000, 64), (32, 0), (0, 10)):
            assert _supported(B, T, O, H, backward) == _rule(B, T, O, H, backward), (B, T, O, H, backward)
    assert _supported(32, 10, 6, 64, 0) == 1 and _supported(32, 10, 6, 64, 1) == 0      # the backward is H = 32 alone
    assert _supported(32, 10, 6, 32, 0) == 1 and _supported(32, 10, 6, 32, 1) == 1
    assert _supported(32, 10, 6, 32, 7) == 1 and _supported(32, 10, 6, 64, 7) == 0      # any non-zero flag is the backward
    for backward in (0, 1):
        assert _supported(-1, 10, 6, 32, backward) == 0 and _supported(32, -1, 6, 32, backward) == 0
        for H in (0, -32, 256):
            assert _supported(32, 10, 6, H, backward) == 0
        for O in (-1, 90):
            assert _supported(32, 10, O, 32, backward) == 0


@pytest.mark.parametrize("B,T,O,H", [(5, 2, 6, 16), (5, 2, 6, 48), (5, 2, 6, 128), (5, 2, 0, 64), (5, 2, 9, 32), (5, 2, 0, 32),
                                     (-1, 2, 6, 64), (5, -1, 6, 32)])
def test_unsupported_shapes_are_refused_before_any_pointer_is_looked_at(B, T, O, H):
    assert _supported(B, T, O, H, 0) == 0 and _supported(B, T, O, H, 1) == 0
    for name, call, n in (("fov_selffed2_decoder_fwd", _fwd, N_FWD_PTRS), ("fov_selffed2_decoder_bwd", _bwd, N_BWD_PTRS)):
        assert call([None] * n, B, T, O, H) == _lib.ERR_UNSUPPORTED
        msg = _lib.lib().fov_last_error().decode()
        assert name in msg and "H=%d" % H in msg and "O=%d" % O in msg, msg


def test_the_backward_refuses_width_64_the_forward_takes():
    assert _bwd([None] * N_BWD_PTRS, 5, 2, 6, 64) == _lib.ERR_UNSUPPORTED
    msg = _lib.lib().fov_last_error().decode()
    assert "fov_selffed2_decoder_bwd" in msg and "H=64" in msg, msg
    assert _fwd([None] * N_FWD_PTRS, 5, 2, 6, 64) == _lib.ERR_INVALID      # a supported shape: the pointers are looked at


def test_missing_pointers_and_unknown_activations_are_invalid_and_an_empty_batch_is_a_no_op():
    some = ctypes.c_void_p(0x1000)      # never dereferenced: B = 0 and T = 0 return before a launch
    assert _fwd([None] * N_FWD_PTRS, 4, 2, 6, 64) == _lib.ERR_INVALID
    assert _bwd([None] * N_BWD_PTRS, 4, 2, 6, 32) == _lib.ERR_INVALID
    # x0 | h1_0, c1_0, h2_0, c2_0 | K1, R1, b1, K2, R2, b2, W | bd, ctx | H1, C1, H2, C2, XY, RES1, RES2, y, hT, cT
    fwd = [some] + [None] * 4 + [some] * 7 + [None] * 2 + [None] * 10
    for H in (32, 64):
        assert _fwd(fwd, 0, 3, 6, H) == _lib.OK and _fwd(fwd, 0, 3, 1, H, _lib.ACT_HARD_SIGMOID) == _lib.OK
        assert _fwd(fwd, 5, 0, 6, H) == _lib.OK                       # no step: nothing is written
        assert _fwd(fwd, 0, 0, 8, H) == _lib.OK
        for act in (2, 5, -1):                                        # no such recurrent activation
            assert _fwd(fwd, 0, 3, 6, H, act) == _lib.ERR_INVALID
        for k in range(5, 12):                                        # every weight is required
            assert _fwd(fwd[:k] + [None] + fwd[k + 1:], 0, 3, 6, H) == _lib.ERR_INVALID, k
    assert _fwd([None] + fwd[1:], 5, 3, 6, 32) == _lib.ERR_INVALID    # x0 missing where there is work
    assert _fwd([None] + fwd[1:], 0, 3, 6, 32) == _lib.OK
    assert _fwd([some, some, None, None, some] + fwd[5:], 0, 3, 6, 32) == _lib.OK      # each state is optional on its own
    # C1, C2, XY, RES1, RES2, dloss | K1, R1, K2, R2, W | DPRE, DZ1, DZ2 | dx0, dh1_0, dc1_0, dh2_0, dc2_0
    bwd = [some] * 6 + [some] * 5 + [some] * 3 + [None] * 5
    assert _bwd(bwd, 0, 3, 6, 32) == _lib.OK and _bwd(bwd, 0, 0, 8, 32, _lib.ACT_HARD_SIGMOID) == _lib.OK
    assert _bwd(bwd, 0, 3, 6, 32, 2) == _lib.ERR_INVALID and _bwd(bwd, 0, 3, 6, 32, -1) == _lib.ERR_INVALID
    for k in range(6, 11):                                            # every weight is required
        assert _bwd(bwd[:k] + [None] + bwd[k + 1:], 0, 3, 6, 32) == _lib.ERR_INVALID, k
    for k in list(range(6)) + [11, 12, 13]:                           # tapes and outputs are required where there is work
        assert _bwd(bwd[:k] + [None] + bwd[k + 1:], 4, 2, 6, 32) == _lib.ERR_INVALID, k
        assert _bwd(bwd[:k] + [None] + bwd[k + 1:], 0, 2, 6, 32) == _lib.OK, k


def test_knob_flips_supported():
    L_ = _lib.lib()
    assert "FOV_NO_SELFFED2_FUSED" not in os.environ
    assert _supported(32, 10, 6, 64, 0) == 1 and _supported(32, 10, 6, 32, 1) == 1
    os.environ["FOV_NO_SELFFED2_FUSED"] = "1"
    try:
        L_.fov_reload_env()
        assert _supported(32, 10, 6, 64, 0) == 0 and _supported(4096, 30, 1, 32, 0) == 0 and _supported(32, 10, 6, 32, 1) == 0
        assert _lib.lib().fov_selffed_decoder_supported(32, 10, 6, 64) == 1       # the one-layer decoder has its own knob
        assert _fwd([None] * N_FWD_PTRS, 4, 2, 6, 64) == _lib.ERR_INVALID         # the entries themselves do not read the knob
        assert _bwd([None] * N_BWD_PTRS, 4, 2, 6, 32) == _lib.ERR_INVALID
    finally:
        del os.environ["FOV_NO_SELFFED2_FUSED"]
        L_.fov_reload_env()
    assert _supported(32, 10, 6, 64, 0) == 1 and _supported(32, 10, 6, 32, 1) == 1


def test_ops_wrapper_follows_the_knob_when_the_environment_changes():
    from longterm360fov_amd import ops
    assert "FOV_NO_SELFFED2_FUSED" in ops._ENV_KNOBS
    assert ops.selffed2_decoder_supported(32, 10, 6, 64) and not ops.selffed2_decoder_supported(32, 10, 6, 64, backward=True)
    assert ops.selffed2_decoder_supported(32, 10, 6, 32, backward=True) and not ops.selffed2_decoder_supported(32, 10, 9, 32)
    os.environ["FOV_NO_SELFFED2_FUSED"] = "1"
    try:
        assert not ops.selffed2_decoder_supported(32, 10, 6, 64) and not ops.selffed2_decoder_supported(32, 10, 6, 32, backward=True)
    finally:
        del os.environ["FOV_NO_SELFFED2_FUSED"]
    assert ops.selffed2_decoder_supported(32, 10, 6, 64) and ops.selffed2_decoder_supported(32, 10, 6, 32, backward=True)
