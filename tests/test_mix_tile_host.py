"""The others-mixing decoder at its own width (H = 32 / 64, mix_tile.hip behind fov_mix_decoder_fwd / _bwd) as far as the host can
see it, with no device: the shape predicate over its edges, the model's opt-in logic, and the two entry points called with fake
pointers in a child process that sees no device (HIP_VISIBLE_DEVICES and ROCR_VISIBLE_DEVICES empty; the child asks for the device
count first and skips if one answers).  A call that passes every check reaches a HIP call and comes back as FOV_ERR_LAUNCH with
the runtime's no-device message: that is "accepted".  The library before these kernels refuses H = 32 with FOV_ERR_UNSUPPORTED."""
import ctypes
import itertools
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from longterm360fov_amd import _lib  # noqa: E402

OK, INVALID, UNSUPPORTED, LAUNCH = _lib.OK, _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED, _lib.ERR_LAUNCH
NO_DEVICE = "no ROCm-capable device"
FAKE_BASE, FAKE_STEP = 0x7F0000000000, 1 << 20
GRID = list(itertools.product((0, 1, 17), (0, 1), (0, 1, 8, 9), (16, 32, 64, 128, 256), (0, 1)))   # B, T_out, O, H, backward


def rule(B, T, O, H, backward):
    """The tile shape rule, written out: what fov_mix_decoder_tile_supported must answer."""
    return int(0 <= B <= 2 ** 30 and 0 <= T <= 2 ** 30 and 1 <= O <= 8 and (H == 32 or (H == 64 and not backward)))


# ----------------------------------------------------------------------------------------------------------------------- child

def _fake(n):
    return [FAKE_BASE + i * FAKE_STEP for i in range(n)]


def call_fwd(L, B, T, H, O, bf16=False, workspace=FAKE_BASE + (1 << 32), nbytes=1 << 40, train=True, final=True):
    p = _fake(29)
    lead, wts, out, fin, tapes = p[:6], p[6:15], p[15], p[16:20], p[20:27]
    if not final:
        fin = [None] * 4
    if not train:
        tapes = [None] * 7
    f = L.fov_mix_decoder_fwd_bf16 if bf16 else L.fov_mix_decoder_fwd
    rc = f(*lead, T * O, O, *wts, out, *fin, *tapes, B, T, H, O, _lib.ACT_SIGMOID, workspace, nbytes, None)
    return int(rc), (L.fov_last_error() or b"").decode("utf-8", "replace")


def call_bwd(L, B, T, H, O, bf16=False, workspace=FAKE_BASE + (1 << 32), nbytes=1 << 40):
    f = L.fov_mix_decoder_bwd_bf16 if bf16 else L.fov_mix_decoder_bwd
    rc = f(*_fake(21), B, T, H, O, _lib.ACT_SIGMOID, workspace, nbytes, None)
    return int(rc), (L.fov_last_error() or b"").decode("utf-8", "replace")


def device_count():
    _lib.lib()
    path = None
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            path = line.split()[-1]
            break
    if path is None:
        return None, None
    n = ctypes.c_int(-1)
    rc = ctypes.CDLL(path).hipGetDeviceCount(ctypes.byref(n))
    return int(rc), int(n.value)


def child(out_path):
    result = {"rows": [], "skipped": None, "error": None}
    rc, n = device_count()
    if rc is None:
        result["error"] = "the HIP runtime of the library was not found among the process's mappings"
    elif not ((rc == 0 and n == 0) or rc == 100):
        result["skipped"] = "a device is visible to the child (hipGetDeviceCount: error %d, %d devices): no call was made" % (rc, n)
    else:
        L = _lib.lib()

        def row(name, got):
            result["rows"].append({"row": name, "rc": got[0], "err": got[1][:300]})

        for H in (32, 64):
            row("fwd H=%d" % H, call_fwd(L, 17, 3, H, 6))
            row("fwd H=%d workspace=NULL" % H, call_fwd(L, 17, 3, H, 6, workspace=None, nbytes=0))
            row("fwd H=%d no tapes" % H, call_fwd(L, 17, 3, H, 6, train=False, final=False))
            row("fwd_bf16 H=%d" % H, call_fwd(L, 17, 3, H, 6, bf16=True))
            row("bwd H=%d" % H, call_bwd(L, 17, 3, H, 6))
            row("bwd H=%d workspace=NULL" % H, call_bwd(L, 17, 3, H, 6, workspace=None, nbytes=0))
            row("bwd_bf16 H=%d" % H, call_bwd(L, 17, 3, H, 6, bf16=True))
        for B, T, O, H, backward in GRID:
            sup = int(L.fov_mix_decoder_tile_supported(B, T, H, O, backward))
            got = (call_bwd if backward else call_fwd)(L, B, T, H, O)
            result["rows"].append({"row": "grid", "shape": [B, T, O, H, backward], "sup": sup, "rc": got[0], "err": got[1][:300]})
    with open(out_path, "w") as f:
        json.dump(result, f)
    print("DONE", flush=True)


# ---------------------------------------------------------------------------------------------------------------------- parent

_RESULT = {}


def rows():
    import pytest
    if not _RESULT:
        env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "rows.json")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], env=env, cwd=ROOT, capture_output=True,
                               text=True, timeout=300)
            _RESULT["returncode"], _RESULT["stderr"] = p.returncode, p.stderr[-2000:]
            _RESULT["data"] = json.load(open(out)) if os.path.exists(out) else None
    r = _RESULT
    assert r["returncode"] == 0 and r["data"] is not None, "the child ended with status %s\n%s" % (r["returncode"], r["stderr"])
    assert not r["data"]["error"], r["data"]["error"]
    if r["data"]["skipped"]:
        pytest.skip(r["data"]["skipped"])
    return r["data"]["rows"]


def named(name):
    (x,) = [x for x in rows() if x["row"] == name]
    return x


def accepted(x):
    return x["rc"] == LAUNCH and NO_DEVICE in x["err"]


def test_predicate_over_its_edges():
    L = _lib.lib()
    for B, T, O, H, backward in GRID:
        assert int(L.fov_mix_decoder_tile_supported(B, T, H, O, backward)) == rule(B, T, O, H, backward), (B, T, O, H, backward)
    for shape, want in (((-1, 1, 32, 6, 0), 0), ((1, -1, 32, 6, 0), 0), ((2 ** 30, 1, 32, 6, 0), 1), ((2 ** 30 + 1, 1, 32, 6, 0), 0),
                        ((1, 2 ** 30, 32, 6, 1), 0), ((33, 64, 64, 8, 0), 1), ((33, 64, 64, 8, 1), 0), ((33, 64, 32, 8, 7), 1)):
        assert int(L.fov_mix_decoder_tile_supported(*shape)) == want, shape


def test_ops_predicates_keep_the_default_path_off_the_tile_kernels():
    from longterm360fov_amd import ops
    assert ops.mix_decoder_supported(256, 6) and not ops.mix_decoder_supported(32, 6) and not ops.mix_decoder_supported(64, 6)
    assert ops.mix_decoder_tile_supported(17, 3, 32, 6) and ops.mix_decoder_tile_supported(17, 3, 32, 6, backward=True)
    assert ops.mix_decoder_tile_supported(17, 3, 64, 6) and not ops.mix_decoder_tile_supported(17, 3, 64, 6, backward=True)
    assert not ops.mix_decoder_tile_supported(17, 3, 256, 6)


def test_model_opt_in_logic():
    import pytest
    from longterm360fov_amd.models import OthersMixingSeq2Seq
    assert OthersMixingSeq2Seq(latent_dim=32, num_user=4, seed=1)._run_width() == 256
    m = OthersMixingSeq2Seq(latent_dim=32, num_user=4, seed=1, native_width=True)
    assert m._run_width() == 32 and m.native_width
    assert OthersMixingSeq2Seq(latent_dim=64, num_user=4, seed=1, native_width=True)._run_width() == 64
    assert [a.shape for a in m.get_weights()] == [a.shape for a in OthersMixingSeq2Seq(latent_dim=32, num_user=4, seed=1).get_weights()]
    for bad in (dict(latent_dim=48), dict(latent_dim=256), dict(latent_dim=256, dtype="bf16"), dict(latent_dim=32, impl="generic"),
                dict(latent_dim=32, num_decoder_tokens=9)):
        with pytest.raises(ValueError):
            OthersMixingSeq2Seq(num_user=4, seed=1, native_width=True, **bad)
    with pytest.raises(ValueError):     # bf16 at width 32 is refused with or without the opt-in
        OthersMixingSeq2Seq(latent_dim=32, num_user=4, dtype="bf16", native_width=True)


def test_forward_is_accepted_at_both_tile_widths():
    for H in (32, 64):
        for name in ("fwd H=%d", "fwd H=%d workspace=NULL", "fwd H=%d no tapes"):
            x = named(name % H)
            assert accepted(x), (name % H, x)


def test_backward_is_accepted_at_32_and_refused_at_64():
    for name in ("bwd H=32", "bwd H=32 workspace=NULL"):
        assert accepted(named(name)), (name, named(name))
    for name in ("bwd H=64", "bwd H=64 workspace=NULL"):
        x = named(name)
        assert x["rc"] == UNSUPPORTED and "LDS" in x["err"], (name, x)     # the message says why


def test_bf16_entries_stay_at_256():
    for name in ("fwd_bf16 H=32", "fwd_bf16 H=64", "bwd_bf16 H=32", "bwd_bf16 H=64"):
        assert named(name)["rc"] == UNSUPPORTED, (name, named(name))


def test_predicate_agrees_with_the_entries_on_every_row():
    grid = [x for x in rows() if x["row"] == "grid"]
    assert len(grid) == len(GRID)
    for x in grid:
        B, T, O, H, backward = x["shape"]
        assert x["sup"] == rule(B, T, O, H, backward), x
        if x["sup"]:            # the entry runs the tile kernel: a launch where there is work, FOV_OK and nothing launched without
            assert (accepted(x) if B > 0 and T > 0 else x["rc"] == OK), x
        elif H == 256 and 1 <= O <= 8:   # the persistent kernel's width: accepted, but not by the tile rule
            assert (accepted(x) if B > 0 and T > 0 else x["rc"] == OK), x
        else:
            assert x["rc"] in (INVALID, UNSUPPORTED), x
            assert x["rc"] == (INVALID if O == 0 else UNSUPPORTED), x


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    child(sys.argv[2])
