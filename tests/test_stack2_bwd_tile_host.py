"""fov_lstm_stack2_bwd at H = 32 / 64 (one workgroup per 16-sequence tile) as the host sees it, with no device.

The predicate and every refusal below are decided from the arguments alone, before any HIP call: the calls are made in one child
process whose HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES are empty, with pointers to host memory that nothing dereferences.

    fov_lstm_stack2_bwd_supported   1 at H 32 / 64 for B in {1, 17, 513} and T in {1, 50}; 0 at H in {16, 48, 128, 256}
    fov_lstm_stack2_bwd             H = 48: FOV_ERR_UNSUPPORTED; at H = 32 a NULL R1 / K2 / R2 / x / dz1 and an unknown act:
                                    FOV_ERR_INVALID; a workspace one byte short: FOV_ERR_WORKSPACE."""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

POINTERS = ("x R1 K2 R2 h0_1 c0_1 h0_2 c0_2 hs1 reserve1 hs2 reserve2 dhs2 dhT2 dcT2 dhT1 dcT1 dz1 dz2 dK1 dR1 db1 dK2 dR2 db2 "
            "dh0_1 dc0_1 dh0_2 dc0_2").split()
REQUIRED = "x R1 K2 R2 hs1 reserve1 hs2 reserve2 dz1 dz2".split()
B, T, F = 17, 3, 6


def child():
    from longterm360fov_amd import _lib
    L = _lib.lib()
    keep = {n: ctypes.create_string_buffer(64) for n in REQUIRED}
    ws = ctypes.create_string_buffer(64)
    ws_ptr = (ctypes.addressof(ws) + 15) & ~15
    out = {"codes": {"INVALID": _lib.ERR_INVALID, "UNSUPPORTED": _lib.ERR_UNSUPPORTED, "WORKSPACE": _lib.ERR_WORKSPACE, "OK": _lib.OK},
           "pred": {}, "calls": {}}
    for H in (16, 32, 48, 64, 128, 256):
        for b in (1, 17, 513):
            for t in (1, 50):
                out["pred"]["%d %d %d" % (H, b, t)] = int(L.fov_lstm_stack2_bwd_supported(b, t, F, H))

    def call(tag, H, null=(), act=_lib.ACT_SIGMOID, ws_delta=0):
        p = [None if (n in null or n not in keep) else ctypes.addressof(keep[n]) for n in POINTERS]
        need = int(L.fov_lstm_stack2_bwd_workspace_bytes(B, T, F, H)) + ws_delta
        rc = int(L.fov_lstm_stack2_bwd(*p, B, T, F, H, act, 0, ws_ptr, need, None))
        out["calls"][tag] = [rc, (L.fov_last_error() or b"").decode("utf-8", "replace") if rc else ""]

    call("H48", 48)
    for n in ("R1", "K2", "R2", "x", "dz1"):
        call("null " + n, 32, null=(n,))
    call("act", 32, act=7)
    call("short", 32, ws_delta=-1)
    call("short64", 64, ws_delta=-1)
    print(json.dumps(out))


_RESULT = {}


def result():
    if not _RESULT:
        env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        _RESULT.update(json.loads(p.stdout.strip().splitlines()[-1]))
    return _RESULT


def test_the_predicate_takes_widths_32_and_64_at_any_batch():
    pred = result()["pred"]
    for key, v in pred.items():
        H = int(key.split()[0])
        assert v == (1 if H in (32, 64) else 0), (key, v)
    assert len(pred) == 36


def test_width_48_is_refused_as_unsupported():
    r, codes = result()["calls"], result()["codes"]
    assert r["H48"][0] == codes["UNSUPPORTED"] and "H=48" in r["H48"][1], r["H48"]


def test_width_32_refuses_missing_operands_and_an_unknown_activation_as_invalid():
    r, codes = result()["calls"], result()["codes"]
    for tag in ("null R1", "null K2", "null R2", "null x", "null dz1", "act"):
        assert r[tag][0] == codes["INVALID"], (tag, r[tag])


def test_a_workspace_one_byte_short_is_refused():
    r, codes = result()["calls"], result()["codes"]
    for tag in ("short", "short64"):
        assert r[tag][0] == codes["WORKSPACE"], (tag, r[tag])


if __name__ == "__main__" and sys.argv[1:] == ["--child"]:
    child()
