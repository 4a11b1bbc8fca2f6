"""Which forward kernel a layer, a fused decode and a decoder-alone call reach, at 256 CUs: one small call per row of the
dispatch, the launch names from the FOV_DBG_TRACE lines and a clean workspace status.  The numbers each form computes are
checked where the form is tested; here a launcher that starts choosing differently fails by name.

The workspace of every case is fresh and sized by the size function for that call: the launch side checks it against the
same plan, so a choice the size function did not count on is refused instead of run."""
import numpy as np
import pytest
import torch

from longterm360fov_amd import _lib
from test_gpu_ragged_guarded import launches, reload_env, traced

pytestmark = pytest.mark.gpu

PERSISTENT = {"wide16 LSTM", "wide LSTM", "cluster", "fused cluster", "seq2seq decode (wide16)"}
RECURRENT = PERSISTENT | {"generic", "lstm_pointwise_fwd"}
T_IN, T_OUT = 3, 2


def dev(rng, *shape, scale=0.1):
    return torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float32)).cuda()


def offset_by_one_float(t):
    """The same values four bytes behind a 16-byte boundary, inside a larger buffer."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def recurrent(ran):
    return [n for n in ran if n in RECURRENT]


def run_layer(capfd, H, F, B, T=T_IN, impl="auto", env=None, misaligned=False):
    from longterm360fov_amd import ops
    rng = np.random.default_rng(H * 1000 + F)
    x, K, R, b = dev(rng, B, T, F, scale=1.0), dev(rng, F, 4 * H), dev(rng, H, 4 * H), dev(rng, 4 * H)
    if misaligned:
        x = offset_by_one_float(x)
    ws = ops.Workspace()

    def call():
        hs, hT, cT = ops.lstm_seq(x, K, R, b, impl=impl, workspace=ws)
        ws.check()
        return hs, hT, cT
    (hs, hT, cT), trace = traced(capfd, call, env or {})
    assert bool(torch.isfinite(hT).all()) and bool(torch.isfinite(cT).all())
    return launches(trace)


# H, F, B, the other conditions, the recurrent launch expected; GEMM: the input projection of a width-512 layer runs in front of it
GEMM = "an input projection first"
LAYER = [
    (512, 6, 16, {}, ["wide16 LSTM"]),
    (512, 6, 144, {}, ["wide LSTM"]),
    (512, 128, 16, {}, [GEMM, "wide LSTM"]),
    (512, 512, 16, {}, ["wide16 LSTM"]),
    (512, 512, 16, {"misaligned": True}, [GEMM, "wide LSTM"]),
    (512, 6, 16, {"env": {"FOV_NO_WIDE16": "1"}}, ["wide LSTM"]),
    (256, 6, 16, {}, ["wide16 LSTM"]),
    (256, 6, 16, {"T": 0}, ["cluster"]),
    (256, 6, 16, {"impl": "cluster"}, ["cluster"]),
    (256, 6, 16, {"env": {"FOV_NO_WIDE16": "1"}}, ["wide LSTM"]),
    (256, 6, 144, {}, ["wide LSTM"]),
    (256, 6, 528, {}, ["cluster"]),
    (256, 128, 16, {}, ["wide LSTM"]),
    (256, 128, 16, {"misaligned": True}, ["generic"]),
    (256, 256, 16, {}, ["wide16 LSTM"]),
    (128, 6, 16, {}, ["wide16 LSTM"]),
    (128, 6, 144, {}, ["cluster"]),
    (64, 6, 16, {}, ["cluster"]),
    (32, 6, 16, {}, ["generic"]),
]


def case_id(row):
    H, F, B, cond = row[:4]
    extra = "-".join("%s=%s" % (k, "+".join(v) if isinstance(v, dict) else v) for k, v in sorted(cond.items()))
    return "H%d-F%d-B%d%s" % (H, F, B, "-" + extra if extra else "")


@pytest.mark.parametrize("H,F,B,cond,want", LAYER, ids=[case_id(r) for r in LAYER])
def test_layer_forward_kernel(capfd, H, F, B, cond, want):
    ran = run_layer(capfd, H, F, B, **cond)
    assert recurrent(ran) == want[-1:] and ran[-1] == want[-1], ran
    assert (len(ran) > 1) == (want[0] is GEMM), ran


@pytest.mark.parametrize("H,F,B,cond", [r[:4] for r in LAYER], ids=[case_id(r) for r in LAYER])
def test_layer_forward_generic_on_request(capfd, H, F, B, cond):
    ran = run_layer(capfd, H, F, B, **dict(cond, impl="generic"))
    assert ran == ["generic"], ran


@pytest.mark.parametrize("H,env", [(1024, {}), (512, {"FOV_DBG_RESIDENT_LIMIT": "8"})], ids=["H1024", "H512-resident8"])
def test_layer_forward_stepwise(capfd, H, env):
    """Widths above the persistent kernels' (or a width-512 layer whose sixteen workgroups per tile are not resident): the
    step-wise form, one GEMM and one pointwise launch per step."""
    ran = run_layer(capfd, H, 6, 16, T=2, env=env)
    assert "lstm_pointwise_fwd" in ran and not set(ran) & (PERSISTENT | {"generic"}), ran


def s2s_weights(rng, H, F_enc, F_dec):
    return {"enc_K": dev(rng, F_enc, 4 * H), "enc_R": dev(rng, H, 4 * H), "enc_b": dev(rng, 4 * H),
            "dec_K": dev(rng, F_dec, 4 * H), "dec_R": dev(rng, H, 4 * H), "dec_b": dev(rng, 4 * H),
            "dense_W": dev(rng, H, F_dec), "dense_b": dev(rng, F_dec)}


def run_decode(capfd, H, B, impl="auto", env=None, F_enc=6, decoder_alone=False):
    from longterm360fov_amd import ops
    rng = np.random.default_rng(H + B)
    w = s2s_weights(rng, H, F_enc, 6)
    enc, dec0 = dev(rng, B, T_IN, F_enc, scale=1.0), dev(rng, B, 1, 6, scale=1.0)
    h0, c0 = dev(rng, B, H), dev(rng, B, H)
    ws = ops.Workspace()

    def call():
        if decoder_alone:
            out = ops.seq2seq_decoder(dec0, h0, c0, w, T_OUT, impl=impl, workspace=ws)
        else:
            out = ops.seq2seq_decode(enc, dec0, w, T_OUT, impl=impl, workspace=ws)
        ws.check()
        return out
    out, trace = traced(capfd, call, env or {})
    assert bool(torch.isfinite(out).all())
    return launches(trace)


DECODE = [
    (256, 16, {}, ["seq2seq decode (wide16)"]),
    (256, 144, {}, ["fused cluster"]),
    (256, 144, {"env": {"FOV_TWO_LAUNCHES": "1"}}, ["cluster", "cluster"]),
    (64, 16, {}, ["fused cluster"]),
]
DECODER = [
    (256, 16, {}, ["seq2seq decode (wide16)"]),
    (256, 144, {}, ["cluster"]),
]


def decode_id(row):
    return "H%d-B%d%s" % (row[0], row[1], "-two-launches" if row[2] else "")


@pytest.mark.parametrize("H,B,cond,want", DECODE, ids=[decode_id(r) for r in DECODE])
def test_decode_kernel(capfd, H, B, cond, want):
    ran = run_decode(capfd, H, B, **cond)
    assert ran == want, ran


@pytest.mark.parametrize("H,B,cond,want", DECODER, ids=[decode_id(r) for r in DECODER])
def test_decoder_alone_kernel(capfd, H, B, cond, want):
    ran = run_decode(capfd, H, B, decoder_alone=True, **cond)
    assert ran == want, ran


@pytest.mark.parametrize("decoder_alone", [False, True], ids=["decode", "decoder"])
@pytest.mark.parametrize("H,B", [(256, 16), (256, 144), (64, 16)])
def test_decode_generic_on_request(capfd, H, B, decoder_alone):
    ran = run_decode(capfd, H, B, impl="generic", decoder_alone=decoder_alone)
    assert ran == ["generic"], ran


def test_cluster_on_request_refuses_a_shape_it_does_not_take(capfd):
    """impl = cluster is a demand, not a preference: a width the cluster kernel does not have comes back FOV_ERR_UNSUPPORTED
    with the launcher's own message and nothing is launched - no silent fallback."""
    from longterm360fov_amd import ops
    with pytest.raises(ops.FovError, match=r"cluster kernel supports H in \{64,128,256\}") as e:
        run_decode(capfd, 512, 16, impl="cluster", F_enc=128)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    reload_env()        # (the knobs went back when the call raised; the library has not re-read them yet)
    assert launches(capfd.readouterr().err) == []
