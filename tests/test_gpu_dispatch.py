"""Which forward kernel a layer, a fused decode and a decoder-alone call reach, and which launches a layer's backward makes, at
256 CUs: one small call per row of the dispatch, the launch names from the FOV_DBG_TRACE lines and a clean workspace status.
The numbers each form computes are checked where the form is tested; here a launcher that starts choosing differently fails by name.

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


# ---------------------------------------------------------------------------------------------------------------------
# Backward: every edge of the plan of a layer's BPTT (lstm_train.hip: plan_lstm_bwd) - the recurrence, the form of the weight
# gradients, where db and dx come from.  A row is one small training forward and, under the trace, one backward call; what it
# asserts is the whole launch sequence of that call, recorded from the library before the plan existed.
# ---------------------------------------------------------------------------------------------------------------------
def bwd_operands(H, B, F, T, dtype="f32", seed=0):
    """The training forward of one layer and the gradients that reach it -> the arguments of ops.lstm_seq_bwd."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(H * 1000 + B + seed)
    x, K, R, b = dev(rng, B, T, F, scale=1.0), dev(rng, F, 4 * H), dev(rng, H, 4 * H), dev(rng, 4 * H)
    h0, c0 = dev(rng, B, H), dev(rng, B, H)
    hs, _, _, res = ops.lstm_seq_train(x, K, R, b, h0, c0, workspace=ops.Workspace(), dtype=dtype)
    torch.cuda.synchronize()
    return {"x": x, "K": K, "R": R, "hs": hs, "reserve": res, "h0": h0, "c0": c0,
            "dhs": dev(rng, B, T, H), "dhT": dev(rng, B, H), "dcT": dev(rng, B, H)}


def grad_buffers(F, H, flat):
    """dK, dR, db from the allocator, or adjacent in one buffer as a trainer's flat gradient vector holds them."""
    if not flat:
        return [torch.empty(s, dtype=torch.float32, device="cuda") for s in ((F, 4 * H), (H, 4 * H), (4 * H,))]
    buf = torch.empty((F + H + 1) * 4 * H, dtype=torch.float32, device="cuda")
    return [buf[:F * 4 * H].view(F, 4 * H), buf[F * 4 * H:(F + H) * 4 * H].view(H, 4 * H), buf[(F + H) * 4 * H:]]


def run_backward(capfd, H, B, F=6, T=T_IN, dtype="f32", env=None, need_dx=False, flat=False, off=()):
    """-> (the outputs of one ops.lstm_seq_bwd call, its launches).  off: operands moved one float off a 16-byte boundary for the
    backward call (the forward ran on the aligned values)."""
    from longterm360fov_amd import ops
    a = bwd_operands(H, B, F, T, dtype)
    for name in off:
        a[name] = offset_by_one_float(a[name])
    dK, dR, db = grad_buffers(F, H, flat)
    scratch = ops.Scratch()

    def call():
        out = ops.lstm_seq_bwd(dK=dK, dR=dR, db=db, need_dx=need_dx, need_state_grads=True, scratch=scratch, dtype=dtype, **a)
        scratch.check()
        return out
    out, trace = traced(capfd, call, env or {})
    assert all(bool(torch.isfinite(v).all()) for v in out.values() if v is not None)
    return out, launches(trace)


def run_stack2_backward(capfd, H, B, F=6, T=T_IN):
    """Two stacked layers through ops.lstm_stack2_bwd -> (outputs with the six weight gradients, launches)."""
    from longterm360fov_amd import ops
    lo = bwd_operands(H, B, F, T)
    up = bwd_operands(H, B, H, T, seed=1)
    hs2, _, _, res2 = ops.lstm_seq_train(lo["hs"], up["K"], up["R"], torch.zeros(4 * H, device="cuda"), up["h0"], up["c0"], workspace=ops.Workspace())
    g1, g2 = grad_buffers(F, H, False), grad_buffers(H, H, False)
    scratch = ops.Scratch()

    def call():
        out = ops.lstm_stack2_bwd(lo["x"], (lo["K"], lo["R"]), (up["K"], up["R"]), (lo["hs"], lo["reserve"], lo["h0"], lo["c0"]),
                                  (hs2, res2, up["h0"], up["c0"]), dhs2=up["dhs"], dhT2=up["dhT"], dcT2=up["dcT"], dhT1=lo["dhT"],
                                  dcT1=lo["dcT"], grads1=g1, grads2=g2, need_state_grads=True, scratch=scratch)
        scratch.check()
        return out
    out, trace = traced(capfd, call, {})
    out.update(zip(("dK1", "dR1", "db1", "dK2", "dR2", "db2"), g1 + g2))
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    return out, launches(trace)


def run_wgrad_pair(capfd, H, B, T2=T_OUT, dz2_off=False):
    """An encoder over T_IN steps and a decoder over T2 through ops.lstm_seq_wgrad_pair, from the dz tapes of two data-path-only
    backward calls -> (the six gradients, launches)."""
    from longterm360fov_amd import ops
    layers, outs = [], {}
    for i, T in enumerate((T_IN, T2)):
        a = bwd_operands(H, B, 6, T, seed=i)
        dz = ops.lstm_seq_bwd(need_weight_grads=False, scratch=ops.Scratch(), **a)["dz"]
        torch.cuda.synchronize()
        g = grad_buffers(6, H, False)
        layers.append((a["x"], a["hs"], a["h0"], offset_by_one_float(dz) if (dz2_off and i) else dz) + tuple(g))
        outs.update(zip(("dK%d" % i, "dR%d" % i, "db%d" % i), g))
    _, trace = traced(capfd, lambda: ops.lstm_seq_wgrad_pair(layers[0], layers[1], scratch=ops.Scratch()), {})
    assert all(bool(torch.isfinite(v).all()) for v in outs.values())
    return outs, launches(trace)


# launches of the GEMM layer behind the recurrence, as it splits these shapes
GS = ["gemm_f32", "splitk_reduce"]
SKINNY = ["skinny_tn", "skinny_reduce"]
DB_SUM = ["colsum_partial", "colsum_reduce"]
STEPS = ["lstm_bwd_pointwise"] + GS                # a step of the host-stepped recurrence; T_IN of them
BF16_PRODUCTS = ["gemm_bf16_tn"] * 3               # dK, dR and the initial state's share of dR
NARROW, GROUPS4 = {"FOV_NO_BWD16_NARROW": "1"}, {"FOV_NO_BWD16_NARROW": "1", "FOV_BWD_GROUPS4": "1"}
# H, B, the other arguments of run_backward, the launches of the backward call
BACKWARD = [
    # the recurrence; few rows: all weight gradients in one wgrad_rows launch behind it
    (512, 16, {}, ["16-unit BPTT", "wgrad_rows"]),
    (512, 144, {}, ["16-unit BPTT", "wgrad_rows"]),
    (256, 16, {}, ["16-unit BPTT", "wgrad_rows"]),
    (256, 128, {}, ["16-unit BPTT", "wgrad_rows"]),
    (256, 144, {}, ["8-group BPTT", "wgrad_rows"]),
    (256, 512, {}, ["8-group BPTT"] + DB_SUM + SKINNY + GS + GS),
    (256, 528, {}, ["bwd cluster"] + DB_SUM + SKINNY + GS + GS),
    (256, 16, {"env": NARROW}, ["8-group BPTT", "wgrad_rows"]),
    (256, 16, {"env": GROUPS4}, ["bwd cluster", "wgrad_rows"]),
    (128, 16, {}, ["16-unit BPTT", "wgrad_rows"]),
    (128, 144, {}, ["bwd cluster", "wgrad_rows"]),
    (64, 16, {}, ["bwd cluster", "wgrad_rows"]),
    (32, 16, {}, STEPS * T_IN + ["gemm_f32"] + GS + ["gemm_f32"] + DB_SUM),
    (1024, 16, {}, STEPS * T_IN + ["gemm_f32"] * 3 + DB_SUM),
    (256, 16, {"env": {"FOV_BWD_STEPPED": "1"}}, STEPS * T_IN + ["gemm_f32"] + GS + ["gemm_f32"] + DB_SUM),
    (512, 16, {"off": ("R",)}, STEPS * T_IN + ["gemm_f32"] * 3 + DB_SUM),
    (128, 16, {"off": ("R",)}, ["bwd cluster", "wgrad_rows"]),
    (256, 16, {"dtype": "bf16"}, ["8-group BPTT"] + DB_SUM + BF16_PRODUCTS),
    (256, 528, {"dtype": "bf16"}, ["8-group BPTT"] + DB_SUM + SKINNY + ["gemm_bf16_tn", "splitk_reduce"] * 2),
    # the weight gradients: 640 rows and one more; dK, dR, db adjacent (F 128: one product and the initial state's share; F 6:
    # dR and db as one product, that share, dK); separate buffers (db: the kernel's partials and a column sum); the knobs
    (256, 128, {"T": 5}, ["16-unit BPTT", "wgrad_rows"]),
    (512, 641, {"T": 1}, ["16-unit BPTT", "wgrad_group"]),
    (256, 641, {"T": 1}, ["bwd cluster"] + DB_SUM + GS + GS),
    (256, 256, {"F": 128, "flat": True}, ["8-group BPTT"] + GS + GS),
    (256, 256, {"flat": True}, ["8-group BPTT"] + GS + GS + GS),
    (256, 256, {"F": 128}, ["8-group BPTT"] + DB_SUM + GS + GS + GS),
    (256, 256, {"F": 128, "flat": True, "env": {"FOV_NO_WGRAD_FUSION": "1"}}, ["8-group BPTT"] + DB_SUM + GS + GS + GS),
    (256, 16, {"env": {"FOV_NO_WGRAD_GROUP": "1"}}, ["16-unit BPTT"] + DB_SUM + ["gemm_f32"] + GS + ["gemm_f32"]),
    (512, 16, {"env": {"FOV_NO_WGRAD_GROUP": "1"}}, ["16-unit BPTT"] + DB_SUM + ["gemm_f32"] * 3),
    # dx at F = H = 256: fp32 on the 8-group kernel as eight partial tapes and a reduce, bf16 inside the kernel; else a product last
    (256, 144, {"F": 256, "need_dx": True}, ["8-group BPTT", "splitk_reduce", "wgrad_rows"]),
    (256, 144, {"F": 256, "need_dx": True, "dtype": "bf16"}, ["8-group BPTT"] + DB_SUM + BF16_PRODUCTS),
    (256, 144, {"F": 256, "need_dx": True, "env": {"FOV_NO_DX_FUSION": "1"}}, ["8-group BPTT", "wgrad_rows"] + GS),
    (256, 144, {"F": 256, "need_dx": True, "dtype": "bf16", "env": {"FOV_NO_DX_FUSION": "1"}},
     ["8-group BPTT"] + DB_SUM + BF16_PRODUCTS + ["gemm_bf16_nt"]),
    (256, 144, {"F": 256, "need_dx": True, "off": ("K",)}, ["8-group BPTT", "wgrad_rows"] + GS),
    (256, 144, {"F": 256, "need_dx": True, "dtype": "bf16", "off": ("K",)}, ["8-group BPTT"] + DB_SUM + BF16_PRODUCTS + GS),
    (256, 144, {"F": 256}, ["8-group BPTT", "wgrad_rows"]),
    (256, 16, {"F": 256, "need_dx": True}, ["16-unit BPTT", "wgrad_rows"] + GS),
]


def backward_id(row):
    H, B, cond = row[:3]
    extra = "-".join("%s=%s" % (k, "+".join(v) if isinstance(v, (dict, tuple)) else v) for k, v in sorted(cond.items()))
    return "H%d-B%d%s" % (H, B, "-" + extra if extra else "")


@pytest.mark.parametrize("H,B,cond,want", BACKWARD, ids=[backward_id(r) for r in BACKWARD])
def test_layer_backward_launches(capfd, H, B, cond, want):
    out, ran = run_backward(capfd, H, B, **cond)
    assert ran == want, ran
    assert (out["dx"] is not None) == bool(cond.get("need_dx"))


def test_two_layer_backward_launch(capfd):
    """Width 512, at most 32 sequences: both recurrences in one launch, all six weight gradients in a second."""
    from longterm360fov_amd import ops
    assert ops.lstm_stack2_bwd_supported(32, T_IN, 6, 512) and not ops.lstm_stack2_bwd_supported(48, T_IN, 6, 512)
    out, ran = run_stack2_backward(capfd, 512, 32)
    assert ran == ["two-layer BPTT", "wgrad_rows"], ran


# H, B, the other arguments of run_wgrad_pair, the launches: one for both layers where the rows form takes both, else each layer's own
WGRAD_PAIR = [
    (256, 16, {}, ["wgrad_rows"]),
    (256, 256, {}, GS + GS + GS + DB_SUM + ["wgrad_rows"]),
    (256, 16, {"dz2_off": True}, ["wgrad_rows", "gemm_f32"] + GS + ["gemm_f32"] + DB_SUM),
    (512, 256, {}, ["wgrad_group", "wgrad_rows"]),
]


@pytest.mark.parametrize("H,B,cond,want", WGRAD_PAIR, ids=[backward_id(r) for r in WGRAD_PAIR])
def test_wgrad_pair_launches(capfd, H, B, cond, want):
    out, ran = run_wgrad_pair(capfd, H, B, **cond)
    assert ran == want, ran


def test_cluster_on_request_refuses_a_shape_it_does_not_take(capfd):
    """impl = cluster is a demand, not a preference: a width the cluster kernel does not have comes back FOV_ERR_UNSUPPORTED
    with the launcher's own message and nothing is launched - no silent fallback."""
    from longterm360fov_amd import ops
    with pytest.raises(ops.FovError, match=r"cluster kernel supports H in \{64,128,256\}") as e:
        run_decode(capfd, 512, 16, impl="cluster", F_enc=128)
    assert e.value.code == _lib.ERR_UNSUPPORTED
    reload_env()        # (the knobs went back when the call raised; the library has not re-read them yet)
    assert launches(capfd.readouterr().err) == []
