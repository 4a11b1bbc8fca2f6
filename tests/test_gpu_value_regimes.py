"""The LSTM / ConvLSTM kernels where their VALUES leave the linear regime: clamped hard_sigmoid gates, saturated sigmoid / tanh,
arguments at which exp overflows or flushes, exact zeros, inputs of order 1e-6, and a cell state that grows over 256 steps.

Every other GPU test draws Glorot / orthogonal weights and inputs in (-1, 1): a gate pre-activation has a standard deviation near
0.3, nothing is ever clamped or saturated and |c| stays below 2.  Here the cases come from oracle/fov_oracle.py's value-regime
generator (regime_lstm and the model builders next to it; the shares it promises are asserted on the CPU in tests/test_oracle.py
for every case table of this file):
  R1 clamped       hard_sigmoid, about 45 % of the i / f / o pre-activations beyond +-2.5
  R2 saturated     sigmoid, 40 % of the gate pre-activations beyond +-17, 65 % of g's and 30 % of c's beyond +-9
  R3 overflow      R2 plus three rows of the first tile whose every pre-activation lies beyond +-100 / +-200 (one of them from
                   mid-sequence on), and a second batch with a zero bias whose second tile is all zero and whose last tile holds
                   inputs of order 1e-6
  R4 accumulating  forget gate at exactly 1, i * g of one sign per unit, T = 256: max |c| passes 200

Reference: the fp64 oracle.  The BACKWARD reference consumes the tape the GPU forward wrote (cast to fp64), so that both sides take
the same branch of hard_sigmoid's derivative at every element; the tape itself is compared with the oracle's (values are
continuous at the kink).  No element is left out of any comparison.

Bounds: the project's written ones (regime_error in the oracle states them as weights: 1e-3 |ref| + 1e-5 and 2e-5 max(1, |ref|) for
fp32 values; 1e-4 of a gradient's scale; bf16 against the bf16-operand restatement: 1e-3 max(1, |ref|), gradients 1e-3 / 2e-3 of
scale).  Where fp32 arithmetic itself may miss them the yardstick is the oracle evaluated twice on the CPU - in fp64 and on fp32
arrays; e_ref is their disagreement in written bounds, and the asserted bound is max(1, 8 e_ref) written bounds (8: fov_common.h
documents 3e-7 for tanh_f / sigmoid_f against NumPy's half ulp of 6e-8, rounded up to a power of two).  8 e_ref never passes 10
(asserted here and on the CPU).  Every check prints e_ref, the bound and the GPU's error.  The bf16 cases keep x K at its ordinary
spread of 0.3 (the bias, added in fp32 and never rounded, carries the regime) and their outputs in (-1, 1) are also held to the
FULL-precision oracle, per element: 5e-3 (LOOSE of test_gpu_bf16.py) plus the distance the bf16-operand restatement itself keeps
from it there - 7e-4 .. 1e-2 over the cases, 0.38 in the decoder's overflowing row (check_loose).

Exact properties, without tolerance: everything finite, |h| <= 1, stored gates in [0, 1], g in [-1, 1]; R1: a hard_sigmoid gate whose
fp64 pre-activation lies beyond +-(2.5 + 1e-3) is stored as exactly 1.0 / 0.0 and its dz is exactly 0.0; R3: beyond +-100 the
stored gates and g are exactly saturated, the tile-mates of the extreme rows are bit-identical to a run without them, the all-zero
tile returns exact zeros for g, c and h; the T = 256 runs repeat bit for bit; Workspace.check() / Scratch.check() are clean.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

pytestmark = pytest.mark.gpu

# ---- case tables (tests/test_oracle.py walks the same tables) -------------------------------------------------------------
# (impl, H, knobs) of ops.lstm_seq / ops.lstm_seq_train, F = 90.  Width 512: lstm_wide16.hip (thirty-two workgroups per tile at these
# batches) and, with FOV_NO_WIDE16=1, the sixteen-workgroup form of lstm_wide.hip
LAYER_FORWARD = [("cluster", 64, {}), ("cluster", 128, {}), ("cluster", 256, {}), ("generic", 256, {}), ("auto", 512, {}),
                 ("auto", 512, {"FOV_NO_WIDE16": "1"})]
LAYER_SHAPE = {"R1": [(37, 8)], "R2": [(37, 8)], "R3": [(37, 8)], "R4": [(16, 256), (21, 256)]}          # (B, T)
# (name, H, knobs, dtype): which BPTT kernel ops.lstm_seq_bwd takes at three tiles (lstm_train.hip, lstm_seq_bwd)
BACKWARD_FORMS = [
    ("bwd_cluster-64", 64, {}, "f32"),
    ("bwd_cluster-128", 128, {"FOV_NO_BWD16_NARROW": "1"}, "f32"),
    ("bwd_cluster-256", 256, {"FOV_NO_BWD16_NARROW": "1", "FOV_BWD_GROUPS4": "1"}, "f32"),
    ("bwd8-256", 256, {"FOV_NO_BWD16_NARROW": "1"}, "f32"),
    ("bwd16-128", 128, {}, "f32"),
    ("bwd16-256", 256, {}, "f32"),
    ("bwd16-512", 512, {}, "f32"),
    ("bwd16-512-groups32", 512, {"FOV_BWD16_GROUPS": "32"}, "f32"),
    ("stepped-256", 256, {"FOV_BWD_STEPPED": "1"}, "f32"),
    ("bwd8-256-bf16", 256, {}, "bf16"),
]
BACKWARD_SHAPE = {"R1": (37, 8), "R2": (37, 8), "R3": (37, 8), "R4": (16, 256)}
# (regime, B, T, recurrent gain, seed offset).  The bf16 cases keep x K at its ordinary spread (O.BF16_XK): the bias carries the regime.
# Gain 4: one bf16 ulp of h moves a pre-activation four times as far; the seed is the ordinary one.
BF16_LAYER = [("R1", 37, 8, 1.0, 0), ("R2", 37, 8, 1.0, 0), ("R3", 37, 8, 1.0, 0), ("R4", 16, 256, 1.0, 0), ("R1", 37, 8, 4.0, 0)]
DECODE = [("R1", 32, "f32", "auto"), ("R2", 32, "f32", "auto"), ("R1", 48, "f32", "auto"), ("R2", 48, "f32", "auto"),
          ("R1", 32, "f32", "cluster"), ("R2", 48, "f32", "cluster"), ("R1", 1000, "f32", "auto"),
          ("R1", 32, "bf16", "auto"), ("R2", 32, "bf16", "auto"), ("R1", 48, "bf16", "auto"), ("R2", 48, "bf16", "auto")]
DECODE_T = (8, 8)
STACK2 = [("R1", 512), ("R2", 512), ("R3", 512)]            # B 32, T 10, F 90
STACK2_SHAPE = (32, 10, 90)
STACK2_BF16 = ["R1", "R2", "R3"]                            # ops.lstm_stack2_bf16: H 256, zero initial states, same shape
TF_STACK = ["R2", "R3"]                                     # StackedTFLSTM, 400 units padded to 512 (tf.contrib cells: sigmoid)
MIX = [(r, d) for r in ("R1", "R2", "R3") for d in ("f32", "bf16")]
MIX_SHAPE = (37, 8, 6)
CONV = [((3, 36, 18, 32, 32, 5), "hard_sigmoid"), ((3, 36, 18, 32, 32, 5), "sigmoid"),
        ((1, 7, 4, 17, 20, 3), "hard_sigmoid"), ((1, 7, 4, 17, 20, 3), "sigmoid")]


def layer_seed(H, regime, B):
    return 1000 + H + 7 * O.REGIMES.index(regime) + B


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def d64(a):
    return None if a is None else (host(a) if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float64)


@contextlib.contextmanager
def knobs(env):
    before = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in before.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def check(tag, got, ref, kind, e_ref):
    """|got - ref| in written bounds <= max(1, 8 e_ref); 8 e_ref <= 10.  Prints the three figures."""
    got = d64(got)
    assert np.isfinite(got).all(), tag + ": non-finite values"
    err, bound = O.regime_error(got, ref, kind), O.regime_bound(e_ref)
    worst = np.unravel_index(int(np.argmax(np.abs(got - ref))), got.shape) if got.size else ()
    print("%-58s e_ref %.3g  bound %.3g  gpu %.3g  (written bounds, %s; max|ref| %.3g; largest |error| at %s)"
          % (tag, e_ref, bound, err, kind, float(np.abs(ref).max()) if np.size(ref) else 0.0, tuple(int(i) for i in worst)))
    assert O.REGIME_YARDSTICK * e_ref <= O.REGIME_YARDSTICK_CAP, (tag, e_ref)
    assert err <= bound, "%s: %.3g written bounds, allowed %.3g" % (tag, err, bound)


LOOSE = 5e-3        # test_gpu_bf16.py: bf16 outputs in (-1, 1) against the FULL-precision oracle


def check_loose(tag, got, restatement, full):
    """bf16 against the full-precision oracle, per element: |got - full| <= 5e-3 + |restatement - full|, the distance the
    bf16-operand restatement itself keeps from it (with the spread on the bias that distance is of the size of 5e-3 itself, not
    the 3e-2 of a wide x K).  Prints both."""
    got, restatement, full = d64(got), np.asarray(restatement, np.float64), np.asarray(full, np.float64)
    own = np.abs(restatement - full)
    err = np.abs(got - full)
    print("%-58s against the full-precision oracle %.2e; the bf16-operand restatement itself %.2e" % (tag, err.max(), own.max()))
    assert (err <= LOOSE + own).all(), "%s: %.3g beyond 5e-3 + the restatement's own distance" % (tag, (err - own).max())


def exact_gate_properties(tag, res, z64, act, overflow=None):
    """res (..., 5, H) stored i, f, g, o, c and their fp64 pre-activations z64 (..., 4H): ranges, and exact saturation where z64
    lies beyond the clamp by 1e-3 (hard_sigmoid) or beyond +-100.  overflow: an index into the leading axes whose elements must
    hold arguments beyond +-200 of both signs."""
    H = res.shape[-1]
    for q, name in ((0, "i"), (1, "f"), (3, "o")):
        a, z = res[..., q, :], z64[..., q * H:(q + 1) * H]
        assert a.min() >= 0.0 and a.max() <= 1.0, (tag, name)
        far = 2.5 + 1e-3 if act == "hard_sigmoid" else 100.0
        hi, lo = z > far, z < -far
        assert (a[hi] == 1.0).all() and (a[lo] == 0.0).all(), (tag, name, "not exactly saturated")
        if act == "hard_sigmoid":
            assert hi.sum() > 0 and lo.sum() > 0, (tag, name)
        if overflow is not None:
            zr = z[overflow]
            assert (zr > 200).sum() > 0 and (zr < -200).sum() > 0, (tag, name, "no overflowing argument in the extreme rows")
    g, zg = res[..., 2, :], z64[..., 2 * H:3 * H]
    assert np.abs(g).max() <= 1.0, tag
    assert (g[zg > 100] == 1.0).all() and (g[zg < -100] == -1.0).all(), (tag, "g not exactly saturated")


def tensors(hs, hT, cT, res):
    """numpy fp32 views of a layer's outputs keyed like O.regime_forward_tensors."""
    return O.regime_forward_tensors(host(hs), host(hT), host(cT), host(res))


def exact_forward_properties(tag, t, z64, act, expect_overflow_rows=None):
    """Ranges, and exact saturation where the fp64 pre-activation z64 (B,T,4H) is far beyond the clamp / the overflow."""
    H = t["hs"].shape[-1]
    for k, v in t.items():
        assert np.isfinite(v).all(), (tag, k)
    assert np.abs(t["hs"]).max() <= 1.0 and np.abs(t["hT"]).max() <= 1.0, tag
    if "i" in t:
        res = np.stack([t[n] for n in "ifgoc"], axis=-2)
        exact_gate_properties(tag, res, z64, act, expect_overflow_rows)


def run_layer(ops, p, x, b, state, impl, dtype, ws):
    h0, c0 = (dev(p["h0"]), dev(p["c0"])) if state else (None, None)
    if dtype == "bf16":
        out = ops.lstm_seq_bf16(dev(x), dev(p["K"]), dev(p["R"]), dev(b), h0, c0, act=p["act"], workspace=ws)
    else:
        out = ops.lstm_seq_train(dev(x), dev(p["K"]), dev(p["R"]), dev(b), h0, c0, act=p["act"], impl=impl, workspace=ws)
    ws.check()
    return out


def layer_forward_case(ops, p, impl, dtype, tag):
    """One layer case, forward: parity of hs, hT, cT and the tape, the exact properties, and the regime's own extras."""
    bf = dtype == "bf16"
    regime, act = p["regime"], p["act"]
    ws = ops.Workspace()
    out = run_layer(ops, p, p["x"], p["b"], True, impl, dtype, ws)
    t = tensors(*out)
    ref, e_ref = O.regime_forward_reference(p, bf16=bf)
    for k in ref:
        check("%s %s" % (tag, k), t[k], ref[k], "bf16" if bf else "f32", e_ref[k])
    if bf:
        full, _ = O.regime_forward_reference(p)
        for k in ("hs", "hT"):
            check_loose("%s %s" % (tag, k), t[k], ref[k], full[k])
    z64 = O.regime_preactivations(d64(p["x"]), d64(p["K"]), d64(p["R"]), d64(p["b"]), ref["hs"], d64(p["h0"]), bf16=bf)
    exact_forward_properties(tag, t, z64, act, p.get("extreme")[:2] if regime == "R3" else None)
    np.testing.assert_array_equal(t["c"][:, -1], t["cT"])
    if not bf:      # the inference entry point of the same kernel family
        hs, hT, cT = ops.lstm_seq(dev(p["x"]), dev(p["K"]), dev(p["R"]), dev(p["b"]), dev(p["h0"]), dev(p["c0"]), act=act, impl=impl,
                                  workspace=ws)
        ws.check()
        for k, v in (("hs", hs), ("hT", hT), ("cT", cT)):
            check("%s lstm_seq %s" % (tag, k), v, ref[k], "f32", e_ref[k])
    if regime == "R4":
        again = tensors(*run_layer(ops, p, p["x"], p["b"], True, impl, dtype, ws))
        for k in t:
            np.testing.assert_array_equal(again[k], t[k], err_msg="%s %s: not repeatable" % (tag, k))
        assert np.abs(t["c"]).max() > 50
    if regime == "R3":
        # the extreme rows' tile-mates do not see them
        rows = p["extreme"]
        calm = p["x"].copy()
        calm[rows] = 0
        t2 = tensors(*run_layer(ops, p, calm, p["b"], True, impl, dtype, ws))
        mates = np.setdiff1d(np.arange(p["x"].shape[0]), rows)
        for k in t:
            np.testing.assert_array_equal(t2[k][mates], t[k][mates], err_msg="%s %s: tile-mates of the extreme rows moved" % (tag, k))
        # zero bias: the all-zero tile and the tile of 1e-6 inputs
        te = tensors(*run_layer(ops, p, p["x_edge"], p["b_edge"], False, impl, dtype, ws))
        for k in ("g", "c", "hs"):
            assert (te[k][16:32] == 0).all(), (tag, k, "the all-zero tile is not exactly zero")
        assert (te["hT"][16:32] == 0).all() and (te["cT"][16:32] == 0).all(), tag
        ref_e, e_ref_e = O.regime_forward_reference(p, bf16=bf, x=p["x_edge"], b=p["b_edge"])
        for k in ref_e:
            check("%s edge batch %s" % (tag, k), te[k], ref_e[k], "bf16" if bf else "abs", e_ref_e[k])


# ---------------------------------------------------------------------------------------------------------------------
# one layer, forward: lstm_cluster (H 64 / 128 / 256), lstm_generic, lstm_layer_bf16
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", O.REGIMES)
@pytest.mark.parametrize("impl,H,env", LAYER_FORWARD)
def test_layer_forward_in_value_regimes(impl, H, env, regime):
    from longterm360fov_amd import ops
    for B, T in LAYER_SHAPE[regime]:
        p = O.regime_lstm(layer_seed(H, regime, B), 90, H, regime, B, T)
        with knobs(env):
            layer_forward_case(ops, p, impl, "f32", "%s%s H%d %s B%d T%d" % (impl, " no-wide16" if env else "", H, regime, B, T))


@pytest.mark.parametrize("regime,B,T,r_gain,seed", BF16_LAYER)
def test_bf16_layer_forward_in_value_regimes(regime, B, T, r_gain, seed):
    from longterm360fov_amd import ops
    p = O.regime_lstm(layer_seed(256, regime, B) + seed, 90, 256, regime, B, T, r_gain=r_gain, xk=O.BF16_XK)
    layer_forward_case(ops, p, "auto", "bf16", "bf16 layer %s B%d T%d gain %g" % (regime, B, T, r_gain))


# ---------------------------------------------------------------------------------------------------------------------
# one layer, backward: every BPTT kernel behind ops.lstm_seq_bwd
# ---------------------------------------------------------------------------------------------------------------------
def exact_zero_gradient_at_the_clamp(tag, res, dz, z64, H):
    """R1: where the fp64 pre-activation of a hard_sigmoid gate lies beyond +-(2.5 + 1e-3) the stored gate is exactly 0 / 1
    and its dz exactly 0."""
    far = 2.5 + 1e-3
    for q in (0, 1, 3):
        z = z64[..., q * H:(q + 1) * H]
        out = np.abs(z) > far
        a, d = res[:, :, q][out], dz[..., q * H:(q + 1) * H][out]
        assert out.mean() > 0.25, (tag, q)
        assert ((a == 0.0) | (a == 1.0)).all(), (tag, q, "clamped gate not stored exactly")
        assert (d == 0.0).all(), (tag, q, "dz of a clamped gate is not exactly zero: %d of %d" % ((d != 0).sum(), d.size))
        inside = np.abs(z) < 2.5 - 1e-3        # (an element's dc is itself exactly zero where o and the next f are both clamped at 0)
        assert (dz[..., q * H:(q + 1) * H][inside] != 0.0).mean() > 0.5, (tag, q, "the linear piece has no gradient")


@pytest.mark.parametrize("regime", O.REGIMES)
@pytest.mark.parametrize("name,H,env,dtype", BACKWARD_FORMS)
def test_layer_backward_in_value_regimes(name, H, env, dtype, regime):
    """Every gradient ops.lstm_seq_bwd returns (dz, dx, dK, dR, db, dh0, dc0) on the GPU's own tape."""
    from longterm360fov_amd import ops
    bf = dtype == "bf16"
    B, T = BACKWARD_SHAPE[regime]
    F = 90 if bf else 11
    p = O.regime_lstm(layer_seed(H, regime, B) + 1, F, H, regime, B, T, xk=O.BF16_XK if bf else None)
    act = p["act"]
    tag = "%s %s B%d T%d" % (name, regime, B, T)
    ws = ops.Workspace()
    hs, hT, cT, res = ops.lstm_seq_train(dev(p["x"]), dev(p["K"]), dev(p["R"]), dev(p["b"]), dev(p["h0"]), dev(p["c0"]), act=act,
                                         workspace=ws, dtype=dtype)
    ws.check()
    ref_f, e_f = O.regime_forward_reference(p, bf16=bf)
    t = tensors(hs, hT, cT, res)
    for k in ref_f:
        check("%s tape %s" % (tag, k), t[k], ref_f[k], "bf16" if bf else "f32", e_f[k])
    if bf:
        check_loose("%s tape hs" % tag, t["hs"], ref_f["hs"], O.regime_forward_reference(p)[0]["hs"])
    ups = O.regime_upstream(layer_seed(H, regime, B) + 2, B, T, H)

    def run():
        with knobs(env):
            sc = ops.Scratch()
            g = ops.lstm_seq_bwd(dev(p["x"]), dev(p["K"]), dev(p["R"]), hs, res, h0=dev(p["h0"]), c0=dev(p["c0"]), dhs=dev(ups[0]),
                                 dhT=dev(ups[1]), dcT=dev(ups[2]), need_dx=True, need_state_grads=True, act=act, scratch=sc, dtype=dtype)
            sc.check()
        return {k: host(g[k]) for k in O.GRAD_KEYS}
    got = run()
    ref = O.regime_backward_reference(p, host(hs), host(res), ups, bf16=bf)
    e_ref = O.regime_backward_e_ref(p, ups, bf16=bf)
    tol = O.regime_grad_bounds(bf)
    for k in O.GRAD_KEYS:
        check("%s %s" % (tag, k), got[k], ref[k], tol[k], e_ref[k])
    if regime == "R1":
        z64 = O.regime_preactivations(d64(p["x"]), d64(p["K"]), d64(p["R"]), d64(p["b"]), ref_f["hs"], d64(p["h0"]), bf16=bf)
        exact_zero_gradient_at_the_clamp(tag, host(res), got["dz"], z64, H)
    if regime == "R4":
        again = run()
        for k in O.GRAD_KEYS:
            np.testing.assert_array_equal(again[k], got[k], err_msg="%s %s: not repeatable" % (tag, k))


# ---------------------------------------------------------------------------------------------------------------------
# fused encoder + free-running decoder: wide16_s2s, the cluster decoder, lstm_s2s_bf16
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime,B,dtype,impl", DECODE)
def test_seq2seq_decode_in_value_regimes(regime, B, dtype, impl):
    """Encoder and DECODER weights in R1 / R2 and a Dense head whose fed-back tanh output saturates (a third of its arguments
    beyond +-9): out, and the decoder's final state."""
    from longterm360fov_amd import ops
    bf = dtype == "bf16"
    T_in, T_out = DECODE_T
    w, enc, dec0, act = O.regime_seq2seq(50 + B, regime, B, T_in, xk=O.BF16_XK if bf else None)
    ws = ops.Workspace()
    hT, cT = torch.empty((B, 256), device="cuda"), torch.empty((B, 256), device="cuda")
    kw = {"dtype": "bf16"} if bf else {"impl": impl}
    out = ops.seq2seq_decode(dev(enc), dev(dec0), {k: dev(v) for k, v in w.items()}, T_out, act=act, workspace=ws, hT=hT, cT=cT, **kw)
    ws.check()
    r64 = O.regime_decode(enc, dec0, w, T_out, act, bf, np.float64)
    r32 = O.regime_decode(enc, dec0, w, T_out, act, bf, np.float32)
    kind = "bf16" if bf else "f32"
    tag = "decode %s %s B%d %s" % (dtype, impl, B, regime)
    for k, v in (("out", out), ("hT", hT), ("cT", cT)):
        check("%s %s" % (tag, k), v, r64[k], kind, O.regime_error(r32[k], r64[k], kind))
    if bf:
        full = O.regime_decode(enc, dec0, w, T_out, act, False, np.float64)
        check_loose("%s out" % tag, out, r64["out"], full["out"])
        check_loose("%s hT" % tag, hT, r64["hT"], full["hT"])
    got = host(out)
    assert np.abs(got).max() <= 1.0 and np.abs(host(hT)).max() <= 1.0
    hi, lo = r64["pre"] > 10.5, r64["pre"] < -10.5        # 2 / (1 + e^21) is far below half an ulp of 1
    assert hi.sum() > 0 and lo.sum() > 0 and (got[hi] == 1.0).all() and (got[lo] == -1.0).all(), tag
    if B == 1000:       # the persistent tile loop: a sequence does not depend on its place in the batch
        perm = np.random.default_rng(1).permutation(B)
        out_p = ops.seq2seq_decode(dev(enc[perm]), dev(dec0[perm]), {k: dev(v) for k, v in w.items()}, T_out, act=act, workspace=ws, **kw)
        ws.check()
        np.testing.assert_array_equal(host(out_p), got[perm])


# ---------------------------------------------------------------------------------------------------------------------
# two stacked width-512 layers: lstm_stack2 (forward, tape, backward) and 400 units padded (StackedTFLSTM)
# ---------------------------------------------------------------------------------------------------------------------
def stack2_case(regime, H):
    B, T, F = STACK2_SHAPE
    layers, x, st, act, p1 = O.regime_stack2(70 + O.REGIMES.index(regime), regime, B, T, F, H)
    dl = [tuple(dev(a) for a in l) for l in layers]
    dst = [None if s is None else (dev(s[0]), dev(s[1])) for s in st]
    return layers, x, st, act, p1, dl, dst


@pytest.mark.parametrize("regime,H", STACK2)
def test_stack2_forward_in_value_regimes(regime, H):
    from longterm360fov_amd import ops
    B, T, F = STACK2_SHAPE
    layers, x, st, act, p1, dl, dst = stack2_case(regime, H)
    assert ops.lstm_stack2_supported(B, T, F, H)
    ws = ops.Workspace()
    o1, o2 = ops.lstm_stack2(dev(x), dl[0], dl[1], dst[0], dst[1], act=act, workspace=ws, reserve=True)
    ws.check()
    f64 = O.regime_stack2_forward(layers, x, st, act, np.float64)
    f32 = O.regime_stack2_forward(layers, x, st, act, np.float32)
    tag = "stack2 %s" % regime
    inp64 = d64(x)
    for l, o in enumerate((o1, o2)):
        t, r64, r32 = tensors(*o), O.regime_forward_tensors(*f64[l]), O.regime_forward_tensors(*f32[l])
        for k in r64:
            check("%s layer %d %s" % (tag, l + 1, k), t[k], r64[k], "f32", O.regime_error(r32[k], r64[k], "f32"))
        K, R, b = (d64(a) for a in layers[l])
        z64 = O.regime_preactivations(inp64, K, R, b, r64["hs"], None if st[l] is None else d64(st[l][0]))
        exact_forward_properties("%s layer %d" % (tag, l + 1), t, z64, act, p1["extreme"][:2] if (regime == "R3" and l == 0) else None)
        inp64 = r64["hs"]
    if regime == "R3":
        calm = x.copy()
        calm[p1["extreme"]] = 0
        c1, c2 = ops.lstm_stack2(dev(calm), dl[0], dl[1], dst[0], dst[1], act=act, workspace=ws, reserve=True)
        ws.check()
        mates = np.setdiff1d(np.arange(B), p1["extreme"])
        for a, b_ in ((o1, c1), (o2, c2)):
            for k in range(4):
                np.testing.assert_array_equal(host(a[k])[mates], host(b_[k])[mates])
        zb = [(dl[l][0], dl[l][1], torch.zeros_like(dl[l][2])) for l in range(2)]
        e1, e2 = ops.lstm_stack2(dev(p1["x_edge"]), zb[0], zb[1], None, None, act=act, workspace=ws, reserve=True)
        ws.check()
        for e in (e1, e2):
            te = tensors(*e)
            for k in ("g", "c", "hs", "hT", "cT"):
                assert (te[k][16:32] == 0).all(), (tag, k)
            assert all(np.isfinite(v).all() for v in te.values())


@pytest.mark.parametrize("regime,H", STACK2)
def test_stack2_backward_in_value_regimes(regime, H):
    """fov_lstm_stack2_bwd on the tapes of the one-launch forward: both layers' dz, weight and state gradients."""
    from longterm360fov_amd import ops
    B, T, F = STACK2_SHAPE
    if not ops.lstm_stack2_bwd_supported(B, T, F, H):
        pytest.skip("the one-launch BPTT of two layers needs 3 x 16 workgroups per tile resident")
    layers, x, st, act, p1, dl, dst = stack2_case(regime, H)
    ws = ops.Workspace()
    o1, o2 = ops.lstm_stack2(dev(x), dl[0], dl[1], dst[0], dst[1], act=act, workspace=ws, reserve=True)
    ws.check()
    f64 = O.regime_stack2_forward(layers, x, st, act, np.float64)
    f32 = O.regime_stack2_forward(layers, x, st, act, np.float32)
    tag = "stack2 %s" % regime
    ups = O.regime_stack2_upstream(80, B, T, H)
    e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    g1, g2 = (e(F, 4 * H), e(H, 4 * H), e(4 * H)), (e(H, 4 * H), e(H, 4 * H), e(4 * H))
    h0 = lambda l, q: None if dst[l] is None else dst[l][q]
    sc = ops.Scratch()
    got = ops.lstm_stack2_bwd(dev(x), dl[0][:2], dl[1][:2], (o1[0], o1[3], h0(0, 0), h0(0, 1)), (o2[0], o2[3], h0(1, 0), h0(1, 1)),
                              dhs2=dev(ups[0]), dhT2=dev(ups[1]), dcT2=dev(ups[2]), dhT1=dev(ups[3]), dcT1=dev(ups[4]), grads1=g1,
                              grads2=g2, need_state_grads=True, act=act, scratch=sc)
    sc.check()
    got.update(dK1=g1[0], dR1=g1[1], db1=g1[2], dK2=g2[0], dR2=g2[1], db2=g2[2])
    gpu_tapes = [(host(o1[0]), host(o1[3])), (host(o2[0]), host(o2[3]))]
    ref = O.regime_stack2_backward(layers, x, st, gpu_tapes, ups, act, np.float64)
    cpu_tapes = [(f32[0][0], f32[0][3]), (f32[1][0], f32[1][3])]
    y64 = O.regime_stack2_backward(layers, x, st, cpu_tapes, ups, act, np.float64)
    y32 = O.regime_stack2_backward(layers, x, st, cpu_tapes, ups, act, np.float32)
    for k in ref:
        check("%s bwd %s" % (tag, k), got[k], ref[k], 1e-4, O.regime_error(y32[k], y64[k], 1e-4))
    if regime == "R1":
        inp64 = d64(x)
        for l, n in ((0, "1"), (1, "2")):
            K, R, b = (d64(a) for a in layers[l])
            z64 = O.regime_preactivations(inp64, K, R, b, f64[l][0], None if st[l] is None else d64(st[l][0]))
            exact_zero_gradient_at_the_clamp("%s layer %s" % (tag, n), gpu_tapes[l][1], host(got["dz" + n]), z64, H)
            inp64 = f64[l][0]


@pytest.mark.parametrize("regime", STACK2_BF16)
def test_stack2_bf16_forward_in_value_regimes(regime):
    """lstm_stack2_bf16 (two bf16 layers of width 256 as one wavefront launch, zero initial states): both layers' hs, final state
    and tape against the bf16-operand restatement."""
    from longterm360fov_amd import ops
    B, T, F = STACK2_SHAPE
    H = 256
    layers, x, st, act, p1 = O.regime_stack2(75 + O.REGIMES.index(regime), regime, B, T, F, H, state=False, xk=O.BF16_XK)
    assert ops.lstm_stack2_bf16_supported(B, T, F, H)
    dl = [tuple(dev(a) for a in l) for l in layers]
    ws = ops.Workspace()
    o1, o2 = ops.lstm_stack2_bf16(dev(x), dl[0], dl[1], act=act, workspace=ws)
    ws.check()
    f64 = O.regime_stack2_forward(layers, x, st, act, np.float64, bf16=True)
    f32 = O.regime_stack2_forward(layers, x, st, act, np.float32, bf16=True)
    full = O.regime_stack2_forward(layers, x, st, act, np.float64)
    inp64 = d64(x)
    for l, o in enumerate((o1, o2)):
        tag = "stack2 bf16 %s layer %d" % (regime, l + 1)
        t, r64, r32 = tensors(*o), O.regime_forward_tensors(*f64[l]), O.regime_forward_tensors(*f32[l])
        for k in r64:
            check("%s %s" % (tag, k), t[k], r64[k], "bf16", O.regime_error(r32[k], r64[k], "bf16"))
        check_loose("%s hs" % tag, t["hs"], r64["hs"], full[l][0])
        K, R, b = (d64(a) for a in layers[l])
        z64 = O.regime_preactivations(inp64, K, R, b, r64["hs"], None, bf16=True)
        exact_forward_properties(tag, t, z64, act, p1["extreme"][:2] if (regime == "R3" and l == 0) else None)
        inp64 = r64["hs"]
    if regime == "R3":
        calm = x.copy()
        calm[p1["extreme"]] = 0
        c1, c2 = ops.lstm_stack2_bf16(dev(calm), dl[0], dl[1], act=act, workspace=ws)
        ws.check()
        mates = np.setdiff1d(np.arange(B), p1["extreme"])
        for a, b_ in ((o1, c1), (o2, c2)):
            for k in range(4):
                np.testing.assert_array_equal(host(a[k])[mates], host(b_[k])[mates])
        zb = [(dl[l][0], dl[l][1], torch.zeros_like(dl[l][2])) for l in range(2)]
        e1, e2 = ops.lstm_stack2_bf16(dev(p1["x_edge"]), zb[0], zb[1], act=act, workspace=ws)
        ws.check()
        for e in (e1, e2):
            te = tensors(*e)
            for k in ("g", "c", "hs", "hT", "cT"):
                assert (te[k][16:32] == 0).all(), (regime, k)
            assert all(np.isfinite(v).all() for v in te.values())


@pytest.mark.parametrize("regime", TF_STACK)
def test_padded_400_unit_stack_in_value_regimes(regime):
    """MultiRNNCell[2 x LSTMCell(400)] zero-padded to width 512 on the persistent kernels, fed state, regime weights mapped to
    tf.contrib's gate order (keras_to_tf_cell): the padding units must stay exactly idle next to saturated neighbours.  R2 and R3
    only: tf.contrib's cell has no hard_sigmoid."""
    from longterm360fov_amd.models import StackedTFLSTM
    B, T, F, H = 32, 10, 90, 400
    layers, x, st, act, p1 = O.regime_stack2(90 + O.REGIMES.index(regime), regime, B, T, F, H)
    assert act == "sigmoid"
    cells = [O.keras_to_tf_cell(*l) for l in layers]
    st0 = np.stack([np.stack([s[1], s[0]]) for s in st]).astype(np.float32)             # (L, 2, B, H): [l, 0] = c, [l, 1] = h
    m = StackedTFLSTM(cells)
    assert m.run_width == 512
    out, state = (d64(a) for a in m.predict(x, st0))
    c64 = lambda dt: [(W.astype(dt), b.astype(dt)) for W, b in cells]
    r64 = O.tf_dynamic_rnn(x.astype(np.float64), c64(np.float64), st0.astype(np.float64))
    r32 = O.tf_dynamic_rnn(x.astype(np.float32), c64(np.float32), st0)
    check("tf stack 400 %s states_series" % regime, out, r64[0], "f32", O.regime_error(r32[0], r64[0], "f32"))
    check("tf stack 400 %s current_state" % regime, state, r64[1], "f32", O.regime_error(r32[1], r64[1], "f32"))
    assert np.abs(out).max() <= 1.0
    if regime == "R3":
        calm = x.copy()
        calm[p1["extreme"]] = 0
        out2, state2 = (d64(a) for a in m.predict(calm, st0))
        mates = np.setdiff1d(np.arange(B), p1["extreme"])
        np.testing.assert_array_equal(out2[mates], out[mates])
        np.testing.assert_array_equal(state2[:, :, mates], state[:, :, mates])
        # zero biases (the cell adds its forget_bias of 1 to a stored -1), zero state: the all-zero tile
        edge = StackedTFLSTM([O.keras_to_tf_cell(K, R, np.zeros_like(b)) for K, R, b in layers])
        out3, state3 = (d64(a) for a in edge.predict(p1["x_edge"]))
        assert (out3[16:32] == 0).all() and (state3[:, :, 16:32] == 0).all() and np.isfinite(out3).all() and np.isfinite(state3).all()


# ---------------------------------------------------------------------------------------------------------------------
# the fused others-mixing decoder: mix_decoder / mix_decoder_bf16 and their BPTT kernels
# ---------------------------------------------------------------------------------------------------------------------
def run_mix_decoder(ops, w, mix_Wp, st, dec0, oth, act, dtype, T):
    """mix_decoder(train=...) -> (tapes keyed M, P, H1, C1, H2, C2, res1, res2 as device tensors, C1 / C2 with their initial row)."""
    B, H = st[0].shape
    O_ = dec0.shape[1]
    e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    C1, C2 = e(T + 1, B, H), e(T + 1, B, H)
    C1[0].copy_(dev(st[1])); C2[0].copy_(dev(st[3]))
    tape = {"P": e(T, B, O_), "H1": e(T, B, H), "C1": C1[1:], "H2": e(T, B, H), "C2": C2[1:], "res1": e(T, B, 5, H), "res2": e(T, B, 5, H)}
    ws = ops.Workspace()
    dw = {k: dev(v) for k, v in w.items()}
    args = (dev(dec0), dev(st[0]), C1[0], dev(st[2]), C2[0], dev(oth), dw, dev(mix_Wp), T)
    tape["M"] = ops.mix_decoder(*args, act=act, workspace=ws, train=tape, dtype=dtype)
    ws.check()
    M_inf = ops.mix_decoder(*args, act=act, workspace=ws, dtype=dtype)
    ws.check()
    assert torch.equal(M_inf, tape["M"]), "the inference form of the decoder differs from the training form"
    return tape, C1, C2


@pytest.mark.parametrize("regime,dtype", MIX)
def test_mix_decoder_forward_and_backward_in_value_regimes(regime, dtype):
    """Both decoder layers in the regime, a wide initial cell state on the pinned units, a saturating head.  R3 reaches layer 1 and
    the head (row 9's first input is +-500, row 3's others-projection is scaled by 100); layer 2 reads a hidden state in (-1, 1) and
    sees no overflowing argument.  Every tape against mix_decoder_train_forward, every gradient of mix_decoder_bwd against
    mix_decoder_backward on the kernel's own tapes, and the exact properties on the decoder's fp64 pre-activations."""
    from longterm360fov_amd import ops
    bf = dtype == "bf16"
    B, T, O_ = MIX_SHAPE
    H = 256
    w, mix_Wp, st, dec0, oth, act, extra = O.regime_mix_decoder(60 + O.REGIMES.index(regime), regime, B, T, H, O_)
    dw = {k: dev(v) for k, v in w.items()}
    e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    tape, C1, C2 = run_mix_decoder(ops, w, mix_Wp, st, dec0, oth, act, dtype, T)
    M = tape["M"]

    def fwd(dt, rounded):
        c_ = lambda a: np.asarray(a, dt)
        return O.mix_decoder_train_forward(c_(dec0), *[c_(s) for s in st], c_(oth), {k: c_(v) for k, v in w.items()}, c_(mix_Wp), T,
                                           act=act, round_fwd=rounded)
    r64, r32 = fwd(np.float64, bf), fwd(np.float32, bf)
    kind = "bf16" if bf else "f32"
    tag = "mix decoder %s %s" % (dtype, regime)
    for k in ("M", "P", "H1", "C1", "H2", "C2", "res1", "res2"):
        check("%s tape %s" % (tag, k), tape[k], r64[k], kind, O.regime_error(r32[k], r64[k], kind))
    if bf:
        full = fwd(np.float64, False)
        for k in ("M", "P", "H1", "H2"):
            check_loose("%s tape %s" % (tag, k), tape[k], r64[k], full[k])
    gpu_tape = {k: host(v) for k, v in tape.items()}
    for k in ("M", "P", "H1", "H2"):
        assert np.abs(gpu_tape[k]).max() <= 1.0, (tag, k)
    f64 = lambda a: np.asarray(a, np.float64)
    z1, z2, pre_m = O.mix_decoder_preactivations(r64, f64(dec0), [f64(a) for a in st], f64(oth), {k: f64(v) for k, v in w.items()},
                                                 f64(mix_Wp), bf16=bf)
    exact_gate_properties(tag + " layer 1", gpu_tape["res1"], z1, act, (0, 9) if regime == "R3" else None)
    exact_gate_properties(tag + " layer 2", gpu_tape["res2"], z2, act)
    assert (gpu_tape["M"][pre_m > 100] == 1.0).all() and (gpu_tape["M"][pre_m < -100] == -1.0).all(), tag
    if regime == "R3":
        assert (pre_m[:, 3] > 200).sum() > 0 and (pre_m[:, 3] < -200).sum() > 0
        # the two extreme rows' tile-mates do not see them
        rows = extra["rows"]
        calm, _, _ = run_mix_decoder(ops, w, mix_Wp, st, extra["dec0_calm"], extra["oth_calm"], act, dtype, T)
        mates = np.setdiff1d(np.arange(B), rows)
        for k in gpu_tape:
            np.testing.assert_array_equal(host(calm[k])[:, mates], gpu_tape[k][:, mates], err_msg="%s %s: tile-mates moved" % (tag, k))
        # zero biases: the all-zero tile (inputs, states and others-projection) returns exact zeros
        edge, _, _ = run_mix_decoder(ops, extra["w_edge"], mix_Wp, extra["st_edge"], extra["dec0_edge"], extra["oth_edge"], act, dtype, T)
        for k in ("M", "P", "H1", "C1", "H2", "C2"):
            assert (host(edge[k])[:, 16:32] == 0).all(), (tag, k, "the all-zero tile is not exactly zero")
        for n in ("res1", "res2"):
            assert (host(edge[n])[:, 16:32, 2] == 0).all() and (host(edge[n])[:, 16:32, 4] == 0).all(), (tag, n)
        assert all(np.isfinite(host(v)).all() for v in edge.values())
    G = (0.2 * np.random.default_rng(61).standard_normal((T, B, O_))).astype(np.float32)

    def bwd_ref(tp, dt):
        c_ = lambda a: np.asarray(a, dt)
        dloss = G * (1 - tp["M"] * tp["M"])
        C1f = np.concatenate([st[1][None], tp["C1"]])
        C2f = np.concatenate([st[3][None], tp["C2"]])
        return O.mix_decoder_backward(c_(tp["M"]), c_(tp["P"]), c_(dloss), c_(tp["res1"]), c_(tp["res2"]), c_(C1f), c_(C2f),
                                      {k: c_(v) for k, v in w.items()}, c_(mix_Wp), act=act, round_rec=bf, round_dx=bf)
    dloss = dev(G * (1 - gpu_tape["M"] * gpu_tape["M"]))
    out = {k: e(T, B, 4 * H) for k in ("DZ1", "DZ2")}
    out.update({k: e(T, B, O_) for k in ("dpre_m", "dpre_p")})
    out.update({k: e(B, H) for k in ("dh1_0", "dc1_0", "dh2_0", "dc2_0")})
    wsb = ops.Workspace()
    ops.mix_decoder_bwd(M, tape["P"], dloss, tape["res1"], tape["res2"], C1, C2, dw, dev(mix_Wp), out, act=act, workspace=wsb, dtype=dtype)
    wsb.check()
    ref = bwd_ref(gpu_tape, np.float64)
    y64, y32 = bwd_ref(r32, np.float64), bwd_ref(r32, np.float32)
    for k in ref:
        tol = ((2e-3 if k in ("dh1_0", "dh2_0") else 1e-3) if bf else 1e-4)
        check("%s bwd %s" % (tag, k), out[k], ref[k], tol, O.regime_error(y32[k], y64[k], tol))
    if regime == "R1":
        for n, dzn, z in (("res1", "DZ1", z1), ("res2", "DZ2", z2)):
            r, dz = gpu_tape[n], host(out[dzn])
            exact_zero_gradient_at_the_clamp("%s %s" % (tag, dzn), r, dz, z, H)
            for q in (0, 1, 3):     # and, keyed on the kernel's own tape: dz of a gate it stored as clamped is exactly zero
                cl = (r[:, :, q] == 0.0) | (r[:, :, q] == 1.0)
                assert cl.mean() > 0.25 and (dz[..., q * H:(q + 1) * H][cl] == 0.0).all(), (tag, dzn, q)


# ---------------------------------------------------------------------------------------------------------------------
# ConvLSTM2D step: the cell epilogue in its LDS-patch and implicit-GEMM forms, and the gates' backward on that tape
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "implicit-gemm"])
@pytest.mark.parametrize("shape,act", CONV)
def test_convlstm_cell_with_overflowing_arguments(shape, act, form):
    from longterm360fov_amd import ops
    B, H, W, C, F, k = shape
    p = O.regime_convlstm_cell(40 + C, B, H, W, C, F, k, act)
    KR = torch.cat([dev(p["K"]), dev(p["R"])], 2).contiguous()
    e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    tag = "convlstm cell %s %s %s" % (shape, act, form)

    def run(x, b, h, c):
        h_out, c_new, gates = e(B, H, W, F), e(B, H, W, F), e(B, H, W, 4 * F)
        with knobs({"FOV_NO_CELL_PATCH": "1"} if form == "implicit-gemm" else {}):
            ops.convlstm_cell(dev(x), dev(h), KR, dev(b), dev(c), h_out, act, c_new=c_new, gates=gates)
            torch.cuda.synchronize()
        return {"h": host(h_out), "c": host(c_new), "gates": host(gates)}
    got = run(p["x"], p["b"], p["h"], p["c"])
    r64, r32 = O.regime_convlstm_reference(p), O.regime_convlstm_reference(p, np.float32)
    for n in ("h", "c", "gates"):
        check("%s %s" % (tag, n), got[n], r64[n], "f32", O.regime_error(r32[n], r64[n], "f32"))
    z, g = r64["z"], got["gates"]
    assert np.abs(got["h"]).max() <= 1.0 and np.abs(g).max() <= 1.0 and g[..., :2 * F].min() >= 0.0 and g[..., 3 * F:].min() >= 0.0
    gate_cols = np.r_[0:2 * F, 3 * F:4 * F]
    zs, gs = z[..., gate_cols], g[..., gate_cols]
    assert (zs > 200).sum() > 0 and (zs < -200).sum() > 0
    assert (gs[zs > 100] == 1.0).all() and (gs[zs < -100] == 0.0).all(), tag
    zt, gt = z[..., 2 * F:3 * F], g[..., 2 * F:3 * F]
    assert (gt[zt > 100] == 1.0).all() and (gt[zt < -100] == -1.0).all(), tag
    if B > 1:       # the other maps of the batch do not see the extreme pixels of map 0
        calm = run(p["x_calm"], p["b"], p["h"], p["c"])
        for n in got:
            np.testing.assert_array_equal(calm[n][1:], got[n][1:])
    ze = run(p["x_edge"], p["b_edge"], p["h_edge"], p["c_edge"])
    assert (ze["h"][-1] == 0).all() and (ze["c"][-1] == 0).all() and (ze["gates"][-1][..., 2 * F:3 * F] == 0).all(), tag
    # the gates' backward on this tape: exact properties only
    dh = dev(np.random.default_rng(5).standard_normal((B, H, W, F)))
    dc = dev(np.random.default_rng(6).standard_normal((B, H, W, F)))
    dz = host(ops.convlstm_gates_bwd(dh, dc, dev(got["gates"]), dev(p["c"]), dev(got["c"]), act))
    assert np.isfinite(dz).all() and np.isfinite(host(dc)).all(), tag
    stored = (gs == 0.0) | (gs == 1.0)
    assert stored.mean() > 0.1 and (dz[..., gate_cols][stored] == 0.0).all(), (tag, "dz of an exactly saturated gate")
    assert (dz[..., 2 * F:3 * F][np.abs(gt) == 1.0] == 0.0).all(), (tag, "dz of an exactly saturated g")
