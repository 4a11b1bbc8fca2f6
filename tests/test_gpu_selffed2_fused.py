"""The self-fed two-layer decoder's unroll as ONE launch per direction (fov_selffed2_decoder_fwd / _bwd, lstm_selffed2.hip)
against fp64 references (tests/test_tile_train_host.py: forward64 / backward64, a NumPy restatement of the entry points' two loops -
forward with every tape, backward on GIVEN tapes - and autograd64, torch.autograd in fp64 for every gradient).  The whole-model
cases also run oracle.others_context_forward (given_others_gt_mean_var_seq2seq.py:203-299, heads target_user_only / others_mlp /
others_lstm).

Bounds - the project's written ones and nothing looser:
    outputs and tapes:  |gpu - ref| <= 2e-5  AND  |gpu - ref| <= 1e-3 |ref| + 1e-5, per element;
    every gradient:     max |gpu - ref| <= 1e-4 max|ref| + 1e-9 per tensor, no element left out.
hard_sigmoid has kinks, where an fp32 pre-activation may fall on the other side than the fp64 one: a case asserts on the CPU, in
fp64, that no hard_sigmoid pre-activation of either layer lies within 1e-4 of +-2.5; a seed that violates that is passed over for
the next one (no element is masked).  Cases are computed once and shared.

Shapes: the forward at both widths, the backward at width 32 (all it takes); one sequence, one whole tile, a ragged second tile,
three tiles; one to three steps (both LDS parities, the first and the last step being the same one), thirty, and one long run;
feedback widths 1, 5, 6, 8 (one and two k-steps, partial ones)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O
from test_tile_train_host import STATES, _step_t, autograd64, backward64, forward64      # the fp64 references, shared with the guarded-view tests

TAPES = O.SELFFED2_TAPES

pytestmark = pytest.mark.gpu

BWD_OUT = ("DPRE", "DZ1", "DZ2", "dx0", "dh1_0", "dc1_0", "dh2_0", "dc2_0")
LAYER_W = ("dec1_K", "dec1_R", "dec1_b", "dec2_K", "dec2_R", "dec2_b")


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float32)).cuda()


def f64(w):
    return {k: v.astype(np.float64) for k, v in w.items()}


def _weights(rng, H, n_out, ctx_shape, bd):
    u = lambda lim, *s: rng.uniform(-lim, lim, s).astype(np.float32)
    w = {"dec1_K": u(np.sqrt(6.0 / (n_out + 4 * H)), n_out, 4 * H), "dec2_K": u(np.sqrt(6.0 / (5 * H)), H, 4 * H)}
    for n in ("dec1", "dec2"):
        w[n + "_R"] = u(np.sqrt(3.0 / H), H, 4 * H)
        w[n + "_b"] = (0.1 * rng.standard_normal(4 * H)).astype(np.float32)
        w[n + "_b"][H:2 * H] += 1.0        # Keras' unit_forget_bias
    w["W"] = u(np.sqrt(6.0 / (H + n_out)), H, n_out)
    if bd:
        w["bd"] = u(0.2, n_out)
    if ctx_shape is not None:
        w["ctx"] = u(0.7, *ctx_shape)
    return w


@functools.lru_cache(maxsize=None)
def _case(H, B, T, n_out, act="sigmoid", ctx=True, bd=False, state=True, bias_clamp=False):
    """One decoder case: weights (the head's W, bd and ctx among them), fp32 inputs, fp64 reference; computed once and shared
    (nobody writes into them).  The first seed whose fp64 pre-activations keep 1e-4 away from hard_sigmoid's kinks is the case's."""
    for attempt in range(16):
        rng = np.random.default_rng(1009 * attempt + 131 * H + 17 * B + 7 * T + n_out)
        w = _weights(rng, H, n_out, (B, T, n_out) if ctx else None, bd)
        if bias_clamp:      # a few gates of every sequence and step driven far into the flat parts of hard_sigmoid
            for n in ("dec1_b", "dec2_b"):
                w[n][[3, H + 17, 3 * H + 30]] = (6.0, -6.0, 6.0)
                w[n][[H - 1, 2 * H - 2]] = (-6.0, 6.0)
        x0 = rng.uniform(-1, 1, (B, n_out)).astype(np.float32)
        st = {k: (rng.uniform(-0.6, 0.6, (B, H)).astype(np.float32) if state else None) for k in STATES}
        dloss = rng.standard_normal((T, B, n_out)).astype(np.float32)
        ref, margin = forward64(x0, st, w, T, act)
        if margin > 1e-4:
            break
    assert margin > 1e-4, "a hard_sigmoid pre-activation within 1e-4 of +-2.5"
    y_t, grads = autograd64(x0, st, w, dloss, T, act)
    assert np.abs(y_t - ref["y"]).max() <= 1e-12                 # the two restatements of the forward agree
    loops = backward64(ref, dloss.astype(np.float64), w, act)    # and so do the backward loop and autograd
    for k in BWD_OUT:
        assert np.abs(loops[k] - grads[k]).max() <= 1e-12 * max(1.0, np.abs(grads[k]).max()), k
    ref.update(grads)
    case = dict(w=w, x0=x0, st=st, dloss=dloss, ref=ref, H=H, B=B, T=T, O=n_out, act=act)
    for a in list(w.values()) + [x0, dloss] + list(st.values()) + list(ref.values()):
        if a is not None:
            a.setflags(write=False)
    return case


def _held(tag, got, ref):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float(err.max()) if err.size else 0.0
    print("%s: max |gpu - fp64| %.3e" % (tag, worst))
    assert (err <= 1e-3 * np.abs(ref) + 1e-5).all() and worst <= 2e-5, (tag, worst)


def _grad_held(tag, got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    scale, err = float(np.abs(ref).max()), float(np.abs(np.asarray(got, dtype=np.float64) - ref).max())
    print("%s: max|ref| %.3e  max err %.3e" % (tag, scale, err))
    assert err <= 1e-4 * scale + 1e-9, (tag, err, scale)


# ------------------------------------------------------------------------------------------------------------------------------
# the calls
# ------------------------------------------------------------------------------------------------------------------------------
def _dw(c):
    return {k: dev(v) for k, v in c["w"].items()}


def _gpu_fwd(c, tape=True, final=True):
    from longterm360fov_amd import ops
    dw = _dw(c)
    e = lambda: torch.empty((2, c["B"], c["H"]), dtype=torch.float32, device="cuda")
    hT, cT = (e(), e()) if final else (None, None)
    y, tp = ops.selffed2_decoder_fwd(dev(c["x0"]), dw, dw["W"], c["T"], states={k: dev(v) for k, v in c["st"].items()},
                                     bd=dw.get("bd"), ctx=dw.get("ctx"), act=c["act"], tape=tape, hT=hT, cT=cT)
    torch.cuda.synchronize()
    return y, tp, hT, cT


def _gpu_bwd(c, tp, **kw):
    from longterm360fov_amd import ops
    dw = _dw(c)
    out = ops.selffed2_decoder_bwd(tp, dev(c["dloss"]), dw, dw["W"], act=c["act"], **kw)
    torch.cuda.synchronize()
    return out


def _walk_fwd(c):
    """The step-by-step walk of OthersContextTrainer.forward_backward on the layer kernels -> the same tapes."""
    from longterm360fov_amd import ops
    dw, B, T, H, n_out, act = _dw(c), c["B"], c["T"], c["H"], c["O"], c["act"]
    e = lambda *s_: torch.empty(s_, dtype=torch.float32, device="cuda")
    tp = {"H1": e(T + 1, B, H), "C1": e(T + 1, B, H), "H2": e(T + 1, B, H), "C2": e(T + 1, B, H), "XY": e(T + 1, B, n_out),
          "RES1": e(T, B, 1, 5, H), "RES2": e(T, B, 1, 5, H)}
    for k, s_ in zip(("H1", "C1", "H2", "C2"), STATES):
        tp[k][0].copy_(torch.zeros(B, H) if c["st"][s_] is None else torch.from_numpy(np.array(c["st"][s_])))
    tp["XY"][0].copy_(dev(c["x0"]))
    for t in range(T):
        ops.lstm_seq_train(tp["XY"][t].view(B, 1, n_out), dw["dec1_K"], dw["dec1_R"], dw["dec1_b"], tp["H1"][t], tp["C1"][t], act=act,
                           out=(tp["H1"][t + 1].view(B, 1, H), None, tp["C1"][t + 1], tp["RES1"][t]))
        ops.lstm_seq_train(tp["H1"][t + 1].view(B, 1, H), dw["dec2_K"], dw["dec2_R"], dw["dec2_b"], tp["H2"][t], tp["C2"][t], act=act,
                           out=(tp["H2"][t + 1].view(B, 1, H), None, tp["C2"][t + 1], tp["RES2"][t]))
        if "ctx" in dw:
            ops.dense_add(tp["H2"][t + 1], dw["W"], dw.get("bd"), dw["ctx"][:, t], activation="tanh", out=tp["XY"][t + 1])
        else:
            ops.dense(tp["H2"][t + 1], dw["W"], dw["bd"], activation="tanh", out=tp["XY"][t + 1])
    torch.cuda.synchronize()
    return tp


def _np(d, keys):
    return {k: None if d[k] is None else d[k].cpu().numpy() for k in keys}


def _check_forward(tag, c, y, tp, hT, cT):
    ref = c["ref"]
    _held(tag + " y", y.cpu().numpy(), ref["y"])
    for k in TAPES:
        _held(tag + " " + k, tp[k].cpu().numpy(), ref[k])
    _held(tag + " hT", hT.cpu().numpy(), ref["hT"])
    _held(tag + " cT", cT.cpu().numpy(), ref["cT"])
    T = c["T"]
    np.testing.assert_array_equal(y.cpu().numpy(), tp["XY"][1:].transpose(0, 1).cpu().numpy())     # y is XY[1:], batch-major
    assert torch.equal(hT[0], tp["H1"][T]) and torch.equal(hT[1], tp["H2"][T])
    assert torch.equal(cT[0], tp["C1"][T]) and torch.equal(cT[1], tp["C2"][T])
    assert torch.equal(tp["XY"][0], dev(c["x0"]))
    for k, s_ in zip(("H1", "C1", "H2", "C2"), STATES):       # row 0 is the initial state, bit for bit
        assert torch.equal(tp[k][0], torch.zeros_like(tp[k][0]) if c["st"][s_] is None else dev(c["st"][s_])), k
    for k, res in (("C1", "RES1"), ("C2", "RES2")):           # the reserve's c is the tape's c
        assert torch.equal(tp[res][:, :, 0, 4], tp[k][1:]), k


# ------------------------------------------------------------------------------------------------------------------------------
# forward and tapes against fp64
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 16, 17, 33])
@pytest.mark.parametrize("H", [32, 64])
def test_forward_and_tapes_over_tiles(H, B):
    c = _case(H, B, 3, 6)
    y, tp, hT, cT = _gpu_fwd(c)
    _check_forward("H%d B%d" % (H, B), c, y, tp, hT, cT)
    y_only, none, _, _ = _gpu_fwd(c, tape=False, final=False)      # predict's call: every tape NULL, the same prediction
    assert none is None and torch.equal(y_only, y)


@pytest.mark.parametrize("H,T,n_out,act,ctx,bd,state", [
    (32, 3, 1, "sigmoid", True, False, True), (64, 3, 1, "sigmoid", True, True, True),        # feedback widths
    (64, 3, 5, "sigmoid", True, False, True), (32, 3, 5, "hard_sigmoid", False, True, True),
    (32, 3, 8, "sigmoid", True, True, True), (64, 3, 8, "hard_sigmoid", True, False, False),
    (32, 3, 6, "sigmoid", False, True, True), (64, 3, 6, "sigmoid", False, True, True),       # ctx NULL with bd
    (32, 3, 6, "sigmoid", True, False, True),                                                 # bd NULL with ctx (H 64: the tiles test)
    (32, 3, 6, "sigmoid", True, True, True), (64, 3, 6, "sigmoid", True, True, True),         # both
    (32, 3, 6, "sigmoid", True, False, False), (64, 3, 6, "sigmoid", True, False, False),     # zero states via NULL
    (32, 3, 6, "hard_sigmoid", True, False, True), (64, 3, 6, "hard_sigmoid", True, True, True),
    (32, 1, 6, "sigmoid", True, False, True), (64, 1, 6, "hard_sigmoid", True, False, True),  # one step, two steps
    (32, 2, 6, "hard_sigmoid", True, True, False), (64, 2, 6, "sigmoid", True, False, True)])
def test_forward_variants(H, T, n_out, act, ctx, bd, state):
    c = _case(H, 17, T, n_out, act, ctx, bd, state)
    y, tp, hT, cT = _gpu_fwd(c)
    _check_forward("H%d T%d O%d %s ctx=%d bd=%d state=%d" % (H, T, n_out, act, ctx, bd, state), c, y, tp, hT, cT)


def test_forward_with_one_state_alone():
    """Each of the four states may be NULL on its own."""
    c = _case(32, 17, 2, 6)
    for keep in STATES:
        st = {k: (v if k == keep else None) for k, v in c["st"].items()}
        ref, _ = forward64(c["x0"], st, c["w"], c["T"], c["act"])
        y, tp, _, _ = _gpu_fwd(dict(c, st=st))
        _held("only " + keep, y.cpu().numpy(), ref["y"])
        _held("only %s, H2" % keep, tp["H2"].cpu().numpy(), ref["H2"])


def test_forward_sixty_four_steps():
    c = _case(32, 16, 64, 6)
    y, tp, hT, cT = _gpu_fwd(c)
    _check_forward("H32 B16 T64", c, y, tp, hT, cT)


# ------------------------------------------------------------------------------------------------------------------------------
# backward (H = 32: all the entry takes)
# ------------------------------------------------------------------------------------------------------------------------------
#            B, T, O, act, ctx, bd, state
BWD_CASES = [(17, 3, 6, "sigmoid", True, False, True), (33, 3, 6, "hard_sigmoid", True, True, True),
             (1, 1, 6, "hard_sigmoid", False, True, False), (17, 1, 8, "sigmoid", True, False, False),
             (33, 30, 1, "sigmoid", False, True, True), (1, 30, 8, "hard_sigmoid", True, False, True),
             (17, 30, 6, "sigmoid", True, False, True), (33, 1, 1, "hard_sigmoid", True, True, False),
             (1, 3, 1, "sigmoid", True, False, True), (17, 3, 8, "hard_sigmoid", False, True, True)]


@pytest.mark.parametrize("B,T,n_out,act,ctx,bd,state", BWD_CASES)
def test_fused_backward_on_the_walks_tapes(B, T, n_out, act, ctx, bd, state):
    """The backward kernel alone: the step-by-step walk writes the tapes, the fused backward reads them."""
    c = _case(32, B, T, n_out, act, ctx, bd, state)
    tp = _walk_fwd(c)
    for k in TAPES:
        _held("walk tape " + k, tp[k].cpu().numpy(), c["ref"][k])
    got = _np(_gpu_bwd(c, tp), BWD_OUT)
    loops = backward64(_np(tp, TAPES), c["dloss"].astype(np.float64), c["w"], act)      # fp64 arithmetic on these very tapes
    for k in BWD_OUT:
        _grad_held("walk tapes, fused vs fp64 loop on them %s" % k, got[k], loops[k])
        _grad_held("walk tapes, fused vs autograd %s" % k, got[k], c["ref"][k])


@pytest.mark.parametrize("B,T,n_out,act,ctx,bd,state", BWD_CASES)
def test_fused_forward_and_backward_against_autograd(B, T, n_out, act, ctx, bd, state):
    c = _case(32, B, T, n_out, act, ctx, bd, state)
    y, tp, hT, cT = _gpu_fwd(c)
    _check_forward("B%d T%d O%d %s" % (B, T, n_out, act), c, y, tp, hT, cT)
    got = _np(_gpu_bwd(c, tp), BWD_OUT)
    for k in BWD_OUT:
        _grad_held("B%d T%d O%d %s %s" % (B, T, n_out, act, k), got[k], c["ref"][k])


def test_backward_without_dx0_and_state_gradients():
    """dx0 = NULL (the trainer's call) and NULL state gradients are accepted: the other outputs keep their bits."""
    c = _case(32, 17, 3, 6)
    _, tp, _, _ = _gpu_fwd(c)
    full = _gpu_bwd(c, tp)
    lean = _gpu_bwd(c, tp, need_dx0=False)
    assert lean["dx0"] is None and all(torch.equal(lean[k], full[k]) for k in BWD_OUT if k != "dx0")
    bare = _gpu_bwd(c, tp, need_dx0=False, need_state_grads=False)
    assert all(bare[k] is None for k in BWD_OUT[3:]) and all(torch.equal(bare[k], full[k]) for k in BWD_OUT[:3])


def test_no_step_backward_zeroes_the_input_and_state_gradients():
    from longterm360fov_amd import ops
    c = _case(32, 5, 1, 6)
    dw = _dw(c)
    y, tp = ops.selffed2_decoder_fwd(dev(c["x0"]), dw, dw["W"], 0, states={k: dev(v) for k, v in c["st"].items()}, act=c["act"])
    assert y.shape == (5, 0, 6) and torch.equal(tp["XY"][0], dev(c["x0"])) and torch.equal(tp["C2"][0], dev(c["st"]["c2_0"]))
    out = ops.selffed2_decoder_bwd(tp, torch.empty((0, 5, 6), dtype=torch.float32, device="cuda"), dw, dw["W"], act=c["act"])
    torch.cuda.synchronize()
    for k in BWD_OUT[3:]:
        assert out[k].shape[0] == 5 and float(out[k].abs().max()) == 0.0, k


# ------------------------------------------------------------------------------------------------------------------------------
# exact properties
# ------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    for H in (32, 64):
        c = _case(H, 33, 3, 6, "hard_sigmoid", True, True, True)
        y1, tp1, hT1, cT1 = _gpu_fwd(c)
        y2, tp2, hT2, cT2 = _gpu_fwd(c)
        assert torch.equal(y1, y2) and torch.equal(hT1, hT2) and torch.equal(cT1, cT2)
        assert all(torch.equal(tp1[k], tp2[k]) for k in TAPES)
    c = _case(32, 33, 3, 6, "hard_sigmoid", True, True, True)
    _, tp, _, _ = _gpu_fwd(c)
    b1, b2 = _gpu_bwd(c, tp), _gpu_bwd(c, tp)
    assert all(torch.equal(b1[k], b2[k]) for k in BWD_OUT)


@pytest.mark.parametrize("H,act", [(32, "hard_sigmoid"), (64, "sigmoid")])
def test_a_sequence_does_not_depend_on_its_place_in_the_batch(H, act):
    c = _case(H, 33, 3, 6, act, True, True, True)
    for row in (5, 32):      # inside a whole tile; alone in the ragged last one
        w1 = dict(c["w"], ctx=c["w"]["ctx"][row:row + 1])
        one = dict(c, B=1, w=w1, x0=c["x0"][row:row + 1], st={k: v[row:row + 1] for k, v in c["st"].items()},
                   dloss=np.ascontiguousarray(c["dloss"][:, row:row + 1]))
        y, tp, hT, cT = _gpu_fwd(c)
        y1, tp1, hT1, cT1 = _gpu_fwd(one)
        assert torch.equal(y[row:row + 1], y1) and torch.equal(hT[:, row:row + 1], hT1) and torch.equal(cT[:, row:row + 1], cT1)
        for k in TAPES:
            assert torch.equal(tp[k][:, row:row + 1], tp1[k]), k
        if H == 32:
            b, b1 = _gpu_bwd(c, tp), _gpu_bwd(one, tp1)
            for k in BWD_OUT[:3]:
                assert torch.equal(b[k][:, row:row + 1], b1[k]), k
            for k in BWD_OUT[3:]:
                assert torch.equal(b[k][row:row + 1], b1[k]), k


def _between_canaries(shapes, canary):
    """Tensors of the given shapes as views into one buffer, 64 canary floats in front of, between and behind them."""
    gap = 64
    total = gap + sum(int(np.prod(s)) + gap for s in shapes.values())
    buf = torch.full((total,), canary, dtype=torch.float32, device="cuda")
    views, gaps, at = {}, [(0, gap)], gap
    for k, s in shapes.items():
        n = int(np.prod(s))
        views[k] = buf[at:at + n].view(*s)
        gaps.append((at + n, at + n + gap))
        at += n + gap
    return buf, views, gaps


@pytest.mark.parametrize("H,B", [(64, 17), (32, 1)])
def test_rows_beyond_the_batch_are_not_written(H, B):
    """Through the C ABI, every output a view between canaries: a ragged last tile stores nothing beyond row B."""
    from longterm360fov_amd import _lib, ops
    T, n_out, canary = 3, 6, 777.25
    c = _case(H, B, T, n_out, "sigmoid", True, True, True)
    y_ref, tp_ref, hT_ref, cT_ref = _gpu_fwd(c)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    dw = _dw(c)
    x0, dloss = dev(c["x0"]), dev(c["dloss"])
    st = [dev(c["st"][k]) for k in STATES]
    buf, v, gaps = _between_canaries({"H1": (T + 1, B, H), "C1": (T + 1, B, H), "H2": (T + 1, B, H), "C2": (T + 1, B, H),
                                      "XY": (T + 1, B, n_out), "RES1": (T, B, 1, 5, H), "RES2": (T, B, 1, 5, H), "y": (B, T, n_out),
                                      "hT": (2, B, H), "cT": (2, B, H)}, canary)
    stream = ops._stream()
    ops.check(_lib.lib().fov_selffed2_decoder_fwd(p(x0), *[p(s_) for s_ in st], *[p(dw[k]) for k in LAYER_W], p(dw["W"]), p(dw["bd"]),
                                                  p(dw["ctx"]), *[p(v[k]) for k in TAPES], p(v["y"]), p(v["hT"]), p(v["cT"]),
                                                  B, T, n_out, H, _lib.ACT_SIGMOID, stream))
    torch.cuda.synchronize()
    for lo, hi in gaps:
        assert bool((buf[lo:hi] == canary).all()), (lo, hi)
    assert torch.equal(v["y"], y_ref) and torch.equal(v["hT"], hT_ref) and torch.equal(v["cT"], cT_ref)
    assert all(torch.equal(v[k], tp_ref[k]) for k in TAPES)
    if H != 32:
        return
    b_ref = _gpu_bwd(c, tp_ref)
    buf2, o, gaps2 = _between_canaries({"DPRE": (T, B, n_out), "DZ1": (T, B, 4 * H), "DZ2": (T, B, 4 * H), "dx0": (B, n_out),
                                        "dh1_0": (B, H), "dc1_0": (B, H), "dh2_0": (B, H), "dc2_0": (B, H)}, canary)
    ops.check(_lib.lib().fov_selffed2_decoder_bwd(*[p(v[k]) for k in ("C1", "C2", "XY", "RES1", "RES2")], p(dloss),
                                                  *[p(dw[k]) for k in ("dec1_K", "dec1_R", "dec2_K", "dec2_R", "W")],
                                                  *[p(o[k]) for k in BWD_OUT], B, T, n_out, H, _lib.ACT_SIGMOID, stream))
    torch.cuda.synchronize()
    for lo, hi in gaps2:
        assert bool((buf2[lo:hi] == canary).all()), (lo, hi)
    assert all(torch.equal(o[k], b_ref[k]) for k in BWD_OUT)


def test_clamped_hard_sigmoid_gates_have_exactly_zero_dz():
    H = 32
    c = _case(H, 17, 3, 6, "hard_sigmoid", True, False, True, True)
    cols = {3: 1.0, H + 17: 0.0, 3 * H + 30: 1.0, H - 1: 0.0, 2 * H - 2: 1.0}      # bias column -> the gate's clamped value
    for res in ("RES1", "RES2"):
        for col, val in cols.items():
            assert (c["ref"][res][:, :, 0, col // H, col % H] == val).all(), "the bias does not clamp gate column %d in fp64" % col
    y, tp, hT, cT = _gpu_fwd(c)
    _check_forward("clamped gates", c, y, tp, hT, cT)
    got = _np(_gpu_bwd(c, tp), BWD_OUT)
    for k in BWD_OUT:
        _grad_held("clamped gates %s" % k, got[k], c["ref"][k])
    for res, dz in (("RES1", "DZ1"), ("RES2", "DZ2")):
        for col, val in cols.items():
            assert (tp[res][:, :, 0, col // H, col % H] == val).all()
            assert (got[dz][:, :, col] == 0.0).all(), (dz, col)
            assert (c["ref"][dz][:, :, col] == 0.0).all()
        assert float(np.abs(got[dz]).max()) > 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# the whole model: OthersContextTrainer / OthersContextSeq2Seq
# ------------------------------------------------------------------------------------------------------------------------------
def _graph64(enc, oth, dec0, tgt, w, mode, act):
    """fp64 torch.autograd restatement of given_others_gt_mean_var_seq2seq.py:203-299 under MSE with the head `mode`
    -> (loss, gradients, prediction, hard_sigmoid margin over every LSTM pre-activation of the graph)."""
    t = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in w.items()}
    H = w["enc1_R"].shape[0]
    zs = []

    def layer(x, n, h, c):
        outs = []
        for tt in range(x.shape[1]):
            h, c = _step_t(x[:, tt], h, c, t[n + "_K"], t[n + "_R"], t[n + "_b"], act, zs)
            outs.append(h)
        return torch.stack(outs, 1), h, c
    e, o_, d0, tg = (torch.tensor(a.astype(np.float64)) for a in (enc, oth, dec0, tgt))
    B, T_out = e.shape[0], tg.shape[1]
    z0 = torch.zeros(B, H, dtype=torch.float64)
    hs1, h1, c1 = layer(e, "enc1", z0, z0)
    _, h2, c2 = layer(hs1, "enc2", z0, z0)
    ctx = None
    if mode == "others_mlp":
        ctx = torch.relu(torch.relu(o_.reshape(B, T_out, -1) @ t["oth_W1"] + t["oth_b1"]) @ t["oth_W2"] + t["oth_b2"])
    elif mode == "others_lstm":
        seq, init = o_.reshape(B, T_out, -1), {"f": (z0, z0), "b": (z0, z0)}
        for j in (1, 2):
            fs, fh, fc = layer(seq, "ol%df" % j, *init["f"])
            bs, bh, bc = layer(torch.flip(seq, (1,)), "ol%db" % j, *init["b"])
            seq, init = torch.cat([fs, torch.flip(bs, (1,))], 2), {"f": (fh, fc), "b": (bh, bc)}
        ctx = seq
    x, outs = d0[:, 0], []
    for tt in range(T_out):
        h1, c1 = _step_t(x, h1, c1, t["dec1_K"], t["dec1_R"], t["dec1_b"], act, zs)
        h2, c2 = _step_t(h1, h2, c2, t["dec2_K"], t["dec2_R"], t["dec2_b"], act, zs)
        x = torch.tanh((h2 if ctx is None else torch.cat([ctx[:, tt], h2], 1)) @ t["dense_W"] + t["dense_b"])
        outs.append(x)
    y = torch.stack(outs, 1)
    loss = torch.mean((y - tg) ** 2)
    loss.backward()
    margin = np.inf
    if act == "hard_sigmoid":
        for z in zs:
            zz = z.detach().numpy()
            margin = min(margin, float(np.abs(np.abs(np.concatenate([zz[:, :2 * H], zz[:, 3 * H:]], 1)) - 2.5).min()))
    return float(loss.detach()), {k: v.grad.numpy() for k, v in t.items()}, y.detach().numpy(), margin


@functools.lru_cache(maxsize=None)
def _model_case(mode, H, act, B=17, U=4, T_in=3, T_out=4):
    from longterm360fov_amd.models import OthersContextSeq2Seq
    from longterm360fov_amd.training import others_context_order
    order = others_context_order(mode)
    for attempt in range(16):
        seed = 211 * attempt + H + B + T_out
        m = OthersContextSeq2Seq(mode, latent_dim=H, num_user=U, recurrent_activation=act, seed=seed, predict_step=T_out)
        rng = np.random.default_rng(seed + 1)
        w = {k: (v + (0.1 * rng.standard_normal(v.shape).astype(np.float32) if k.endswith(("_b", "b1", "b2")) else 0))
             for k, v in zip(order, m.get_weights())}
        enc, dec0, tgt, oth = O.synthetic_batch(seed + 2, B, T_in, T_out, num_others=U - 1)
        loss, grads, y, margin = _graph64(enc, oth, dec0, tgt, w, mode, act)
        if margin > 1e-4:
            break
    assert margin > 1e-4, "a hard_sigmoid pre-activation within 1e-4 of +-2.5"
    y_o = O.others_context_forward(enc.astype(np.float64), oth.astype(np.float64), dec0.astype(np.float64), f64(w), T_out, mode, act)
    np.testing.assert_allclose(y_o, y, atol=1e-12)
    return dict(mode=mode, H=H, act=act, w=w, enc=enc, oth=oth, dec0=dec0, tgt=tgt, loss=loss, grads=grads, y=y, order=order, U=U,
                T_out=T_out)


def _counting(monkeypatch, names=("lstm_seq_train", "lstm_seq_bwd", "dense_add", "dense", "lstm_seq", "selffed2_decoder_fwd",
                                  "selffed2_decoder_bwd")):
    from longterm360fov_amd import ops
    counts = {n: 0 for n in names}

    def wrap(n, fn):
        def counted(*a, **k):
            counts[n] += 1
            return fn(*a, **k)
        return counted
    for n in names:
        monkeypatch.setattr(ops, n, wrap(n, getattr(ops, n)))
    return counts


@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("mode,act", [("target_user_only", "sigmoid"), ("others_mlp", "hard_sigmoid"), ("others_lstm", "sigmoid")])
def test_trainer_against_autograd(monkeypatch, mode, act, H):
    """Width 32: fused both ways.  Width 64: the fused forward, the walk's backward on its tapes."""
    from longterm360fov_amd.training import OthersContextTrainer
    mc = _model_case(mode, H, act)
    counts = _counting(monkeypatch)
    tr = OthersContextTrainer(mc["w"], mode, act=act)
    loss, y = tr.forward_backward(dev(mc["enc"]), dev(mc["oth"]), dev(mc["dec0"]), dev(mc["tgt"]))
    torch.cuda.synchronize()
    tr.ws.check(); tr.bwd_scratch.check()
    assert counts["selffed2_decoder_fwd"] == 1 and counts["selffed2_decoder_bwd"] == (1 if H == 32 else 0)
    assert abs(float(loss.item()) - mc["loss"]) <= 1e-5 * mc["loss"] + 1e-9
    _held("%s H%d prediction" % (mode, H), y.cpu().numpy(), mc["y"])
    for k in mc["order"]:
        _grad_held("%s H%d grad %s" % (mode, H, k), tr.g[k].detach().cpu().numpy(), mc["grads"][k])


def _model(mc, T_out=None):
    from longterm360fov_amd.models import OthersContextSeq2Seq
    m = OthersContextSeq2Seq(mc["mode"], latent_dim=mc["H"], num_user=mc["U"], recurrent_activation=mc["act"], seed=1,
                             predict_step=mc["T_out"] if T_out is None else T_out)
    m.set_weights([mc["w"][k] for k in mc["order"]])
    return m


@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("mode,act", [("target_user_only", "sigmoid"), ("others_mlp", "hard_sigmoid"), ("others_lstm", "sigmoid")])
def test_predict_is_one_fused_call(monkeypatch, mode, act, H):
    mc = _model_case(mode, H, act)
    counts = _counting(monkeypatch)
    m = _model(mc)
    xin = [mc["enc"], mc["dec0"]] if mode == "target_user_only" else [mc["enc"], mc["oth"], mc["dec0"]]
    got = m.predict(xin)
    n_ctx = {"target_user_only": 0, "others_mlp": 0, "others_lstm": 4}[mode]
    assert counts["selffed2_decoder_fwd"] == 1 and counts["lstm_seq"] == 2 + n_ctx and counts["dense_add"] == 0
    _held("%s H%d predict" % (mode, H), got, mc["y"])
    assert "FOV_NO_SELFFED2_FUSED" not in os.environ
    os.environ["FOV_NO_SELFFED2_FUSED"] = "1"
    try:
        walk = m.predict(xin)
    finally:
        del os.environ["FOV_NO_SELFFED2_FUSED"]
    assert counts["selffed2_decoder_fwd"] == 1 and counts["lstm_seq"] == 2 * (2 + n_ctx) + 2 * mc["T_out"]
    _held("%s H%d predict, walk" % (mode, H), walk, mc["y"])
    _held("%s H%d predict, fused vs walk" % (mode, H), got, walk.astype(np.float64))


def _step_counts(monkeypatch, mc, T_out):
    """One default train_step at T_out steps -> (calls per op, loss, prediction, gradients)."""
    from longterm360fov_amd.training import OthersContextTrainer
    enc, dec0, tgt, oth = O.synthetic_batch(5, 17, 3, T_out, num_others=mc["U"] - 1)
    with monkeypatch.context() as mp:
        counts = _counting(mp)
        tr = OthersContextTrainer(mc["w"], mc["mode"], act=mc["act"])
        loss, y = tr.forward_backward(dev(enc), dev(oth), dev(dec0), dev(tgt))
        out = dict(counts), float(loss.item()), y.cpu().numpy(), {k: v.detach().cpu().numpy() for k, v in tr.g.items()}
        loss_s = float(tr.train_step(dev(enc), dev(oth), dev(dec0), dev(tgt)).item())      # the optimizer step takes the same path
        assert abs(loss_s - out[1]) <= 1e-6 * out[1]
        assert all(counts[k] == 2 * out[0][k] for k in counts), (counts, out[0])
    return out


@pytest.mark.parametrize("mode", ["target_user_only", "others_mlp", "others_lstm"])
def test_default_training_step_makes_no_call_that_grows_with_the_steps(monkeypatch, mode):
    mc = _model_case(mode, 32, "sigmoid")
    per_step = ("lstm_seq_train", "lstm_seq_bwd", "dense_add", "dense")
    c2, _, _, _ = _step_counts(monkeypatch, mc, 2)
    c5, loss_f, y_f, g_f = _step_counts(monkeypatch, mc, 5)
    assert all(c2[k] == c5[k] for k in per_step), (c2, c5)
    assert c5["selffed2_decoder_fwd"] == 1 and c5["selffed2_decoder_bwd"] == 1
    assert "FOV_NO_SELFFED2_FUSED" not in os.environ
    os.environ["FOV_NO_SELFFED2_FUSED"] = "1"
    try:
        w2, _, _, _ = _step_counts(monkeypatch, mc, 2)
        w5, loss_w, y_w, g_w = _step_counts(monkeypatch, mc, 5)
    finally:
        del os.environ["FOV_NO_SELFFED2_FUSED"]
    assert w5["selffed2_decoder_fwd"] == 0 and w5["selffed2_decoder_bwd"] == 0                 # the walk returns
    assert w5["lstm_seq_train"] - w2["lstm_seq_train"] == 6 and w5["lstm_seq_bwd"] - w2["lstm_seq_bwd"] == 6
    head = "dense" if mode == "target_user_only" else "dense_add"
    assert w5[head] - w2[head] == 3
    assert all(w2[k] == c2[k] + {"lstm_seq_train": 4, "lstm_seq_bwd": 4, head: 2}.get(k, 0) for k in per_step), (w2, c2)
    assert abs(loss_f - loss_w) <= 1e-5 * loss_w + 1e-9
    _held("%s fused vs walk prediction" % mode, y_f, y_w.astype(np.float64))
    for k in g_w:
        _grad_held("%s fused vs walk grad %s" % (mode, k), g_f[k], g_w[k])


def test_widths_the_kernels_do_not_take_keep_the_walk(monkeypatch):
    from longterm360fov_amd.training import OthersContextTrainer
    mc = _model_case("target_user_only", 128, "sigmoid")
    counts = _counting(monkeypatch)
    tr = OthersContextTrainer(mc["w"], "target_user_only", act="sigmoid")
    loss, y = tr.forward_backward(dev(mc["enc"]), dev(mc["oth"]), dev(mc["dec0"]), dev(mc["tgt"]))
    assert counts["selffed2_decoder_fwd"] == 0 and counts["selffed2_decoder_bwd"] == 0 and counts["lstm_seq_train"] == 2 + 2 * mc["T_out"]
    _held("H128 prediction", y.cpu().numpy(), mc["y"])
    _model(mc).predict([mc["enc"], mc["dec0"]])
    assert counts["selffed2_decoder_fwd"] == 0


@pytest.mark.parametrize("H", [32, 64])
def test_four_adam_steps_fused_and_walk_agree(H):
    from longterm360fov_amd.training import OthersContextTrainer
    mc = _model_case("others_mlp", H, "sigmoid")
    enc, dec0, tgt, oth = (dev(a) for a in O.synthetic_batch(9, 32, 4, 10, num_others=mc["U"] - 1))
    fused, walk = OthersContextTrainer(mc["w"], "others_mlp"), OthersContextTrainer(mc["w"], "others_mlp")
    la = [float(fused.train_step(enc, oth, dec0, tgt).item()) for _ in range(4)]
    assert "FOV_NO_SELFFED2_FUSED" not in os.environ
    os.environ["FOV_NO_SELFFED2_FUSED"] = "1"
    try:
        lb = [float(walk.train_step(enc, oth, dec0, tgt).item()) for _ in range(4)]
    finally:
        del os.environ["FOV_NO_SELFFED2_FUSED"]
    print("fused", la, "walk", lb)
    for a, b in zip(la, lb):
        assert abs(a - b) <= 1e-5 * abs(b), (la, lb)
    assert la[-1] < la[0] and lb[-1] < lb[0]
