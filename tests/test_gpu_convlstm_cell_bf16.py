"""The ConvLSTM heat-map model's cells with bf16 matrix-core operands (fov_convlstm_cell_pack_bf16, fov_convlstm_cell_fwd_bf16,
ops.convlstm_cell_bf16, ConvLSTMSeq2Seq(cell_dtype='bf16')), through the C ABI.

Operator level: h, c_new and the gates tape of ops.convlstm_cell_bf16 against one ConvLSTM2D step on bf16-rounded x, h, K, R
in fp64 (cell_bf16_ref of tests/test_convlstm_cell_bf16_host.py), |gpu - ref| <= 1e-5 max|ref| per tensor.  The host file
holds the shapes, the inputs and the CPU check of that bound: the reference's own fp32 / fp64 disagreement is below a tenth
of it, every operand mistake at least ten times beyond it.  Each form is compared with the reference, never with the other.

Model level: TIGHT against the all-bf16 restatement in fp64 (cells, and the head when the model runs it in bf16), LOOSE
against the full-precision fp64 oracle, each as tol * |ref| + 1e-5."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_convlstm_bf16_host import (FULL, FULL_ROWS, LOOSE, TIGHT, f64, full_inputs, full_weights, small_inputs,  # noqa: E402
                                     worst)
from test_convlstm_cell_bf16_host import (ACTS, MISTAKE_SHAPE, MODEL_CASES, OP_TOL, PATCH_SHAPES, PLAIN_SHAPES,  # noqa: E402
                                          REGIME_SHAPES, as64, cached_inputs, cell_bf16_ref, cell_step, cells_bf16_forward,
                                          truncate_bf16)

pytestmark = pytest.mark.gpu

EXTRA = 8       # channels a wider map has beyond x


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.cpu().numpy().astype(np.float64)


def op_close(got, ref, tag):
    got = host(got)
    assert got.shape == ref.shape, tag
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    print("%s: max err %.3e = %.3e of max|ref|" % (tag, err, err / scale))
    assert np.isfinite(got).all(), tag
    assert (np.abs(got - ref) <= OP_TOL * scale).all(), "%s: max err %.3e of max|ref| %.3e" % (tag, err, scale)


class plain_form:
    """FOV_NO_CELL_PATCH=1 for the block: every convlstm_cell_bf16 call on the plain kernel."""

    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        from longterm360fov_amd import _lib
        if self.on:
            os.environ["FOV_NO_CELL_PATCH"] = "1"
            _lib.lib().fov_reload_env()

    def __exit__(self, *exc):
        from longterm360fov_amd import _lib
        os.environ.pop("FOV_NO_CELL_PATCH", None)
        _lib.lib().fov_reload_env()
        return False


@functools.lru_cache(maxsize=None)
def refs(shape, act):
    """The fp64 references of every variant test_convlstm_cell_bf16_against_the_rounded_operand_reference runs, computed once
    per (shape, activation) and shared by the two forms."""
    B, H, W, C, F, k = shape
    q = as64(cached_inputs(shape, EXTRA))
    x, xs = q["x"][..., :C], q["x"][..., 4:4 + C]          # x itself / the channel slice and sequence step of the views
    return {"main": cell_bf16_ref(x, q["h"], q["c"], q["K"], q["R"], q["b"], act),
            "no bias": cell_bf16_ref(x, q["h"], q["c"], q["K"], q["R"], None, act),
            "zero state": cell_bf16_ref(x, None, None, q["K"], q["R"], q["b"], act),
            "views": cell_bf16_ref(xs, q["h"], q["c"], q["K"], q["R"], q["b"], act)}


def run_cell(ops, x, h, KR, b, c, act, F, packed, slot=False, gates=True, alias=False):
    """One call with NaN-filled outputs -> (h, c_new, gates): h_out a slot of a wider concat map with `slot`, c_new = c_prev
    with `alias`."""
    B, H, W, _ = x.shape
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    wide = nan(B, H, W, F + 7)
    h_out = wide[..., 3:3 + F] if slot else nan(B, H, W, F)
    c_prev = None if c is None else c.clone()
    c_new = c_prev if alias else nan(B, H, W, F)
    g = nan(B, H, W, 4 * F) if gates else None
    ho, co = ops.convlstm_cell_bf16(x, h, KR, b, c_prev, h_out, act, c_new=c_new, gates=g, packed=packed)
    assert ho is h_out and co is c_new
    if slot:
        assert torch.isnan(wide[..., :3]).all() and torch.isnan(wide[..., 3 + F:]).all(), "h_out wrote outside its slot"
    return h_out, c_new, g


def check_cell_against_the_reference(shape, act, tag):
    from longterm360fov_amd import ops
    B, H, W, C, F, k = shape
    p = cached_inputs(shape, EXTRA)
    r = refs(shape, act)
    xw = dev(p["x"])                                                 # (B,H,W,C + EXTRA)
    x = xw[..., :C].contiguous()
    h, c, b = dev(p["h"]), dev(p["c"]), dev(p["b"])
    K = dev(p["K"])
    KR = torch.cat([K, dev(p["R"])], 2).contiguous()
    packed, packed_k = ops.convlstm_cell_pack_bf16(KR), ops.convlstm_cell_pack_bf16(K)
    assert packed.dtype == torch.uint8 and torch.equal(packed, ops.convlstm_cell_pack_bf16(KR)), tag + ": packing not deterministic"

    def close(got, ref, what, gates=True):
        for n, t in zip(("h", "c", "gates") if gates else ("h", "c"), got):
            op_close(t, ref[n], "%s %s %s" % (tag, what, n))

    first = run_cell(ops, x, h, KR, b, c, act, F, packed)
    close(first, r["main"], "main")
    again = run_cell(ops, x, h, KR, b, c, act, F, packed)
    assert all(torch.equal(a, f) for a, f in zip(again, first)), tag + ": not deterministic"
    inside = run_cell(ops, x, h, KR, b, c, act, F, None)
    assert all(torch.equal(a, f) for a, f in zip(inside, first)), tag + ": packing inside the call gives another result"
    # h_out in a slot of a wider concat map, c_new aliasing c_prev, no gates tape: the same bits
    slot = run_cell(ops, x, h, KR, b, c, act, F, packed, slot=True, gates=False, alias=True)
    assert torch.equal(slot[0], first[0]) and torch.equal(slot[1], first[1]), tag + ": slot / alias / no tape changes the result"
    close(run_cell(ops, x, h, KR, None, c, act, F, packed), r["no bias"], "no bias")
    close(run_cell(ops, x, None, K, b, None, act, F, packed_k), r["zero state"], "zero state, K alone")
    # x as a channel slice of a wider map, and as one time step of a (B,T,H,W,C) sequence
    close(run_cell(ops, xw[..., 4:4 + C], h, KR, b, c, act, F, packed, slot=True), r["views"], "channel slice of a wider map")
    seq = torch.stack([x, xw[..., 4:4 + C].contiguous()], 1)
    close(run_cell(ops, seq[:, 1], h, KR, b, c, act, F, packed), r["views"], "one step of a sequence")
    torch.cuda.synchronize()


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("form", ["default", "plain"])
@pytest.mark.parametrize("shape", PATCH_SHAPES)
def test_convlstm_cell_bf16_against_the_rounded_operand_reference(shape, form, act):
    with plain_form(form == "plain"):
        check_cell_against_the_reference(shape, act, "cell_bf16 %s %s %s" % (shape, form, act))


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", PLAIN_SHAPES)
def test_convlstm_cell_bf16_shapes_of_the_plain_kernel(shape, act):
    check_cell_against_the_reference(shape, act, "cell_bf16 %s %s" % (shape, act))


@pytest.mark.parametrize("act", ACTS)
def test_convlstm_cell_bf16_on_an_x_view_eight_bytes_off_alignment(act):
    """(2,9,6,8,8,3) is a shape the patch form takes, but here x starts two floats into a 16-byte aligned map: the call must
    fall back to the plain kernel's gather and still meet the reference."""
    from longterm360fov_amd import ops
    shape = (2, 9, 6, 8, 8, 3)
    B, H, W, C, F, k = shape
    p = cached_inputs(shape, EXTRA)
    q = as64(p)
    ref = cell_bf16_ref(q["x"][..., 2:2 + C], q["h"], q["c"], q["K"], q["R"], q["b"], act)
    xv = dev(p["x"])[..., 2:2 + C]
    assert xv.data_ptr() % 16 == 8 and xv.stride(2) % 4 == 0
    KR = torch.cat([dev(p["K"]), dev(p["R"])], 2).contiguous()
    got = run_cell(ops, xv, dev(p["h"]), KR, dev(p["b"]), dev(p["c"]), act, F, None)
    for n, t in zip(("h", "c", "gates"), got):
        op_close(t, ref[n], "x view 8 bytes off alignment %s %s %s" % (shape, act, n))


def test_convlstm_cell_bf16_rounds_both_operands_to_nearest_even():
    """The operand mistakes the bound must catch are caught: against the reference with the weights left unrounded, with the
    inputs left unrounded and with truncation instead of round-to-nearest-even the kernel is OUTSIDE the bound, on h and on c."""
    from longterm360fov_amd import ops
    shape, act = MISTAKE_SHAPE, "hard_sigmoid"
    B, H, W, C, F, k = shape
    p = cached_inputs(shape, EXTRA)
    q = as64(p)
    x64 = q["x"][..., :C]
    KR = torch.cat([dev(p["K"]), dev(p["R"])], 2).contiguous()
    got = run_cell(ops, dev(p["x"][..., :C]), dev(p["h"]), KR, dev(p["b"]), dev(p["c"]), act, F, None)
    ident = lambda a: a
    wrong = {"weights unrounded": dict(rw=ident), "inputs unrounded": dict(rx=ident), "truncated": dict(rx=truncate_bf16, rw=truncate_bf16)}
    for name, kw in wrong.items():
        ref = cell_step(x64, q["h"], q["c"], q["K"], q["R"], q["b"], act, **kw)
        for n, t in zip(("h", "c"), got):
            e = float(np.abs(host(t) - ref[n]).max() / np.abs(ref[n]).max())
            print("%s %s: %.3e of max|ref|" % (name, n, e))
            assert e > OP_TOL, (name, n)


def test_convlstm_cell_bf16_empty_batch_and_errors():
    from longterm360fov_amd import ops, _lib
    shape = (2, 9, 6, 8, 8, 3)
    B, H, W, C, F, k = shape
    p = cached_inputs(shape, EXTRA)
    KR = torch.cat([dev(p["K"]), dev(p["R"])], 2).contiguous()
    packed = ops.convlstm_cell_pack_bf16(KR)
    e = lambda *s: torch.empty(s, device="cuda")
    ho, co = ops.convlstm_cell_bf16(e(0, H, W, C), e(0, H, W, F), KR, dev(p["b"]), e(0, H, W, F), e(0, H, W, F), packed=packed)
    assert ho.shape == (0, H, W, F) and co.shape == (0, H, W, F)
    L = _lib.lib()
    assert L.fov_convlstm_cell_bf16_packed_bytes(C + F, F, k, k) == packed.numel() and packed.numel() % 16 == 0
    assert L.fov_convlstm_cell_bf16_packed_bytes(C, F, k, k) == ops.convlstm_cell_pack_bf16(dev(p["K"])).numel()
    assert L.fov_convlstm_cell_bf16_packed_bytes(0, F, k, k) == 0
    x, h, c = dev(p["x"][..., :C]), dev(p["h"]), dev(p["c"])
    h_out, c_new = e(B, H, W, F), e(B, H, W, F)
    args = lambda **kw: [x.data_ptr(), C, H * W * C, C, kw.get("h", h.data_ptr()), F, H * W * F, kw.get("p", packed.data_ptr()), None,
                         c.data_ptr(), c_new.data_ptr(), kw.get("ho", h_out.data_ptr()), F, None, kw.get("B", B), H, W, F,
                         kw.get("kh", k), k, kw.get("act", 1), None]
    assert L.fov_convlstm_cell_fwd_bf16(*args()) == 0
    assert L.fov_convlstm_cell_fwd_bf16(*args(B=0)) == 0                                          # the empty batch
    assert L.fov_convlstm_cell_fwd_bf16(*args(kh=2)) == _lib.ERR_INVALID                          # even kernel
    assert L.fov_convlstm_cell_fwd_bf16(*args(act=2)) == _lib.ERR_INVALID                         # sigmoid / hard_sigmoid only
    assert L.fov_convlstm_cell_fwd_bf16(*args(p=None)) == _lib.ERR_INVALID
    assert L.fov_convlstm_cell_fwd_bf16(*args(p=packed.data_ptr() + 4)) == _lib.ERR_INVALID       # packed weights: 16-byte aligned
    assert L.fov_convlstm_cell_fwd_bf16(*args(ho=h.data_ptr())) == _lib.ERR_INVALID               # h must not alias h_prev
    assert b"fov_convlstm_cell_fwd_bf16" in L.fov_last_error()
    assert L.fov_convlstm_cell_pack_bf16(KR.data_ptr(), packed.data_ptr(), C + F, F, 2, k, None) == _lib.ERR_INVALID
    assert L.fov_convlstm_cell_pack_bf16(KR.data_ptr(), packed.data_ptr() + 4, C + F, F, k, k, None) == _lib.ERR_INVALID
    with pytest.raises(AssertionError):
        ops.convlstm_cell_bf16(x, h, KR, None, c, h_out, packed=packed[:-16])                     # a buffer packed for another shape
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------
# saturated regime
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "plain"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", REGIME_SHAPES)
def test_convlstm_cell_bf16_with_overflowing_arguments(shape, act, form):
    """O.regime_convlstm_cell (R3: saturated gates, a wide cell state, pre-activations beyond +-200) against the rounded-operand
    reference in fp64: 1e-5 max|ref| per tensor and the written fp32 bound per element; finite, gates in [0, 1], |h| <= 1."""
    from longterm360fov_amd import ops
    B, H, W, C, F, k = shape
    p = O.regime_convlstm_cell(40 + C, B, H, W, C, F, k, act)
    ref = cell_bf16_ref(*[p[n].astype(np.float64) for n in ("x", "h", "c", "K", "R", "b")], act)
    KR = torch.cat([dev(p["K"]), dev(p["R"])], 2).contiguous()
    with plain_form(form == "plain"):
        got = run_cell(ops, dev(p["x"]), dev(p["h"]), KR, dev(p["b"]), dev(p["c"]), act, F, None)
        torch.cuda.synchronize()
    tag = "regime cell_bf16 %s %s %s" % (shape, act, form)
    for n, t in zip(("h", "c", "gates"), got):
        e = O.regime_error(host(t), ref[n], "f32")
        print("%s %s: %.3f of the written bound" % (tag, n, e))
        op_close(t, ref[n], "%s %s" % (tag, n))
        assert e <= 1.0, (tag, n)
    hh, g = host(got[0]), host(got[2])
    assert np.abs(hh).max() <= 1.0 and np.abs(g).max() <= 1.0 and g[..., :2 * F].min() >= 0.0 and g[..., 3 * F:].min() >= 0.0, tag


# ---------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------
def _model_check(name, out, enc, dec0, w, T_out, head, act, head_bf16):
    e64, d64 = enc.astype(np.float64), dec0.astype(np.float64)
    ref_t = cells_bf16_forward(e64, d64, f64(w), T_out, head, act, head_bf16)
    ref_l = O.convlstm_seq2seq_forward(e64, d64, f64(w), T_out, head, act)
    t, l = worst(out, ref_t, TIGHT), worst(out, ref_l, LOOSE)
    print("%s: %.3f of TIGHT (max abs %.3e), %.3f of LOOSE (max abs %.3e)"
          % (name, t, np.abs(out - ref_t).max(), l, np.abs(out - ref_l).max()))
    assert np.isfinite(out).all()
    assert t <= 1.0 and l <= 1.0


@pytest.mark.parametrize("name,head,B,T_in,T_out,H,W,C,L,hf,seed,dtype,act", MODEL_CASES)
def test_bf16_cells_predict_small_models(name, head, B, T_in, T_out, H, W, C, L, hf, seed, dtype, act):
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    w = O.init_convlstm_seq2seq(seed, C=C, latent_dim=L, head=head, head_filters=hf)
    enc, dec0 = small_inputs(head, B, T_in, H, W, C)
    m = ConvLSTMSeq2Seq(w, head=head, recurrent_activation=act, dtype=dtype, cell_dtype="bf16")
    out = m.predict([enc, dec0], predict_step=T_out)
    _model_check("%s, %s head, %s" % (name, dtype, act), out, enc, dec0, w, T_out, head, act, dtype == "bf16")
    np.testing.assert_allclose(out.sum(-1), 1.0, atol=1e-5)
    np.testing.assert_array_equal(out, m.predict_on_batch([enc, dec0], predict_step=T_out))
    f32 = ConvLSTMSeq2Seq(w, head=head, recurrent_activation=act, dtype=dtype).predict([enc, dec0], predict_step=T_out)
    assert np.abs(out - f32).max() > 0                      # the bf16 cells are really taken


def test_bf16_cells_predict_full_size():
    """configs[3] at full size (B 256, T 10 -> 10, head 512 -> 1024 -> 30), cells and head in bf16: two sequences of the batch
    against both restatements."""
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    T = FULL["T"]
    x, d0 = full_inputs()
    w = full_weights()
    m = ConvLSTMSeq2Seq(w, head="conv2d", dtype="bf16", cell_dtype="bf16")
    out = m.predict([x, d0], predict_step=T)
    assert out.shape == (FULL["B"], T, FULL["H"], FULL["W"], FULL["C"]) and np.isfinite(out).all()
    np.testing.assert_allclose(out.sum(-1), 1.0, atol=1e-5)
    rows = FULL_ROWS[1:3]
    _model_check("configs[3] full size, all bf16, two sequences", out[rows], x[rows], d0[rows], w, T, "conv2d", "hard_sigmoid", True)


def _stepped_predict(w, enc, dec0, T_out, head_bf16, act="hard_sigmoid"):
    """predict_device of a 'conv2d' model with bf16 cells as the sequence of ops calls it makes: bf16 cells on packed [K ; R]
    stacks over 32-channel maps, three conv2d / conv2d_bf16, softmax, feedback."""
    from longterm360fov_amd import ops
    dw = {k: dev(v) for k, v in w.items()}
    xe, inp = dev(enc), dev(dec0)[:, 0]
    B, T_in, H, W, C = xe.shape
    pad = (-C) % 4
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    if pad:
        xe = torch.cat([xe, z(B, T_in, H, W, pad)], -1)
        inp = torch.cat([inp, z(B, H, W, pad)], -1)
    KR = {}
    for side in ("enc", "dec"):
        for l in range(3):
            K, R = dw["%s%d_K" % (side, l)], dw["%s%d_R" % (side, l)]
            if l == 0 and pad:
                K = torch.cat([K, z(*(K.shape[:2] + (pad, K.shape[3])))], 2)
            KR[side, l] = torch.cat([K, R], 2).contiguous()
    filters = [dw["enc%d_R" % l].shape[2] for l in range(3)]
    offs = [0, filters[0], filters[0] + filters[1]]
    seq = [xe[:, t] for t in range(T_in)]
    states = []
    for l, F in enumerate(filters):
        h, c = z(B, H, W, F), z(B, H, W, F)
        nxt = []
        for t in range(T_in):
            hn = torch.empty((B, H, W, F), dtype=torch.float32, device="cuda")
            ops.convlstm_cell_bf16(seq[t], h, KR["enc", l], dw["enc%d_b" % l], c, hn, act)
            h = hn
            nxt.append(h)
        seq = nxt
        states.append([h, c])
    conv = ops.conv2d_bf16 if head_bf16 else ops.conv2d
    outs = []
    for t in range(T_out):
        feat = torch.empty((B, H, W, sum(filters)), dtype=torch.float32, device="cuda")
        cur = inp
        for l, F in enumerate(filters):
            hslot = feat[..., offs[l]:offs[l] + F]
            ops.convlstm_cell_bf16(cur, states[l][0], KR["dec", l], dw["dec%d_b" % l], states[l][1], hslot, act)
            states[l][0] = hslot
            cur = hslot
        y = conv(feat, dw["head0_W"], dw["head0_b"], activation="relu")
        y = conv(y, dw["head1_W"], dw["head1_b"], activation="relu")
        y = conv(y, dw["head2_W"], dw["head2_b"], activation="relu")
        y = ops.softmax_lastdim(y)
        outs.append(y)
        inp = inp.clone()
        inp[..., :C] = y
    return torch.stack(outs, 1)


def _onehot(rng, B, T, H=36, W=18, C=30):
    x = np.zeros((B, T, H, W, C), np.float32)
    idx = rng.integers(0, H * W, size=(B, T, C))
    bi, ti, ci = np.meshgrid(np.arange(B), np.arange(T), np.arange(C), indexing="ij")
    x[bi, ti, idx // W, idx % W, ci] = 1.0
    return x


CELL_P = sorted("%s%d_P" % (s, l) for s in ("enc", "dec") for l in range(3))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bf16_cells_predict_device_is_the_stepped_sequence_of_ops_calls(dtype):
    """Plumbing, exact: 36 x 18 maps (the patch-resident cell runs in all three layers), bit for bit the ops calls stepped by
    hand; the model with fp32 cells differs somewhere (the bf16 path is really taken) and agrees within LOOSE."""
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    w = O.init_convlstm_seq2seq(3, C=30, latent_dim=16, head="conv2d", head_filters=(64, 96))
    enc = _onehot(np.random.default_rng(4), 2, 2)
    dec0 = enc[:, -1:]
    m = ConvLSTMSeq2Seq(w, head="conv2d", dtype=dtype, cell_dtype="bf16")
    got = m.predict_device(dev(enc), dev(dec0), 2)
    assert torch.equal(got, _stepped_predict(w, enc, dec0, 2, dtype == "bf16"))
    head_p = ["head0_P", "head1_P", "head2_P"] if dtype == "bf16" else []
    assert sorted(k for k in m._dw if k.endswith("_P")) == sorted(CELL_P + head_p)
    f32 = ConvLSTMSeq2Seq(w, head="conv2d", dtype=dtype)
    ref = f32.predict_device(dev(enc), dev(dec0), 2)
    assert not any(k in f32._dw for k in CELL_P)
    assert not torch.equal(got, ref)
    assert worst(got.cpu().numpy(), ref.cpu().numpy(), LOOSE) <= 1.0


def test_default_cell_dtype_leaves_a_bf16_model_bit_for_bit():
    """dtype='bf16' alone keeps fp32 cells: cell_dtype='f32' spelled out, left out, and the hand-stepped fp32-cell sequence of
    tests/test_gpu_convlstm_bf16.py give the same bits."""
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    from test_gpu_convlstm_bf16 import _stepped_predict as stepped_f32_cells
    w = O.init_convlstm_seq2seq(3, C=30, latent_dim=16, head="conv2d", head_filters=(64, 96))
    enc = _onehot(np.random.default_rng(4), 2, 2)
    dec0 = enc[:, -1:]
    a = ConvLSTMSeq2Seq(w, head="conv2d", dtype="bf16").predict_device(dev(enc), dev(dec0), 2)
    b = ConvLSTMSeq2Seq(w, head="conv2d", dtype="bf16", cell_dtype="f32").predict_device(dev(enc), dev(dec0), 2)
    assert torch.equal(a, b) and torch.equal(a, stepped_f32_cells(w, enc, dec0, 2))


def test_bf16_cells_set_weights_rebuilds_the_packed_cells():
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    kw = dict(C=30, latent_dim=16, head="conv2d", head_filters=(64, 96))
    w1, w2 = O.init_convlstm_seq2seq(3, **kw), O.init_convlstm_seq2seq(8, **kw)
    enc = _onehot(np.random.default_rng(5), 2, 2)
    x = [enc, enc[:, -1:]]
    m = ConvLSTMSeq2Seq(w1, head="conv2d", dtype="bf16", cell_dtype="bf16")
    first = m.predict(x, predict_step=2)
    mixed = dict(w1)
    for k in w2:
        if k.endswith("_K") or k.endswith("_R"):
            mixed[k] = w2[k]               # different cell kernels only: nothing but a stale packed copy could hide them
    m.set_weights([mixed[k] for k in m._order])
    second = m.predict(x, predict_step=2)
    fresh = ConvLSTMSeq2Seq(mixed, head="conv2d", dtype="bf16", cell_dtype="bf16").predict(x, predict_step=2)
    np.testing.assert_array_equal(second, fresh)
    assert np.abs(second - first).max() > 0


def test_bf16_cells_batch_permutation_permutes_the_output():
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    w = O.init_convlstm_seq2seq(3, C=30, latent_dim=16, head="conv2d", head_filters=(64, 96))
    enc = _onehot(np.random.default_rng(6), 5, 2)
    perm = np.array([3, 0, 4, 1, 2])
    m = ConvLSTMSeq2Seq(w, head="conv2d", dtype="bf16", cell_dtype="bf16")
    out = m.predict([enc, enc[:, -1:]], predict_step=2)
    outp = m.predict([enc[perm], enc[perm][:, -1:]], predict_step=2)
    np.testing.assert_array_equal(outp, out[perm])
    assert np.abs(out[0] - out[1]).max() > 0
