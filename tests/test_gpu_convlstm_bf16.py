"""The ConvLSTM heat-map model's prediction head with bf16 matrix-core operands (fov_conv2d_pack_bf16, fov_conv2d_fwd_bf16,
ops.conv2d_bf16, ConvLSTMSeq2Seq(dtype='bf16')), through the C ABI.

Operator level: ops.conv2d_bf16 against conv2d_same(round_bf16(x), round_bf16(w)) + b in fp64, |gpu - ref| <= 1e-5 max|ref|
per element.  With identical rounded operands fp32 and fp64 accumulation differ by 1.1e-7 .. 2.3e-7 of max|ref| on these
shapes, the smallest operand mistake (weights left unrounded) moves the result by 1.6e-3 and truncation instead of
round-to-nearest-even by 6e-3: the bound is 40 x the reference's own noise and 160 x below the smallest mistake.

Model level: TIGHT against the bf16-operand restatement in fp64, LOOSE against the full-precision fp64 oracle, each as
tol * |ref| + 1e-5 (tests/test_convlstm_bf16_host.py holds the restatement, the cases and the CPU check of these bounds)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_convlstm_bf16_host import (ATOL, FULL, FULL_ROWS, LOOSE, SMALL_CASES, TIGHT, conv2d_bf16_ref, f64, full_inputs,  # noqa: E402
                                     full_weights, head_bf16_forward, small_inputs, worst)

pytestmark = pytest.mark.gpu

OP_TOL = 1e-5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def op_inputs(seed, B, H, W, C, N, kh, kw):
    """x = relu(N(0,1)), w Glorot-uniform, b = 0.05 N(0,1)."""
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((B, H, W, C)), 0).astype(np.float32)
    lim = np.sqrt(6.0 / (kh * kw * C + kh * kw * N))
    w = rng.uniform(-lim, lim, (kh, kw, C, N)).astype(np.float32)
    b = (0.05 * rng.standard_normal(N)).astype(np.float32)
    return x, w, b


def op_close(got, ref, tag):
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, tag
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    print("%s: max err %.3e = %.3e of max|ref|" % (tag, err, err / scale))
    assert np.isfinite(got).all(), tag
    assert (np.abs(got - ref) <= OP_TOL * scale).all(), "%s: max err %.3e of max|ref| %.3e" % (tag, err, scale)


class plain_form:
    """FOV_NO_CONV_PATCH=1 for the block: every conv2d_bf16 call on the plain kernel."""

    def __enter__(self):
        from longterm360fov_amd import _lib
        os.environ["FOV_NO_CONV_PATCH"] = "1"
        _lib.lib().fov_reload_env()

    def __exit__(self, *exc):
        from longterm360fov_amd import _lib
        os.environ.pop("FOV_NO_CONV_PATCH", None)
        _lib.lib().fov_reload_env()
        return False


# the three head layers at 36 x 18, its transpose, a 3 x 3 kernel, a narrow last block, B 1: shapes the map-resident form takes
FAST_SHAPES = [(3, 36, 18, 56, 512, 5, 5), (2, 36, 18, 512, 1024, 5, 5), (2, 36, 18, 1024, 30, 5, 5), (2, 18, 36, 64, 56, 3, 3),
               (1, 36, 18, 96, 40, 5, 5)]
# the Conv1D head's layers, small maps, ragged channel counts: the plain kernel
PLAIN_SHAPES = [(3, 1, 30, 56, 32, 1, 7), (3, 1, 30, 48, 3, 1, 7), (2, 9, 6, 22, 24, 5, 5), (2, 4, 5, 3, 7, 3, 3), (2, 4, 5, 17, 7, 3, 3),
                (1, 9, 6, 40, 17, 5, 5), (2, 36, 18, 30, 20, 5, 5), (2, 36, 18, 57, 20, 3, 3)]


@pytest.mark.parametrize("B,H,W,C,N,kh,kw", FAST_SHAPES + PLAIN_SHAPES)
def test_conv2d_bf16_against_the_rounded_operand_reference(B, H, W, C, N, kh, kw):
    """Both forms against the fp64 reference (never against each other), relu and linear, with and without bias, on a channel
    slice of a wider map and on one time step of a sequence; the same call twice is bit-identical; packing is deterministic."""
    from longterm360fov_amd import ops
    x, w, b = op_inputs(B * 1000 + C + N, B, H, W, C, N, kh, kw)
    ref = conv2d_bf16_ref(x.astype(np.float64), w.astype(np.float64), b.astype(np.float64))
    dx, dw, db = dev(x), dev(w), dev(b)
    packed = ops.conv2d_pack_bf16(dw)
    assert packed.dtype == torch.uint8 and torch.equal(packed, ops.conv2d_pack_bf16(dw))
    rng = np.random.default_rng(C)
    wide = np.maximum(rng.standard_normal((B, H, W, C + 12)), 0).astype(np.float32)
    seq = np.maximum(rng.standard_normal((B, 2, H, W, C)), 0).astype(np.float32)
    ref_wide = conv2d_bf16_ref(wide[..., 8:8 + C].astype(np.float64), w.astype(np.float64))
    ref_seq = conv2d_bf16_ref(seq[:, 1].astype(np.float64), w.astype(np.float64), b.astype(np.float64))

    def run(tag):
        got = ops.conv2d_bf16(dx, dw, db, packed=packed)
        op_close(got, ref, tag + " linear")
        assert torch.equal(got, ops.conv2d_bf16(dx, dw, db, packed=packed)), tag + ": not deterministic"
        assert torch.equal(got, ops.conv2d_bf16(dx, dw, db)), tag + ": packing inside the call gives another result"
        op_close(ops.conv2d_bf16(dx, dw, db, activation="relu", packed=packed), np.maximum(ref, 0), tag + " relu")
        op_close(ops.conv2d_bf16(dx, dw, packed=packed), ref - b, tag + " no bias")
        out = torch.full((B, H, W, N), float("nan"), device="cuda")
        assert ops.conv2d_bf16(dx, dw, db, out=out, packed=packed) is out and torch.equal(out, got)
        op_close(ops.conv2d_bf16(dev(wide)[..., 8:8 + C], dw, packed=packed), ref_wide, tag + " channel slice of a wider map")
        op_close(ops.conv2d_bf16(dev(seq)[:, 1], dw, db, activation="relu", packed=packed), np.maximum(ref_seq, 0),
                 tag + " batch-strided input")

    run("conv2d_bf16 %s" % ((B, H, W, C, N, kh, kw),))
    if (B, H, W, C, N, kh, kw) in FAST_SHAPES:
        with plain_form():
            run("conv2d_bf16 plain form %s" % ((B, H, W, C, N, kh, kw),))


def test_conv2d_bf16_rounds_both_operands_to_nearest_even():
    """The operand mistakes the bound must catch are caught: against the reference with the weights left unrounded, with the
    input left unrounded and with truncation instead of round-to-nearest-even the kernel is OUTSIDE the bound."""
    from longterm360fov_amd import ops
    B, H, W, C, N, kh, kw = 2, 36, 18, 56, 512, 5, 5
    x, w, b = op_inputs(11, B, H, W, C, N, kh, kw)
    got = ops.conv2d_bf16(dev(x), dev(w), dev(b)).cpu().numpy().astype(np.float64)
    x64, w64, b64 = x.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    trunc = lambda a: (a.astype(np.float32).view(np.uint32) & 0xFFFF0000).view(np.float32).astype(np.float64)
    wrong = {"weights unrounded": O.conv2d_same(O.round_bf16(x64), w64, b64),
             "input unrounded": O.conv2d_same(x64, O.round_bf16(w64), b64),
             "truncated": O.conv2d_same(trunc(x), trunc(w), b64)}
    for name, ref in wrong.items():
        e = float(np.abs(got - ref).max() / np.abs(ref).max())
        print("%s: %.3e of max|ref|" % (name, e))
        assert e > 10 * OP_TOL, name


def test_conv2d_bf16_empty_batch_and_errors():
    from longterm360fov_amd import ops, _lib
    x, w, b = op_inputs(5, 2, 9, 6, 8, 12, 3, 3)
    dw = dev(w)
    packed = ops.conv2d_pack_bf16(dw)
    y = ops.conv2d_bf16(torch.empty((0, 9, 6, 8), device="cuda"), dw, dev(b), packed=packed)
    assert y.shape == (0, 9, 6, 12)
    L = _lib.lib()
    assert L.fov_conv2d_bf16_packed_bytes(8, 12, 3, 3) == packed.numel() and packed.numel() % 16 == 0
    dx, out = dev(x), torch.empty((2, 9, 6, 12), device="cuda")
    args = lambda **k: [k.get("x", dx.data_ptr()), 8, 9 * 6 * 8, k.get("p", packed.data_ptr()), None, out.data_ptr(), 2, 9, 6, 8, 12,
                        k.get("kh", 3), 3, k.get("act", 0), None]
    assert L.fov_conv2d_fwd_bf16(*args()) == 0
    assert L.fov_conv2d_fwd_bf16(*args(kh=2)) == _lib.ERR_INVALID                         # even kernel
    assert L.fov_conv2d_fwd_bf16(*args(act=1)) == _lib.ERR_INVALID                        # activations 0 and 2 only
    assert L.fov_conv2d_fwd_bf16(*args(p=None)) == _lib.ERR_INVALID
    assert L.fov_conv2d_fwd_bf16(*args(p=packed.data_ptr() + 4)) == _lib.ERR_INVALID      # packed weights: 16-byte aligned
    assert b"fov_conv2d_fwd_bf16" in L.fov_last_error()
    assert L.fov_conv2d_pack_bf16(dw.data_ptr(), packed.data_ptr(), 8, 12, 2, 3, None) == _lib.ERR_INVALID
    with pytest.raises(AssertionError):
        ops.conv2d_bf16(dx, dw, packed=packed[:-16])                                      # a buffer packed for another shape
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------
def _model_check(name, out, enc, dec0, w, T_out, head):
    ref_t = head_bf16_forward(enc.astype(np.float64), dec0.astype(np.float64), f64(w), T_out, head)
    ref_l = O.convlstm_seq2seq_forward(enc.astype(np.float64), dec0.astype(np.float64), f64(w), T_out, head)
    t, l = worst(out, ref_t, TIGHT), worst(out, ref_l, LOOSE)
    print("%s: %.3f of TIGHT (max abs %.3e), %.3f of LOOSE (max abs %.3e)"
          % (name, t, np.abs(out - ref_t).max(), l, np.abs(out - ref_l).max()))
    assert np.isfinite(out).all()
    assert t <= 1.0 and l <= 1.0


@pytest.mark.parametrize("name,head,B,T_in,T_out,H,W,C,L,hf,seed", SMALL_CASES)
def test_bf16_predict_small_models(name, head, B, T_in, T_out, H, W, C, L, hf, seed):
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    w = O.init_convlstm_seq2seq(seed, C=C, latent_dim=L, head=head, head_filters=hf)
    enc, dec0 = small_inputs(head, B, T_in, H, W, C)
    m = ConvLSTMSeq2Seq(w, head=head, dtype="bf16")
    out = m.predict([enc, dec0], predict_step=T_out)
    _model_check(name, out, enc, dec0, w, T_out, head)
    np.testing.assert_allclose(out.sum(-1), 1.0, atol=1e-5)
    np.testing.assert_array_equal(out, m.predict_on_batch([enc, dec0], predict_step=T_out))


def test_bf16_predict_full_size():
    """configs[3] at full size (B 256, T 10 -> 10, head 512 -> 1024 -> 30): five sequences spread over the batch against both
    restatements; the same rows predicted as a small batch agree with the full batch within TIGHT (a last-bit difference in
    a cell output can flip one bf16 rounding in the head); the fp32 model's output differs somewhere and agrees within
    LOOSE."""
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    T = FULL["T"]
    x, d0 = full_inputs()
    w = full_weights()
    m = ConvLSTMSeq2Seq(w, head="conv2d", dtype="bf16")
    out = m.predict([x, d0], predict_step=T)
    assert out.shape == (FULL["B"], T, FULL["H"], FULL["W"], FULL["C"]) and np.isfinite(out).all()
    np.testing.assert_allclose(out.sum(-1), 1.0, atol=1e-5)
    rows = FULL_ROWS
    _model_check("configs[3] full size, five sequences", out[rows], x[rows], d0[rows], w, T, "conv2d")
    small = m.predict([x[rows], d0[rows]], predict_step=T)
    s = worst(small, out[rows], TIGHT)
    print("small batch vs full batch: %.3f of TIGHT" % s)
    assert s <= 1.0
    f32 = ConvLSTMSeq2Seq(w, head="conv2d").predict([x[rows], d0[rows]], predict_step=T)
    d = worst(small, f32, LOOSE)
    print("bf16 vs fp32 model: max abs difference %.3e, %.3f of LOOSE" % (np.abs(small - f32).max(), d))
    assert d <= 1.0 and np.abs(small - f32).max() > 0


def _stepped_predict(w, enc, dec0, T_out, act="hard_sigmoid"):
    """predict_device of a bf16 'conv2d' model as the sequence of ops calls it makes: fp32 cells on [K ; R] stacks over
    32-channel maps, three conv2d_bf16, softmax, feedback."""
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
            ops.convlstm_cell(seq[t], h, KR["enc", l], dw["enc%d_b" % l], c, hn, act)
            h = hn
            nxt.append(h)
        seq = nxt
        states.append([h, c])
    outs = []
    for t in range(T_out):
        feat = torch.empty((B, H, W, sum(filters)), dtype=torch.float32, device="cuda")
        cur = inp
        for l, F in enumerate(filters):
            hslot = feat[..., offs[l]:offs[l] + F]
            ops.convlstm_cell(cur, states[l][0], KR["dec", l], dw["dec%d_b" % l], states[l][1], hslot, act)
            states[l][0] = hslot
            cur = hslot
        y = ops.conv2d_bf16(feat, dw["head0_W"], dw["head0_b"], activation="relu")
        y = ops.conv2d_bf16(y, dw["head1_W"], dw["head1_b"], activation="relu")
        y = ops.conv2d_bf16(y, dw["head2_W"], dw["head2_b"], activation="relu")
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


def test_bf16_predict_device_is_the_stepped_sequence_of_ops_calls():
    """Plumbing, exact: 36 x 18 maps with a 64 -> 96 head (the map-resident kernel runs), bit for bit the ops calls stepped by
    hand; the fp32 model of the same weights differs somewhere (the bf16 path is really taken) and agrees within LOOSE."""
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    w = O.init_convlstm_seq2seq(3, C=30, latent_dim=16, head="conv2d", head_filters=(64, 96))
    enc = _onehot(np.random.default_rng(4), 2, 2)
    dec0 = enc[:, -1:]
    m = ConvLSTMSeq2Seq(w, head="conv2d", dtype="bf16")
    got = m.predict_device(dev(enc), dev(dec0), 2)
    assert torch.equal(got, _stepped_predict(w, enc, dec0, 2))
    assert sorted(k for k in m._dw if k.endswith("_P")) == ["head0_P", "head1_P", "head2_P"]
    f32 = ConvLSTMSeq2Seq(w, head="conv2d")
    ref = f32.predict_device(dev(enc), dev(dec0), 2)
    assert not any(k.endswith("_P") for k in f32._dw)
    assert not torch.equal(got, ref)
    assert worst(got.cpu().numpy(), ref.cpu().numpy(), LOOSE) <= 1.0


def test_bf16_set_weights_rebuilds_the_packed_head():
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    kw = dict(C=30, latent_dim=16, head="conv2d", head_filters=(64, 96))
    w1, w2 = O.init_convlstm_seq2seq(3, **kw), O.init_convlstm_seq2seq(8, **kw)
    enc = _onehot(np.random.default_rng(5), 2, 2)
    x = [enc, enc[:, -1:]]
    m = ConvLSTMSeq2Seq(w1, head="conv2d", dtype="bf16")
    first = m.predict(x, predict_step=2)
    mixed = dict(w1)
    for k in w2:
        if k.startswith("head"):
            mixed[k] = w2[k]               # different head weights only: a stale packed copy would go unnoticed by the cells
    m.set_weights([mixed[k] for k in m._order])
    second = m.predict(x, predict_step=2)
    fresh = ConvLSTMSeq2Seq(mixed, head="conv2d", dtype="bf16").predict(x, predict_step=2)
    np.testing.assert_array_equal(second, fresh)
    assert np.abs(second - first).max() > 0


def test_bf16_predict_trajectories_equals_predict_on_host_built_maps():
    from longterm360fov_amd import utility
    from longterm360fov_amd.models import ConvLSTMSeq2Seq

    def host_maps(xyz):
        ti, pi = utility.theta_phi_index_for_onehot(xyz)
        return utility.create_one_hot(ti, pi).transpose(0, 1, 3, 4, 2).astype(np.float32)

    rng = np.random.default_rng(3)
    w = O.init_convlstm_seq2seq(1234, C=30, latent_dim=8, k=3, head="conv2d", head_filters=(24, 40))
    v = rng.standard_normal((3, 3, 30, 3))
    enc_xyz = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    dec_xyz = enc_xyz[:, -1:]
    m = ConvLSTMSeq2Seq(w, head="conv2d", dtype="bf16")
    ref = m.predict([host_maps(enc_xyz), host_maps(dec_xyz)], predict_step=2)
    got = m.predict_trajectories(enc_xyz, dec_xyz, predict_step=2)
    assert got.shape == (3, 2, 36, 18, 30)
    np.testing.assert_array_equal(got, ref)
    got2 = m.predict_trajectories(torch.from_numpy(enc_xyz[:, :, None]).cuda(), torch.from_numpy(dec_xyz).cuda(), batch_size=2,
                                  predict_step=2)
    np.testing.assert_array_equal(got2, m.predict([host_maps(enc_xyz), host_maps(dec_xyz)], batch_size=2, predict_step=2))
