"""The 2- and 3-layer seq2seq model's training graph as one launch per direction (fov_stacked_seq2seq_train_fwd / _bwd,
lstm_stacked_train.hip), the grouped weight gradients (fov_lstm_seq_wgrad_layers), and the trainer / model paths built on them.

References: the fp64 autograd graph test_gpu_train._torch_stacked_graph (loss, prediction, every weight gradient) and
oracle.fov_oracle (stacked_seq2seq_forward; lstm_layer_train / lstm_layer_backward in fp64 for the tapes: h, the activated gates,
c, and dz), which must agree with each other to 1e-10 before anything is compared with the GPU.

Bounds - the project's own, from test_gpu_train.test_stacked_seq2seq_layers:
    prediction  atol 2e-5          loss  1e-5 relative + 1e-9          every gradient (and dz tape)  1e-4 max|ref| + 1e-9
    tapes (h, gates, c)  2e-5 max(1, max|ref|)
Shapes are the smallest at which each seam exists (ragged tiles B 1 / 16 / 17 / 33, T 1 / 2 / 3 for both LDS parities, T = 0 on
the forward, the K_0 k-block seams F_enc 1 / 6 / 16 / 17 / 90 / 96, F_dec 1 / 6 / 8): they are not the workload's."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_defer_order as DO
import test_gpu_train as TR
from oracle import fov_oracle as O
from test_guarded_views_host import OutView, guarded, same_bits

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def names(L):
    return ["%s%d_%s" % (side, l, k) for side in ("enc", "dec") for l in range(L) for k in "KRb"]


def _weights(L, H, F_enc, F_dec):
    """As tests/test_gpu_train.py::test_stacked_seq2seq_layers builds them."""
    rng = np.random.default_rng(L * 1000 + H + 7 * F_enc + 131 * F_dec)
    w = {}
    for side, f0 in (("enc", F_enc), ("dec", F_dec)):
        for l in range(L):
            k_, r_, b_ = O.init_lstm(rng, f0 if l == 0 else H, H)
            w["%s%d_K" % (side, l)], w["%s%d_R" % (side, l)] = k_, r_
            w["%s%d_b" % (side, l)] = (b_ + 0.1 * rng.standard_normal(4 * H)).astype(np.float32)
    w["dense_W"] = rng.uniform(-0.3, 0.3, (H, F_dec)).astype(np.float32)
    w["dense_b"] = rng.uniform(-0.1, 0.1, F_dec).astype(np.float32)
    return w


@functools.lru_cache(maxsize=None)
def _case(L, H, F_enc, F_dec, B, T_in, T_out, act):
    """Weights, inputs and the fp64 reference of one case, computed once and shared (nobody writes into them).
    ref: enc_hs / enc_res / dec_hs / dec_res / hT / cT as the forward lays them out, y, loss, dhs_top (the head's input gradient
    of the mean squared error), enc_dz / dec_dz, and g: every weight gradient."""
    w = _weights(L, H, F_enc, F_dec)
    rng = np.random.default_rng(B * 100 + T_in * 10 + T_out)
    enc = rng.uniform(-1, 1, (B, T_in, F_enc)).astype(np.float32)
    dec_in = rng.uniform(-1, 1, (B, T_out, F_dec)).astype(np.float32)
    tgt = rng.uniform(-0.9, 0.9, (B, T_out, F_dec)).astype(np.float32)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    r = {}
    x, est = enc.astype(np.float64), []
    for l in range(L):
        hs, h, c, res = O.lstm_layer_train(x, w64["enc%d_K" % l], w64["enc%d_R" % l], w64["enc%d_b" % l], act=act)
        est.append((x, hs, res, h, c))
        x = hs
    x, dst = dec_in.astype(np.float64), []
    for l in range(L):
        hs, _, _, res = O.lstm_layer_train(x, w64["dec%d_K" % l], w64["dec%d_R" % l], w64["dec%d_b" % l], est[l][3], est[l][4], act=act)
        dst.append((x, hs, res))
        x = hs
    r["enc_hs"], r["enc_res"] = np.stack([s[1] for s in est]), np.stack([s[2] for s in est])
    r["dec_hs"], r["dec_res"] = np.stack([s[1] for s in dst]), np.stack([s[2] for s in dst])
    r["hT"], r["cT"] = np.stack([s[3] for s in est]), np.stack([s[4] for s in est])
    y = np.tanh(x @ w64["dense_W"] + w64["dense_b"])
    r["y"] = y
    if T_out:
        np.testing.assert_allclose(y, O.stacked_seq2seq_forward(enc.astype(np.float64), dec_in.astype(np.float64), w64, L, act), atol=1e-12)
    n = max(y.size, 1)
    r["loss"] = float(((y - tgt) ** 2).sum() / n)
    dpre = 2.0 * (y - tgt) / n * (1.0 - y * y)
    r["dhs_top"] = dpre @ w64["dense_W"].T
    if not (T_in and T_out):      # forward-only cases
        for a in list(w.values()) + [enc, dec_in, tgt] + [v for v in r.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        return w, enc, dec_in, tgt, r
    g = {"dense_W": x.reshape(-1, H).T @ dpre.reshape(-1, F_dec), "dense_b": dpre.reshape(-1, F_dec).sum(0)}
    d_cur, dstate, ddz, edz = r["dhs_top"], [None] * L, [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        b = O.lstm_layer_backward(dst[l][0], w64["dec%d_K" % l], w64["dec%d_R" % l], est[l][3], est[l][4], dst[l][1], dst[l][2],
                                  dhs=d_cur, act=act)
        g["dec%d_K" % l], g["dec%d_R" % l], g["dec%d_b" % l] = b["dK"], b["dR"], b["db"]
        d_cur, dstate[l], ddz[l] = b["dx"], (b["dh0"], b["dc0"]), b["dz"]
    d_cur = None
    for l in range(L - 1, -1, -1):
        b = O.lstm_layer_backward(est[l][0], w64["enc%d_K" % l], w64["enc%d_R" % l], None, None, est[l][1], est[l][2], dhs=d_cur,
                                  dhT=dstate[l][0], dcT=dstate[l][1], act=act)
        g["enc%d_K" % l], g["enc%d_R" % l], g["enc%d_b" % l] = b["dK"], b["dR"], b["db"]
        d_cur, edz[l] = b["dx"], b["dz"]
    r["dec_dz"], r["enc_dz"], r["g"] = np.stack(ddz), np.stack(edz), g
    loss_t, g_t, y_t = TR._torch_stacked_graph(enc, dec_in, tgt, w, L, act)      # the two references agree before either is used
    assert abs(loss_t - r["loss"]) <= 1e-12 and np.abs(y_t - y).max() <= 1e-12
    for k, v in g.items():
        assert np.abs(g_t[k] - v).max() <= 1e-10 * max(np.abs(v).max(), 1e-30) + 1e-14, k
    for a in list(w.values()) + [enc, dec_in, tgt] + [v for v in r.values() if isinstance(v, np.ndarray)] + list(g.values()):
        a.setflags(write=False)
    return w, enc, dec_in, tgt, r


def held_tape(what, got, ref):
    err = float(np.abs(got.astype(np.float64) - ref).max()) if ref.size else 0.0
    bound = 2e-5 * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    print("%-28s max|ref| %.3e  max err %.3e  bound %.1e" % (what, float(np.abs(ref).max()) if ref.size else 0.0, err, bound))
    assert err <= bound, (what, err, bound)


def held_grad(what, got, ref):
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    err = float(np.abs(got.astype(np.float64) - ref).max()) if ref.size else 0.0
    print("%-28s max|ref| %.3e  max err %.3e" % (what, scale, err))
    assert err <= 1e-4 * scale + 1e-9, (what, err, scale)


def held_step(what, loss, y, grads, r):
    """loss, prediction and every gradient of one training step against fp64."""
    print("%-28s loss %.9f ref %.9f" % (what, loss, r["loss"]))
    assert abs(loss - r["loss"]) <= 1e-5 * r["loss"] + 1e-9
    np.testing.assert_allclose(y, r["y"], atol=2e-5)
    for k, ref in r["g"].items():
        held_grad("%s grad %s" % (what, k), grads[k], ref)


TAPES = ("enc_hs", "enc_res", "dec_hs", "dec_res", "hT", "cT")

# L, H, F_enc, F_dec, B, T_in, T_out, act, off
PRIMITIVE_CASES = [(2, 32, 6, 6, 17, 3, 2, "sigmoid", 0), (3, 32, 17, 1, 1, 1, 3, "hard_sigmoid", 1),
                   (2, 64, 90, 8, 33, 2, 1, "hard_sigmoid", 0), (3, 64, 96, 6, 16, 1, 2, "sigmoid", 0),
                   (2, 32, 1, 6, 33, 2, 3, "sigmoid", 0), (3, 64, 16, 8, 17, 3, 1, "sigmoid", 0)]


def _shapes(L, H, B, T_in, T_out):
    return {"enc_hs": (L, B, T_in, H), "enc_res": (L, B, T_in, 5, H), "dec_hs": (L, B, T_out, H), "dec_res": (L, B, T_out, 5, H),
            "hT": (L, B, H), "cT": (L, B, H)}


def _layers(L, side, x0, hs, h0, dz, out):
    return [(x0 if l == 0 else hs[l - 1], hs[l], None if h0 is None else h0[l], dz[l], out["%s%d_K" % (side, l)],
             out["%s%d_R" % (side, l)], out["%s%d_b" % (side, l)]) for l in range(L)]


@pytest.mark.parametrize("L,H,F_enc,F_dec,B,T_in,T_out,act,off", PRIMITIVE_CASES)
def test_primitives_on_guarded_views(L, H, F_enc, F_dec, B, T_in, T_out, act, off):
    """train_fwd, train_bwd and lstm_seq_wgrad_layers on operands inside NaN buffers and outputs inside sentinel buffers: every
    sentinel survives, no NaN is left in a written view, and everything holds its fp64 bound.  off = 1: every operand and output
    starts one float behind a 16-byte boundary (the weight gradients then take the per-layer form)."""
    from longterm360fov_amd import ops
    w, enc, dec_in, _, r = _case(L, H, F_enc, F_dec, B, T_in, T_out, act)
    g = lambda a: guarded(a, off=off, device="cuda")
    gw = {k: g(w[k]) for k in names(L)}
    genc, gdec = g(enc), g(dec_in)
    views = {k: OutView(s, off=off, device="cuda") for k, s in _shapes(L, H, B, T_in, T_out).items()}
    tp = ops.stacked_seq2seq_train_fwd(genc, gdec, gw, L, act=act, out={k: v.v for k, v in views.items()})
    got = {k: views[k].result() for k in TAPES}
    for k in TAPES:
        held_tape("fwd %s" % k, got[k], r[k])
    # the inference forward: no tape pointer, the top layer's h alone - the same bits
    top = OutView((B, T_out, H), off=off, device="cuda")
    ops.stacked_seq2seq_train_fwd(genc, gdec, gw, L, act=act, tape=False, out={"top": top.v})
    assert same_bits(top.result(), got["dec_hs"][L - 1])
    # backward from the fp64 head gradient, on the GPU forward's own tapes
    dzv = {"enc_dz": OutView((L, B, T_in, 4 * H), off=off, device="cuda"), "dec_dz": OutView((L, B, T_out, 4 * H), off=off, device="cuda")}
    ops.stacked_seq2seq_train_bwd(tp, g(r["dhs_top"]), gw, L, act=act, scratch=ops.Scratch(), out={k: v.v for k, v in dzv.items()})
    for k in ("dec_dz", "enc_dz"):
        held_grad("bwd %s" % k, dzv[k].result(), r[k])
    gv = {k: OutView(w[k].shape, off=off, device="cuda") for k in names(L)}
    out = {k: v.v for k, v in gv.items()}
    ops.lstm_seq_wgrad_layers(_layers(L, "dec", gdec, tp["dec_hs"], tp["hT"], dzv["dec_dz"].v, out), scratch=ops.Scratch())
    ops.lstm_seq_wgrad_layers(_layers(L, "enc", genc, tp["enc_hs"], None, dzv["enc_dz"].v, out), scratch=ops.Scratch())
    for k in names(L):
        held_grad("wgrad %s" % k, gv[k].result(), r["g"][k])


@pytest.mark.parametrize("L,H,F_enc,F_dec,B,T_in,T_out,act", [(2, 32, 6, 6, 17, 0, 2, "sigmoid"), (3, 64, 90, 8, 5, 2, 0, "hard_sigmoid"),
                                                             (2, 64, 6, 6, 33, 0, 0, "sigmoid")])
def test_forward_without_encoder_or_decoder_steps(L, H, F_enc, F_dec, B, T_in, T_out, act):
    """T_in = 0: the decoder starts from zero states and hT / cT are zeros; T_out = 0: the encoder stack alone."""
    from longterm360fov_amd import ops
    w, enc, dec_in, _, r = _case(L, H, F_enc, F_dec, B, T_in, T_out, act)
    gw = {k: guarded(w[k], device="cuda") for k in names(L)}
    views = {k: OutView(s, device="cuda") for k, s in _shapes(L, H, B, T_in, T_out).items()}
    ops.stacked_seq2seq_train_fwd(guarded(enc, device="cuda"), guarded(dec_in, device="cuda"), gw, L, act=act,
                                  out={k: v.v for k, v in views.items()})
    for k in TAPES:
        held_tape("T_in %d T_out %d %s" % (T_in, T_out, k), views[k].result(), r[k])
    if T_in == 0:
        assert not views["hT"].result().any() and not views["cT"].result().any()


@pytest.mark.parametrize("L,H,act", [(2, 32, "sigmoid"), (3, 64, "hard_sigmoid")])
def test_rows_do_not_depend_on_their_tile_mates(L, H, act):
    """Row r of a B = 33 call equals the B = 1 call on that row bit for bit: the tapes and the dz tapes."""
    from longterm360fov_amd import ops
    F_enc, F_dec, B, T_in, T_out = 17, 6, 33, 3, 2
    w, enc, dec_in, _, r = _case(L, H, F_enc, F_dec, B, T_in, T_out, act)
    dw = {k: dev(w[k]) for k in names(L)}
    dtop = r["dhs_top"].astype(np.float32)

    def run(rows):
        tp = ops.stacked_seq2seq_train_fwd(dev(enc[rows]), dev(dec_in[rows]), dw, L, act=act)
        dz = ops.stacked_seq2seq_train_bwd(tp, dev(dtop[rows]), dw, L, act=act, scratch=ops.Scratch())
        return {k: host(v) for k, v in list(tp.items()) + list(dz.items()) if k != "top"}
    full = run(slice(0, B))
    for row in (0, 15, 16, 32):
        one = run(slice(row, row + 1))
        for k, v in one.items():
            assert same_bits(v, full[k][:, row:row + 1]), (k, row)


@pytest.fixture(scope="module")
def arena():
    return torch.empty(DO.ARENA_FLOATS, dtype=torch.float32, device="cuda")


def _wgrad_case(B, T1, T2, H, F, seed):
    """Two stacked layers of a decoder-like stack with their own time lengths: (x, hs, h0, dz) each, fp32 arrays."""
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
    return [(u(B, T1, F), u(B, T1, H), None, u(B, T1, 4 * H)), (u(B, T2, H), u(B, T2, H), u(B, H), u(B, T2, 4 * H))]


def _wgrad_refs(lays):
    out = []
    for x, hs, h0, dz in lays:
        B, T, H = hs.shape
        hp = np.concatenate([(np.zeros((B, H)) if h0 is None else h0.astype(np.float64))[:, None], hs[:, :-1].astype(np.float64)], axis=1)
        z = dz.astype(np.float64).reshape(B * T, -1)
        out += [x.astype(np.float64).reshape(B * T, -1).T @ z, hp.reshape(B * T, H).T @ z, z.sum(0)]
    return out


@pytest.mark.parametrize("B,T1,T2,H,F,form", [(17, 3, 2, 32, 6, "rows"), (33, 2, 3, 64, 90, "rows"), (70, 10, 3, 32, 6, "per layer")])
@pytest.mark.parametrize("acc", [0, 1])
def test_grouped_weight_gradients_equal_the_per_layer_calls(B, T1, T2, H, F, form, acc):
    """lstm_seq_wgrad_layers against lstm_seq_wgrad layer by layer, bit for bit (accumulate on and off), and against fp64; the
    third shape has more rows than the one-launch form takes, so the grouped call is the per-layer calls."""
    from longterm360fov_amd import ops
    lays = _wgrad_case(B, T1, T2, H, F, 7 * B + H)
    dl = [tuple(None if a is None else dev(a) for a in lay) for lay in lays]
    shapes = [s for x, hs, _, _ in lays for s in ((x.shape[2], 4 * H), (H, 4 * H), (4 * H,))]
    layout = DO.Layout(shapes)
    base = np.random.default_rng(3).uniform(-1, 1, layout.total).astype(np.float32)

    def fresh():
        flat, views = layout.new()
        flat.copy_(dev(base))
        return flat, views
    flat_g, vg = fresh()
    ops.lstm_seq_wgrad_layers([dl[i] + tuple(vg[3 * i:3 * i + 3]) for i in range(2)], accumulate=bool(acc), scratch=ops.Scratch())
    flat_p, vp = fresh()
    for i in range(2):
        x, hs, h0, dz = dl[i]
        ops.lstm_seq_wgrad(x, hs, dz, dK=vp[3 * i], dR=vp[3 * i + 1], db=vp[3 * i + 2], h0=h0, accumulate=bool(acc), scratch=ops.Scratch())
    assert torch.equal(flat_g, flat_p), form
    for i, (v, ref) in enumerate(zip(vg, _wgrad_refs(lays))):
        want = ref + (base[layout.offs[i]:layout.offs[i] + ref.size].reshape(ref.shape) if acc else 0.0)
        held_grad("%s wgrad view %d" % (form, i), host(v), want)


@pytest.mark.parametrize("acc", [0, 1])
def test_grouped_weight_gradients_keep_order_in_a_deferral_region(arena, capfd, acc):
    """Inside an open reduce_defer region with a pending split product over two of its outputs, the one-launch form flushes
    first: the same bits as without a region (the pattern of tests/test_gpu_defer_order.py)."""
    from longterm360fov_amd import ops
    B, T1, T2, H, F = 17, 3, 2, 32, 6
    lays = _wgrad_case(B, T1, T2, H, F, 11)
    dl = [tuple(None if a is None else dev(a) for a in lay) for lay in lays]
    layout = DO.Layout([s for x, hs, _, _ in lays for s in ((x.shape[2], 4 * H), (H, 4 * H), (4 * H,))])
    rng = np.random.default_rng(5)
    pending = {i: DO.Pending(rng, layout.shapes[i]) for i in (1, 5)}      # dR of the first layer, db of the second

    def writer(views, acc_, sc):
        ops.lstm_seq_wgrad_layers([dl[i] + tuple(views[3 * i:3 * i + 3]) for i in range(2)], accumulate=bool(acc_), scratch=sc)
    DO._check(layout, pending, writer, lambda _: _wgrad_refs(lays), acc, arena, 2e-5, capfd, "wgrad_rows: 4 problems")


def _trainer(w, L, act, fused):
    from longterm360fov_amd.training import StackedSeq2SeqTrainer
    tr = StackedSeq2SeqTrainer(w, L, act=act)
    tr.fused_stack = fused
    tr.fused_stack_max_batch = None      # (the dispatch's bound on the batch is a matter of speed; the large case is about the code)
    return tr


def _step(tr, enc, dec_in, tgt):
    loss, y = tr.forward_backward(dev(enc), dev(dec_in), dev(tgt))
    tr.ws.check(); tr.bwd_scratch.check()
    return float(loss.item()), host(y).copy(), {k: host(v).copy() for k, v in tr.g.items()}


# the third: more rows than the one-launch head and the one-launch weight gradients take (the three-call head, per-layer products)
TRAINER_CASES = [(2, 32, 6, 21, 3, 2, "sigmoid"), (3, 64, 90, 33, 2, 3, "hard_sigmoid"), (2, 32, 6, 1400, 2, 3, "sigmoid")]


@pytest.mark.parametrize("L,H,F_enc,B,T_in,T_out,act", TRAINER_CASES)
def test_trainer_fused_against_per_layer(L, H, F_enc, B, T_in, T_out, act, monkeypatch):
    """fused_stack True and False from the same weights: both hold the fp64 bounds for loss, prediction and every gradient;
    with the per-layer wrappers made to raise, the fused step still runs (it needs none of them)."""
    from longterm360fov_amd import ops
    w, enc, dec_in, tgt, r = _case(L, H, F_enc, 6, B, T_in, T_out, act)
    held_step("per-layer", *_step(_trainer(w, L, act, False), enc, dec_in, tgt), r)

    def boom(*a, **k):
        raise AssertionError("a per-layer launch")
    monkeypatch.setattr(ops, "lstm_seq_train", boom)
    monkeypatch.setattr(ops, "lstm_seq_bwd", boom)
    held_step("fused", *_step(_trainer(w, L, act, True), enc, dec_in, tgt), r)
    # validation: a forward of its own, no backward
    tr = _trainer(w, L, act, True)
    monkeypatch.setattr(ops, "stacked_seq2seq_train_bwd", boom)
    loss, y = tr._eval_forward(dev(enc), dev(dec_in), dev(tgt))
    assert abs(float(loss.item()) - r["loss"]) <= 1e-5 * r["loss"] + 1e-9
    np.testing.assert_allclose(host(y), r["y"], atol=2e-5)


@pytest.mark.parametrize("L,H,B,act", [(2, 32, 21, "sigmoid"), (3, 64, 33, "hard_sigmoid")])
def test_trainer_paths_agree_after_adam_steps(L, H, B, act):
    """After 3 Adam steps from the same weights the two paths' weights agree within 1e-5 max|w|, tensor by tensor."""
    w, enc, dec_in, tgt, _ = _case(L, H, 6, 6, B, 3, 2, act)
    out = []
    for fused in (True, False):
        tr = _trainer(w, L, act, fused)
        losses = [float(tr.train_step(dev(enc), dev(dec_in), dev(tgt)).item()) for _ in range(3)]
        tr.check()
        assert losses[-1] < losses[0]
        out.append(tr.weights_numpy())
    for k in out[0]:
        scale = float(np.abs(out[1][k]).max())
        err = float(np.abs(out[0][k] - out[1][k]).max())
        print("after 3 steps %-8s max|w| %.3e  max diff %.3e" % (k, scale, err))
        assert err <= 1e-5 * scale, (k, err, scale)
        assert float(np.abs(out[0][k] - w[k]).max()) > 0.0, k      # the step moved it


def test_knob_keeps_the_per_layer_path(monkeypatch):
    """Under FOV_NO_STACKED_TRAIN=1 the trainer and predict never reach the one-launch forward (made to raise here) and still
    hold the bounds; without the knob the same patch raises."""
    from longterm360fov_amd import ops
    from longterm360fov_amd.models import StackedSeq2SeqLSTM
    from longterm360fov_amd.training import stacked_weight_order
    L, H, B, T_in, T_out, act = 2, 32, 21, 3, 2, "sigmoid"
    w, enc, dec_in, tgt, r = _case(L, H, 6, 6, B, T_in, T_out, act)

    def boom(*a, **k):
        raise AssertionError("the one-launch forward")
    monkeypatch.setattr(ops, "stacked_seq2seq_train_fwd", boom)
    m = StackedSeq2SeqLSTM(num_encoder_tokens=6, latent_dim=H, num_layers=L, recurrent_activation=act)
    m.set_weights([w[k] for k in stacked_weight_order(L)])
    monkeypatch.setenv("FOV_NO_STACKED_TRAIN", "1")
    held_step("knob", *_step(_trainer(w, L, act, True), enc, dec_in, tgt), r)
    np.testing.assert_allclose(m.predict([enc, dec_in]), r["y"], atol=2e-5)
    monkeypatch.delenv("FOV_NO_STACKED_TRAIN")
    with pytest.raises(AssertionError, match="the one-launch forward"):
        _step(_trainer(w, L, act, True), enc, dec_in, tgt)
    with pytest.raises(AssertionError, match="the one-launch forward"):
        m.predict([enc, dec_in])


@pytest.mark.parametrize("H", [20, 32, 40])
def test_model_predict_and_fit(H):
    """predict against fp64 at a padded and an exact width; fit with validation and the accuracy metric lowers the loss; a
    padded model's padded slices stay zero through training."""
    from longterm360fov_amd.models import StackedSeq2SeqLSTM
    from longterm360fov_amd.training import PaddedTrainer, stacked_weight_order
    L, B, T_in, T_out, act = 2 + (H == 40), 40, 3, 2, "sigmoid"
    w, enc, dec_in, tgt, r = _case(L, H, 6, 6, B, T_in, T_out, act)
    m = StackedSeq2SeqLSTM(num_encoder_tokens=6, latent_dim=H, num_layers=L, recurrent_activation=act)
    m.set_weights([w[k] for k in stacked_weight_order(L)])
    np.testing.assert_allclose(m.predict([enc, dec_in]), r["y"], atol=2e-5)
    np.testing.assert_allclose(m.predict([enc, dec_in], batch_size=17), r["y"], atol=2e-5)
    m.compile(optimizer="Adam", loss="mean_squared_error", metrics=["accuracy"])
    h = m.fit([enc, dec_in], tgt, batch_size=16, epochs=2, validation_split=0.2)
    assert len(h.history["loss"]) == 2 and h.history["loss"][1] < h.history["loss"][0]
    assert "val_loss" in h.history and "acc" in h.history and "val_acc" in h.history
    tr = m._get_trainer()
    assert isinstance(tr, PaddedTrainer) == (H != 32)
    if H != 32:
        assert tr.padded_slices_are_zero()
    for k, v in zip(stacked_weight_order(L), m.get_weights()):
        assert v.shape == w[k].shape and float(np.abs(v - w[k]).max()) > 0.0, k


def test_model_dataset_methods():
    """predict_dataset equals predict on the arrays ds.batch hands out; evaluate_dataset and fit_dataset run."""
    import test_gpu_traj_dataset as TD
    from longterm360fov_amd.models import StackedSeq2SeqLSTM
    ds, _ = TD.case(1, False, True)
    m = StackedSeq2SeqLSTM(num_encoder_tokens=6, latent_dim=20, num_layers=2, seed=4)
    m.compile(optimizer="Adam")
    x, y = TD.host_arrays(m, ds, "mean_var")
    assert len(ds) > 0 and x[0].shape[2] == 6 and x[1].shape == y.shape
    for bs in (None, 5):
        pred = m.predict_dataset(ds, batch_size=bs)
        assert pred.shape == y.shape and np.array_equal(pred, m.predict(x, batch_size=bs))
    ev = m.evaluate_dataset(ds)
    assert ev["loss"] == m.evaluate(x, y, batch_size=len(y))
    h = m.fit_dataset(ds, batch_size=8, epochs=2, shuffle=False)
    assert len(h.history["loss"]) == 2 and h.history["loss"][1] < h.history["loss"][0]


def test_unsupported_shapes_are_refused_with_outputs_untouched():
    from longterm360fov_amd import ops
    from longterm360fov_amd._lib import ERR_UNSUPPORTED, FovError
    L, H, B, T_in, T_out = 2, 48, 5, 2, 2
    w = {k: dev(v) for k, v in _weights(L, H, 6, 6).items()}
    rng = np.random.default_rng(1)
    enc, dec_in = dev(rng.uniform(-1, 1, (B, T_in, 6))), dev(rng.uniform(-1, 1, (B, T_out, 6)))
    views = {k: OutView(s, device="cuda") for k, s in _shapes(L, H, B, T_in, T_out).items()}
    with pytest.raises(FovError) as e:
        ops.stacked_seq2seq_train_fwd(enc, dec_in, w, L, out={k: v.v for k, v in views.items()})
    assert e.value.code == ERR_UNSUPPORTED
    tp = {"enc_res": dev(rng.uniform(0, 1, (L, B, T_in, 5, H))), "dec_res": dev(rng.uniform(0, 1, (L, B, T_out, 5, H))),
          "cT": dev(rng.uniform(-1, 1, (L, B, H)))}
    dzv = {"enc_dz": OutView((L, B, T_in, 4 * H), device="cuda"), "dec_dz": OutView((L, B, T_out, 4 * H), device="cuda")}
    with pytest.raises(FovError) as e:
        ops.stacked_seq2seq_train_bwd(tp, dev(rng.uniform(-1, 1, (B, T_out, H))), w, L, out={k: v.v for k, v in dzv.items()})
    assert e.value.code == ERR_UNSUPPORTED
    for v in list(views.values()) + list(dzv.values()):
        assert v.untouched()
