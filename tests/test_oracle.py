"""Pins the CPU oracle: known-answer cases, torch.nn.LSTM cross-check, numpy<->C agreement,
and the committed LSTM golden vectors (tests/golden/lstm_small.npz, made by make_lstm_fixtures.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import c_oracle as C
from oracle import fov_oracle as O


def test_hard_sigmoid_known_answers():
    x = np.array([-3.0, -2.5, -1.0, 0.0, 1.0, 2.5, 3.0], np.float32)
    np.testing.assert_allclose(O.hard_sigmoid(x), [0, 0, 0.3, 0.5, 0.7, 1, 1], atol=1e-7)


def test_lstm_step_hand_computed():
    # H=1, F=1: z = x*K + h*R + b with all gates driven by the same scalar pre-activation
    K = np.array([[1.0, 2.0, 3.0, 4.0]], np.float64)
    R = np.array([[0.5, -0.5, 0.25, -0.25]], np.float64)
    b = np.array([0.1, 1.0, -0.1, 0.0], np.float64)
    x = np.array([[0.2]]); h = np.array([[0.4]]); c = np.array([[-0.3]])
    z = 0.2 * K[0] + 0.4 * R[0] + b                     # [0.5, 1.2, 0.6, 0.7]
    np.testing.assert_allclose(z, [0.5, 1.2, 0.6, 0.7], atol=1e-12)
    sig = lambda v: 1 / (1 + np.exp(-v))
    c1 = sig(1.2) * -0.3 + sig(0.5) * np.tanh(0.6)
    h1 = sig(0.7) * np.tanh(c1)
    hn, cn = O.lstm_step(x, h, c, K, R, b, "sigmoid")
    np.testing.assert_allclose([hn[0, 0], cn[0, 0]], [h1, c1], atol=1e-12)
    hs = lambda v: min(max(0.2 * v + 0.5, 0), 1)         # hard_sigmoid: 0.6, 0.74, 0.64
    c1 = hs(1.2) * -0.3 + hs(0.5) * np.tanh(0.6)
    h1 = hs(0.7) * np.tanh(c1)
    hn, cn = O.lstm_step(x, h, c, K, R, b, "hard_sigmoid")
    np.testing.assert_allclose([hn[0, 0], cn[0, 0]], [h1, c1], atol=1e-12)


@pytest.mark.parametrize("H,F", [(16, 6), (64, 90)])
def test_lstm_layer_matches_torch(H, F):
    """Independent implementation with the same gate order (i,f,g,o): W_ih = K^T, W_hh = R^T."""
    rng = np.random.default_rng(5)
    K, R, b = O.init_lstm(rng, F, H, np.float64)
    b = b + 0.1 * rng.standard_normal(b.shape)
    x = rng.standard_normal((7, 9, F))
    h0 = 0.3 * rng.standard_normal((7, H)); c0 = 0.3 * rng.standard_normal((7, H))
    hs, hT, cT = O.lstm_layer(x, K, R, b, h0, c0, "sigmoid")
    m = torch.nn.LSTM(F, H, batch_first=True).double()
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.from_numpy(K.T)); m.weight_hh_l0.copy_(torch.from_numpy(R.T))
        m.bias_ih_l0.copy_(torch.from_numpy(b)); m.bias_hh_l0.zero_()
        ths, (thT, tcT) = m(torch.from_numpy(x), (torch.from_numpy(h0)[None], torch.from_numpy(c0)[None]))
    np.testing.assert_allclose(hs, ths.numpy(), atol=1e-12)
    np.testing.assert_allclose(hT, thT[0].numpy(), atol=1e-12)
    np.testing.assert_allclose(cT, tcT[0].numpy(), atol=1e-12)


@pytest.mark.parametrize("act", [0, 1])
def test_c_oracle_matches_numpy(act):
    w = O.init_seq2seq(11, H=64, bias_noise=0.1)
    enc, dec0, tgt = O.synthetic_batch(12, 21, 6, 5)       # ragged vs the C tile of 8
    a = O.seq2seq_decode(enc, dec0, w, 5, act)
    b = C.seq2seq_decode(enc, dec0, w, 5, act)
    np.testing.assert_allclose(a, b, atol=2e-6)
    dec_in = np.concatenate([dec0, tgt[:, :-1]], axis=1)
    a = O.seq2seq_teacher_forced(enc, dec_in, w, act)
    b = C.seq2seq_teacher_forced(enc, dec_in, w, act)
    np.testing.assert_allclose(a, b, atol=2e-6)
    hs, hT, cT = O.lstm_layer(enc, w["enc_K"], w["enc_R"], w["enc_b"], act=act)
    chs, chT, ccT = C.lstm_layer(enc, w["enc_K"], w["enc_R"], w["enc_b"], act=act)
    np.testing.assert_allclose(hs, chs, atol=2e-6)
    np.testing.assert_allclose(cT, ccT, atol=2e-6)


def test_empty_batch():
    w = O.init_seq2seq(1, H=16)
    enc = np.zeros((0, 4, 90), np.float32); dec0 = np.zeros((0, 1, 6), np.float32)
    assert C.seq2seq_decode(enc, dec0, w, 3).shape == (0, 3, 6)


def test_meanvar_matches_reference_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "data_helpers.npz"))
    np.testing.assert_array_equal(O.meanvar_xyz(g["fut"]), g["gt_fut"])
    np.testing.assert_array_equal(O.meanvar_xyz(g["fut"].reshape(12, 10, 30, 3)), g["gt_fut_4d"])
    oth = g["pu_oth_fut"].transpose(1, 2, 0, 3).reshape(12, 10, 2, 30, 3)
    np.testing.assert_array_equal(O.meanvar_xyz_oth(oth), g["gt_oth_fut"])


def test_others_mixing_flatten_order():
    """Mixing input is user-major with the prediction LAST (given_others...py:261-264): a mixing
    matrix that only reads the last 6 inputs must reproduce tanh(pred)."""
    w = O.init_others_mixing(3, H=8, num_user=4, dtype=np.float64)
    w["mix_W"][:] = 0
    w["mix_W"][-6:] = np.eye(6)
    enc, dec0, tgt, oth = O.synthetic_batch(4, 3, 4, 3, num_others=3, dtype=np.float64)
    out = O.others_mixing_forward(enc, oth, dec0, w)
    # recompute step 0 by hand
    hs1, h1, c1 = O.lstm_layer(enc, w["enc1_K"], w["enc1_R"], w["enc1_b"])
    _, h2, c2 = O.lstm_layer(hs1, w["enc2_K"], w["enc2_R"], w["enc2_b"])
    h1, c1 = O.lstm_step(dec0[:, 0], h1, c1, w["dec1_K"], w["dec1_R"], w["dec1_b"])
    h2, c2 = O.lstm_step(h1, h2, c2, w["dec2_K"], w["dec2_R"], w["dec2_b"])
    p = O.dense(h2, w["dense_W"], w["dense_b"])
    np.testing.assert_allclose(out[:, 0], np.tanh(p), atol=1e-14)


def test_lstm_golden_vectors(golden_dir):
    """Committed input/output vectors (fp64 oracle run, stored fp32) guard against silent edits."""
    g = np.load(os.path.join(golden_dir, "lstm_small.npz"))
    for act in (0, 1):
        w = {k[2:]: g[k] for k in g.files if k.startswith("w_")}
        out = O.seq2seq_decode(g["enc"], g["dec0"], w, int(g["T_out"]), act)
        np.testing.assert_allclose(out, g["decode_act%d" % act], atol=5e-6)
        dec_in = np.concatenate([g["dec0"], g["tgt"][:, :-1]], axis=1)
        out = O.seq2seq_teacher_forced(g["enc"], dec_in, w, act)
        np.testing.assert_allclose(out, g["tf_act%d" % act], atol=5e-6)
    wm = {k[3:]: g[k] for k in g.files if k.startswith("wm_")}
    out = O.others_mixing_forward(g["enc"], g["oth"], g["dec0"], wm, 0)
    np.testing.assert_allclose(out, g["mix_act0"], atol=5e-6)


def test_bptt_matches_torch_autograd():
    """Closed-form BPTT of the oracle vs torch.autograd on the same teacher-forced graph (fp64)."""
    H, B, T_in, T_out = 12, 4, 5, 3
    w = {k: v.astype(np.float64) for k, v in O.init_seq2seq(31, H=H, bias_noise=0.2).items()}
    enc, dec0, tgt = O.synthetic_batch(32, B, T_in, T_out, dtype=np.float64)
    dec_in = np.concatenate([dec0, tgt[:, :-1]], axis=1)
    loss, g, y = O.seq2seq_loss_and_grads(enc, dec_in, tgt, w)
    tw = {k: torch.tensor(v, requires_grad=True) for k, v in w.items()}

    def layer(x, K, R, b, h, c):
        hs = []
        for t in range(x.shape[1]):
            z = x[:, t] @ K + b + h @ R
            i, f, gg, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])
            c = f * c + i * gg
            h = o * torch.tanh(c)
            hs.append(h)
        return torch.stack(hs, 1), h, c

    z0 = torch.zeros(B, H, dtype=torch.float64)
    _, h, c = layer(torch.tensor(enc), tw["enc_K"], tw["enc_R"], tw["enc_b"], z0, z0)
    hs, _, _ = layer(torch.tensor(dec_in), tw["dec_K"], tw["dec_R"], tw["dec_b"], h, c)
    ty = torch.tanh(hs @ tw["dense_W"] + tw["dense_b"])
    tl = torch.mean((ty - torch.tensor(tgt)) ** 2)
    tl.backward()
    assert abs(float(tl) - loss) < 1e-14
    np.testing.assert_allclose(y, ty.detach().numpy(), atol=1e-13)
    for k in w:
        np.testing.assert_allclose(g[k], tw[k].grad.numpy(), atol=1e-13, err_msg=k)


def test_bptt_hard_sigmoid_finite_differences():
    H, B = 6, 3
    w = {k: v.astype(np.float64) for k, v in O.init_seq2seq(41, H=H, bias_noise=0.3).items()}
    enc, dec0, tgt = O.synthetic_batch(42, B, 4, 3, dtype=np.float64)
    dec_in = np.concatenate([dec0, tgt[:, :-1]], axis=1)
    loss, g, _ = O.seq2seq_loss_and_grads(enc, dec_in, tgt, w, "hard_sigmoid")
    rng = np.random.default_rng(0)
    for k in w:
        for _ in range(4):
            idx = tuple(rng.integers(0, s) for s in w[k].shape)
            wp = {a: b.copy() for a, b in w.items()}; wp[k][idx] += 1e-6
            wm = {a: b.copy() for a, b in w.items()}; wm[k][idx] -= 1e-6
            fd = (O.seq2seq_loss_and_grads(enc, dec_in, tgt, wp, "hard_sigmoid")[0] -
                  O.seq2seq_loss_and_grads(enc, dec_in, tgt, wm, "hard_sigmoid")[0]) / 2e-6
            assert abs(fd - g[k][idx]) < 1e-7 + 1e-5 * abs(fd), (k, idx, fd, g[k][idx])


# ---------------------------------------------------------------------------------------------------------------
# bf16 rounding switches of the backward restatements (the references of tests/test_gpu_bf16_backward.py)
# ---------------------------------------------------------------------------------------------------------------
def _layer_train_before_switches(x, K, R, b, h0, c0, act):
    """lstm_layer_train / lstm_layer_backward as they read before the rounding switches: the pin of 'switches off =
    bit-identical'."""
    B, T, _ = x.shape
    H = R.shape[0]
    h = np.zeros((B, H)) if h0 is None else h0
    c = np.zeros((B, H)) if c0 is None else c0
    s = O.hard_sigmoid if act == "hard_sigmoid" else O.sigmoid
    hs, res = np.empty((B, T, H)), np.empty((B, T, 5, H))
    for t in range(T):
        z = x[:, t] @ K + b + h @ R
        i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
        c = f * c + i * g
        h = o * np.tanh(c)
        hs[:, t] = h
        res[:, t, 0], res[:, t, 1], res[:, t, 2], res[:, t, 3], res[:, t, 4] = i, f, g, o, c
    return hs, h, c, res


def _layer_backward_before_switches(x, K, R, h0, c0, hs, res, dhs, dhT, dcT, act):
    B, T, F = x.shape
    H = R.shape[0]
    h0 = np.zeros((B, H)) if h0 is None else h0
    c0 = np.zeros((B, H)) if c0 is None else c0
    dh = np.zeros((B, H)) if dhT is None else dhT.copy()
    dc = np.zeros((B, H)) if dcT is None else dcT.copy()
    dz_all = np.empty((B, T, 4 * H))
    ag = (lambda a: np.where((a > 0) & (a < 1), 0.2, 0.0)) if act == "hard_sigmoid" else (lambda a: a * (1 - a))
    for t in range(T - 1, -1, -1):
        i, f, g, o, c = (res[:, t, q] for q in range(5))
        c_prev = res[:, t - 1, 4] if t > 0 else c0
        if dhs is not None:
            dh = dh + dhs[:, t]
        tc = np.tanh(c)
        do = dh * tc
        dc = dc + dh * o * (1 - tc * tc)
        dz = np.concatenate([dc * g * ag(i), dc * c_prev * ag(f), dc * i * (1 - g * g), do * ag(o)], axis=1)
        dz_all[:, t] = dz
        dc = dc * f
        dh = dz @ R.T
    hprev = np.concatenate([h0[:, None], hs[:, :-1]], axis=1)
    dz2 = dz_all.reshape(B * T, 4 * H)
    return {"dx": (dz2 @ K.T).reshape(B, T, F), "dK": x.reshape(B * T, F).T @ dz2,
            "dR": hprev.reshape(B * T, H).T @ dz2, "db": dz2.sum(axis=0), "dh0": dh, "dc0": dc, "dz": dz_all}


def _layer_case(seed, B, T, F, H, state):
    rng = np.random.default_rng(seed)
    K, R, b = (a.astype(np.float64) for a in O.init_lstm(rng, F, H))
    b = b + 0.2 * rng.standard_normal(b.shape)
    x = rng.uniform(-1, 1, (B, T, F))
    h0 = 0.3 * rng.standard_normal((B, H)) if state else None
    c0 = 0.3 * rng.standard_normal((B, H)) if state else None
    up = [0.1 * rng.standard_normal(s) for s in ((B, T, H), (B, H), (B, H))]
    return x, K, R, b, h0, c0, up


@pytest.mark.parametrize("act,state", [("sigmoid", True), ("hard_sigmoid", False)])
def test_layer_rounding_switches_off_are_bit_identical(act, state):
    x, K, R, b, h0, c0, (dhs, dhT, dcT) = _layer_case(7, 5, 4, 6, 8, state)
    new = O.lstm_layer_train(x, K, R, b, h0, c0, act=act)
    old = _layer_train_before_switches(x, K, R, b, h0, c0, act)
    for u, v in zip(new, old):
        np.testing.assert_array_equal(u, v)
    hs, _, _, res = old
    gn = O.lstm_layer_backward(x, K, R, h0, c0, hs, res, dhs, dhT, dcT, act=act)
    go = _layer_backward_before_switches(x, K, R, h0, c0, hs, res, dhs, dhT, dcT, act)
    for k in go:
        np.testing.assert_array_equal(gn[k], go[k], err_msg=k)


def _torch_layer_grads(x, K, R, b, h0, c0, dhs, dhT, dcT, act, fwd, rec, dx, wgrad):
    """Independent reference: autograd through the layer with bf16_autograd's product -> (tapes, grads)."""
    from oracle import bf16_autograd as A
    B, T, _ = x.shape
    H = R.shape[0]
    t = {k: A.leaf(v) for k, v in (("x", x), ("K", K), ("R", R), ("b", b))}
    h = A.leaf(h0) if h0 is not None else torch.zeros(B, H, dtype=torch.float64)
    c = A.leaf(c0) if c0 is not None else torch.zeros(B, H, dtype=torch.float64)
    h_in, c_in, keep, hs = h, c, [], []
    for s in range(T):
        h, c = A.lstm_step(t["x"][:, s], h, c, t["K"], t["R"], t["b"], act, fwd, rec, dx, wgrad, keep)
        hs.append(h)
    hs = torch.stack(hs, 1)
    loss = (hs * torch.tensor(dhs)).sum() + (h * torch.tensor(dhT)).sum() + (c * torch.tensor(dcT)).sum()
    loss.backward()
    g = {"dx": t["x"].grad, "dK": t["K"].grad, "dR": t["R"].grad, "db": t["b"].grad,
         "dz": torch.stack([z.grad for z, _ in keep], 1)}
    if h0 is not None:
        g["dh0"], g["dc0"] = h_in.grad, c_in.grad
    tape = (hs.detach().numpy(), torch.stack([q for _, q in keep], 1).detach().numpy())
    return tape, {k: v.numpy() for k, v in g.items()}


@pytest.mark.parametrize("rec,dx,wgrad", [(True, True, True), (True, False, False), (False, True, False), (False, False, True),
                                          (False, False, False)])
@pytest.mark.parametrize("act,state", [("sigmoid", True), ("hard_sigmoid", False)])
def test_layer_backward_rounding_matches_autograd(rec, dx, wgrad, act, state):
    """Each switch of lstm_layer_backward against torch.autograd in fp64 with the bf16-operand product rounding exactly the
    same products (forward rounded too, through lstm_layer_train's switch), to 1e-10 of each tensor's scale."""
    x, K, R, b, h0, c0, (dhs, dhT, dcT) = _layer_case(11, 6, 5, 7, 8, state)
    (ths, tres), tg = _torch_layer_grads(x, K, R, b, h0, c0, dhs, dhT, dcT, act, True, rec, dx, wgrad)
    hs, _, _, res = O.lstm_layer_train(x, K, R, b, h0, c0, act=act, round_fwd=True)
    assert np.abs(hs - ths).max() <= 1e-12 and np.abs(res - tres).max() <= 1e-12
    g = O.lstm_layer_backward(x, K, R, h0, c0, hs, res, dhs, dhT, dcT, act=act, round_rec=rec, round_dx=dx, round_wgrad=wgrad)
    plain = O.lstm_layer_backward(x, K, R, h0, c0, hs, res, dhs, dhT, dcT, act=act)
    for k in tg:
        scale = np.abs(tg[k]).max()
        assert np.abs(g[k] - tg[k]).max() <= 1e-10 * scale + 1e-300, k
    # the switches do something: each rounded product moves its outputs by far more than the agreement above
    moved = {"dK": wgrad or rec, "dR": wgrad or rec, "dx": dx or rec, "dz": rec}
    for k, on in moved.items():
        d = np.abs(g[k] - plain[k]).max() / np.abs(plain[k]).max()
        assert (d > 1e-5) if on else (d < 1e-12), (k, d)


def _decoder_case(seed, B, T, H, O_, act):
    rng = np.random.default_rng(seed)
    w = {k: v.astype(np.float64) for k, v in O.init_others_mixing(seed, F_enc=5, F_dec=O_, H=H, num_user=3, bias_noise=0.2).items()}
    mix_Wp = w["mix_W"][-O_:]
    st = [0.4 * rng.standard_normal((B, H)) for _ in range(4)]
    dec0 = rng.uniform(-1, 1, (B, O_))
    oth = 0.3 * rng.standard_normal((B, T, O_))
    G = 0.2 * rng.standard_normal((T, B, O_))
    return w, mix_Wp, st, dec0, oth, G


def _torch_decoder(w, mix_Wp, st, dec0, oth, G, T, act, fwd, rec, dx):
    """Autograd through the unrolled decoder of oracle.mix_decoder_train_forward, loss sum_t <G_t, m_t>."""
    from oracle import bf16_autograd as A
    tw = {k: A.leaf(w[k]) for k in ("dec1_K", "dec1_R", "dec1_b", "dec2_K", "dec2_R", "dec2_b", "dense_W", "dense_b")}
    s0 = [A.leaf(a) for a in st]
    h1, c1, h2, c2 = s0
    x = torch.tensor(dec0)
    k1, k2, pre_p, pre_m, ms, ps = [], [], [], [], [], []
    for t in range(T):
        h1, c1 = A.lstm_step(x, h1, c1, tw["dec1_K"], tw["dec1_R"], tw["dec1_b"], act, fwd, rec, dx, False, k1)
        h2, c2 = A.lstm_step(h1, h2, c2, tw["dec2_K"], tw["dec2_R"], tw["dec2_b"], act, fwd, rec, dx, False, k2)
        a = A.mm(h2, tw["dense_W"], fwd) + tw["dense_b"]
        p = torch.tanh(a)
        zm = p @ torch.tensor(mix_Wp) + torch.tensor(oth[:, t])
        x = torch.tanh(zm)
        for v, l in ((a, pre_p), (zm, pre_m)):
            v.retain_grad()
            l.append(v)
        ms.append(x)
        ps.append(p)
    M = torch.stack(ms)
    (M * torch.tensor(G)).sum().backward()
    g = {"DZ1": torch.stack([z.grad for z, _ in k1]), "DZ2": torch.stack([z.grad for z, _ in k2]),
         "dpre_m": torch.stack([v.grad for v in pre_m]), "dpre_p": torch.stack([v.grad for v in pre_p]),
         "dh1_0": s0[0].grad, "dc1_0": s0[1].grad, "dh2_0": s0[2].grad, "dc2_0": s0[3].grad}
    tape = {"M": M, "P": torch.stack(ps), "res1": torch.stack([q for _, q in k1]), "res2": torch.stack([q for _, q in k2])}
    return {k: v.detach().numpy() for k, v in tape.items()}, {k: v.numpy() for k, v in g.items()}


@pytest.mark.parametrize("fwd,rec,dx", [(False, False, False), (True, True, True), (True, True, False), (True, False, True)])
@pytest.mark.parametrize("act", ["sigmoid", "hard_sigmoid"])
def test_mix_decoder_restatement_matches_autograd(fwd, rec, dx, act):
    """oracle.mix_decoder_train_forward / mix_decoder_backward (head, both layers, the feedback x_{t+1} = m_t) against
    torch.autograd in fp64 on the same decoder graph, to 1e-10 of each tensor's scale: rounding off, and with the bf16
    product rounding the recurrences and / or the data-gradient products of both layers."""
    B, T, H, O_ = 5, 4, 8, 3
    w, mix_Wp, st, dec0, oth, G = _decoder_case(3, B, T, H, O_, act)
    tt, tg = _torch_decoder(w, mix_Wp, st, dec0, oth, G, T, act, fwd, rec, dx)
    tp = O.mix_decoder_train_forward(dec0, *st, oth, w, mix_Wp, T, act=act, round_fwd=fwd)
    for k in tt:
        assert np.abs(tp[k] - tt[k]).max() <= 1e-12, k
    C1 = np.concatenate([st[1][None], tp["C1"]])        # row t = cell state before step t
    C2 = np.concatenate([st[3][None], tp["C2"]])
    dloss = G * (1 - tp["M"] ** 2)
    g = O.mix_decoder_backward(tp["M"], tp["P"], dloss, tp["res1"], tp["res2"], C1, C2, w, mix_Wp, act=act,
                               round_rec=rec, round_dx=dx)
    plain = O.mix_decoder_backward(tp["M"], tp["P"], dloss, tp["res1"], tp["res2"], C1, C2, w, mix_Wp, act=act)
    for k in tg:
        scale = np.abs(tg[k]).max()
        assert scale > 0 and np.abs(g[k] - tg[k]).max() <= 1e-10 * scale, (k, np.abs(g[k] - tg[k]).max(), scale)
    d = max(np.abs(g[k] - plain[k]).max() / np.abs(plain[k]).max() for k in ("DZ1", "dh1_0"))
    assert (d > 1e-5) if (rec or dx) else (d == 0)


def test_adam_matches_torch_with_keras_epsilon_placement():
    """Keras applies eps OUTSIDE the bias-corrected sqrt: p -= lr_t*m/(sqrt(v)+eps).  torch.optim.Adam
    uses eps/sqrt(1-b2^t) scaling differently, so compare against the formula, and against torch for a
    case where eps is negligible."""
    rng = np.random.default_rng(1)
    p = rng.standard_normal(50); g = rng.standard_normal(50)
    m = np.zeros(50); v = np.zeros(50)
    tp = torch.tensor(p.copy(), requires_grad=True)
    opt = torch.optim.Adam([tp], lr=1e-3, betas=(0.9, 0.999), eps=1e-30)
    for t in range(1, 4):
        O.adam_step(p, g, m, v, t, eps=1e-30)
        tp.grad = torch.tensor(g.copy()); opt.step()
    np.testing.assert_allclose(p, tp.detach().numpy(), atol=1e-12)
    a = np.zeros(50); q = rng.standard_normal(50); q0 = q.copy()
    O.rmsprop_step(q, g, a)
    np.testing.assert_allclose(q, q0 - 1e-3 * g / (np.sqrt(0.1 * g * g) + 1e-7), atol=1e-15)


def test_tf_lstmcell_equals_keras_cell_after_mapping():
    """The tf.contrib LSTMCell restatement and the Keras cell agree once the kernel is split, the
    gate columns permuted (i,j,f,o -> i,f,c,o) and forget_bias folded into the bias."""
    from longterm360fov_amd.models import convert_tf_lstmcell
    rng = np.random.default_rng(2)
    H, F, B = 5, 3, 4
    W = rng.standard_normal((F + H, 4 * H)); b = rng.standard_normal(4 * H)
    x = rng.standard_normal((B, F)); c = rng.standard_normal((B, H)); h = rng.standard_normal((B, H))
    c1, h1 = O.tf_lstm_cell_step(x, c, h, W, b, forget_bias=1.0)
    K, R, bk = convert_tf_lstmcell(W, b, 1.0)
    h2, c2 = O.lstm_step(x, h, c, K.astype(np.float64), R.astype(np.float64), bk.astype(np.float64), "sigmoid")
    np.testing.assert_allclose(h1, h2, atol=1e-6)
    np.testing.assert_allclose(c1, c2, atol=1e-6)


def test_xyz2thetaphi_matches_reference_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "data_helpers.npz"))
    th, ph = O.xyz2thetaphi(g["eval_xyz"][:, 0], g["eval_xyz"][:, 1], g["eval_xyz"][:, 2])
    np.testing.assert_array_equal(th, g["eval_theta"])
    np.testing.assert_array_equal(ph, g["eval_phi"])


def test_hit_rate_known_answers():
    e = lambda th, ph: np.array([np.cos(th + np.pi) * np.sin(ph), np.sin(th + np.pi) * np.sin(ph), -np.cos(ph)])
    # identical centres -> full overlap; far apart -> 0; half a span apart in theta -> 1/2
    a = e(0.3, 1.2)
    assert abs(O.fov_hit_rate(a[None], a[None])[0] - 1.0) < 1e-12
    assert O.fov_hit_rate(e(0.3, 1.2)[None], e(-2.5, 1.2)[None])[0] == 0.0
    half = O.fov_hit_rate(e(0.3 + np.pi / 3, 1.2)[None], e(0.3, 1.2)[None])[0]
    assert abs(half - 0.5) < 1e-9
    # straddling the theta seam: centres 20 degrees apart across +-pi must still overlap (5/6 in theta)
    seam = O.fov_hit_rate(e(np.pi - np.pi / 18, 1.2)[None], e(-np.pi + np.pi / 18, 1.2)[None])[0]
    assert abs(seam - (1 - (np.pi / 9) / (2 * np.pi / 3))) < 1e-9


def test_onelayer_no_teacher_forcing_oracle_properties():
    """FoV_seq2seq_no_teac_forc.py:29,98-99: with `decoder_no_init_state` the decoder starts from zero state, so the
    prediction cannot depend on the encoder input; seeded with the encoder state and without the optional links
    the model is exactly the autoregressive decode of FoV_seq2seq.py:154-178."""
    from oracle import fov_oracle as O
    w = {k: v.astype(np.float64) for k, v in O.init_seq2seq(5, H=16).items()}
    enc, dec0, _ = O.synthetic_batch(6, 4, 3, 5)
    enc, dec0 = enc.astype(np.float64), dec0.astype(np.float64)
    a = O.onelayer_tar_seq2seq_forward(enc, dec0, w, 5)
    b = O.onelayer_tar_seq2seq_forward(enc[::-1].copy(), dec0, w, 5)
    np.testing.assert_array_equal(a, b)
    c = O.onelayer_tar_seq2seq_forward(enc, dec0, w, 5, decoder_no_init_state=False)
    np.testing.assert_allclose(c, O.seq2seq_decode(enc, dec0, w, 5), atol=1e-15)
    assert np.abs(c - a).max() > 1e-4
    w["res_W"], w["res_b"] = np.eye(6) * 0.3, np.zeros(6)
    d = O.onelayer_tar_seq2seq_forward(enc, dec0, w, 5, decoder_no_init_state=False, add_residual_link=True)
    assert np.abs(d).max() <= 2.0 and np.abs(d - c).max() > 1e-4      # tanh + tanh
    # cfg.embed_frame_state_enc2dec (:47-52) only matters when the decoder is seeded; the reconstruction decoder (:56-59,
    # 120-126) is a second output that leaves the prediction alone and is bounded by its tanh head
    rng = np.random.default_rng(0)
    w.update(emb1_W=rng.normal(size=(16, 16)), emb1_b=np.zeros(16), emb2_W=rng.normal(size=(16, 16)), emb2_b=np.zeros(16))
    w["rec_K"], w["rec_R"], w["rec_b"] = (v.astype(np.float64) for v in O.init_lstm(rng, 90, 16))
    w["recd_W"], w["recd_b"] = rng.normal(size=(16, 90)) * 0.3, np.zeros(90)
    np.testing.assert_array_equal(O.onelayer_tar_seq2seq_forward(enc, dec0, w, 5, embed_frame_state_enc2dec=True), a)
    e = O.onelayer_tar_seq2seq_forward(enc, dec0, w, 5, decoder_no_init_state=False, embed_frame_state_enc2dec=True)
    assert np.abs(e - c).max() > 1e-4
    y, rec = O.onelayer_tar_seq2seq_forward(enc, dec0, w, 5, decoder_no_init_state=False, has_reconstruct_loss=True)
    np.testing.assert_array_equal(y, c)
    assert rec.shape == (4, 5, 90) and np.abs(rec).max() < 1.0
    _, rec2 = O.onelayer_tar_seq2seq_forward(enc[::-1].copy(), dec0, w, 5, has_reconstruct_loss=True)
    assert np.abs(rec2[::-1] - rec).max() < 1e-15       # the reconstruction is seeded by the encoder whatever decoder_no_init_state says


def _load_torch_lstm(m, layer, suffix, K, R, b):
    with torch.no_grad():
        getattr(m, "weight_ih_l%d%s" % (layer, suffix)).copy_(torch.from_numpy(K.T))
        getattr(m, "weight_hh_l%d%s" % (layer, suffix)).copy_(torch.from_numpy(R.T))
        getattr(m, "bias_ih_l%d%s" % (layer, suffix)).copy_(torch.from_numpy(b))
        getattr(m, "bias_hh_l%d%s" % (layer, suffix)).zero_()


def test_bidirectional_and_stacked_restatements_match_torch():
    """Independent implementations of the two sibling structures: torch.nn.LSTM(bidirectional=True) for the oracle's
    Keras-Bidirectional restatement (backward outputs reversed back, concat [fwd | bwd], per-direction final states) and
    torch.nn.LSTM(num_layers=2) with the encoder's per-layer final states as the decoder's initial states for the stacked
    seq2seq of Fov_seq2seq_2layers.py."""
    from oracle import fov_oracle as O
    rng = np.random.default_rng(17)
    B, T, F, H = 5, 6, 12, 8
    x = rng.standard_normal((B, T, F))
    wf = [a.astype(np.float64) for a in O.init_lstm(rng, F, H, np.float64)]
    wb = [a.astype(np.float64) for a in O.init_lstm(rng, F, H, np.float64)]
    wf[2] = wf[2] + 0.1 * rng.standard_normal(4 * H); wb[2] = wb[2] + 0.1 * rng.standard_normal(4 * H)
    seq, fh, fc, bh, bc = O.bidirectional_lstm(x, wf, wb)
    m = torch.nn.LSTM(F, H, batch_first=True, bidirectional=True).double()
    _load_torch_lstm(m, 0, "", *wf)
    _load_torch_lstm(m, 0, "_reverse", *wb)
    with torch.no_grad():
        ts, (th, tc) = m(torch.from_numpy(x))
    np.testing.assert_allclose(seq, ts.numpy(), atol=1e-12)
    np.testing.assert_allclose(np.stack([fh, bh]), th.numpy(), atol=1e-12)
    np.testing.assert_allclose(np.stack([fc, bc]), tc.numpy(), atol=1e-12)
    # seeded form (the list the first Bidirectional returns becomes the second one's initial state)
    init = tuple(0.3 * rng.standard_normal((B, H)) for _ in range(4))
    seq2 = O.bidirectional_lstm(x, wf, wb, init)[0]
    with torch.no_grad():
        ts2, _ = m(torch.from_numpy(x), (torch.from_numpy(np.stack([init[0], init[2]])), torch.from_numpy(np.stack([init[1], init[3]]))))
    np.testing.assert_allclose(seq2, ts2.numpy(), atol=1e-12)
    # two-layer teacher-forced seq2seq
    w = {}
    for side, f0 in (("enc", 6), ("dec", 6)):
        for l in range(2):
            K, R, b = O.init_lstm(rng, 6 if l == 0 else H, H, np.float64)
            w["%s%d_K" % (side, l)], w["%s%d_R" % (side, l)], w["%s%d_b" % (side, l)] = K, R, b + 0.1 * rng.standard_normal(4 * H)
    w["dense_W"], w["dense_b"] = rng.uniform(-0.3, 0.3, (H, 6)), rng.uniform(-0.1, 0.1, 6)
    enc, dec_in = rng.standard_normal((B, 4, 6)), rng.standard_normal((B, 5, 6))
    y = O.stacked_seq2seq_forward(enc, dec_in, w, 2)
    e, d = torch.nn.LSTM(6, H, 2, batch_first=True).double(), torch.nn.LSTM(6, H, 2, batch_first=True).double()
    for l in range(2):
        _load_torch_lstm(e, l, "", w["enc%d_K" % l], w["enc%d_R" % l], w["enc%d_b" % l])
        _load_torch_lstm(d, l, "", w["dec%d_K" % l], w["dec%d_R" % l], w["dec%d_b" % l])
    with torch.no_grad():
        _, st = e(torch.from_numpy(enc))
        hs, _ = d(torch.from_numpy(dec_in), st)
    np.testing.assert_allclose(y, np.tanh(hs.numpy() @ w["dense_W"] + w["dense_b"]), atol=1e-12)


def test_sampled_refeed_restatements():
    """lstm_keras.py's planar layout with the variance as stddev, and lstm.py's interleaved layout with sqrt(var): with zero
    noise the re-fed second is the predicted mean repeated over the frames in the respective layout."""
    from oracle import fov_oracle as O
    rng = np.random.default_rng(3)
    w0 = O.init_seq2seq(4, H=8)
    w = {"K": w0["enc_K"].astype(np.float64), "R": w0["enc_R"].astype(np.float64), "b": w0["enc_b"].astype(np.float64),
         "dense_W": w0["dense_W"].astype(np.float64), "dense_b": w0["dense_b"].astype(np.float64)}
    x = rng.uniform(-1, 1, (3, 1, 90))
    y0 = O.single_lstm_keras_forward(x, w, 3, True, np.zeros((2, 3, 90)))
    # step 1 must equal a plain step on the planar repetition of step 0's means from step 0's state
    h, c = O.lstm_step(x[:, 0], np.zeros((3, 8)), np.zeros((3, 8)), w["K"], w["R"], w["b"])
    planar = np.repeat(y0[:, 0, :3], 30, axis=1)
    h, c = O.lstm_step(planar, h, c, w["K"], w["R"], w["b"])
    np.testing.assert_allclose(y0[:, 1], np.tanh(h @ w["dense_W"] + w["dense_b"]), atol=1e-14)
    # the constant-input form differs from it, and the per-step form consumes one input second per step
    assert np.abs(O.single_lstm_keras_forward(x, w, 3, True, None)[:, 1] - y0[:, 1]).max() > 1e-6
    xs = rng.uniform(-1, 1, (3, 4, 90))
    np.testing.assert_allclose(O.single_lstm_keras_forward(xs, w)[:, :2], O.single_lstm_keras_forward(xs[:, :2], w), atol=1e-14)


def test_cpu_baseline_legs_compute_the_same_graphs_as_the_oracle():
    """bench.py's cpu_baseline legs (oracle/torch_cpu.py) are timed as 'the reference's CPU path restated': each must be the
    SAME arithmetic as the oracle - the sgemm-loop leg and the torch-op legs of the target-only model, the others-mixing
    model and the ConvLSTM encoder."""
    from oracle import torch_cpu as TC
    w = O.init_seq2seq(1, H=64, bias_noise=0.05)
    enc, dec0, _ = O.synthetic_batch(2, 9, 5, 4)
    f64 = lambda d: {k: v.astype(np.float64) for k, v in d.items()}
    ref = O.seq2seq_decode(enc.astype(np.float64), dec0.astype(np.float64), f64(w), 4)
    assert np.abs(TC.Seq2SeqSgemmCPU(w, threads=2).decode(enc, dec0, 4) - ref).max() < 2e-6
    assert np.abs(TC.Seq2SeqCPU(w, threads=2).decode(enc, dec0, 4) - ref).max() < 2e-6
    wm = O.init_others_mixing(3, H=32, num_user=5, bias_noise=0.05)
    e, d0, t, oth = O.synthetic_batch(4, 7, 3, 4, num_others=4)
    refm = O.others_mixing_forward(e.astype(np.float64), oth.astype(np.float64), d0.astype(np.float64), f64(wm))
    assert np.abs(TC.OthersMixingCPU(wm, threads=2).predict(e, oth, d0) - refm).max() < 2e-6
    wc = O.init_convlstm_seq2seq(1, C=6, latent_dim=4, head="conv2d")
    x = np.random.default_rng(0).random((2, 3, 6, 5, 6)).astype(np.float32)
    layers = [(wc["enc%d_K" % l], wc["enc%d_R" % l], wc["enc%d_b" % l]) for l in range(3)]
    seq = x.astype(np.float64)
    for K, R, b in layers:
        seq = O.convlstm2d_layer(seq, K.astype(np.float64), R.astype(np.float64), b.astype(np.float64))[0]
    assert np.abs(TC.convlstm_encoder_cpu(x, layers, 2) - seq).max() < 2e-6


# ---- lstm.py's GMM / raw branches (oracle restatements of TF-1.x pieces; parity unpinned, cross-checked here) ----
def _gmm_params(rng, B, n, rho_scale):
    pre = 0.6 * rng.standard_normal((B, 10 * n))
    pre[:, 7 * n:] += rho_scale * rng.choice([-1.0, 1.0], (B, 3 * n))
    e = np.exp(pre[:, :n])
    return e / e.sum(1, keepdims=True), pre[:, n:4 * n], np.exp(pre[:, 4 * n:7 * n] - 0.7), np.tanh(pre[:, 7 * n:])


def test_gmm3d_density_against_scipy_and_repair_rule():
    """mvn3_prob = scipy's multivariate normal density; gmm3d_covariance applies cost.py:335-348 exactly: untouched when the
    smallest eigenvalue is >= 0, shifted by -10 * min_eig otherwise (new smallest eigenvalue = 9 |min_eig| > 0)."""
    from scipy.stats import multivariate_normal
    rng = np.random.default_rng(0)
    B, n = 6, 20
    pi, us, sig, rho = _gmm_params(rng, B, n, 1.5)
    s, r = sig.reshape(B, n, 3), rho.reshape(B, n, 3)
    cov = O.gmm3d_covariance(s, r)
    raw = O.gmm3d_covariance(s, 0 * r)          # diagonal: never repaired
    assert np.allclose(raw, np.eye(3) * (s ** 2)[..., None, :])
    n_rep = 0
    for b in range(B):
        for m in range(n):
            S = np.array([[s[b, m, 0] ** 2, r[b, m, 0] * s[b, m, 0] * s[b, m, 1], r[b, m, 1] * s[b, m, 0] * s[b, m, 2]],
                          [r[b, m, 0] * s[b, m, 0] * s[b, m, 1], s[b, m, 1] ** 2, r[b, m, 2] * s[b, m, 1] * s[b, m, 2]],
                          [r[b, m, 1] * s[b, m, 0] * s[b, m, 2], r[b, m, 2] * s[b, m, 1] * s[b, m, 2], s[b, m, 2] ** 2]])
            lam = np.linalg.eigvalsh(S)[0]
            if lam < 0:
                n_rep += 1
                assert np.allclose(cov[b, m], S - 10 * lam * np.eye(3))
                assert abs(np.linalg.eigvalsh(cov[b, m])[0] - 9 * abs(lam)) < 1e-9
            else:
                assert np.array_equal(cov[b, m], S)
            y = rng.uniform(-1, 1, 3)
            want = multivariate_normal(us.reshape(B, n, 3)[b, m], cov[b, m]).pdf(y)
            assert abs(O.mvn3_prob(y, us.reshape(B, n, 3)[b, m], cov[b, m]) - want) <= 1e-10 * want + 1e-300
    assert 10 < n_rep < B * n


def test_mixture_3d_gaussian_loss_known_answers():
    """One mixture, unit sigmas, zero rhos, y = mu: density (2 pi)^-1.5 per frame -> loss = fps * 1.5 log(2 pi) / (running_length
    * fps) for batch 1; mixture_pi does not enter (cost.py:532-538) unless weight_by_pi; only second 0 is scored."""
    B, n, fps = 1, 2, 30
    pi = np.array([[0.25, 0.75]])
    us = np.zeros((B, 3 * n)); sig = np.ones((B, 3 * n)); rho = np.zeros((B, 3 * n))
    us[:, 3:] = 50.0          # second component far away: contributes nothing
    y = np.zeros((B, 4, 3 * fps))
    y[:, 1:] = 7.0            # later seconds must be ignored
    got = O.mixture_3d_gaussian_loss(y, (pi, us, sig, rho), batch_size=1, running_length=10, fps=fps)
    assert abs(got - fps * 1.5 * np.log(2 * np.pi) / (10 * fps)) < 1e-12
    gw = O.mixture_3d_gaussian_loss(y, (pi, us, sig, rho), 1, 10, fps, weight_by_pi=True)
    assert abs(gw - fps * (1.5 * np.log(2 * np.pi) - np.log(0.25)) / (10 * fps)) < 1e-12
    # per-frame layout: (B,T,3), divided by batch * running_length only
    yf = np.zeros((B, 5, 3))
    gf = O.mixture_3d_gaussian_loss(yf, (pi, us, sig, rho), 1, 10, fps, process_in_seconds=False)
    assert abs(gf - 5 * 1.5 * np.log(2 * np.pi) / 10) < 1e-12


def test_gmm_head_split_and_raw_head_centre_tap():
    rng = np.random.default_rng(1)
    B, H, n = 4, 24, 20
    dims = [H, 64, 128, 256, 10 * n]
    head = {}
    for l in range(4):
        head["fc%d_W" % (l + 1)] = rng.standard_normal((dims[l], dims[l + 1])) / np.sqrt(dims[l])
        head["fc%d_b" % (l + 1)] = 0.1 * rng.standard_normal(dims[l + 1])
    h = rng.standard_normal((B, H))
    (pi, us, sig, rho), (a1, a2, a3) = O.tf_gmm3d_head(h, head)
    assert pi.shape == (B, 20) and us.shape == (B, 60) and sig.shape == (B, 60) and rho.shape == (B, 60)
    assert np.allclose(pi.sum(1), 1) and (sig > 0).all() and (np.abs(rho) < 1).all() and (a3 >= 0).all()
    m = [(rng.random((B, 64)) < 0.8) / 0.8, None]
    (pi2, _, _, _), (b1, _, _) = O.tf_gmm3d_head(h, head, masks=m)
    assert np.array_equal(b1, a1 * m[0]) and not np.allclose(pi2, pi)
    # raw head: an explicit 'same' conv1d over ONE step equals the centre-tap products
    rh = {}
    cd = [H, 128, 256, 90]
    for l in range(3):
        rh["conv%d_W" % (l + 1)] = rng.standard_normal((5, cd[l], cd[l + 1])) / np.sqrt(cd[l])
        rh["conv%d_b" % (l + 1)] = 0.1 * rng.standard_normal(cd[l + 1])

    def conv1d_same(x, w, b):       # x (B,T,C), w (k,C,N): zero padding, cross-correlation (tf.layers.conv1d)
        k = w.shape[0]
        xp = np.pad(x, ((0, 0), (k // 2, k // 2), (0, 0)))
        return np.stack([sum(xp[:, t + j] @ w[j] for j in range(k)) for t in range(x.shape[1])], 1) + b

    z = h[:, None, :]
    z = np.maximum(conv1d_same(z, rh["conv1_W"], rh["conv1_b"]), 0)
    z = np.maximum(conv1d_same(z, rh["conv2_W"], rh["conv2_b"]), 0)
    z = np.tanh(conv1d_same(z, rh["conv3_W"], rh["conv3_b"]))
    out, _ = O.tf_raw_head(h, rh)
    assert out.shape == (B, 1, 90) and np.allclose(out, z, atol=1e-13)
    # pred_raw_loss_tf on one time step: the total-variation term is exactly zero (cost.py:608-618 slices axis 1)
    y = rng.uniform(-1, 1, (B, 1, 90))
    assert O.total_variation_loss_tf(out) == 0.0
    assert abs(O.pred_raw_loss_tf(y, out) - ((y - out) ** 2).mean()) < 1e-15
    assert O.pred_raw_loss_tf(y, out, use_reg=True) > O.pred_raw_loss_tf(y, out)
    two = np.concatenate([out, out + 0.1], 1)
    assert O.total_variation_loss_tf(two) > 0


def test_sample_mixture_3d_statistics():
    """Inverse-CDF component choice + Cholesky draw: a single dominant component reproduces its mean and covariance."""
    rng = np.random.default_rng(2)
    B, n, P = 1, 3, 20000
    pi = np.array([[0.0, 1.0, 0.0]])
    us = np.array([[9, 9, 9, 0.1, -0.2, 0.3, -9, -9, -9.0]])
    sig = np.array([[1, 1, 1, 0.5, 0.2, 0.3, 1, 1, 1.0]])
    rho = np.array([[0, 0, 0, 0.3, -0.2, 0.1, 0, 0, 0.0]])
    out = O.sample_mixture_3d((pi, us, sig, rho), rng.random((B, P)), rng.standard_normal((B, P, 3))).reshape(P, 3)
    cov = O.gmm3d_covariance(sig.reshape(1, 3, 3), rho.reshape(1, 3, 3))[0, 1]
    assert np.abs(out.mean(0) - us[0, 3:6]).max() < 0.02
    assert np.abs(np.cov(out.T) - cov).max() < 0.01


def test_dilated_conv_and_convlstm_step_against_torch():
    """cfg.dilation_rate (config.py:105): the oracle's dilated 'same' convolution is torch's conv2d(dilation=d, padding=d*(k//2)),
    and the ConvLSTM step dilates the input convolution only (Keras 2.2 ConvLSTM2DCell: input_conv gets dilation_rate,
    recurrent_conv does not)."""
    import torch
    import torch.nn.functional as TF
    rng = np.random.default_rng(4)
    x = rng.standard_normal((2, 9, 7, 5))
    K = rng.standard_normal((5, 5, 5, 12)) * 0.1
    R = rng.standard_normal((5, 5, 3, 12)) * 0.1
    b = rng.standard_normal(12) * 0.1
    tc = lambda a, w, d: TF.conv2d(torch.tensor(a).permute(0, 3, 1, 2), torch.tensor(w).permute(3, 2, 0, 1), padding=(2 * d, 2 * d),
                                   dilation=d).permute(0, 2, 3, 1).numpy()
    for d in (1, 2, 3):
        assert np.abs(O.conv2d_same(x, K, b, dilation=d) - (tc(x, K, d) + b)).max() < 1e-12
    h = rng.standard_normal((2, 9, 7, 3))
    c = rng.standard_normal((2, 9, 7, 3))
    z = tc(x, K, 2) + b + tc(h, R, 1)
    hs = lambda v: np.clip(0.2 * v + 0.5, 0, 1)
    cn = hs(z[..., 3:6]) * c + hs(z[..., :3]) * np.tanh(z[..., 6:9])
    hn = hs(z[..., 9:]) * np.tanh(cn)
    h2, c2 = O.convlstm2d_step(x, h, c, K, R, b, "hard_sigmoid", dilation=2)
    assert np.abs(h2 - hn).max() < 1e-12 and np.abs(c2 - cn).max() < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# The value-regime generator (tests/test_gpu_value_regimes.py): for every case of that file's tables the promised shares of
# clamped / saturated / overflowing pre-activations hold in the fp64 forward, and the yardstick's condition holds: 8 e_ref
# (fp64 against the same functions on fp32 arrays, in written bounds) is at most 10.  A later edit of the generator cannot
# quietly move the cases back into the linear regime or into one where the reference itself is ill-conditioned.
# ---------------------------------------------------------------------------------------------------------------------
def _cap(tag, e_ref):
    for k, v in e_ref.items():
        assert O.REGIME_YARDSTICK * v <= O.REGIME_YARDSTICK_CAP, "%s %s: 8 e_ref = %.3g" % (tag, k, 8 * v)


def _assert_shares(tag, regime, sh, state=True):
    if regime == "R1":
        assert 0.30 <= sh["gate_clamped"] <= 0.70, (tag, sh)
    if regime in ("R2", "R3"):
        assert sh["gate_sat"] >= 0.20 and sh["g_sat"] >= 0.20 and sh["tanh_sat"] >= 0.20, (tag, sh)
        if state:
            assert sh["c_sat"] >= 0.20, (tag, sh)
    if regime == "R4":
        assert sh["c_max"] > 50, (tag, sh)


def _regime_layer_case(tag, p, bf16, backward_seed=None):
    regime = p["regime"]
    B = p["x"].shape[0]
    if regime == "R3":
        rows = p["extreme"]
        _assert_shares(tag, regime, O.regime_shares(p, np.setdiff1d(np.arange(16), rows)))       # the tile-mates stay in R2
        ex = O.regime_shares(p, rows[:2])
        assert ex["z100"] >= 0.10 and ex["z200"] >= 0.05, (tag, ex)                               # both signs, each
        late = O.regime_shares({**p, "x": p["x"][:, :p["x"].shape[1] // 2]}, rows[2:])
        assert late["z100"] == 0.0, (tag, late)                                                   # ordinary until mid-sequence
        xe = p["x_edge"]
        assert (xe[16:32] == 0).all() and 0 < np.abs(xe[32:]).max() <= 1e-6 and (p["b_edge"] == 0).all()
        _cap(tag + " edge", O.regime_forward_reference(p, bf16=bf16, x=xe, b=p["b_edge"])[1])
    else:
        sh = O.regime_shares(p)
        _assert_shares(tag, regime, sh)
        if regime == "R4":
            H = p["R"].shape[0]
            res = O.lstm_layer_train(*[None if p[k] is None else p[k].astype(np.float64) for k in ("x", "K", "R", "b", "h0", "c0")],
                                     act=p["act"])[3]
            assert (res[:, :, 1].astype(np.float32) == 1.0).all()                                 # forget gate: exactly 1 in fp32
            ig = res[:, :, 0] * res[:, :, 2]
            assert ((ig > 0).all(axis=(0, 1)) | (ig < 0).all(axis=(0, 1))).all()                  # one sign per unit
            assert p["b"].astype(np.float32)[H:2 * H].min() >= 10.0
    _cap(tag, O.regime_forward_reference(p, bf16=bf16)[1])
    if backward_seed is not None:
        T, H = p["x"].shape[1], p["R"].shape[0]
        _cap(tag + " backward", O.regime_backward_e_ref(p, O.regime_upstream(backward_seed, B, T, H), bf16=bf16))


@pytest.mark.parametrize("regime", O.REGIMES)
def test_value_regime_layer_cases_hold_their_shares_and_the_yardstick_condition(regime):
    import test_gpu_value_regimes as V
    for impl, H in sorted({(i, h) for i, h, _ in V.LAYER_FORWARD}):
        for B, T in V.LAYER_SHAPE[regime]:
            _regime_layer_case("%s H%d %s B%d" % (impl, H, regime, B), O.regime_lstm(V.layer_seed(H, regime, B), 90, H, regime, B, T), False)
    for r, B, T, gain, seed in V.BF16_LAYER:
        if r == regime:
            _regime_layer_case("bf16 layer %s gain %g" % (r, gain), O.regime_lstm(V.layer_seed(256, r, B) + seed, 90, 256, r, B, T, r_gain=gain, xk=O.BF16_XK), True)
    B, T = V.BACKWARD_SHAPE[regime]
    for name, H, _, dtype in V.BACKWARD_FORMS:
        bf = dtype == "bf16"
        p = O.regime_lstm(V.layer_seed(H, regime, B) + 1, 90 if bf else 11, H, regime, B, T, xk=O.BF16_XK if bf else None)
        _regime_layer_case("%s %s" % (name, regime), p, bf, backward_seed=V.layer_seed(H, regime, B) + 2)


def test_value_regime_generator_is_seeded_and_keeps_the_recurrent_kernel_orthogonal():
    a, b = O.regime_lstm(3, 11, 64, "R3", 37, 8), O.regime_lstm(3, 11, 64, "R3", 37, 8)
    for k in ("K", "R", "b", "x", "h0", "c0", "x_edge"):
        np.testing.assert_array_equal(a[k], b[k])
    for gain in (1.0, 2.0, 4.0):
        R = O.regime_lstm(4, 11, 64, "R1", 16, 2, r_gain=gain)["R"].astype(np.float64)
        np.testing.assert_allclose(R @ R.T, gain * gain * np.eye(64), atol=1e-5)


def test_value_regime_model_cases_hold_their_shares_and_the_yardstick_condition():
    import test_gpu_value_regimes as V
    H = 256
    T_in, T_out = V.DECODE_T
    for regime, B, dtype, _ in V.DECODE:
        bf = dtype == "bf16"
        w, enc, dec0, act = O.regime_seq2seq(50 + B, regime, B, T_in, xk=O.BF16_XK if bf else None)
        if not bf:      # regime_decode exposes the pre-activations; it is seq2seq_decode, bit for bit
            np.testing.assert_array_equal(O.regime_decode(enc, dec0, w, T_out, act)["out"],
                                          O.seq2seq_decode(enc.astype(np.float64), dec0.astype(np.float64),
                                                           {k: v.astype(np.float64) for k, v in w.items()}, T_out, act))
        r64, r32 = O.regime_decode(enc, dec0, w, T_out, act, bf, np.float64), O.regime_decode(enc, dec0, w, T_out, act, bf, np.float32)
        z = r64["z"]
        gates = np.concatenate([z[..., :2 * H], z[..., 3 * H:]], axis=-1)
        tag = "decode %s B%d %s" % (regime, B, dtype)
        if regime == "R1":
            assert 0.30 <= (np.abs(gates) > 2.5).mean() <= 0.70, tag
        else:
            assert (np.abs(gates) > 17).mean() >= 0.20, tag
            assert (np.abs(np.concatenate([z[..., 2 * H:3 * H], r64["c"]], axis=-1)) > 9).mean() >= 0.20, tag
        assert (np.abs(r64["pre"]) > 9).mean() >= 0.20 and (r64["pre"] > 10.5).any() and (r64["pre"] < -10.5).any(), tag
        kind = "bf16" if bf else "f32"
        _cap(tag, {k: O.regime_error(r32[k], r64[k], kind) for k in ("out", "hT", "cT")})
    B, T, F = V.STACK2_SHAPE
    for regime, Hh in V.STACK2:
        layers, x, st, act, p1 = O.regime_stack2(70 + O.REGIMES.index(regime), regime, B, T, F, Hh)
        f64, f32 = O.regime_stack2_forward(layers, x, st, act, np.float64), O.regime_stack2_forward(layers, x, st, act, np.float32)
        for l in range(2):
            tag = "stack2 H%d %s layer %d" % (Hh, regime, l + 1)
            keep = np.setdiff1d(np.arange(B), p1["extreme"]) if regime == "R3" else np.arange(B)
            _assert_shares(tag, regime, O.regime_tape_shares(f64[l][3][keep], act))
            t64, t32 = O.regime_forward_tensors(*f64[l]), O.regime_forward_tensors(*f32[l])
            _cap(tag, {k: O.regime_error(t32[k], t64[k], "f32") for k in t64})
        ups = O.regime_stack2_upstream(80, B, T, Hh)
        tapes = [(f32[0][0], f32[0][3]), (f32[1][0], f32[1][3])]
        y64 = O.regime_stack2_backward(layers, x, st, tapes, ups, act, np.float64)
        y32 = O.regime_stack2_backward(layers, x, st, tapes, ups, act, np.float32)
        _cap("stack2 %s backward" % regime, {k: O.regime_error(y32[k], y64[k], 1e-4) for k in y64})
    for regime in V.STACK2_BF16:
        layers, x, st, act, p1 = O.regime_stack2(75 + O.REGIMES.index(regime), regime, B, T, F, 256, state=False, xk=O.BF16_XK)
        f64 = O.regime_stack2_forward(layers, x, st, act, np.float64, bf16=True)
        f32 = O.regime_stack2_forward(layers, x, st, act, np.float32, bf16=True)
        keep = np.setdiff1d(np.arange(B), p1["extreme"]) if regime == "R3" else np.arange(B)
        for l in range(2):
            tag = "stack2 bf16 %s layer %d" % (regime, l + 1)
            _assert_shares(tag, regime, O.regime_tape_shares(f64[l][3][keep], act), state=False)
            t64, t32 = O.regime_forward_tensors(*f64[l]), O.regime_forward_tensors(*f32[l])
            _cap(tag, {k: O.regime_error(t32[k], t64[k], "bf16") for k in t64})
    for regime in V.TF_STACK:       # the same two layers at 400 units, through the tf.contrib cell (one product over [x, h])
        layers, x, st, act, p1 = O.regime_stack2(90 + O.REGIMES.index(regime), regime, B, T, F, 400)
        f64 = O.regime_stack2_forward(layers, x, st, act, np.float64)
        keep = np.setdiff1d(np.arange(B), p1["extreme"]) if regime == "R3" else np.arange(B)
        for l in range(2):
            _assert_shares("tf stack %s layer %d" % (regime, l + 1), regime, O.regime_tape_shares(f64[l][3][keep], act))
        cells = [O.keras_to_tf_cell(*l) for l in layers]
        st0 = np.stack([np.stack([s_[1], s_[0]]) for s_ in st]).astype(np.float32)
        r64 = O.tf_dynamic_rnn(x.astype(np.float64), [(W.astype(np.float64), b.astype(np.float64)) for W, b in cells], st0.astype(np.float64))
        r32 = O.tf_dynamic_rnn(x, cells, st0)
        np.testing.assert_allclose(r64[0], f64[1][0], atol=1e-6)       # the mapping to tf.contrib's gate order (b_f - 1 rounds in fp32)
        _cap("tf stack %s" % regime, {"states_series": O.regime_error(r32[0], r64[0], "f32"),
                                      "current_state": O.regime_error(r32[1], r64[1], "f32")})
    B, T, O_ = V.MIX_SHAPE
    for regime, dtype in V.MIX:
        bf = dtype == "bf16"
        w, mix_Wp, st, dec0, oth, act, extra = O.regime_mix_decoder(60 + O.REGIMES.index(regime), regime, B, T, H, O_)

        def fwd(dt):
            c_ = lambda a: np.asarray(a, dt)
            return O.mix_decoder_train_forward(c_(dec0), *[c_(s) for s in st], c_(oth), {k: c_(v) for k, v in w.items()}, c_(mix_Wp), T,
                                               act=act, round_fwd=bf)
        r64, r32 = fwd(np.float64), fwd(np.float32)
        tag = "mix decoder %s %s" % (regime, dtype)
        for n in ("res1", "res2"):
            _assert_shares(tag + " " + n, regime, O.regime_tape_shares(r64[n], act))
        if regime == "R3":      # layer 1 at row 9, step 0 and the mixing head at row 3 see overflowing arguments of both signs
            f64_ = lambda a: np.asarray(a, np.float64)
            z1, z2, pre_m = O.mix_decoder_preactivations(r64, f64_(dec0), [f64_(a) for a in st], f64_(oth),
                                                         {k: f64_(v) for k, v in w.items()}, f64_(mix_Wp), bf16=bf)
            for t_ in (100, 200):
                assert (z1[0, 9] > t_).sum() >= 50 and (z1[0, 9] < -t_).sum() >= 50, (tag, t_)
            assert (pre_m[:, 3] > 200).sum() > 0 and (pre_m[:, 3] < -200).sum() > 0, tag
            assert np.abs(z2).max() < 100                                       # layer 2 is not reached
            for k in ("dec0_edge", "oth_edge"):
                assert (extra[k][16:32] == 0).all()
            assert all((a[16:32] == 0).all() for a in extra["st_edge"]) and all((extra["w_edge"][k] == 0).all() for k in w if k.endswith("_b"))
            keep = np.setdiff1d(np.arange(B), extra["rows"])
            np.testing.assert_array_equal(extra["dec0_calm"][keep], dec0[keep])
            np.testing.assert_array_equal(extra["oth_calm"][keep], oth[keep])
        kind = "bf16" if bf else "f32"
        _cap(tag, {k: O.regime_error(r32[k], r64[k], kind) for k in r64})
        G = (0.2 * np.random.default_rng(61).standard_normal((T, B, O_))).astype(np.float32)
        C1, C2 = np.concatenate([st[1][None], r32["C1"]]), np.concatenate([st[3][None], r32["C2"]])

        def bwd(dt):
            c_ = lambda a: np.asarray(a, dt)
            return O.mix_decoder_backward(c_(r32["M"]), c_(r32["P"]), c_(G * (1 - r32["M"] * r32["M"])), c_(r32["res1"]), c_(r32["res2"]),
                                          c_(C1), c_(C2), {k: c_(v) for k, v in w.items()}, c_(mix_Wp), act=act, round_rec=bf, round_dx=bf)
        y64, y32 = bwd(np.float64), bwd(np.float32)
        _cap(tag + " backward", {k: O.regime_error(y32[k], y64[k], ((2e-3 if k in ("dh1_0", "dh2_0") else 1e-3) if bf else 1e-4))
                                 for k in y64})
    for shape, act in V.CONV:
        p = O.regime_convlstm_cell(40 + shape[3], *shape, act)
        r64, r32 = O.regime_convlstm_reference(p), O.regime_convlstm_reference(p, np.float32)
        z = r64["z"]
        assert min((z > 100).sum(), (z < -100).sum(), (z > 200).sum(), (z < -200).sum()) >= 100, (shape, act)
        assert (p["x_edge"][-1] == 0).all() and (p["h_edge"][-1] == 0).all() and (p["c_edge"][-1] == 0).all()
        _cap("convlstm cell %s %s" % (shape, act), {k: O.regime_error(r32[k], r64[k], "f32") for k in ("h", "c", "gates")})


# --------------------------------------------------------------------------------------
# References of tests/test_gpu_loss_optim_edges.py: each against torch.autograd in fp64 (1e-10 relative), and the input
# generators' population / near-clip conditions for every shape the GPU file uses (a bad seed shows here, without a GPU).
# --------------------------------------------------------------------------------------
def _t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("i", range(len(O.NLL_EDGE_SHAPES)))
@pytest.mark.parametrize("scale", [1.0, 0.37])
def test_gauss_nll_reference_matches_autograd_and_populations(i, scale):
    B, Ty, fps = O.NLL_EDGE_SHAPES[i]
    mu, var, y, again = O.nll_edge_inputs(100 + i, B, Ty, fps)
    (loss, dmu, dvar), (wm, wv), l = O.gauss_nll(mu, var, y, fps, scale)
    tm, tv = _t64(mu, True), _t64(var, True)
    ve = tv[:, None, :] + O.r32(1e-20)
    lt = torch.log(ve) + (_t64(y).reshape(B, -1, 3) - tm[:, None, :]) ** 2 / ve
    lr = O.r32(scale) * torch.clamp(lt, -10, 10).sum() / B
    lr.backward()
    assert abs(loss - lr.item()) <= 1e-10 * abs(lr.item())
    assert _rel(dmu, tm.grad.numpy()) <= 1e-10 and _rel(dvar, tv.grad.numpy()) <= 1e-10
    assert (wm >= np.abs(dmu)).all() and (wv >= np.abs(dvar) * (1 - 1e-12)).all()
    lo, hi, mid, dist = O.nll_populations(mu, var, y, fps)
    print("nll %s: low %.3f high %.3f interior %.3f, drawn again %d of %d, least distance from a clip %.2e" % ((B, Ty, fps), lo, hi, mid, again, l.size, dist))
    assert dist >= 1e-3
    if l.size >= 90:      # (three elements cannot hold 5 % + 5 % + 50 %)
        assert lo >= 0.05 and hi >= 0.05 and mid >= 0.5 and again < 0.01 * l.size
        # the case tests the mask: without it the gradients are far outside any rounding bound
        (_, dmu_n, dvar_n), _, _ = O.gauss_nll(mu, var, y, fps, scale, clip_mask=False)
        assert (np.abs(dvar_n - dvar) > 1e-3 * wv).any() and (np.abs(dmu_n - dmu) > 1e-3 * wm).any()


def test_gauss_nll_dvar_spans_orders_of_magnitude():
    """Why the GPU bound is per element: with tiny variances present |dvar| spans seven orders of magnitude."""
    mu, var, y, _ = O.nll_edge_inputs(105, 300, 3, 30)
    dvar = np.abs(O.gauss_nll(mu, var, y, 30, 1.0)[0][2])
    assert dvar.max() / np.median(dvar) > 1e6


@pytest.mark.parametrize("i", range(len(O.CCE_EDGE_SHAPES)))
def test_categorical_crossentropy_reference_matches_autograd(i):
    n_pix, C = O.CCE_EDGE_SHAPES[i]
    p, t, onehot = O.cce_edge_inputs(200 + i, n_pix, C)
    (loss, dp), w, q = O.categorical_crossentropy(p, t)
    tp = _t64(p, True)
    hi = float(np.float32(1) - np.float32(1e-7))
    assert hi == 1 - 2.0 ** -23
    lr = torch.mean(-(_t64(t) * torch.log(torch.clamp(tp / tp.sum(-1, keepdim=True), O.r32(1e-7), hi))).sum(-1))
    lr.backward()
    assert abs(loss - lr.item()) <= 1e-10 * abs(lr.item())
    ref = tp.grad.numpy()
    # torch's clamp passes the gradient AT a bound (q == 1 of the one-hot rows); Keras' clip_by_value does too, but there
    # d q / d p is exactly zero (q = p / p), so both are zero
    assert np.abs(dp - ref).max() <= 1e-10 * np.abs(ref).max() + 1e-300
    assert (w >= np.abs(dp) * (1 - 1e-12)).all()
    near = O.cce_near_clip_rows(p, onehot)
    assert near.sum() <= 0.01 * n_pix and not near.any()
    if n_pix >= 255:
        r = np.arange(n_pix)
        assert (np.abs(p.sum(-1) - 1) > 1e-3).mean() > 0.9                       # unnormalised
        assert (dp[onehot] == 0).all() and onehot.mean() >= 0.05                 # upper clip
        if C > 1:
            tiny = (r % 5 == 1) & ~onehot & (r % 7 != 3)
            assert tiny.mean() >= 0.05 and (dp[tiny] == 0).all()                 # lower clip under a one-hot target
            assert ((t > 0).sum(-1) > 1).mean() >= 0.05                          # soft targets


@pytest.mark.parametrize("C", [3, 6])
def test_xyz_sum1_reference_matches_autograd(C):
    rng = np.random.default_rng(31)
    p = rng.standard_normal((257, C)).astype(np.float32)
    dp0 = rng.standard_normal((257, C)).astype(np.float32)
    (reg, dp), w = O.xyz_sum1(p, dp0)
    tp = _t64(p, True)
    rr = 0.5 * torch.mean((tp[:, 0] ** 2 + tp[:, 1] ** 2 + tp[:, 2] ** 2 - 1) ** 2)
    rr.backward()
    assert abs(reg - rr.item()) <= 1e-10 * rr.item()
    assert _rel(dp - dp0, tp.grad.numpy()) <= 1e-10 and (dp[:, 3:] == dp0[:, 3:]).all()
    assert (w >= np.abs(dp) * (1 - 1e-12)).all()


@pytest.mark.parametrize("clip", [0.0, 1.0])
def test_rmsprop_tf_reference_matches_autograd_form(clip):
    """TF RMSProp as a gradient step of torch: p - lr * g_c / sqrt(ms' + eps), ms' from ONE (ms starts at one)."""
    g = np.array([0.5, -3.0, 0.0, 1.0, -1.0, 1.0000001, 2e-3], np.float32)
    p = np.linspace(-1, 1, g.size).astype(np.float32)
    (pn, msn), w = O.rmsprop_tf_step(p, g, np.ones_like(p), lr=0.1, decay=0.9, eps=1e-10, clip=clip)
    tg = _t64(g)
    gc = torch.clamp(tg, -O.r32(clip), O.r32(clip)) if clip > 0 else tg
    ms = O.r32(0.9) * 1.0 + (1 - O.r32(0.9)) * gc * gc
    ref = _t64(p) - O.r32(0.1) * gc / torch.sqrt(ms + O.r32(1e-10))
    assert _rel(pn, ref.numpy()) <= 1e-10 and _rel(msn, ms.numpy()) <= 1e-10
    if clip > 0:
        assert msn[1] == msn[3] == msn[4] == msn[5]      # below, at and above the clip: the same clipped magnitude


@pytest.mark.parametrize("std", ["sqrt", "var"])
@pytest.mark.parametrize("planar", [False, True])
def test_sample_refeed_reference_matches_autograd(std, planar):
    rng = np.random.default_rng(32)
    B, fps = 5, 22
    mu = rng.uniform(-1, 1, (B, 3)); var = rng.uniform(0.01, 1, (B, 3)); var[0, 0] = 1e-6
    noise = rng.standard_normal((B, 3 * fps)); dx = rng.standard_normal((B, 3 * fps))
    dmu0, dvar0 = rng.standard_normal((B, 3)), rng.standard_normal((B, 3))
    tm, tv = _t64(mu, True), _t64(var, True)
    sd = torch.sqrt(tv) if std == "sqrt" else tv
    if planar:
        x = torch.cat([tm[:, k:k + 1] + sd[:, k:k + 1] * _t64(noise)[:, k * fps:(k + 1) * fps] for k in range(3)], -1)
    else:
        x = (tm[:, None, :] + sd[:, None, :] * _t64(noise).reshape(B, fps, 3)).reshape(B, 3 * fps)
    (x * _t64(dx)).sum().backward()
    xr, wx = O.sample_refeed(mu, var, noise, std, planar)
    assert _rel(xr, x.detach().numpy()) <= 1e-10 and (wx >= np.abs(xr)).all()
    (gm, gv), _ = O.sample_refeed_bwd(dx, var, noise, std, planar)
    assert _rel(gm, tm.grad.numpy()) <= 1e-10 and _rel(gv, tv.grad.numpy()) <= 1e-10
    (gm2, gv2), (wm, wv) = O.sample_refeed_bwd(dx, var, noise, std, planar, dmu0, dvar0)
    assert _rel(gm2, tm.grad.numpy() + dmu0) <= 1e-10 and _rel(gv2, tv.grad.numpy() + dvar0) <= 1e-10
    assert (wm >= np.abs(gm2) * (1 - 1e-12)).all() and (wv >= np.abs(gv2) * (1 - 1e-12)).all()


@pytest.mark.parametrize("act", ["tanh", "linear"])
def test_mse_dense_reference_matches_autograd(act):
    rng = np.random.default_rng(33)
    T, B, Od = 3, 5, 6
    y = np.tanh(rng.standard_normal((T, B, Od))).astype(np.float32)
    tgt = rng.uniform(-1, 1, (B, T, Od)).astype(np.float32)
    pre = _t64(np.arctanh(y.astype(np.float64)) if act == "tanh" else y, True)
    yy = torch.tanh(pre) if act == "tanh" else pre
    lr = O.r32(O.r32(0.37) / np.float32(y.size)) * ((yy - _t64(tgt).transpose(0, 1)) ** 2).sum()
    lr.backward()
    (loss, dpre), w = O.mse_dense(y, tgt, act, 0.37, time_major=True)
    assert abs(loss - lr.item()) <= 1e-10 * lr.item() and _rel(dpre, pre.grad.numpy()) <= 1e-10
    assert (w >= np.abs(dpre) * (1 - 1e-12)).all()
    (_, wrong), _ = O.mse_dense(y, tgt, act, 0.37, time_major=True, transpose_target=False)
    assert (np.abs(wrong - dpre) > 1e-3 * w).any()


def test_adam_reference_with_fp32_rounded_arguments_is_the_fp32_step():
    """One Adam step: the fp64 reference on fp32-ROUNDED betas / lr_t / eps agrees with an fp32 NumPy emulation of the kernel's
    arithmetic to a few ulp of each element's terms; the same reference on the exact fp64 betas is 1.3e-5 (200 times 2^-24) away in v."""
    rng = np.random.default_rng(34)
    n = 4099
    f = np.float32
    p, g = rng.standard_normal(n).astype(f), rng.standard_normal(n).astype(f)
    m, v = (0.1 * rng.standard_normal(n)).astype(f), (rng.random(n) * 0.01).astype(f)
    assert abs((1 - O.r32(0.999)) / (1 - 0.999) - 1) > 1.2e-5
    for t in (1, 2, 1000):
        lr_t, b1, b2, eps = f(O.adam_lr_t(t)), f(0.9), f(0.999), f(1e-7)
        mi = b1 * m + (f(1) - b1) * g
        vi = b2 * v + (f(1) - b2) * g * g
        pi = p - lr_t * mi / (np.sqrt(vi) + eps)
        assert mi.dtype == vi.dtype == pi.dtype == f
        (pr, mr, vr), w = O.adam_step_f32args(p, g, m, v, t)
        em, ev, ep = np.abs(mi - mr) / w["m"], np.abs(vi - vr) / w["v"], np.abs(pi - pr) / w["p"]
        print("adam t=%d: fp32 emulation vs fp64 on rounded arguments, in 2^-24 of the terms: m %.2f v %.2f p %.2f" % (t, em.max() / O.U24, ev.max() / O.U24, ep.max() / O.U24))
        assert em.max() <= 4 * O.U24 and ev.max() <= 5 * O.U24 and ep.max() <= 8 * O.U24
        (_, _, vx), _ = O.adam_step_f32args(p, g, m, v, t, exact_betas=True)
        assert (np.abs(vi - vx) / w["v"]).max() > 20 * O.U24
