"""The self-fed one-layer decoder's unroll as ONE launch per direction (fov_selffed_decoder_fwd / _bwd, lstm_selffed.hip) against
fp64 references: oracle.fov_oracle.onelayer_tar_seq2seq_forward (FoV_seq2seq_no_teac_forc.py:37-149) for the prediction and an
fp64 torch.autograd restatement of the same graph, written here, for the tapes and every gradient.

Bounds - the project's written ones and nothing looser:
    outputs and tapes:  |gpu - ref| <= 2e-5  AND  |gpu - ref| <= 1e-3 |ref| + 1e-5, per element;
    every gradient:     max |gpu - ref| <= 1e-4 max|ref| + 1e-9 per tensor, no element left out.
hard_sigmoid and relu have kinks, where an fp32 pre-activation may fall on the other side than the fp64 one: a case asserts on
the CPU, in fp64, that no hard_sigmoid pre-activation lies within 1e-4 of +-2.5 and no relu-head pre-activation within 1e-4 of
0; a seed that violates that is passed over for the next one (no element is masked).  Cases are computed once and shared.

Shapes: both widths; one sequence, one whole tile, a ragged second tile, three tiles; one to five steps (both LDS parities, the
first and the last step being the same one) and one long run; feedback widths 1, 3, 6, 8 (one and two k-steps, partial ones)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

pytestmark = pytest.mark.gpu

TAPES = ("Hs", "Cs", "XA", "A", "RES")
BWD_OUT = ("DY", "DPRE", "DZ", "dx0", "dh0", "dc0")


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()


def f64(w):
    return {k: v.astype(np.float64) for k, v in w.items()}


# ------------------------------------------------------------------------------------------------------------------------------
# fp64 references
# ------------------------------------------------------------------------------------------------------------------------------
def _rec(act):
    return torch.sigmoid if act == "sigmoid" else (lambda z: torch.clamp(0.2 * z + 0.5, 0, 1))


def _head(dact):
    return torch.tanh if dact == "tanh" else torch.relu


def _step64(x, h, c, K, R, b, act, log):
    H = R.shape[0]
    z = x @ K + b + h @ R
    z.retain_grad()
    s = _rec(act)
    i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
    c = f * c + i * g
    h = o * torch.tanh(c)
    log["z"].append(z)
    log["gates"].append(torch.stack([i, f, g, o, c], 1))
    return h, c


def _unroll64(x, h, c, r, K, R, b, W, bd, T, act, dact, log):
    """The unrolled decoder on torch tensors: y_t = dact(h_t W + bd) + r fed back.  log collects every step's tensors."""
    fa = _head(dact)
    for k in ("Hs", "Cs", "XA"):
        log[k] = []
    log["Hs"].append(h); log["Cs"].append(c); log["XA"].append(x)
    for k in ("A", "P", "z", "gates"):
        log.setdefault(k, [])
    zs = len(log["z"])
    for _ in range(T):
        h, c = _step64(x, h, c, K, R, b, act, log)
        p = h @ W + bd
        p.retain_grad()
        a = fa(p)
        x = a if r is None else a + r
        x.retain_grad()
        log["P"].append(p); log["A"].append(a)
        log["Hs"].append(h); log["Cs"].append(c); log["XA"].append(x)
    log["dec_z"] = log["z"][zs:]
    return torch.stack(log["XA"][1:], 1) if T else torch.zeros(x.shape[0], 0, x.shape[1], dtype=torch.float64)


def _margins(log, act, dact, H):
    """(distance of the nearest hard_sigmoid pre-activation to +-2.5, of the nearest relu pre-activation to 0), fp64."""
    m_rec = m_relu = np.inf
    if act == "hard_sigmoid":
        for z in log["z"]:
            zz = z.detach().numpy()
            gates = np.concatenate([zz[:, :2 * H], zz[:, 3 * H:]], 1)
            m_rec = min(m_rec, float(np.abs(np.abs(gates) - 2.5).min()))
    if dact == "relu":
        for p in log["P"] + log.get("P_extra", []):
            m_relu = min(m_relu, float(np.abs(p.detach().numpy()).min()))
    return m_rec, m_relu


def _weights(H, n_out, seed):
    w = O.init_seq2seq(seed, F_dec=n_out, H=H, bias_noise=0.1)
    rng = np.random.default_rng(seed + 5)
    w["res_W"] = rng.uniform(-0.5, 0.5, (n_out, n_out)).astype(np.float32)
    w["res_b"] = rng.uniform(-0.1, 0.1, n_out).astype(np.float32)
    return w


def _decoder_inputs(w, seed, B, T, n_out, act, dact, state, residual):
    """fp32 inputs of the decoder alone: x0 from the trajectories' (mu, var) second, the state an encoder's final one."""
    enc, dec0, _ = O.synthetic_batch(seed, B, 2, max(T, 1))
    dec0 = np.concatenate([dec0, dec0], -1)[..., :n_out]
    x0 = np.ascontiguousarray(dec0[:, 0], dtype=np.float32)
    h0 = c0 = r = None
    if state:
        _, h0, c0 = O.lstm_layer(enc.astype(np.float64), *(w[k].astype(np.float64) for k in ("enc_K", "enc_R", "enc_b")), act=act)
        h0, c0 = h0.astype(np.float32), c0.astype(np.float32)
    if residual:
        pre = x0.astype(np.float64) @ w["res_W"].astype(np.float64) + w["res_b"]
        r = (np.tanh(pre) if dact == "tanh" else np.maximum(pre, 0)).astype(np.float32)
    dloss = np.random.default_rng(seed + 11).standard_normal((T, B, n_out)).astype(np.float32)
    return enc, dec0, x0, h0, c0, r, dloss


def _decoder64(w, x0, h0, c0, r, dloss, T, act, dact):
    """fp64 forward tapes and, through torch.autograd, every gradient of sum_t <y_t, dloss_t>."""
    leaf = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    B, H = x0.shape[0], w["dec_R"].shape[0]
    K, R, b, W, bd = (leaf(w[k]) for k in ("dec_K", "dec_R", "dec_b", "dense_W", "dense_b"))
    x0_, h0_, c0_ = leaf(x0), leaf(np.zeros((B, H)) if h0 is None else h0), leaf(np.zeros((B, H)) if c0 is None else c0)
    r_ = None if r is None else leaf(r)
    log = {}
    y = _unroll64(x0_, h0_, c0_, r_, K, R, b, W, bd, T, act, dact, log)
    (y * torch.tensor(dloss.astype(np.float64)).transpose(0, 1)).sum().backward()
    st = lambda seq: np.stack([a.detach().numpy() for a in seq])
    gr = lambda seq: np.stack([a.grad.numpy() for a in seq])
    ref = {"y": y.detach().numpy(), "Hs": st(log["Hs"]), "Cs": st(log["Cs"]), "XA": st(log["XA"]),
           "A": st(log["A"]) if r is not None else None, "RES": st(log["gates"])[:, :, None],
           "DY": gr(log["XA"][1:]), "DPRE": gr(log["P"]), "DZ": gr(log["z"]), "dx0": x0_.grad.numpy(), "dh0": h0_.grad.numpy(),
           "dc0": c0_.grad.numpy()}
    return ref, _margins(log, act, dact, H)


@functools.lru_cache(maxsize=None)
def _case(H, B, T, n_out, act, dact, state, residual, bias_clamp=False):
    """One decoder case: weights, fp32 inputs, fp64 reference; computed once and shared (nobody writes into them).  The first
    seed whose fp64 pre-activations keep 1e-4 away from the kinks of hard_sigmoid and relu is the case's."""
    for attempt in range(16):
        seed = 97 * attempt + H + 3 * B + 7 * T + n_out
        w = _weights(H, n_out, seed)
        if bias_clamp:      # a few gates of every sequence and step driven far into the flat parts of hard_sigmoid
            w["dec_b"][[3, H + 17, 3 * H + 30]] = (4.0, -4.0, 4.0)
            w["dec_b"][[H - 1, 2 * H - 2]] = (-4.0, 4.0)
        enc, dec0, x0, h0, c0, r, dloss = _decoder_inputs(w, seed, B, T, n_out, act, dact, state, residual)
        ref, (m_rec, m_relu) = _decoder64(w, x0, h0, c0, r, dloss, T, act, dact)
        if m_rec > 1e-4 and m_relu > 1e-4:
            break
    assert m_rec > 1e-4, "a hard_sigmoid pre-activation within 1e-4 of +-2.5"
    assert m_relu > 1e-4, "a relu-head pre-activation within 1e-4 of 0"
    # the restatement against the oracle (which runs the encoder in fp64 and keeps r in fp64: inputs differ by fp32 rounding)
    wo = f64(w)
    y_o = O.onelayer_tar_seq2seq_forward(enc.astype(np.float64), dec0.astype(np.float64), wo, T, act=act, decoder_no_init_state=not state,
                                         add_residual_link=residual, dense_activation=dact)
    assert np.abs(y_o - ref["y"]).max() <= 1e-6
    case = dict(w=w, x0=x0, h0=h0, c0=c0, r=r, dloss=dloss, ref=ref, H=H, B=B, T=T, O=n_out, act=act, dact=dact)
    for a in list(w.values()) + [x0, h0, c0, r, dloss] + list(ref.values()):
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


def _dec_w(w):
    return [dev(w[k]) for k in ("dec_K", "dec_R", "dec_b", "dense_W", "dense_b")]


def _gpu_fwd(c, tape=True):
    from longterm360fov_amd import ops
    opt = lambda a: None if a is None else dev(a)
    y, tp = ops.selffed_decoder_fwd(dev(c["x0"]), *_dec_w(c["w"]), c["T"], h0=opt(c["h0"]), c0=opt(c["c0"]), r=opt(c["r"]),
                                    act=c["act"], dense_activation=c["dact"], tape=tape)
    torch.cuda.synchronize()
    return y, tp


def _gpu_bwd(c, tp):
    from longterm360fov_amd import ops
    K, R, _, W, _ = _dec_w(c["w"])
    out = ops.selffed_decoder_bwd(tp, dev(c["dloss"]), K, R, W, act=c["act"], dense_activation=c["dact"])
    torch.cuda.synchronize()
    return out


def _np(d, keys):
    return {k: None if d[k] is None else d[k].cpu().numpy() for k in keys}


def _check_forward(tag, c, y, tp):
    ref = c["ref"]
    _held(tag + " y", y.cpu().numpy(), ref["y"])
    for k in TAPES:
        if ref[k] is None:
            assert tp[k] is None
        else:
            _held(tag + " " + k, tp[k].cpu().numpy(), ref[k])
    np.testing.assert_array_equal(y.cpu().numpy(), tp["XA"][1:].transpose(0, 1).cpu().numpy())     # y is XA[1:], batch-major
    if c["r"] is not None:      # y_t = a_t + r is one fp32 addition
        assert torch.equal(tp["XA"][1:], tp["A"] + dev(c["r"])[None])


# ------------------------------------------------------------------------------------------------------------------------------
# forward and tapes against fp64
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 16, 17, 33])
@pytest.mark.parametrize("H", [32, 64])
def test_forward_and_tapes_over_tiles_and_lengths(H, B):
    for T in (1, 2, 3, 5):
        act = "hard_sigmoid" if (B + T) % 2 else "sigmoid"
        c = _case(H, B, T, 6, act, "tanh", T != 2, T == 3)
        y, tp = _gpu_fwd(c)
        _check_forward("H%d B%d T%d %s" % (H, B, T, act), c, y, tp)
        y_only, none = _gpu_fwd(c, tape=False)      # predict's call: no tape pointer, the same prediction
        assert none is None and torch.equal(y_only, y)


@pytest.mark.parametrize("H,n_out,act,dact,state,residual", [
    (64, 6, "sigmoid", "tanh", False, False), (64, 6, "sigmoid", "tanh", True, False),       # zero / given state
    (32, 6, "hard_sigmoid", "tanh", True, True), (64, 6, "sigmoid", "relu", False, True),    # residual, both heads
    (32, 6, "sigmoid", "relu", True, False), (64, 6, "hard_sigmoid", "relu", True, True),
    (64, 1, "sigmoid", "tanh", True, True), (32, 3, "hard_sigmoid", "relu", False, False),   # feedback widths
    (64, 8, "hard_sigmoid", "tanh", False, True), (32, 8, "sigmoid", "relu", True, True), (32, 1, "sigmoid", "tanh", False, False)])
def test_forward_variants(H, n_out, act, dact, state, residual):
    c = _case(H, 17, 3, n_out, act, dact, state, residual)
    y, tp = _gpu_fwd(c)
    _check_forward("H%d O%d %s %s state=%d res=%d" % (H, n_out, act, dact, state, residual), c, y, tp)


def test_forward_sixty_four_steps():
    c = _case(64, 17, 64, 6, "sigmoid", "tanh", True, False)
    y, tp = _gpu_fwd(c)
    _check_forward("H64 B17 T64", c, y, tp)


# ------------------------------------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------------------------------------
BWD_CASES = [(64, 17, 5, 6, "sigmoid", "tanh", True, False), (32, 33, 3, 6, "hard_sigmoid", "relu", True, True),
             (64, 1, 1, 6, "hard_sigmoid", "tanh", False, True), (32, 16, 2, 3, "sigmoid", "relu", False, False),
             (64, 33, 4, 8, "hard_sigmoid", "relu", True, True), (32, 17, 5, 1, "sigmoid", "tanh", True, False)]


def _trainer(c, **flags):
    from longterm360fov_amd.training import SelfFedSeq2SeqTrainer
    w = {k: v for k, v in c["w"].items() if c["r"] is not None or not k.startswith("res_")}
    tr = SelfFedSeq2SeqTrainer(w, act=c["act"], dense_activation=c["dact"], decoder_no_init_state=c["h0"] is None,
                               add_residual_link=c["r"] is not None)
    for k, v in flags.items():
        setattr(tr, k, v)
    return tr


def _unroll_backward(tr, tp, dloss):
    """_unroll_backward's six results; DPRE and DZ are taken where the weight-gradient products receive them."""
    seen = {}
    products = tr._unroll_wgrads
    tr._unroll_wgrads = lambda tp_, DPRE, DZ: (seen.update(DPRE=DPRE, DZ=DZ), products(tp_, DPRE, DZ))
    try:
        tr.grad.zero_()
        dx0, dh0, dc0, DY = tr._unroll_backward(tp, dloss)
    finally:
        del tr._unroll_wgrads
    torch.cuda.synchronize()
    out = dict(DY=DY, DPRE=seen["DPRE"], DZ=seen["DZ"], dx0=dx0, dh0=dh0, dc0=dc0)
    return {k: v.cpu().numpy() for k, v in out.items()}, tr.grad.clone()


@pytest.mark.parametrize("H,B,T,n_out,act,dact,state,residual", BWD_CASES)
def test_fused_backward_on_the_loops_tape(H, B, T, n_out, act, dact, state, residual):
    """The backward kernel alone: the step-by-step forward writes the tape, then both backwards read that same tape."""
    c = _case(H, B, T, n_out, act, dact, state, residual)
    opt = lambda a: None if a is None else dev(a)
    tr = _trainer(c, fused_unroll=False, fused_unroll_bwd=False)
    tp = tr._unroll_forward("dec", "dense", dev(c["x0"]), opt(c["h0"]), opt(c["c0"]), T, dact, opt(c["r"]))
    assert "y" not in tp
    loop, g_loop = _unroll_backward(tr, tp, dev(c["dloss"]))
    tr.fused_unroll_bwd = True
    fused, g_fused = _unroll_backward(tr, tp, dev(c["dloss"]))
    for k in BWD_OUT:
        _grad_held("loop tape, fused vs loop %s" % k, fused[k], loop[k])
        _grad_held("loop tape, fused vs fp64 %s" % k, fused[k], c["ref"][k])
    for name, _ in tr.shapes:        # and the weight-gradient products over the fused kernel's DPRE / DZ
        if name.startswith(("dec_", "dense_")):
            lo = tr.offset[name]
            n = tr.g[name].numel()
            _grad_held("loop tape, weight gradient " + name, g_fused[lo:lo + n].cpu().numpy(), g_loop[lo:lo + n].cpu().numpy())


@pytest.mark.parametrize("H,B,T,n_out,act,dact,state,residual", BWD_CASES + [(64, 32, 30, 6, "sigmoid", "tanh", False, False)])
def test_fused_forward_and_backward_against_autograd(H, B, T, n_out, act, dact, state, residual):
    c = _case(H, B, T, n_out, act, dact, state, residual)
    y, tp = _gpu_fwd(c)
    got = _np(_gpu_bwd(c, tp), BWD_OUT)
    for k in BWD_OUT:
        _grad_held("H%d B%d T%d O%d %s" % (H, B, T, n_out, k), got[k], c["ref"][k])


def _graph64(enc, dec0, tgt, w, act, no_init, residual, enc_as_in, dact):
    """fp64 torch.autograd restatement of FoV_seq2seq_no_teac_forc.py:37-149 (onelayer_tar_seq2seq) under MSE."""
    t = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in w.items()}
    H = w["enc_R"].shape[0]
    fa = _head(dact)
    e, d0, tg = (torch.tensor(a.astype(np.float64)) for a in (enc, dec0, tgt))
    B = e.shape[0]
    log = {"z": [], "gates": [], "P_extra": []}
    h = c = torch.zeros(B, H, dtype=torch.float64)
    for tt in range(e.shape[1]):
        h, c = _step64(e[:, tt], h, c, t["enc_K"], t["enc_R"], t["enc_b"], act, log)
    if enc_as_in:
        p0 = h @ t["dense_W"] + t["dense_b"]
        log["P_extra"].append(p0)
        x0 = fa(p0)
    else:
        x0 = d0[:, 0]
    r = None
    if residual:
        pr = x0 @ t["res_W"] + t["res_b"]
        log["P_extra"].append(pr)
        r = fa(pr)
    z0 = torch.zeros(B, H, dtype=torch.float64)
    y = _unroll64(x0, z0 if no_init else h, z0 if no_init else c, r, t["dec_K"], t["dec_R"], t["dec_b"], t["dense_W"], t["dense_b"],
                  tg.shape[1], act, dact, log)
    loss = torch.mean((y - tg) ** 2)
    loss.backward()
    grads = {k: (np.zeros_like(w[k], dtype=np.float64) if v.grad is None else v.grad.numpy()) for k, v in t.items()}
    return float(loss.detach()), grads, y.detach().numpy(), _margins(log, act, dact, H)


@functools.lru_cache(maxsize=None)
def _graph_case(H, B, T_in, T_out, act, no_init, residual, enc_as_in, dact):
    for attempt in range(16):
        seed = 131 * attempt + H + B
        w = _weights(H, 6, 90 + seed)
        if not residual:
            del w["res_W"], w["res_b"]
        enc, dec0, tgt = O.synthetic_batch(91 + seed, B, T_in, T_out)
        if dact == "relu":
            tgt = np.abs(tgt)
        loss, grads, y, (m_rec, m_relu) = _graph64(enc, dec0, tgt, w, act, no_init, residual, enc_as_in, dact)
        if m_rec > 1e-4 and m_relu > 1e-4:
            break
    assert m_rec > 1e-4, "a hard_sigmoid pre-activation within 1e-4 of +-2.5"
    assert m_relu > 1e-4, "a relu pre-activation within 1e-4 of 0"
    kw = dict(decoder_no_init_state=no_init, add_residual_link=residual, enc_last_out_as_dec_in=enc_as_in)
    y_o = O.onelayer_tar_seq2seq_forward(enc.astype(np.float64), dec0.astype(np.float64), f64(w), T_out, act=act, dense_activation=dact, **kw)
    np.testing.assert_allclose(y_o, y, atol=1e-12)
    return w, enc, dec0, tgt, kw, loss, grads, y


GRAPH_CASES = [(64, 21, 4, 5, "sigmoid", True, False, False, "tanh"),          # the script as committed
               (32, 33, 5, 4, "hard_sigmoid", False, False, False, "tanh"),    # decoder seeded with the encoder state
               (64, 40, 3, 6, "sigmoid", False, True, False, "tanh"),          # cfg.add_residual_link
               (64, 17, 4, 3, "hard_sigmoid", True, False, True, "tanh"),      # cfg.enc_last_out_as_dec_in
               (32, 9, 3, 4, "sigmoid", False, True, True, "relu")]            # all of them + cfg.rescale_input


@pytest.mark.parametrize("H,B,T_in,T_out,act,no_init,residual,enc_as_in,dact", GRAPH_CASES)
def test_training_step_gradients_against_autograd(H, B, T_in, T_out, act, no_init, residual, enc_as_in, dact):
    from longterm360fov_amd import ops
    from longterm360fov_amd.training import SelfFedSeq2SeqTrainer
    w, enc, dec0, tgt, kw, loss_ref, g_ref, y_ref = _graph_case(H, B, T_in, T_out, act, no_init, residual, enc_as_in, dact)
    tr = SelfFedSeq2SeqTrainer(w, act=act, dense_activation=dact, **kw)
    calls = []
    fwd, bwd = ops.selffed_decoder_fwd, ops.selffed_decoder_bwd
    ops.selffed_decoder_fwd = lambda *a, **k: (calls.append("fwd"), fwd(*a, **k))[1]
    ops.selffed_decoder_bwd = lambda *a, **k: (calls.append("bwd"), bwd(*a, **k))[1]
    try:
        loss, y = tr.forward_backward(dev(enc), dev(dec0), dev(tgt))
    finally:
        ops.selffed_decoder_fwd, ops.selffed_decoder_bwd = fwd, bwd
    assert calls == ["fwd", "bwd"]
    tr.ws.check(); tr.bwd_scratch.check()
    assert abs(float(loss.item()) - loss_ref) <= 1e-5 * loss_ref + 1e-9
    _held("forward_backward prediction", y.cpu().numpy(), y_ref)
    for k in tr.g:
        _grad_held("H%d grad %s" % (H, k), tr.g[k].detach().cpu().numpy(), g_ref[k])
    if no_init and not enc_as_in:       # reference quirk: the encoder does not reach the loss
        assert float(tr.g["enc_K"].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# exact properties
# ------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    c = _case(64, 33, 5, 6, "hard_sigmoid", "relu", True, True)
    y1, tp1 = _gpu_fwd(c)
    y2, tp2 = _gpu_fwd(c)
    assert torch.equal(y1, y2) and all(torch.equal(tp1[k], tp2[k]) for k in TAPES)
    b1, b2 = _gpu_bwd(c, tp1), _gpu_bwd(c, tp1)
    assert all(torch.equal(b1[k], b2[k]) for k in BWD_OUT)


@pytest.mark.parametrize("H,act,dact", [(64, "sigmoid", "tanh"), (32, "hard_sigmoid", "relu")])
def test_a_sequence_does_not_depend_on_its_place_in_the_batch(H, act, dact):
    c = _case(H, 33, 4, 6, act, dact, True, True)
    row = 5
    one = dict(c, B=1, **{k: c[k][row:row + 1] for k in ("x0", "h0", "c0", "r")}, dloss=np.ascontiguousarray(c["dloss"][:, row:row + 1]))
    y, tp = _gpu_fwd(c)
    y1, tp1 = _gpu_fwd(one)
    assert torch.equal(y[row:row + 1], y1)
    for k in TAPES:
        assert torch.equal(tp[k][:, row:row + 1], tp1[k]), k
    b, b1 = _gpu_bwd(c, tp), _gpu_bwd(one, tp1)
    for k in ("DY", "DPRE", "DZ"):
        assert torch.equal(b[k][:, row:row + 1], b1[k]), k
    for k in ("dx0", "dh0", "dc0"):
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
    c = _case(H, B, T, n_out, "sigmoid", "tanh", True, True)
    y_ref, tp_ref = _gpu_fwd(c)
    b_ref = _gpu_bwd(c, tp_ref)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    K, R, b, W, bd = _dec_w(c["w"])
    x0, h0, c0, r, dloss = (dev(c[k]) for k in ("x0", "h0", "c0", "r", "dloss"))
    buf, v, gaps = _between_canaries({"Hs": (T + 1, B, H), "Cs": (T + 1, B, H), "XA": (T + 1, B, n_out), "A": (T, B, n_out),
                                      "RES": (T, B, 1, 5, H), "y": (B, T, n_out)}, canary)
    st = ops._stream()
    ops.check(_lib.lib().fov_selffed_decoder_fwd(p(x0), p(h0), p(c0), p(K), p(R), p(b), p(W), p(bd), p(r), p(v["Hs"]), p(v["Cs"]),
                                                 p(v["XA"]), p(v["A"]), p(v["RES"]), p(v["y"]), B, T, n_out, H, _lib.ACT_SIGMOID, 1, st))
    buf2, o, gaps2 = _between_canaries({"DY": (T, B, n_out), "DPRE": (T, B, n_out), "DZ": (T, B, 4 * H), "dx0": (B, n_out),
                                        "dh0": (B, H), "dc0": (B, H)}, canary)
    ops.check(_lib.lib().fov_selffed_decoder_bwd(p(v["Cs"]), p(v["XA"]), p(v["A"]), p(v["RES"]), p(dloss), p(K), p(R), p(W), p(o["DY"]),
                                                 p(o["DPRE"]), p(o["DZ"]), p(o["dx0"]), p(o["dh0"]), p(o["dc0"]), B, T, n_out, H,
                                                 _lib.ACT_SIGMOID, 1, 1, st))
    torch.cuda.synchronize()
    for lo, hi in gaps:
        assert bool((buf[lo:hi] == canary).all()), (lo, hi)
    for lo, hi in gaps2:
        assert bool((buf2[lo:hi] == canary).all()), (lo, hi)
    assert torch.equal(v["y"], y_ref) and all(torch.equal(v[k], tp_ref[k]) for k in TAPES)
    assert all(torch.equal(o[k], b_ref[k]) for k in BWD_OUT)


@pytest.mark.parametrize("H", [32, 64])
def test_clamped_hard_sigmoid_gates_have_exactly_zero_dz(H):
    c = _case(H, 17, 3, 6, "hard_sigmoid", "tanh", True, False, True)
    cols = {3: 1.0, H + 17: 0.0, 3 * H + 30: 1.0, H - 1: 0.0, 2 * H - 2: 1.0}      # dec_b column -> the gate's clamped value
    gate = lambda col: c["ref"]["RES"][:, :, 0, col // H, col % H]
    for col, val in cols.items():
        assert (gate(col) == val).all(), "the bias does not clamp gate column %d in fp64" % col
    y, tp = _gpu_fwd(c)
    _check_forward("clamped gates H%d" % H, c, y, tp)
    got = _np(_gpu_bwd(c, tp), BWD_OUT)
    for k in BWD_OUT:
        _grad_held("clamped gates H%d %s" % (H, k), got[k], c["ref"][k])
    for col, val in cols.items():
        assert (tp["RES"][:, :, 0, col // H, col % H] == val).all()
        assert (got["DZ"][:, :, col] == 0.0).all(), col
        assert (c["ref"]["DZ"][:, :, col] == 0.0).all()
    assert float(np.abs(got["DZ"]).max()) > 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# dispatch
# ------------------------------------------------------------------------------------------------------------------------------
def _per_step_launches_raise(monkeypatch):
    """ops.lstm_seq_train on a one-step sequence, ops.lstm_seq_bwd and ops.dense raise.  The encoder's forward (a whole sequence)
    stays: forward_backward runs it even where the reference's quirk keeps its gradient at zero and skips its BPTT."""
    from longterm360fov_amd import ops
    layer = ops.lstm_seq_train

    def boom(*a, **k):
        raise AssertionError("a per-step launch")

    def layer_or_boom(x, *a, **k):
        if x.shape[1] == 1:
            boom()
        return layer(x, *a, **k)
    monkeypatch.setattr(ops, "lstm_seq_train", layer_or_boom)
    monkeypatch.setattr(ops, "lstm_seq_bwd", boom)
    monkeypatch.setattr(ops, "dense", boom)


def _default_flag_step(H=64, B=32, T_in=4, T_out=5):
    w = {k: v for k, v in _weights(H, 6, 90 + H).items() if not k.startswith("res_")}
    enc, dec0, tgt = O.synthetic_batch(91 + B, B, T_in, T_out)
    return w, dev(enc), dev(dec0), dev(tgt)


def test_default_training_step_takes_no_per_step_launch(monkeypatch):
    from longterm360fov_amd.training import SelfFedSeq2SeqTrainer
    w, enc, dec0, tgt = _default_flag_step()
    _per_step_launches_raise(monkeypatch)
    tr = SelfFedSeq2SeqTrainer(w)
    assert tr.fused_unroll and tr.fused_unroll_bwd
    loss = float(tr.train_step(enc, dec0, tgt).item())
    assert np.isfinite(loss) and loss > 0
    for flags in (dict(fused_unroll=False), dict(fused_unroll_bwd=False)):
        loop = SelfFedSeq2SeqTrainer(w)
        for k, v in flags.items():
            setattr(loop, k, v)
        with pytest.raises(AssertionError, match="a per-step launch"):
            loop.train_step(enc, dec0, tgt)
    wide = {k: v for k, v in _weights(128, 6, 5).items() if not k.startswith("res_")}
    with pytest.raises(AssertionError, match="a per-step launch"):      # wider than the kernels take: the loop is still the path
        SelfFedSeq2SeqTrainer(wide).train_step(enc, dec0, tgt)


def test_knob_keeps_the_loop_and_both_paths_agree(monkeypatch):
    from longterm360fov_amd import ops
    from longterm360fov_amd.training import SelfFedSeq2SeqTrainer
    H, B, T_in, T_out, act, no_init, residual, enc_as_in, dact = GRAPH_CASES[2]
    w, enc, dec0, tgt, kw, loss_ref, g_ref, y_ref = _graph_case(H, B, T_in, T_out, act, no_init, residual, enc_as_in, dact)
    steps = []
    layer = ops.lstm_seq_train
    monkeypatch.setattr(ops, "lstm_seq_train", lambda x, *a, **k: (steps.append(x.shape[1]), layer(x, *a, **k))[1])
    tr = SelfFedSeq2SeqTrainer(w, act=act, dense_activation=dact, **kw)
    loss_f, y_f = tr.forward_backward(dev(enc), dev(dec0), dev(tgt))
    g_f, y_f, loss_f = {k: v.clone() for k, v in tr.g.items()}, y_f.clone(), float(loss_f.item())
    assert steps == [T_in]
    assert "FOV_NO_SELFFED_FUSED" not in os.environ
    os.environ["FOV_NO_SELFFED_FUSED"] = "1"
    try:
        loss_l, y_l = tr.forward_backward(dev(enc), dev(dec0), dev(tgt))
        torch.cuda.synchronize()
    finally:
        del os.environ["FOV_NO_SELFFED_FUSED"]
    assert steps == [T_in, T_in] + [1] * T_out          # the loop ran
    assert ops.selffed_decoder_supported(B, T_out, 6, H)
    _held("knob: loop prediction", y_l.cpu().numpy(), y_ref)
    _held("knob: loop vs fused prediction", y_l.cpu().numpy(), y_f.cpu().numpy().astype(np.float64))
    assert abs(float(loss_l.item()) - loss_f) <= 1e-5 * loss_f + 1e-9
    for k in tr.g:
        _grad_held("knob: loop vs fp64 " + k, tr.g[k].cpu().numpy(), g_ref[k])
        _grad_held("knob: fused vs loop " + k, g_f[k].cpu().numpy(), tr.g[k].cpu().numpy())


@pytest.mark.parametrize("case", [2, 4])
def test_predict_with_a_residual_link_is_the_fused_forward(monkeypatch, case):
    from longterm360fov_amd import ops
    from longterm360fov_amd.models import NoTeacherForcingSeq2Seq
    from longterm360fov_amd.training import self_fed_weight_order
    H, B, T_in, T_out, act, no_init, residual, enc_as_in, dact = GRAPH_CASES[case]
    w, enc, dec0, tgt, kw, loss_ref, g_ref, y_ref = _graph_case(H, B, T_in, T_out, act, no_init, residual, enc_as_in, dact)
    layer, calls = ops.lstm_seq, []

    def layer_or_boom(x, *a, **k):
        if x.shape[1] == 1:
            raise AssertionError("a per-step launch")
        return layer(x, *a, **k)
    fwd = ops.selffed_decoder_fwd
    monkeypatch.setattr(ops, "lstm_seq", layer_or_boom)
    monkeypatch.setattr(ops, "selffed_decoder_fwd", lambda *a, **k: (calls.append(k.get("tape")), fwd(*a, **k))[1])
    m = NoTeacherForcingSeq2Seq(latent_dim=H, recurrent_activation=act, predict_step=T_out, rescale_input=(dact == "relu"), **kw)
    m.set_weights([w[k] for k in self_fed_weight_order(add_residual_link=True)])
    got = m.predict(enc if enc_as_in else [enc, dec0])
    assert calls == [False]
    _held("predict, residual link, H%d" % H, got, y_ref)
    m.fused_unroll = False
    with pytest.raises(AssertionError, match="a per-step launch"):
        m.predict(enc if enc_as_in else [enc, dec0])


# ------------------------------------------------------------------------------------------------------------------------------
# training
# ------------------------------------------------------------------------------------------------------------------------------
def test_four_adam_steps_fused_and_loop_agree():
    from longterm360fov_amd.training import SelfFedSeq2SeqTrainer
    w, enc, dec0, tgt = _default_flag_step(H=64, B=32, T_in=4, T_out=10)
    fused, loop = SelfFedSeq2SeqTrainer(w), SelfFedSeq2SeqTrainer(w)
    loop.fused_unroll = loop.fused_unroll_bwd = False
    la = [float(fused.train_step(enc, dec0, tgt).item()) for _ in range(4)]
    lb = [float(loop.train_step(enc, dec0, tgt).item()) for _ in range(4)]
    print("fused", la, "loop", lb)
    for a, b in zip(la, lb):
        assert abs(a - b) <= 1e-5 * abs(b), (la, lb)
    assert la[-1] < la[0] and lb[-1] < lb[0]
