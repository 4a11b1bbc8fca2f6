"""The others-mixing decoder at its own width: the one-workgroup-per-tile kernels behind fov_mix_decoder_fwd (H = 32, 64) and
fov_mix_decoder_bwd (H = 32) (mix_tile.hip), the trainer's tile_decoder opt-in and the model's native_width opt-in.

References: oracle.mix_decoder_train_forward / mix_decoder_backward in fp64 for the kernels, an fp64 torch.autograd graph of the
whole model written here for the trainer, oracle.others_mixing_forward for the model.

Bounds - those the H = 256 kernels are held to, nothing looser:
    forward and every tape: 1e-4 absolute (test_mix_decoder_backward_matches_its_rounding_contract, fp32);
    kernel gradients:       1e-4 of each tensor's scale;
    trainer:                loss 1e-5 relative, prediction 2e-5, gradients 1e-4 of scale (test_others_mixing_gradients_and_training);
    fused against step-wise trainer: loss 1e-6 relative, gradients 2e-5 of scale (the same test's bound between its two runs);
    model:                  2e-5 against the oracle and against the padded-256 model.

Shapes: one sequence, one whole tile, a ragged second tile, three tiles; one step, three (both LDS parities) and one long run;
feedback widths 1, 5 (crosses a lane group), 6 and 8 (fills two).  Cases are computed once and shared."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

pytestmark = pytest.mark.gpu

TAPES = ("P", "H1", "C1", "H2", "C2", "res1", "res2")
BWD_OUT = ("DZ1", "DZ2", "dpre_m", "dpre_p", "dh1_0", "dc1_0", "dh2_0", "dc2_0")
CANARY = 12345.0

# (H, B, T, O, act)
CASES = [(H, B, 3, 6, "sigmoid") for H in (32, 64) for B in (1, 16, 17, 33)] + \
        [(32, 17, 3, 1, "hard_sigmoid"), (64, 17, 3, 5, "sigmoid"), (32, 33, 3, 8, "hard_sigmoid"), (64, 5, 3, 8, "hard_sigmoid"),
         (32, 17, 1, 6, "hard_sigmoid"), (64, 17, 1, 5, "sigmoid"), (64, 17, 64, 6, "sigmoid"), (32, 20, 30, 5, "sigmoid")]


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()


def d64(a):
    return a.detach().cpu().numpy().astype(np.float64) if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)


def f64(w):
    return {k: v.astype(np.float64) for k, v in w.items()}


def near(tag, got, ref, rel):
    got, ref = d64(got), d64(ref)
    scale, err = np.abs(ref).max(), np.abs(got - ref).max()
    print("%s: max|ref| %.3e err %.3e" % (tag, scale, err))
    assert err <= rel * scale + 1e-9, (tag, err, scale)


@functools.lru_cache(maxsize=None)
def inputs(H, B, T, O_, act):
    rng = np.random.default_rng(1000 * H + 37 * B + 5 * T + O_)
    w = O.init_others_mixing(H + B + T, F_dec=O_, H=H, num_user=4, bias_noise=0.1)
    return dict(H=H, B=B, T=T, O=O_, act=act, w=w, mix_Wp=(0.5 * rng.standard_normal((O_, O_))).astype(np.float32),
                st=[(0.4 * rng.standard_normal((B, H))).astype(np.float32) for _ in range(4)],
                dec0=rng.uniform(-1, 1, (B, O_)).astype(np.float32), oth=(0.3 * rng.standard_normal((B, T, O_))).astype(np.float32),
                G=(0.2 * rng.standard_normal((T, B, O_))).astype(np.float32))


def forward(c, train=True, oth=None, final=True):
    """ops.mix_decoder on the case -> dict M, tapes (C1 / C2 as T + 1 rows with the initial state in row 0), final states."""
    from longterm360fov_amd import ops
    H, B, T, O_ = c["H"], c["B"], c["T"], c["O"]
    e = lambda *s: torch.full(s, CANARY, dtype=torch.float32, device="cuda")
    st = [dev(s) for s in c["st"]]
    r = {"C1s": e(T + 1, B, H), "C2s": e(T + 1, B, H)}
    r["C1s"][0].copy_(st[1]); r["C2s"][0].copy_(st[3])
    tape = None
    if train:
        tape = {"P": e(T, B, O_), "H1": e(T, B, H), "C1": r["C1s"][1:], "H2": e(T, B, H), "C2": r["C2s"][1:], "res1": e(T, B, 5, H),
                "res2": e(T, B, 5, H)}
        r.update(tape)
    fs = tuple(e(B, H) for _ in range(4)) if final else None
    ws = ops.Workspace()
    r["M"] = ops.mix_decoder(dev(c["dec0"]), *st, dev(c["oth"]) if oth is None else oth, {k: dev(v) for k, v in c["w"].items()},
                             dev(c["mix_Wp"]), T, act=c["act"], workspace=ws, train=tape, final_state=fs, out=e(T, B, O_))
    ws.check()
    r["final"] = fs
    return r


def backward(c, M, P, res1, res2, C1s, C2s):
    from longterm360fov_amd import ops
    H, B, T, O_ = c["H"], c["B"], c["T"], c["O"]
    e = lambda *s: torch.full(s, CANARY, dtype=torch.float32, device="cuda")
    dloss = dev(c["G"]) * (1 - M * M)
    out = {k: e(T, B, 4 * H) for k in ("DZ1", "DZ2")}
    out.update({k: e(T, B, O_) for k in ("dpre_m", "dpre_p")})
    out.update({k: e(B, H) for k in ("dh1_0", "dc1_0", "dh2_0", "dc2_0")})
    ws = ops.Workspace()
    ops.mix_decoder_bwd(M, P, dloss, res1, res2, C1s, C2s, {k: dev(v) for k, v in c["w"].items()}, dev(c["mix_Wp"]), out, act=c["act"],
                        workspace=ws)
    ws.check()
    return out, dloss


@functools.lru_cache(maxsize=None)
def case(H, B, T, O_, act):
    """The case's inputs, the kernel's training forward, the fp64 oracle forward and (H = 32) the kernel's backward: once."""
    c = dict(inputs(H, B, T, O_, act))
    c["got"] = forward(c)
    c["ref"] = O.mix_decoder_train_forward(d64(c["dec0"]), *[d64(s) for s in c["st"]], d64(c["oth"]), f64(c["w"]), d64(c["mix_Wp"]), T,
                                           act=act)
    if H == 32:
        g = c["got"]
        c["bwd"], c["dloss"] = backward(c, g["M"], g["P"], g["res1"], g["res2"], g["C1s"], g["C2s"])
    return c


# ------------------------------------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,B,T,O_,act", CASES)
def test_forward_and_every_tape_against_fp64(H, B, T, O_, act):
    c = case(H, B, T, O_, act)
    for k in ("M",) + TAPES:
        err = np.abs(d64(c["got"][k]) - c["ref"][k]).max()
        print("tile decoder H=%d B=%d T=%d O=%d %s tape %-4s err %.3e" % (H, B, T, O_, act, k, err))
        assert err <= 1e-4, (k, err)
    for k, got in zip(("H1", "C1", "H2", "C2"), c["got"]["final"]):      # the final states are the last tape rows
        assert torch.equal(got, c["got"][k][T - 1]), k


@pytest.mark.parametrize("H,B,T,O_,act", [x for x in CASES if x[0] == 32])
def test_backward_on_the_kernels_own_tapes(H, B, T, O_, act):
    c = case(H, B, T, O_, act)
    g = c["got"]
    ref = O.mix_decoder_backward(d64(g["M"]), d64(g["P"]), d64(c["dloss"]), d64(g["res1"]), d64(g["res2"]), d64(g["C1s"]), d64(g["C2s"]),
                                 f64(c["w"]), d64(c["mix_Wp"]), act=act)
    for k in BWD_OUT:
        near("tile decoder bwd B=%d T=%d O=%d %s %s" % (B, T, O_, act, k), c["bwd"][k], ref[k], 1e-4)


@pytest.mark.parametrize("B,T,O_,act", [(17, 3, 6, "sigmoid"), (33, 2, 5, "hard_sigmoid")])
def test_backward_on_the_step_wise_walks_tapes(B, T, O_, act):
    """The tapes come from the per-step entry points (the trainer's walk), so the backward kernel is checked without the
    forward kernel."""
    from longterm360fov_amd import ops
    H = 32
    c = inputs(H, B, T, O_, act)
    dw = {k: dev(v) for k, v in c["w"].items()}
    e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    H1, C1, H2, C2 = e(T + 1, B, H), e(T + 1, B, H), e(T + 1, B, H), e(T + 1, B, H)
    for buf, s in zip((H1, C1, H2, C2), c["st"]):
        buf[0].copy_(dev(s))
    XM, P, R1, R2 = e(T + 1, B, O_), e(T, B, O_), e(T, B, 1, 5, H), e(T, B, 1, 5, H)
    XM[0].copy_(dev(c["dec0"]))
    oth, Wp = dev(c["oth"]), dev(c["mix_Wp"])
    ws = ops.Workspace()
    for t in range(T):
        ops.lstm_seq_train(XM[t].view(B, 1, O_), dw["dec1_K"], dw["dec1_R"], dw["dec1_b"], H1[t], C1[t], act=act, workspace=ws,
                           out=(H1[t + 1].view(B, 1, H), None, C1[t + 1], R1[t]))
        zx = ops.matmul(H1[t + 1], dw["dec2_K"]).reshape(B, 1, 4 * H)
        ops.lstm_seq_zx(zx, dw["dec2_R"], dw["dec2_b"], H2[t], C2[t], act=act, workspace=ws, reserve=R2[t],
                        out=(H2[t + 1].view(B, 1, H), None, C2[t + 1]))
        ops.mix_head_fwd(H2[t + 1], dw["dense_W"], dw["dense_b"], Wp, oth[:, t], P[t], XM[t + 1])
    ws.check()
    M, r1, r2 = XM[1:], R1.view(T, B, 5, H), R2.view(T, B, 5, H)
    out, dloss = backward(c, M, P, r1, r2, C1, C2)
    ref = O.mix_decoder_backward(d64(M), d64(P), d64(dloss), d64(r1), d64(r2), d64(C1), d64(C2), f64(c["w"]), d64(c["mix_Wp"]), act=act)
    for k in BWD_OUT:
        near("tile decoder bwd on walked tapes B=%d %s" % (B, k), out[k], ref[k], 1e-4)


@pytest.mark.parametrize("H,B,T,O_,act", [(32, 17, 3, 6, "sigmoid"), (64, 33, 3, 6, "sigmoid"), (64, 17, 3, 5, "sigmoid")])
def test_inference_call_gives_the_training_calls_bits(H, B, T, O_, act):
    c = case(H, B, T, O_, act)
    inf = forward(c, train=False)
    assert torch.equal(inf["M"], c["got"]["M"])
    for a, b in zip(inf["final"], c["got"]["final"]):
        assert torch.equal(a, b)
    again = forward(c)                                    # two calls give the same bits
    for k in ("M",) + TAPES:
        assert torch.equal(again[k], c["got"][k]), k
    if H == 32:
        g = c["got"]
        out, _ = backward(c, g["M"], g["P"], g["res1"], g["res2"], g["C1s"], g["C2s"])
        for k in BWD_OUT:
            assert torch.equal(out[k], c["bwd"][k]), k


@pytest.mark.parametrize("H", [32, 64])
def test_strided_and_broadcast_others_projection(H):
    B, T, O_, act = 17, 3, 6, "sigmoid"
    c = case(H, B, T, O_, act)
    big = torch.full((B, T + 2, O_ + 3), CANARY, dtype=torch.float32, device="cuda")
    view = big[:, 1:T + 1, :O_]                          # both strides larger than the dense ones
    view.copy_(dev(c["oth"]))
    assert view.stride(0) > T * O_ and view.stride(1) > O_ and view.stride(2) == 1
    got = forward(c, oth=view)
    for k in ("M",) + TAPES:
        assert torch.equal(got[k], c["got"][k]), k
    row = dev(c["oth"][:1, :1])                           # one row for every sequence and step: both strides 0
    bc = dict(c, oth=np.broadcast_to(c["oth"][:1, :1], (B, T, O_)).copy())
    got = forward(bc, oth=row.expand(B, T, O_))
    assert row.expand(B, T, O_).stride()[:2] == (0, 0)
    ref = O.mix_decoder_train_forward(d64(c["dec0"]), *[d64(s) for s in c["st"]], d64(bc["oth"]), f64(c["w"]), d64(c["mix_Wp"]), T, act=act)
    for k in ("M",) + TAPES:
        assert np.abs(d64(got[k]) - ref[k]).max() <= 1e-4, k
    assert torch.equal(got["M"], forward(bc)["M"])


def _guarded(shape, pad=64):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * pad,), CANARY, dtype=torch.float32, device="cuda")
    return buf, buf[pad:pad + n].view(*shape)


@pytest.mark.parametrize("H,B", [(64, 17), (32, 1)])
def test_rows_beyond_the_batch_are_not_written(H, B):
    """Every output lies between canaries: a store for a row of the ragged tile beyond B would land in them (the row behind the
    last one of the last step, or of a (B,H) state)."""
    from longterm360fov_amd import ops
    T, O_, act = 3, 6, "sigmoid"
    c = case(H, B, T, O_, act)
    shapes = {"M": (T, B, O_), "P": (T, B, O_), "H1": (T, B, H), "C1": (T, B, H), "H2": (T, B, H), "C2": (T, B, H), "res1": (T, B, 5, H),
              "res2": (T, B, 5, H), "h1T": (B, H), "c1T": (B, H), "h2T": (B, H), "c2T": (B, H)}
    g = {k: _guarded(s) for k, s in shapes.items()}
    st = [dev(s) for s in c["st"]]
    dw = {k: dev(v) for k, v in c["w"].items()}
    ws = ops.Workspace()
    ops.mix_decoder(dev(c["dec0"]), *st, dev(c["oth"]), dw, dev(c["mix_Wp"]), T, act=act, workspace=ws, out=g["M"][1],
                    train={k: g[k][1] for k in TAPES}, final_state=tuple(g[k][1] for k in ("h1T", "c1T", "h2T", "c2T")))
    ws.check()
    for k in ("M",) + TAPES:
        assert torch.equal(g[k][1], c["got"][k]), k
    if H == 32:
        C1s, C2s = torch.cat([st[1][None], g["C1"][1][:-1]]), torch.cat([st[3][None], g["C2"][1][:-1]])
        bs = {"DZ1": (T, B, 4 * H), "DZ2": (T, B, 4 * H), "dpre_m": (T, B, O_), "dpre_p": (T, B, O_), "dh1_0": (B, H), "dc1_0": (B, H),
              "dh2_0": (B, H), "dc2_0": (B, H)}
        gb = {k: _guarded(s) for k, s in bs.items()}
        ops.mix_decoder_bwd(g["M"][1], g["P"][1], c["dloss"], g["res1"][1], g["res2"][1], C1s, C2s, dw, dev(c["mix_Wp"]),
                            {k: gb[k][1] for k in BWD_OUT}, act=act, workspace=ws)
        for k in BWD_OUT:
            assert torch.equal(gb[k][1], c["bwd"][k]), k
        g.update(gb)
    for k, (buf, view) in g.items():
        pad = (buf.numel() - view.numel()) // 2
        assert bool((buf[:pad] == CANARY).all()) and bool((buf[-pad:] == CANARY).all()), k
        assert not bool((view == CANARY).any()), k        # and every row inside B was written


@pytest.mark.parametrize("H", [32, 64])
def test_a_sequence_does_not_depend_on_its_place_in_the_batch(H):
    B, T, O_, act = 33, 3, 6, "sigmoid"
    c = case(H, B, T, O_, act)
    for row in (5, 32):
        one = dict(c, B=1, st=[s[row:row + 1] for s in c["st"]], dec0=c["dec0"][row:row + 1], oth=c["oth"][row:row + 1],
                   G=c["G"][:, row:row + 1])
        got = forward(one)
        for k in ("M",) + TAPES:
            assert torch.equal(got[k][:, 0], c["got"][k][:, row]), (k, row)
        if H == 32:
            out, _ = backward(one, got["M"], got["P"], got["res1"], got["res2"], got["C1s"], got["C2s"])
            for k in BWD_OUT:
                a, b = (out[k][:, 0], c["bwd"][k][:, row]) if out[k].dim() == 3 else (out[k][0], c["bwd"][k][row])
                assert torch.equal(a, b), (k, row)


def test_null_workspace_is_accepted_and_the_wide_backward_is_refused():
    from longterm360fov_amd import _lib, ops
    H, B, T, O_, act = 64, 17, 3, 6, "sigmoid"
    c = case(H, B, T, O_, act)
    L = _lib.lib()
    dw = {k: dev(v) for k, v in c["w"].items()}
    st = [dev(s) for s in c["st"]]
    dec0, oth, Wp = dev(c["dec0"]), dev(c["oth"]), dev(c["mix_Wp"])
    out = torch.empty((T, B, O_), dtype=torch.float32, device="cuda")
    p = lambda t: t.data_ptr()
    rc = L.fov_mix_decoder_fwd(p(dec0), *[p(s) for s in st], p(oth), T * O_, O_,
                               *[p(dw[k]) for k in ("dec1_K", "dec1_R", "dec1_b", "dec2_K", "dec2_R", "dec2_b", "dense_W", "dense_b")], p(Wp),
                               p(out), *([None] * 11), B, T, H, O_, _lib.ACT_SIGMOID, None, 0, ops._stream())
    assert rc == _lib.OK, L.fov_last_error()
    assert torch.equal(out, c["got"]["M"])
    g = c["got"]
    with pytest.raises(_lib.FovError) as ei:
        backward(c, g["M"], g["P"], g["res1"], g["res2"], g["C1s"], g["C2s"])
    assert ei.value.code == _lib.ERR_UNSUPPORTED
    c32 = case(32, 17, 3, 6, "sigmoid")
    g = c32["got"]
    dloss = c32["dloss"]
    o = {k: torch.empty_like(v) for k, v in c32["bwd"].items()}
    dw = {k: dev(v) for k, v in c32["w"].items()}
    rc = L.fov_mix_decoder_bwd(p(g["M"]), p(g["P"]), p(dloss), p(g["res1"]), p(g["res2"]), p(g["C1s"]), p(g["C2s"]),
                               *[p(dw[k]) for k in ("dec1_K", "dec1_R", "dec2_K", "dec2_R", "dense_W")], p(dev(c32["mix_Wp"])),
                               *[p(o[k]) for k in BWD_OUT], 17, 3, 32, 6, _lib.ACT_SIGMOID, None, 0, ops._stream())
    assert rc == _lib.OK, L.fov_last_error()
    for k in BWD_OUT:
        assert torch.equal(o[k], c32["bwd"][k]), k


# ------------------------------------------------------------------------------------------------------------------------------
# trainer
# ------------------------------------------------------------------------------------------------------------------------------
def _torch_graph(enc, oth, dec0, tgt, w, act):
    """The whole model's training graph (given_others_gt_mean_var_seq2seq.py:203-308, mlp_mixing) in fp64 on torch.autograd."""
    t = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in w.items()}
    H = w["enc1_R"].shape[0]
    s = torch.sigmoid if act == "sigmoid" else (lambda z: torch.clamp(0.2 * z + 0.5, 0, 1))

    def step(x, h, c, K, R, b):
        z = x @ K + b + h @ R
        i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
        c = f * c + i * g
        return o * torch.tanh(c), c

    e, o_, d0, tg = (torch.tensor(a.astype(np.float64)) for a in (enc, oth, dec0, tgt))
    B = e.shape[0]
    h1 = c1 = h2 = c2 = torch.zeros(B, H, dtype=torch.float64)
    for tt in range(e.shape[1]):
        h1, c1 = step(e[:, tt], h1, c1, t["enc1_K"], t["enc1_R"], t["enc1_b"])
        h2, c2 = step(h1, h2, c2, t["enc2_K"], t["enc2_R"], t["enc2_b"])
    x = d0[:, 0]
    outs = []
    for tt in range(o_.shape[1]):
        h1, c1 = step(x, h1, c1, t["dec1_K"], t["dec1_R"], t["dec1_b"])
        h2, c2 = step(h1, h2, c2, t["dec2_K"], t["dec2_R"], t["dec2_b"])
        p = torch.tanh(h2 @ t["dense_W"] + t["dense_b"])
        x = torch.tanh(torch.cat([o_[:, tt], p[:, None, :]], dim=1).reshape(B, -1) @ t["mix_W"] + t["mix_b"])
        outs.append(x)
    y = torch.stack(outs, 1)
    loss = torch.mean((y - tg) ** 2)
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in t.items()}, y.detach().numpy()


@functools.lru_cache(maxsize=None)
def model_case(H, act, B=17, U=4, T_in=3, T_out=4):
    w = O.init_others_mixing(70 + H, H=H, num_user=U, bias_noise=0.1)
    enc, dec0, tgt, oth = O.synthetic_batch(71 + B + H, B, T_in, T_out, num_others=U - 1)
    loss, grads, y = _torch_graph(enc, oth, dec0, tgt, w, act)
    return dict(H=H, act=act, U=U, w=w, enc=enc, dec0=dec0, tgt=tgt, oth=oth, loss=loss, grads=grads, y=y)


def _count_all(monkeypatch):
    """Every public function of ops, counted by name."""
    import types
    from longterm360fov_amd import ops
    counts = {}

    def wrap(n, fn):
        def counted(*a, **k):
            counts[n] = counts.get(n, 0) + 1
            return fn(*a, **k)
        return counted
    for n, fn in list(vars(ops).items()):
        if isinstance(fn, types.FunctionType) and fn.__module__ == ops.__name__ and not n.startswith("_"):
            monkeypatch.setattr(ops, n, wrap(n, fn))
    return counts


PER_STEP = ("lstm_seq_train", "lstm_seq_zx", "lstm_seq", "mix_head_fwd", "mix_head_bwd", "dense_add")


@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("act", ["sigmoid", "hard_sigmoid"])
def test_trainer_against_autograd_and_the_step_wise_trainer(monkeypatch, H, act):
    from longterm360fov_amd.training import OthersMixingTrainer, _MIX_ORDER
    mc = model_case(H, act)
    args = [dev(mc[k]) for k in ("enc", "oth", "dec0", "tgt")]
    tr = OthersMixingTrainer(mc["w"], act=act, tile_decoder=True)
    counts = _count_all(monkeypatch)
    loss, y = tr.forward_backward(*args)
    torch.cuda.synchronize()
    tr.ws.check(); tr.bwd_scratch.check()
    # the forward is one call at both widths; the backward one call at 32 and the walk on the fused forward's tapes at 64
    assert counts.get("mix_decoder") == 1 and counts.get("stacked_seq2seq_train_fwd") == 1 and "mix_decoder_prepack" not in counts
    assert counts.get("mix_decoder_bwd", 0) == (1 if H == 32 else 0) and counts.get("mix_head_bwd", 0) == (0 if H == 32 else 4)
    assert all(counts.get(n, 0) == 0 for n in ("lstm_seq_train", "lstm_seq_zx", "mix_head_fwd"))
    loss0 = float(loss.item())                           # the loss lives in a slot of the flat buffer: read it before the next step
    assert abs(loss0 - mc["loss"]) <= 1e-5 * mc["loss"] + 1e-9
    np.testing.assert_allclose(y.cpu().numpy(), mc["y"], atol=2e-5)
    for k in _MIX_ORDER:
        near("tile trainer H%d %s grad %s" % (H, act, k), tr.g[k], mc["grads"][k], 1e-4)
    tr2 = OthersMixingTrainer(mc["w"], act=act, tile_decoder=True)
    tr2.fused_decoder = tr2.fused_decoder_bwd = False
    for step in range(4):                                # four Adam steps, fused against step-wise on the same trainer class
        l1, l2 = float(tr.train_step(*args).item()), float(tr2.train_step(*args).item())
        assert abs(l1 - l2) <= 1e-6 * abs(l2) + 1e-9, step
        for k in _MIX_ORDER:
            d = (tr.g[k] - tr2.g[k]).abs().max().item()
            assert d <= 2e-5 * tr2.g[k].abs().max().item() + 1e-9, (step, k, d)
    assert l1 < loss0


def test_trainer_refuses_what_the_tile_path_does_not_have():
    from longterm360fov_amd.training import OthersMixingTrainer
    with pytest.raises(AssertionError):
        OthersMixingTrainer(O.init_others_mixing(1, H=48, num_user=4), tile_decoder=True)
    with pytest.raises(AssertionError):
        OthersMixingTrainer(O.init_others_mixing(1, H=256, num_user=4), tile_decoder=True, dtype="bf16")


@pytest.mark.parametrize("H", [32, 64])
def test_no_call_count_grows_with_the_horizon(monkeypatch, H):
    """A training step and a prediction at 3 and at 6 decoder steps make the same calls, except the walk's at H = 64."""
    from longterm360fov_amd.models import OthersMixingSeq2Seq
    from longterm360fov_amd.training import OthersMixingTrainer, _MIX_ORDER
    per = {}
    for T_out in (3, 6):
        mc = model_case(H, "sigmoid", T_out=T_out)
        tr = OthersMixingTrainer(mc["w"], tile_decoder=True)
        args = [dev(mc[k]) for k in ("enc", "oth", "dec0", "tgt")]
        tr.train_step(*args)                              # the first step of a shape runs its side work in line
        m = OthersMixingSeq2Seq(latent_dim=H, num_user=mc["U"], seed=1, native_width=True)
        m.set_weights([mc["w"][k] for k in _MIX_ORDER])
        with monkeypatch.context() as mp:
            counts = _count_all(mp)
            tr.train_step(*args)
            torch.cuda.synchronize()
            per["train", T_out] = dict(counts)
        with monkeypatch.context() as mp:
            counts = _count_all(mp)
            got = m.predict([mc["enc"], mc["oth"], mc["dec0"]])
            per["predict", T_out] = dict(counts)
        np.testing.assert_allclose(got, mc["y"], atol=2e-5)
        assert per["predict", T_out].get("mix_decoder") == 1 and all(per["predict", T_out].get(n, 0) == 0 for n in PER_STEP)
        assert per["train", T_out].get("mix_decoder") == 1
    assert per["predict", 3] == per["predict", 6]
    if H == 32:
        assert per["train", 3] == per["train", 6], (per["train", 3], per["train", 6])
        assert per["train", 3].get("mix_decoder_bwd") == 1 and all(per["train", 3].get(n, 0) == 0 for n in PER_STEP + ("lstm_seq_bwd_step",))
    else:      # the forward is one call, the backward is the walk: its calls are the only ones that grow
        grew = {n for n in set(per["train", 3]) | set(per["train", 6]) if per["train", 3].get(n, 0) != per["train", 6].get(n, 0)}
        assert "mix_decoder_bwd" not in per["train", 6] and per["train", 6]["mix_head_bwd"] == 6 and per["train", 3]["mix_head_bwd"] == 3
        assert "mix_head_bwd" in grew and not (grew & {"mix_decoder", "lstm_seq_train", "lstm_seq_zx", "mix_head_fwd", "lstm_seq"}), grew


# ------------------------------------------------------------------------------------------------------------------------------
# model surface
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,act", [(32, "sigmoid"), (64, "hard_sigmoid")])
def test_native_width_model_surface(H, act):
    from longterm360fov_amd.models import OthersMixingSeq2Seq
    from longterm360fov_amd.training import OthersMixingTrainer, PaddedTrainer, _MIX_ORDER
    mc = model_case(H, act)
    x = [mc["enc"], mc["oth"], mc["dec0"]]
    y_o = O.others_mixing_forward(mc["enc"].astype(np.float64), mc["oth"].astype(np.float64), mc["dec0"].astype(np.float64), f64(mc["w"]),
                                  act=act)
    np.testing.assert_allclose(y_o, mc["y"], atol=1e-12)
    m = OthersMixingSeq2Seq(latent_dim=H, num_user=mc["U"], recurrent_activation=act, seed=1, native_width=True)
    m.set_weights([mc["w"][k] for k in _MIX_ORDER])
    assert m._run_width() == H
    got = m.predict(x)
    np.testing.assert_allclose(got, y_o, atol=2e-5)
    d = OthersMixingSeq2Seq(latent_dim=H, num_user=mc["U"], recurrent_activation=act, seed=1)      # the default: padded to 256
    d.set_weights([mc["w"][k] for k in _MIX_ORDER])
    assert d._run_width() == 256
    np.testing.assert_allclose(got, d.predict(x), atol=2e-5)
    assert [a.shape for a in m.get_weights()] == [mc["w"][k].shape for k in _MIX_ORDER]
    m.compile(optimizer="Adam", loss="mean_squared_error", metrics=["accuracy"])
    tr = m._get_trainer()
    assert isinstance(tr, OthersMixingTrainer) and not isinstance(tr, PaddedTrainer) and tr.tile_decoder
    losses = [m.train_on_batch(x, mc["tgt"]) for _ in range(4)]
    first = losses[0][0] if isinstance(losses[0], (list, tuple)) else losses[0]
    last = losses[-1][0] if isinstance(losses[-1], (list, tuple)) else losses[-1]
    assert abs(first - mc["loss"]) <= 1e-5 * mc["loss"] + 1e-9 and last < first
    h = m.fit(x, mc["tgt"], batch_size=8, epochs=2, validation_split=0.2)
    assert len(h.history["loss"]) == 2 and "val_loss" in h.history and any("acc" in k for k in h.history)
    with tempfile.TemporaryDirectory() as tmp:
        m.save_weights(os.path.join(tmp, "mixing_native.h5"))
        m2 = OthersMixingSeq2Seq(latent_dim=H, num_user=mc["U"], recurrent_activation=act, seed=9, native_width=True)
        m2.load_weights(os.path.join(tmp, "mixing_native.h5"))
        np.testing.assert_array_equal(m2.predict(x), m.predict(x))
