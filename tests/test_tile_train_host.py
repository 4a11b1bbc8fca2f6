"""The tile kernels that train - the self-fed two-layer decoder (fov_selffed2_decoder_fwd / _bwd, lstm_selffed2.hip), the
others-mixing decoder at H = 32 / 64 (fov_mix_decoder_fwd / _bwd, mix_tile.hip) and the stacked model's training graph
(fov_stacked_seq2seq_train_fwd / _bwd, lstm_stacked_train.hip) - on guarded views and at their value edges: the case tables of
tests/test_gpu_tile_train.py, the fp64 restatements they are held to, and everything that can be checked without a GPU.

Tables.  Shapes are the smallest at which each seam exists: B in {1, 16, 17, 30} (33 where R3 needs its extreme rows and a third
tile), step counts in {0, 1, 2, 3} (both LDS parities; T = 0 in the GPU module's own tests), one run of 64 steps per forward kernel
and of 30 at least per backward.  The two decoders run every feedback width O = 1 .. 8 at both widths (the backward at 32, all it
takes), the context and the head's bias on and off, the initial states all, none and one alone, the others' projection dense, with a
padded step stride and with both strides 0; the stacked graph runs _STACKED_ROWS of tests/test_tile_decoders_host.py (every
F_dec = 1 .. 8, F_enc of {1, 15, 16, 17, 32, 95, 96}, the empty phases) in each of its four instantiations.  The kernels' dispatch
code is read for its template instantiations, and each must be reached by a case.

References.  oracle.fov_oracle: selffed2_forward / selffed2_backward (the restatements that tests/test_gpu_selffed2_fused.py wrote,
moved there and imported back here as forward64 / backward64 with autograd64), mix_tile_forward / mix_tile_backward (the oracle's
mix_decoder_train_forward / mix_decoder_backward), stacked_train_forward / stacked_train_backward.  Each backward is checked here
against torch.autograd in fp64.

Asserted here for every regime case (R1 clamped hard_sigmoid, R2 saturated sigmoid / tanh, R3 overflowing rows, R4 a growing cell
state; a layer fed by a computed input has xk = 0.25): the shares of clamped / saturated pre-activations of every layer of every
phase, the overflow of R3's extreme rows, max |c| of R4, the shares of the fed-back tanh's arguments beyond 9 and inside +-1; that
8 e_ref (the restatement in fp32 against itself in fp64, in written bounds, forward and backward) stays below
REGIME_YARDSTICK_CAP; that each reference that is WRONG ON PURPOSE (SELFFED2_MISTAKES, MIX_TILE_MISTAKES, STACKED_TRAIN_MISTAKES)
misses the GPU test's bound by MARGIN = 10 at least on every case it applies to; and the guarded views of every case."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O
from test_guarded_views_host import MARGIN, OutView, margin_floats, same_bits, seed_of
from test_tile_decoders_host import _STACKED_ROWS, GRAD, INSTANTIATIONS, _assert_shares, _check_view, _frozen, offsets, stacked_weights, view, worst

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "longterm360fov_amd", "csrc")
BATCHES = (1, 16, 17, 30)
STATES, SF2_TAPES, SF2_GRADS = O.SELFFED2_STATES, O.SELFFED2_TAPES, O.SELFFED2_GRADS
LAYER_W = ("dec1_K", "dec1_R", "dec1_b", "dec2_K", "dec2_R", "dec2_b")
SF2_IN = ("x0",) + STATES + LAYER_W + ("W", "bd", "ctx")                      # each list in the C ABI's order
SF2_OUT = SF2_TAPES + ("y", "hT", "cT")
SF2_BWD_IN = ("C1", "C2", "XY", "RES1", "RES2", "dloss", "dec1_K", "dec1_R", "dec2_K", "dec2_R", "W")
MT_IN = ("dec0", "h1", "c1", "h2", "c2", "oth") + LAYER_W + ("dense_W", "dense_b", "mix_Wp")
MT_FINAL, MT_TRAIN = ("h1T", "c1T", "h2T", "c2T"), ("P", "H1", "C1", "H2", "C2", "res1", "res2")
MT_OUT = ("M",) + MT_FINAL + MT_TRAIN
MT_BWD_IN = ("M", "P", "dloss", "res1", "res2", "C1s", "C2s", "dec1_K", "dec1_R", "dec2_K", "dec2_R", "dense_W", "mix_Wp")
MT_GRADS = O.MIX_TILE_GRADS
ST_TAPES, ST_GRADS = O.STACKED_TRAIN_TAPES, ("enc_dz", "dec_dz")

# ---------------------------------------------------------------------------------------------------------------------
# the restatements of tests/test_gpu_selffed2_fused.py: the NumPy loops live in the oracle, the autograd graph here
# ---------------------------------------------------------------------------------------------------------------------
forward64, backward64 = O.selffed2_forward, O.selffed2_backward


def _rec_t(act):
    return torch.sigmoid if act == "sigmoid" else (lambda z: torch.clamp(0.2 * z + 0.5, 0, 1))


def _step_t(x, h, c, K, R, b, act, zs):
    H = R.shape[0]
    z = b + x @ K + h @ R
    z.retain_grad()
    zs.append(z)
    s = _rec_t(act)
    i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
    c = f * c + i * g
    return o * torch.tanh(c), c


def autograd64(x0, st, w, dloss, T, act):
    """The same unroll on fp64 torch tensors -> (y, every gradient of sum_t <y_t, dloss_t> the backward entry returns)."""
    leaf = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    B, H = x0.shape[0], w["dec1_R"].shape[0]
    t = {k: leaf(v) for k, v in w.items()}
    x = x0_ = leaf(x0)
    s0 = {k: leaf(np.zeros((B, H)) if st.get(k) is None else st[k]) for k in STATES}
    h1, c1, h2, c2 = (s0[k] for k in STATES)
    z1s, z2s, ps, ys = [], [], [], []
    for tt in range(T):
        h1, c1 = _step_t(x, h1, c1, t["dec1_K"], t["dec1_R"], t["dec1_b"], act, z1s)
        h2, c2 = _step_t(h1, h2, c2, t["dec2_K"], t["dec2_R"], t["dec2_b"], act, z2s)
        p = h2 @ t["W"]
        if "bd" in t:
            p = t["bd"] + p
        if "ctx" in t:
            p = p + t["ctx"][:, tt]
        p.retain_grad()
        x = torch.tanh(p)
        ps.append(p); ys.append(x)
    y = torch.stack(ys, 1)
    (y * torch.tensor(dloss.astype(np.float64)).transpose(0, 1)).sum().backward()
    gr = lambda seq: np.stack([a.grad.numpy() for a in seq])
    g = {"DPRE": gr(ps), "DZ1": gr(z1s), "DZ2": gr(z2s), "dx0": x0_.grad.numpy()}
    g.update({"d" + k: s0[k].grad.numpy() for k in STATES})
    return y.detach().numpy(), g


# ---------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------
_CTX_BD = ((True, False), (False, True), (True, True), (False, False))
_STATE_FORMS = ("all", "none") + STATES
_OTH_FORMS = ("dense", "padded", "bcast")


def selffed2_cases():
    """-> [dict(id, H, O, B, T, act, ctx, bd, state)]: every O = 1 .. 8 at both widths; a case of width 32 runs the backward too."""
    out = []
    for k, H in enumerate((32, 64)):
        for i in range(8):
            B, T = BATCHES[(i + k) % 4], (1, 2, 3)[(i + 2 * k) % 3]
            act = "hard_sigmoid" if (i + k) % 2 else "sigmoid"
            (ctx, bd), state = _CTX_BD[(i + 3 * k) % 4], _STATE_FORMS[(i + 2 * k) % 6]
            out.append(dict(id="selffed2-H%d-O%d-B%d-T%d-%s-ctx%d-bd%d-%s" % (H, i + 1, B, T, act, ctx, bd, state), H=H, O=i + 1, B=B, T=T,
                            act=act, ctx=ctx, bd=bd, state=state))
    return out


def mix_tile_cases():
    """-> [dict(id, H, O, B, T, act, oth_form)]: every O = 1 .. 8 at both widths; a case of width 32 runs the backward too.  Every case
    runs with the training tapes and without them."""
    out = []
    for k, H in enumerate((32, 64)):
        for i in range(8):
            B, T = BATCHES[(i + k + 1) % 4], (1, 2, 3)[(i + k) % 3]
            act = "hard_sigmoid" if (i + k) % 2 == 0 else "sigmoid"
            form = _OTH_FORMS[(i + 2 * k) % 3]
            out.append(dict(id="mixtile-H%d-O%d-B%d-T%d-%s-%s" % (H, i + 1, B, T, act, form), H=H, O=i + 1, B=B, T=T, act=act, oth_form=form))
    return out


def stacked_train_cases():
    """-> [dict(id, L, H, F_enc, F_dec, B, T_in, T_out, act)]: _STACKED_ROWS in each instantiation, B and the activation rotating."""
    out = []
    for k, (H, L) in enumerate(INSTANTIATIONS):
        for i, (F_dec, F_enc, T_in, T_out) in enumerate(_STACKED_ROWS):
            B = BATCHES[(i + k + 2) % 4]
            act = "hard_sigmoid" if (i + k) % 2 == 0 else "sigmoid"
            out.append(dict(id="sttrain-H%d-L%d-O%d-F%d-B%d-T%d-%d" % (H, L, F_dec, F_enc, B, T_in, T_out), L=L, H=H, F_enc=F_enc,
                            F_dec=F_dec, B=B, T_in=T_in, T_out=T_out, act=act))
    return out


# (regime, H, O, B, T, bd): O of 3 .. 6, where TILE_HEAD_BIAS has its thirds; R3 needs rows 3 and 9 and a third tile; the runs of 30
# and 64 steps (the backward walks them too)
SELFFED2_REGIME_CASES = [("R1", 32, 5, 17, 3, True), ("R1", 64, 6, 30, 3, False), ("R1", 32, 4, 16, 30, True),
                         ("R2", 32, 6, 17, 3, False), ("R2", 64, 4, 17, 2, True), ("R2", 32, 3, 30, 2, True),
                         ("R3", 32, 6, 33, 3, True), ("R3", 64, 5, 33, 2, False),
                         ("R4", 32, 6, 17, 64, True), ("R4", 64, 5, 17, 64, False)]
# (regime, H, O, B, T)
MIX_TILE_REGIME_CASES = [("R1", 32, 6, 17, 3), ("R1", 64, 4, 30, 2), ("R1", 32, 3, 16, 30), ("R2", 32, 5, 17, 3), ("R2", 64, 6, 17, 2),
                         ("R2", 32, 4, 30, 2), ("R3", 32, 5, 33, 3), ("R3", 64, 6, 33, 2), ("R4", 32, 5, 17, 64), ("R4", 64, 6, 17, 64)]
# (regime, HP, L, F_enc, F_dec, B, T_in, T_out): one per regime and instantiation; 4 + 60 = 64 steps, 10 + 20 = 30
STACKED_TRAIN_REGIME_CASES = [
    ("R1", 32, 2, 17, 5, 17, 2, 3), ("R1", 32, 3, 90, 8, 30, 3, 2), ("R1", 64, 2, 96, 4, 16, 10, 20), ("R1", 64, 3, 15, 7, 17, 2, 3),
    ("R2", 32, 2, 95, 7, 17, 3, 3), ("R2", 32, 3, 16, 4, 17, 2, 2), ("R2", 64, 2, 32, 5, 17, 3, 2), ("R2", 64, 3, 90, 6, 30, 2, 3),
    ("R3", 32, 2, 90, 6, 33, 4, 3), ("R3", 32, 3, 17, 3, 33, 10, 20), ("R3", 64, 2, 95, 8, 33, 2, 3), ("R3", 64, 3, 90, 6, 33, 4, 60)]


def selffed2_regime_id(c):
    return "selffed2-%s-H%d-O%d-B%d-T%d-bd%d" % c


def mix_tile_regime_id(c):
    return "mixtile-%s-H%d-O%d-B%d-T%d" % c


def stacked_train_regime_id(c):
    return "sttrain-%s-H%d-L%d-F%d-O%d-B%d-T%d-%d" % c


def _two_layers(rng, H, n_out):
    """Glorot / orthogonal layers with a bias of 0.1 N(0, 1) on top of Keras' unit forget bias: ordinary data."""
    w = {}
    for n, F in (("dec1", n_out), ("dec2", H)):
        K, R, b = O.init_lstm(rng, F, H)
        w[n + "_K"], w[n + "_R"], w[n + "_b"] = K, R, (b + 0.1 * rng.standard_normal(4 * H)).astype(np.float32)
    return w


# ---- self-fed two-layer decoder ----
def _sf2_finish(p):
    p["ref"] = forward64(p["x0"], p["st"], p["w"], p["T"], p["act"])[0]
    p["tape32"] = forward64(p["x0"], p["st"], p["w"], p["T"], p["act"], np.float32)[0]
    _frozen(p)
    return p


@functools.lru_cache(maxsize=None)
def selffed2_case(cid):
    """One ordinary case: weights (W, and bd / ctx where the case has them), fp32 inputs, the fp64 forward and the fp32 one."""
    c = {x["id"]: x for x in selffed2_cases()}[cid]
    H, n_out, B, T = c["H"], c["O"], c["B"], c["T"]
    rng = np.random.default_rng(seed_of(cid))
    w = _two_layers(rng, H, n_out)
    w["W"] = rng.uniform(-0.5, 0.5, (H, n_out)).astype(np.float32)
    if c["bd"]:
        w["bd"] = rng.uniform(-0.2, 0.2, n_out).astype(np.float32)
    if c["ctx"]:
        w["ctx"] = rng.uniform(-0.7, 0.7, (B, T, n_out)).astype(np.float32)
    keep = STATES if c["state"] == "all" else () if c["state"] == "none" else (c["state"],)
    st = {k: (0.3 * rng.standard_normal((B, H))).astype(np.float32) if k in keep else None for k in STATES}
    return _sf2_finish(dict(c, w=w, st=st, x0=rng.uniform(-1, 1, (B, n_out)).astype(np.float32),
                            dloss=rng.standard_normal((T, B, n_out)).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def selffed2_regime_case(c):
    regime, H, n_out, B, T, bd = c
    p = O.regime_selffed2(seed_of(selffed2_regime_id(c)) % (1 << 31), regime, H, n_out, B, T, bd)
    p.update(id=selffed2_regime_id(c), H=H, O=n_out, B=B, T=T)
    return _sf2_finish(p)


def selffed2_operands(p):
    src = dict(p["w"], x0=p["x0"], **p["st"])
    return {k: src.get(k) for k in SF2_IN}


def selffed2_grads(p, tape, dt=np.float64, mistake=None):
    return backward64(tape, p["dloss"], p["w"], p["act"], dt, mistake)


def selffed2_e_ref(p):
    """-> (forward, backward): per output, the fp32 restatement against the fp64 one in written bounds; per gradient, the backward
    on fp32 arrays against fp64, both on the fp32 forward's tapes, in units of 1e-4 max |ref| + 1e-9."""
    fwd = {k: O.regime_error(p["tape32"][k], p["ref"][k], "f32") for k in SF2_OUT}
    g64, g32 = selffed2_grads(p, p["tape32"]), selffed2_grads(p, p["tape32"], np.float32)
    return fwd, {k: O.regime_error(g32[k], g64[k], GRAD) for k in SF2_GRADS}


# ---- others-mixing decoder at a tile width ----
def mix_tile_outputs(tape, T):
    """The forward's outputs by the C ABI's names from the restatement's tapes (the final states are the last tape rows)."""
    out = {k: tape[k] for k in ("M",) + MT_TRAIN}
    out.update({k + "T": tape[k.upper()][T - 1] for k in ("h1", "c1", "h2", "c2")})
    return out


def mix_tile_bwd_tape(p, fwd):
    """The backward's inputs from a forward's outputs (numpy): C1s / C2s whose row t is the cell state BEFORE step t, and dloss =
    G (1 - M^2), the gradient that reaches the mixing tanh's argument from the loss alone, in fp32."""
    M = np.asarray(fwd["M"], np.float32)
    tape = {k: fwd[k] for k in ("M", "P", "res1", "res2")}
    tape["C1s"] = np.concatenate([p["st"][1][None], np.asarray(fwd["C1"], np.float32)[:-1]])
    tape["C2s"] = np.concatenate([p["st"][3][None], np.asarray(fwd["C2"], np.float32)[:-1]])
    return tape, (p["G"] * (np.float32(1) - M * M)).astype(np.float32)


def _mt_finish(p):
    args = (p["dec0"], p["st"], p["oth"], p["w"], p["mix_Wp"], p["T"], p["act"])
    p["ref"] = mix_tile_outputs(O.mix_tile_forward(*args), p["T"])
    p["tape32"] = mix_tile_outputs(O.mix_tile_forward(*args, np.float32), p["T"])
    _frozen(p)
    return p


@functools.lru_cache(maxsize=None)
def mix_tile_case(cid):
    c = {x["id"]: x for x in mix_tile_cases()}[cid]
    H, n_out, B, T = c["H"], c["O"], c["B"], c["T"]
    rng = np.random.default_rng(seed_of(cid))
    w = _two_layers(rng, H, n_out)
    w["dense_W"], w["dense_b"] = rng.uniform(-0.5, 0.5, (H, n_out)).astype(np.float32), rng.uniform(-0.2, 0.2, n_out).astype(np.float32)
    oth = (0.3 * rng.standard_normal((1, 1, n_out) if c["oth_form"] == "bcast" else (B, T, n_out))).astype(np.float32)
    return _mt_finish(dict(c, w=w, mix_Wp=(0.5 * rng.standard_normal((n_out, n_out))).astype(np.float32),
                           st=[(0.4 * rng.standard_normal((B, H))).astype(np.float32) for _ in range(4)],
                           dec0=rng.uniform(-1, 1, (B, n_out)).astype(np.float32), oth=np.broadcast_to(oth, (B, T, n_out)).copy(),
                           G=rng.standard_normal((T, B, n_out)).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def mix_tile_regime_case(c):
    regime, H, n_out, B, T = c
    p = O.regime_mix_tile(seed_of(mix_tile_regime_id(c)) % (1 << 31), regime, H, n_out, B, T)
    p.update(id=mix_tile_regime_id(c), H=H, O=n_out, B=B, T=T, oth_form="dense")
    return _mt_finish(p)


def mix_tile_operands(p):
    src = dict(p["w"], dec0=p["dec0"], oth=p["oth"], mix_Wp=p["mix_Wp"], **dict(zip(("h1", "c1", "h2", "c2"), p["st"])))
    return {k: src[k] for k in MT_IN}


def mix_tile_grads(p, tape, dloss, dt=np.float64, mistake=None):
    return O.mix_tile_backward(tape, dloss, p["w"], p["mix_Wp"], p["act"], dt, mistake)


def mix_tile_e_ref(p):
    fwd = {k: O.regime_error(p["tape32"][k], p["ref"][k], "f32") for k in MT_OUT}
    tape, dloss = mix_tile_bwd_tape(p, p["tape32"])
    g64, g32 = mix_tile_grads(p, tape, dloss), mix_tile_grads(p, tape, dloss, np.float32)
    return fwd, {k: O.regime_error(g32[k], g64[k], GRAD) for k in MT_GRADS}


# ---- stacked training graph ----
def _st_finish(p):
    p["ref"] = O.stacked_train_forward(p["w"], p["enc"], p["dec_in"], p["L"], p["act"])
    p["tape32"] = O.stacked_train_forward(p["w"], p["enc"], p["dec_in"], p["L"], p["act"], np.float32)
    _frozen(p)
    return p


def _st_inputs(rng, p):
    """The teacher-forced decoder inputs and the gradient that reaches the top decoder layer from the head."""
    p["dec_in"] = rng.uniform(-1, 1, (p["B"], p["T_out"], p["F_dec"])).astype(np.float32)
    p["dhs_top"] = (0.1 * rng.standard_normal((p["B"], p["T_out"], p["H"]))).astype(np.float32)
    return p


@functools.lru_cache(maxsize=None)
def stacked_train_case(cid):
    c = {x["id"]: x for x in stacked_train_cases()}[cid]
    rng = np.random.default_rng(seed_of(cid + " inputs"))
    enc = rng.uniform(-1, 1, (c["B"], c["T_in"], c["F_enc"])).astype(np.float32)
    return _st_finish(_st_inputs(rng, dict(c, w=stacked_weights(c), enc=enc)))


@functools.lru_cache(maxsize=None)
def stacked_train_regime_case(c):
    regime, H, L, F_enc, F_dec, B, T_in, T_out = c
    p = O.regime_stacked_seq2seq(seed_of(stacked_train_regime_id(c)) % (1 << 31), regime, L, H, F_enc, F_dec, B, T_in)
    p.update(id=stacked_train_regime_id(c), L=L, H=H, F_enc=F_enc, F_dec=F_dec, B=B, T_in=T_in, T_out=T_out)
    return _st_finish(_st_inputs(np.random.default_rng(seed_of(p["id"] + " inputs")), p))


def stacked_train_operands(p):
    ops = {"enc": p["enc"], "dec_in": p["dec_in"]}
    ops.update({"%s%d_%s" % (side, l, k): p["w"]["%s%d_%s" % (side, l, k)] for side in ("enc", "dec") for l in range(p["L"]) for k in "KRb"})
    return ops


def stacked_train_grads(p, tape, dt=np.float64, mistake=None):
    return O.stacked_train_backward(tape, p["dhs_top"], p["w"], p["L"], p["act"], dt, mistake)


def stacked_train_e_ref(p):
    fwd = {k: O.regime_error(p["tape32"][k], p["ref"][k], "f32") for k in ST_TAPES}
    g64, g32 = stacked_train_grads(p, p["tape32"]), stacked_train_grads(p, p["tape32"], np.float32)
    return fwd, {k: O.regime_error(g32[k], g64[k], GRAD) for k in ST_GRADS}


def all_cases(family):
    cases, regime_cases, case, regime_case = {"selffed2": (selffed2_cases, SELFFED2_REGIME_CASES, selffed2_case, selffed2_regime_case),
                                              "mixtile": (mix_tile_cases, MIX_TILE_REGIME_CASES, mix_tile_case, mix_tile_regime_case),
                                              "sttrain": (stacked_train_cases, STACKED_TRAIN_REGIME_CASES, stacked_train_case,
                                                          stacked_train_regime_case)}[family]
    return [case(c["id"]) for c in cases()] + [regime_case(c) for c in regime_cases]


# ---------------------------------------------------------------------------------------------------------------------
# the tables cover what they say, and every template instantiation of the three files
# ---------------------------------------------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _acts(text, kernel):
    """The activation template arguments `kernel` is instantiated with in its launcher."""
    return {{"FOV_ACT_SIGMOID": "sigmoid", "FOV_ACT_HARD_SIGMOID": "hard_sigmoid"}[a] for a in re.findall(kernel + r"<[^<>]*?(FOV_ACT_\w+)>", text)}


def instantiations():
    """{(kernel, HP, L or 0, act)} read from the dispatch code of the three files."""
    out = set()
    for name, fwd, bwd, fwd_launch, bwd_launch in (("lstm_selffed2.hip", "selffed2_fwd_kernel", "selffed2_bwd_kernel", "launch_selffed2_fwd",
                                                    "launch_selffed2_bwd"),
                                                   ("mix_tile.hip", "mix_tile_fwd_kernel", "mix_tile_bwd_kernel", "launch_mix_tile_fwd",
                                                    "mix_tile_bwd_launch")):
        text = _source(name)
        widths = {int(h) for h in re.findall(fwd_launch + r"<(\d+)>\(p", text)}
        (bwd_width,) = re.findall(r"int " + bwd_launch + r"\([^)]*\) \{\s*constexpr int HP = (\d+);", text)
        assert widths and len(_acts(text, fwd)) == 2 and len(_acts(text, bwd)) == 2, name
        out |= {(fwd, h, 0, a) for h in widths for a in _acts(text, fwd)} | {(bwd, int(bwd_width), 0, a) for a in _acts(text, bwd)}
    text = _source("lstm_stacked_train.hip")
    for kernel, launch in (("stacked_train_fwd_kernel", "launch_train_fwd"), ("stacked_train_bwd_kernel", "launch_train_bwd")):
        pairs = {(int(h), int(l)) for h, l in re.findall(launch + r"<(\d+), (\d+)>\(p", text)}
        assert pairs and len(_acts(text, kernel)) == 2, kernel
        out |= {(kernel, h, l, a) for h, l in pairs for a in _acts(text, kernel)}
    return out


def reached():
    """{(kernel, HP, L or 0, act)} that the tables run (a backward where the entry point has one for the width)."""
    out = set()
    for fam, fwd, bwd in (("selffed2", "selffed2_fwd_kernel", "selffed2_bwd_kernel"), ("mixtile", "mix_tile_fwd_kernel", "mix_tile_bwd_kernel")):
        for p in all_cases(fam):
            out.add((fwd, p["H"], 0, p["act"]))
            if p["H"] == 32:
                out.add((bwd, 32, 0, p["act"]))
    for p in all_cases("sttrain"):
        out |= {(k, p["H"], p["L"], p["act"]) for k in ("stacked_train_fwd_kernel", "stacked_train_bwd_kernel")}
    return out


def test_every_template_instantiation_is_reached_by_a_case():
    have, run = instantiations(), reached()
    assert len(have) == 4 + 2 + 4 + 2 + 8 + 8, sorted(have)
    assert have == run, (sorted(have - run), sorted(run - have))


def test_tables_cover_every_width_state_and_layout():
    for H in (32, 64):
        mine = [c for c in selffed2_cases() if c["H"] == H]
        assert {c["O"] for c in mine} == set(range(1, 9)) and {c["B"] for c in mine} == set(BATCHES) and {c["T"] for c in mine} == {1, 2, 3}
        for k in ("act", "ctx", "bd"):
            assert len({c[k] for c in mine}) == 2, (H, k)
        assert {c["state"] for c in mine} == set(_STATE_FORMS) and {(c["ctx"], c["bd"]) for c in mine} == set(_CTX_BD)
        mine = [c for c in mix_tile_cases() if c["H"] == H]
        assert {c["O"] for c in mine} == set(range(1, 9)) and {c["B"] for c in mine} == set(BATCHES) and {c["T"] for c in mine} == {1, 2, 3}
        assert {c["oth_form"] for c in mine} == set(_OTH_FORMS) and {c["act"] for c in mine} == {"sigmoid", "hard_sigmoid"}
        for table in (SELFFED2_REGIME_CASES, MIX_TILE_REGIME_CASES):
            assert {c[0] for c in table if c[1] == H} == {"R1", "R2", "R3", "R4"}
            assert [c for c in table if c[1] == H and c[4] == 64] and all(c[3] > 32 for c in table if c[0] == "R3")
            assert [c for c in table if c[0] == "R2" and c[3] == 17 and c[1] == H]                   # the row-alone check's cases
    assert [c for c in SELFFED2_REGIME_CASES if c[1] == 32 and c[4] >= 30] and [c for c in MIX_TILE_REGIME_CASES if c[1] == 32 and c[4] >= 30]
    assert {c[2] <= 4 for c in SELFFED2_REGIME_CASES} == {True, False} and {c[2] <= 4 for c in MIX_TILE_REGIME_CASES} == {True, False}
    for H, L in INSTANTIATIONS:
        mine = [c for c in stacked_train_cases() if (c["H"], c["L"]) == (H, L)]
        assert {c["F_dec"] for c in mine if c["T_out"] > 0} == set(range(1, 9))
        assert {c["F_enc"] for c in mine if c["T_in"] > 0} == {1, 15, 16, 17, 32, 95, 96}
        assert [c for c in mine if c["T_out"] == 0 and c["T_in"] > 0] and [c for c in mine if c["T_in"] == 0 and c["T_out"] > 0]
        assert {c["B"] for c in mine} == set(BATCHES) and {c["act"] for c in mine} == {"sigmoid", "hard_sigmoid"}
        assert {c["T_in"] for c in mine} == {0, 1, 2, 3} and {c["T_in"] % 2 for c in mine if c["T_out"]} == {0, 1}
        assert {r[0] for r in STACKED_TRAIN_REGIME_CASES if (r[1], r[2]) == (H, L)} == {"R1", "R2", "R3"}
    assert [r for r in STACKED_TRAIN_REGIME_CASES if r[6] + r[7] == 64] and [r for r in STACKED_TRAIN_REGIME_CASES if r[6] + r[7] == 30]
    assert all(r[5] > 32 for r in STACKED_TRAIN_REGIME_CASES if r[0] == "R3")
    assert [r for r in STACKED_TRAIN_REGIME_CASES if r[0] == "R2" and r[5] == 17]
    batches = {p["B"] for fam in ("selffed2", "mixtile", "sttrain") for p in all_cases(fam)}
    assert batches == set(BATCHES) | {33}, batches


# ---------------------------------------------------------------------------------------------------------------------
# shares and the yardstick
# ---------------------------------------------------------------------------------------------------------------------
def _assert_head(tag, pre):
    """The fed-back tanh: at least 0.30 of its arguments beyond +-9 (1 - y^2 cancels in the backward), 0.30 inside +-1."""
    far, near = float((np.abs(pre) > 9).mean()), float((np.abs(pre) < 1).mean())
    print("%-56s head: %.2f beyond +-9, %.2f inside +-1" % (tag, far, near))
    assert far >= 0.30 and near >= 0.30, (tag, far, near)


def _assert_yardstick(p, fwd, bwd):
    print("%-56s e_ref forward %.3f backward %.3f" % (p["id"], max(fwd.values()), max(bwd.values())))
    for k, v in list(fwd.items()) + list(bwd.items()):
        assert O.REGIME_YARDSTICK * v < O.REGIME_YARDSTICK_CAP, (p["id"], k, v)


def _assert_extreme_rows(p, z_first, pre_rows):
    """R3: the first row's head arguments and the second row's layer-1 pre-activations of step 0 pass +-100 and +-200."""
    assert (pre_rows > 200).any() and (pre_rows < -200).any(), p["id"]
    assert (z_first > 100).any() and (z_first < -100).any() and (z_first > 200).any() and (z_first < -200).any(), p["id"]


@pytest.mark.parametrize("c", SELFFED2_REGIME_CASES, ids=selffed2_regime_id)
def test_selffed2_regime_shares_and_yardstick(c):
    p = selffed2_regime_case(c)
    ref = p["ref"]
    for l in (1, 2):
        _assert_shares("%s layer %d" % (p["id"], l), p["regime"], ref["z%d" % l], p["H"])
    _assert_head(p["id"], ref["pre"])
    if p["regime"] == "R3":
        _assert_extreme_rows(p, ref["z1"][0, 9], ref["pre"][:, 3])
    if p["regime"] == "R4":
        c_max = max(float(np.abs(ref["C1"]).max()), float(np.abs(ref["C2"]).max()))
        print("%-56s max |c| %.1f" % (p["id"], c_max))
        assert float(np.abs(ref["C1"]).max()) > 50 and float(np.abs(ref["C2"]).max()) > 50
    assert all(np.isfinite(ref[k]).all() for k in SF2_OUT)
    _assert_yardstick(p, *selffed2_e_ref(p))


@pytest.mark.parametrize("c", MIX_TILE_REGIME_CASES, ids=mix_tile_regime_id)
def test_mix_tile_regime_shares_and_yardstick(c):
    p = mix_tile_regime_case(c)
    f64 = lambda a: np.asarray(a, np.float64)
    tape = O.mix_tile_forward(p["dec0"], p["st"], p["oth"], p["w"], p["mix_Wp"], p["T"], p["act"])
    z1, z2, pre_m = O.mix_decoder_preactivations(tape, f64(p["dec0"]), [f64(s) for s in p["st"]], f64(p["oth"]), {k: f64(v) for k, v in p["w"].items()},
                                                 f64(p["mix_Wp"]))
    _assert_shares(p["id"] + " layer 1", p["regime"], z1, p["H"])
    _assert_shares(p["id"] + " layer 2", p["regime"], z2, p["H"])
    _assert_head(p["id"], pre_m)                                # the mixing tanh is the one that is fed back
    pre_p = np.arctanh(np.clip(tape["P"], -1 + 1e-16, 1 - 1e-16))
    far = float((np.abs(pre_p) > 9).mean())
    print("%-56s Dense head: %.2f beyond +-9" % (p["id"], far))
    assert far >= 0.30                                          # _regime_head's bias at these widths: 1 - p^2 cancels too
    if p["regime"] == "R3":
        _assert_extreme_rows(p, z1[0, 9], pre_m[:, 3])
    if p["regime"] == "R4":
        assert float(np.abs(tape["C1"]).max()) > 50 and float(np.abs(tape["C2"]).max()) > 50
    assert all(np.isfinite(p["ref"][k]).all() for k in MT_OUT)
    _assert_yardstick(p, *mix_tile_e_ref(p))


@pytest.mark.parametrize("c", STACKED_TRAIN_REGIME_CASES, ids=stacked_train_regime_id)
def test_stacked_train_regime_shares_and_yardstick(c):
    p = stacked_train_regime_case(c)
    ref = p["ref"]
    for phase in ("z_enc", "z_dec"):
        for l, z in enumerate(ref[phase]):
            assert z.shape[1] > 0
            _assert_shares("%s %s layer %d" % (p["id"], phase, l), p["regime"], z, p["H"])
    if p["regime"] == "R3":
        z0 = ref["z_enc"][0]
        a, b = p["extreme"][:2]
        assert (z0[a] > 100).any() and (z0[a] < -100).any() and (z0[b] > 200).any() and (z0[b] < -200).any()
    assert all(np.isfinite(ref[k]).all() for k in ST_TAPES)
    _assert_yardstick(p, *stacked_train_e_ref(p))


# ---------------------------------------------------------------------------------------------------------------------
# the references that are wrong on purpose
# ---------------------------------------------------------------------------------------------------------------------
def selffed2_mistake_applies(mistake, p):
    """A pinned forget gate (R4) has a derivative of exactly zero: c_{t-1} reaches nothing through it.  With both layers' gates
    saturated (R2, R3) dz1 is next to nothing almost everywhere, and so is the feedback dz1 . K1^T beside a dloss of order 1: a
    bound taken from the tensor's largest element cannot see it there (the ordinary cases, R1 and R4 do)."""
    return {"ctx of step t + 1 at step t": "ctx" in p["w"], "layer 2 reads h1 of the previous parity": True,
            "feedback gradient dropped": p["T"] >= 2 and p["H"] == 32 and p.get("regime") not in ("R2", "R3"), "c_prev one step late": p.get("regime") != "R4" and p["H"] == 32,
            "dz2 . K2^T left out of dh1": p["H"] == 32}[mistake]


def mix_tile_mistake_applies(mistake, p):
    """As selffed2_mistake_applies; the regimes' mixing stage has a gain of 0.15 (its slope outputs stay on the slope) under a
    tanh a third of which is saturated: the feedback is below what a bound from the largest element sees in every regime."""
    return {"mix_Wp transposed": p["O"] >= 2, "oth_proj of step t + 1 at step t": p["oth_form"] != "bcast",
            "dp without 1 - p^2": p["H"] == 32, "feedback gradient dropped": p["T"] >= 2 and p["H"] == 32 and "regime" not in p,
            "c_prev one step late": p.get("regime") != "R4" and p["H"] == 32}[mistake]


def stacked_train_mistake_applies(mistake, p):
    both = p["T_in"] > 0 and p["T_out"] > 0
    return {"decoder layer l seeded from encoder layer l - 1": both, "partial k-block dropped": p["F_enc"] % 16 != 0 and p["F_enc"] > 16 and p["T_in"] > 0,
            "decoder input rows 0..3": p["F_dec"] >= 5 and p["T_out"] > 0, "dx of the layer above dropped": p["T_out"] > 0,
            "c_prev one step late": p["T_out"] > 0, "decoder dc_0 not handed to the encoder": both}[mistake]


FORWARD_MISTAKES = {"ctx of step t + 1 at step t", "layer 2 reads h1 of the previous parity", "mix_Wp transposed",
                    "oth_proj of step t + 1 at step t", "decoder layer l seeded from encoder layer l - 1", "partial k-block dropped",
                    "decoder input rows 0..3"}


def _miss(p, mistake, e_ref, forward, backward, out_keys, grad_keys):
    """The wrong reference's error in asserted bounds: a forward mistake against the fp64 forward, a backward one against the fp64
    backward on the same (fp32) tapes."""
    regime = "regime" in p
    if mistake in FORWARD_MISTAKES:
        wrong = forward(mistake)
        ok = all(np.isfinite(wrong[k]).all() for k in out_keys)
        return ok, worst(wrong, p["ref"], out_keys, "f32", e_ref(p)[0] if regime else None)
    ref, wrong = backward(None), backward(mistake)
    return all(np.isfinite(v).all() for v in wrong.values()), worst(wrong, ref, grad_keys, GRAD, e_ref(p)[1] if regime else None)


@pytest.mark.parametrize("mistake", O.SELFFED2_MISTAKES)
def test_wrong_selffed2_references_miss_the_bound(mistake):
    n = 0
    for p in all_cases("selffed2"):
        if selffed2_mistake_applies(mistake, p):
            ok, r = _miss(p, mistake, selffed2_e_ref, lambda m: forward64(p["x0"], p["st"], p["w"], p["T"], p["act"], mistake=m)[0],
                          lambda m: selffed2_grads(p, p["tape32"], mistake=m), SF2_OUT, SF2_GRADS)
            assert ok and r >= MARGIN, (p["id"], mistake, r)
            n += 1
    assert n >= 4


@pytest.mark.parametrize("mistake", O.MIX_TILE_MISTAKES)
def test_wrong_mix_tile_references_miss_the_bound(mistake):
    n = 0
    for p in all_cases("mixtile"):
        if mix_tile_mistake_applies(mistake, p):
            fwd = lambda m: mix_tile_outputs(O.mix_tile_forward(p["dec0"], p["st"], p["oth"], p["w"], p["mix_Wp"], p["T"], p["act"], mistake=m), p["T"])
            tape, dloss = mix_tile_bwd_tape(p, p["tape32"])
            ok, r = _miss(p, mistake, mix_tile_e_ref, fwd, lambda m: mix_tile_grads(p, tape, dloss, mistake=m), MT_OUT, MT_GRADS)
            assert ok and r >= MARGIN, (p["id"], mistake, r)
            n += 1
    assert n >= 4


@pytest.mark.parametrize("mistake", O.STACKED_TRAIN_MISTAKES)
def test_wrong_stacked_train_references_miss_the_bound(mistake):
    n = 0
    for p in all_cases("sttrain"):
        if stacked_train_mistake_applies(mistake, p):
            ok, r = _miss(p, mistake, stacked_train_e_ref, lambda m: O.stacked_train_forward(p["w"], p["enc"], p["dec_in"], p["L"], p["act"], mistake=m),
                          lambda m: stacked_train_grads(p, p["tape32"], mistake=m), ST_TAPES, ST_GRADS)
            assert ok and r >= MARGIN, (p["id"], mistake, r)
            n += 1
    assert n >= 4


# ---------------------------------------------------------------------------------------------------------------------
# each backward restatement against torch.autograd, fp64, on ordinary cases away from the kinks
# ---------------------------------------------------------------------------------------------------------------------
def _away_from_kinks(zs, H):
    for z in zs:
        gates = np.concatenate([z[..., :2 * H], z[..., 3 * H:]], -1)
        assert np.abs(np.abs(gates) - 2.5).min() > 1e-6


@pytest.mark.parametrize("act,ctx,bd,keep", [("sigmoid", True, False, STATES), ("hard_sigmoid", False, True, ("c1_0",)), ("hard_sigmoid", True, True, ())])
def test_selffed2_backward_against_autograd(act, ctx, bd, keep):
    B, T, H, n_out = 5, 4, 32, 5
    rng = np.random.default_rng(seed_of("selffed2 autograd " + act + str(ctx)))
    w = _two_layers(rng, H, n_out)
    w["W"] = rng.uniform(-0.5, 0.5, (H, n_out))
    if bd:
        w["bd"] = rng.uniform(-0.2, 0.2, n_out)
    if ctx:
        w["ctx"] = rng.uniform(-0.7, 0.7, (B, T, n_out))
    st = {k: 0.3 * rng.standard_normal((B, H)) if k in keep else None for k in STATES}
    x0, dloss = rng.uniform(-1, 1, (B, n_out)), rng.standard_normal((T, B, n_out))
    ref, margin = forward64(x0, st, w, T, act)
    assert margin > 1e-6
    y, want = autograd64(x0, st, w, dloss, T, act)
    np.testing.assert_allclose(y, ref["y"], rtol=0, atol=1e-13)
    got = backward64(ref, dloss, w, act)
    for k in SF2_GRADS:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-11, atol=1e-13, err_msg=k)


@pytest.mark.parametrize("act", ["sigmoid", "hard_sigmoid"])
def test_mix_tile_backward_against_autograd(act):
    B, T, H, n_out = 5, 4, 32, 5
    rng = np.random.default_rng(seed_of("mix tile autograd " + act))
    w = {k: v.astype(np.float64) for k, v in _two_layers(rng, H, n_out).items()}
    w["dense_W"], w["dense_b"] = rng.uniform(-0.5, 0.5, (H, n_out)), rng.uniform(-0.2, 0.2, n_out)
    Wp, st = 0.5 * rng.standard_normal((n_out, n_out)), [0.4 * rng.standard_normal((B, H)) for _ in range(4)]
    dec0, oth, G = rng.uniform(-1, 1, (B, n_out)), 0.3 * rng.standard_normal((B, T, n_out)), rng.standard_normal((T, B, n_out))
    tape = O.mix_tile_forward(dec0, st, oth, w, Wp, T, act)
    z1, z2, _ = O.mix_decoder_preactivations(tape, dec0, st, oth, w, Wp)
    if act == "hard_sigmoid":
        _away_from_kinks([z1, z2], H)
    leaf = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    t, s0 = {k: leaf(v) for k, v in w.items()}, [leaf(s) for s in st]
    tWp, (h1, c1, h2, c2), x = leaf(Wp), s0, torch.tensor(dec0)
    z1s, z2s, pps, pms, ms = [], [], [], [], []
    for tt in range(T):
        h1, c1 = _step_t(x, h1, c1, t["dec1_K"], t["dec1_R"], t["dec1_b"], act, z1s)
        h2, c2 = _step_t(h1, h2, c2, t["dec2_K"], t["dec2_R"], t["dec2_b"], act, z2s)
        pp = h2 @ t["dense_W"] + t["dense_b"]
        pm = torch.tanh(pp) @ tWp + torch.tensor(oth[:, tt])
        pp.retain_grad(); pm.retain_grad()
        x = torch.tanh(pm)
        pps.append(pp); pms.append(pm); ms.append(x)
    M = torch.stack(ms)
    np.testing.assert_allclose(M.detach().numpy(), tape["M"], rtol=0, atol=1e-13)
    (M * torch.tensor(G)).sum().backward()
    gr = lambda seq: np.stack([a.grad.numpy() for a in seq])
    want = {"DZ1": gr(z1s), "DZ2": gr(z2s), "dpre_m": gr(pms), "dpre_p": gr(pps)}
    want.update({k: s.grad.numpy() for k, s in zip(("dh1_0", "dc1_0", "dh2_0", "dc2_0"), s0)})
    p = dict(st=st, G=G, w=w, mix_Wp=Wp, act=act)
    bt = {k: tape[k] for k in ("M", "P", "res1", "res2")}
    bt["C1s"], bt["C2s"] = np.concatenate([st[1][None], tape["C1"][:-1]]), np.concatenate([st[3][None], tape["C2"][:-1]])
    got = mix_tile_grads(p, bt, G * (1 - tape["M"] ** 2))
    for k in MT_GRADS:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-11, atol=1e-13, err_msg=k)


@pytest.mark.parametrize("L,act,T_in,T_out", [(2, "sigmoid", 3, 2), (3, "hard_sigmoid", 2, 3), (2, "hard_sigmoid", 0, 3)])
def test_stacked_train_backward_against_autograd(L, act, T_in, T_out):
    B, H, F_enc, F_dec = 5, 32, 17, 5
    c = dict(id="sttrain autograd %d %s %d" % (L, act, T_in), L=L, H=H, F_enc=F_enc, F_dec=F_dec)
    w = {k: v.astype(np.float64) for k, v in stacked_weights(c).items()}
    rng = np.random.default_rng(seed_of(c["id"]))
    enc, dec_in, top = rng.uniform(-1, 1, (B, T_in, F_enc)), rng.uniform(-1, 1, (B, T_out, F_dec)), rng.standard_normal((B, T_out, H))
    ref = O.stacked_train_forward(w, enc, dec_in, L, act)
    if act == "hard_sigmoid":
        _away_from_kinks([z for z in ref["z_enc"] + ref["z_dec"] if z.size], H)
    t = {k: torch.tensor(v, dtype=torch.float64) for k, v in w.items()}
    zero = torch.zeros(B, H, dtype=torch.float64)
    enc_leaf = torch.tensor(enc, dtype=torch.float64, requires_grad=True)
    dec_leaf = torch.tensor(dec_in, dtype=torch.float64, requires_grad=True)
    h, cc = [zero] * L, [zero] * L
    zs = {(side, l): [] for side in ("enc", "dec") for l in range(L)}
    tops = []
    for side, seq, T in (("enc", enc_leaf, T_in), ("dec", dec_leaf, T_out)):
        for tt in range(T):
            x = seq[:, tt]
            for l in range(L):
                h[l], cc[l] = _step_t(x, h[l], cc[l], t["%s%d_K" % (side, l)], t["%s%d_R" % (side, l)], t["%s%d_b" % (side, l)], act, zs[side, l])
                x = h[l]
            if side == "dec":
                tops.append(x)
    hs_top = torch.stack(tops, 1)
    np.testing.assert_allclose(hs_top.detach().numpy(), ref["dec_hs"][L - 1], rtol=0, atol=1e-13)
    (hs_top * torch.tensor(top)).sum().backward()
    got = O.stacked_train_backward(ref, top, w, L, act)
    for side, key, T in (("enc", "enc_dz", T_in), ("dec", "dec_dz", T_out)):
        for l in range(L):
            want = np.stack([z.grad.numpy() for z in zs[side, l]], 1) if T else np.zeros((B, 0, 4 * H))
            np.testing.assert_allclose(got[key][l], want, rtol=1e-11, atol=1e-13, err_msg="%s layer %d" % (key, l))


# ---------------------------------------------------------------------------------------------------------------------
# the guarded views of every case
# ---------------------------------------------------------------------------------------------------------------------
def test_guarded_inputs_of_every_case():
    seen, tables = {}, []
    for p in all_cases("selffed2"):
        tables.append((p["id"], selffed2_operands(p), list(SF2_OUT)))
        if p["H"] == 32:
            tables.append((p["id"] + " bwd", {k: dict(p["tape32"], dloss=p["dloss"], **p["w"])[k] for k in SF2_BWD_IN}, list(SF2_GRADS)))
    for p in all_cases("mixtile"):
        tables.append((p["id"], mix_tile_operands(p), list(MT_OUT)))
        if p["H"] == 32:
            tape, dloss = mix_tile_bwd_tape(p, p["tape32"])
            tables.append((p["id"] + " bwd", {k: dict(tape, dloss=dloss, mix_Wp=p["mix_Wp"], **p["w"])[k] for k in MT_BWD_IN}, list(MT_GRADS)))
    for p in all_cases("sttrain"):
        tables.append((p["id"], stacked_train_operands(p), list(ST_TAPES)))
        bwd = dict(stacked_train_operands(p), enc_res=p["tape32"]["enc_res"], dec_res=p["tape32"]["dec_res"], cT=p["tape32"]["cT"], dhs_top=p["dhs_top"])
        tables.append((p["id"] + " bwd", {k: v for k, v in bwd.items() if not (k.endswith("_b") or k in ("enc", "dec_in", "enc0_K", "dec0_K"))},
                       list(ST_GRADS)))
    for cid, operands, outputs in tables:
        off = offsets(cid, list(operands) + outputs)          # as the GPU tests ask for them (which also run every case flipped)
        for name, a in operands.items():
            if a is None:
                continue
            cls = name.translate({ord(d): None for d in "012"}) if cid.startswith("sttrain") else name      # enc0_K, enc1_K: one class
            seen.setdefault((cid.split("-")[0], cid.endswith(" bwd"), cls), set()).add(off[name])
            _check_view("%s %s" % (cid, name), view(a, off[name]), np.asarray(a, np.float32), off[name])
    assert all(v == {0, 1} for v in seen.values()), {k: v for k, v in seen.items() if v != {0, 1}}
    for shape in [(0, 17, 1, 5, 32), (2, 17, 64), (3, 17, 0, 128)]:
        for off in ((0, 1) if np.prod(shape) else (0,)):      # a zero-length output stands on the boundary
            o = OutView(shape, off=off)
            m = margin_floats(shape)
            assert o.lo >= m and o.buf.numel() - o.hi >= m and m >= 1024 and o.untouched()
    assert same_bits(view(np.zeros((4, 0, 6), np.float32), 1).numpy(), np.zeros((4, 0, 6), np.float32))
