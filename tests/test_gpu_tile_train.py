"""The tile kernels that train - fov_selffed2_decoder_fwd / _bwd, fov_mix_decoder_fwd / _bwd at H = 32 / 64 and
fov_stacked_seq2seq_train_fwd / _bwd - through the C ABI on GUARDED VIEWS and at their value edges.
tests/test_tile_train_host.py owns the case tables and the references and shows on the CPU what these checks can see (the regimes'
shares, the yardstick, references that are wrong on purpose).

Every tensor input is a view inside a NaN buffer, every output a view inside a sentinel buffer pre-filled with NaN, with margins of
16 operand rows and 1024 floats at least and with the alignment the case's table gives it (0 or 1 float behind a 16-byte boundary).
A read one row or one k-block past an operand - load_frag of R1 / K2 / R2, the K1 rows at 4 g4 + r >= O, the head's W column at
n >= O, the context row of step t + 1 at the last step, a tape row of step t - 1 at t = 0 - makes a NaN where it is used; a write
past a ragged tile breaks a sentinel; an unwritten element stays NaN.  Every call is made twice into the same views and once more
with every alignment flipped, and must give the same bits.  Each optional output pointer is passed as NULL on its own: the others
keep their bits, the absent one's buffer stays untouched.  An operand without elements is a zero-length view passed by its address.

Bounds.  Forward tensors and tapes against fp64: regime_error(., "f32") <= regime_bound(e_ref), which is 1 outside the regimes.
Gradients: 1e-4 of the tensor's max |ref| + 1e-9 on the worst element (times regime_bound(e_ref) in a regime), against the fp64
backward on the GPU forward's OWN tapes: both sides take the same branch at every kink, no element is masked.  Each check prints
its error in written bounds before it asserts; when the module is through, the worst per entry point and regime is printed."""
import functools

import numpy as np
import pytest
import torch

import test_tile_train_host as TT
from oracle import fov_oracle as O
from test_guarded_views_host import OutView, same_bits
from test_tile_decoders_host import GRAD, addr, offsets, view

pytestmark = pytest.mark.gpu

WORST = {}          # (entry point, regime) -> [checks, worst error in written bounds, worst e_ref]


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    """After the module's last test: the table that DESIGN.md quotes.  The bounds themselves are asserted check by check."""
    yield
    for (entry, regime), (n, err, e_ref) in sorted(WORST.items()):
        print("\n%-24s %-10s checks %4d   worst gpu error %.3f written bounds   worst e_ref %.3f" % (entry, regime, n, err, e_ref), end="")
    print()


def gv(a, off=0):
    return None if a is None else view(np.array(a, dtype=np.float32), off, "cuda")


def ov(shape, off=0):
    """An overwritten output (pre-filled with NaN); a zero-length one stands on the 16-byte boundary."""
    return OutView(shape, None, off if int(np.prod(shape)) else 0, torch.float32, "cuda")


def oaddr(o):
    return None if o is None else o.buf.data_ptr() + 4 * o.lo


def held(tag, family, got, ref, kind="f32", e_ref=0.0):
    """The error in written bounds <= regime_bound(e_ref) (1 outside the regimes); prints the figures first."""
    assert np.isfinite(got).all(), tag + ": non-finite values"
    err, bound = O.regime_error(got, ref, kind), O.regime_bound(e_ref)
    print("%-72s e_ref %.3g  bound %.3g  gpu %.3g  (written bounds, %s; max |ref| %.3g)"
          % (tag, e_ref, bound, err, kind, float(np.abs(ref).max()) if np.size(ref) else 0.0))
    w = WORST.setdefault(family, [0, 0.0, 0.0])
    w[0], w[1], w[2] = w[0] + 1, max(w[1], err), max(w[2], e_ref)
    assert O.REGIME_YARDSTICK * e_ref <= O.REGIME_YARDSTICK_CAP, (tag, e_ref)
    assert err <= bound, "%s: %.3g written bounds, allowed %.3g" % (tag, err, bound)


def lib():
    from longterm360fov_amd import _lib
    return _lib.lib()


def launch(fn, *args):
    from longterm360fov_amd import ops
    ops.check(fn(*args, ops._stream()))
    torch.cuda.synchronize()


def run(outs, call, absent=(), repeat=True):
    """The call into the views `outs` (twice with repeat: the same bits) -> {name: numpy} of the views that were handed over; those
    in `absent` (made, but passed as NULL) must stay untouched."""
    call()
    got = {k: o.result() for k, o in outs.items() if k not in absent}
    if repeat:
        for o in outs.values():
            o.reset()
        call()
        for k in got:
            assert same_bits(got[k], outs[k].result()), k + ": two calls differ"
    assert all(outs[k].untouched() for k in absent), "an output whose pointer is NULL was written"
    return got


def family(p, entry):
    return (entry, p.get("regime", "ordinary"))


def e_refs(p, fn):
    """(forward, backward) e_ref of a regime case; zeros (a bound of 1) for an ordinary one."""
    if "regime" in p:
        return fn(p)
    return dict.fromkeys(TT.SF2_OUT + TT.MT_OUT + TT.ST_TAPES, 0.0), dict.fromkeys(TT.SF2_GRADS + TT.MT_GRADS + TT.ST_GRADS, 0.0)


def rows_of(a, rows, axis=0):
    if a is None or rows is None:
        return a
    return np.ascontiguousarray(np.take(a, np.arange(*rows.indices(a.shape[axis])), axis=axis))


# ---------------------------------------------------------------------------------------------------------------------
# self-fed two-layer decoder
# ---------------------------------------------------------------------------------------------------------------------
def sf2_forward(p, T=None, absent=(), flip=0, rows=None, repeat=True):
    """fov_selffed2_decoder_fwd on guarded views -> {name: numpy}.  rows: a slice of the batch run as a batch of its own."""
    T = p["T"] if T is None else T
    H, n_out = p["H"], p["O"]
    src = TT.selffed2_operands(p)
    for k in ("x0", "ctx") + TT.STATES:
        src[k] = rows_of(src[k], rows)
    if src["ctx"] is not None:
        src["ctx"] = np.ascontiguousarray(src["ctx"][:, :T])
    B = src["x0"].shape[0]
    off = {k: v ^ flip for k, v in offsets(p["id"], TT.SF2_IN + TT.SF2_OUT).items()}
    ins = {k: gv(src[k], off[k]) for k in TT.SF2_IN}
    shapes = {"H1": (T + 1, B, H), "C1": (T + 1, B, H), "H2": (T + 1, B, H), "C2": (T + 1, B, H), "XY": (T + 1, B, n_out),
              "RES1": (T, B, 1, 5, H), "RES2": (T, B, 1, 5, H), "y": (B, T, n_out), "hT": (2, B, H), "cT": (2, B, H)}
    outs = {k: ov(shapes[k], off[k]) for k in TT.SF2_OUT}
    args = [addr(ins[k]) for k in TT.SF2_IN] + [None if k in absent else oaddr(outs[k]) for k in TT.SF2_OUT] + \
        [B, T, n_out, H, O.act_code(p["act"])]
    call = lambda: launch(lib().fov_selffed2_decoder_fwd, *args)
    if B == 0 or T == 0:        # nothing is launched and nothing written
        call()
        assert all(o.untouched() for o in outs.values()), "the forward wrote something without a step or a sequence"
        return None
    return run(outs, call, absent, repeat)


def sf2_backward(p, tape, T=None, absent=(), flip=0, rows=None, repeat=True):
    """fov_selffed2_decoder_bwd with every tape a guarded view -> {name: numpy}."""
    T = p["T"] if T is None else T
    H, n_out = p["H"], p["O"]
    src = dict(tape, dloss=rows_of(p["dloss"], rows, 1)[:T], **{k: p["w"][k] for k in TT.SF2_BWD_IN[6:]})
    B = src["dloss"].shape[1]
    off = {k: v ^ flip for k, v in offsets(p["id"] + " bwd", TT.SF2_BWD_IN + TT.SF2_GRADS).items()}
    ins = {k: gv(src[k], off[k]) for k in TT.SF2_BWD_IN}
    shapes = {"DPRE": (T, B, n_out), "DZ1": (T, B, 4 * H), "DZ2": (T, B, 4 * H), "dx0": (B, n_out)}
    outs = {k: ov(shapes.get(k, (B, H)), off[k]) for k in TT.SF2_GRADS}
    args = [addr(ins[k]) for k in TT.SF2_BWD_IN] + [None if k in absent else oaddr(outs[k]) for k in TT.SF2_GRADS] + \
        [B, T, n_out, H, O.act_code(p["act"])]
    call = lambda: launch(lib().fov_selffed2_decoder_bwd, *args)
    if B == 0:
        call()
        assert all(o.untouched() for o in outs.values())
        return None
    if T == 0:                  # no step: exact zeros in the five gradients of the inputs, nothing else
        call()
        assert all(outs[k].untouched() for k in ("DPRE", "DZ1", "DZ2") + tuple(absent))
        return {k: outs[k].result() for k in TT.SF2_GRADS[3:] if k not in absent}
    return run(outs, call, absent, repeat)


def sf2_tape(got):
    return {k: got[k] for k in ("C1", "C2", "XY", "RES1", "RES2")}


@functools.lru_cache(maxsize=None)
def _sf2_gpu_forward(kind, key):
    p = TT.selffed2_case(key) if kind == "ordinary" else TT.selffed2_regime_case(key)
    got = sf2_forward(p)
    for a in got.values():
        a.setflags(write=False)
    return got


def sf2_check_forward(p, got, e_ref):
    T = p["T"]
    for k in TT.SF2_OUT:
        held("%s %s" % (p["id"], k), family(p, "selffed2 forward"), got[k], p["ref"][k], "f32", e_ref[k])
    assert same_bits(got["y"], np.ascontiguousarray(got["XY"][1:].swapaxes(0, 1)))          # y is XY[1:], batch-major
    assert same_bits(got["hT"], np.stack([got["H1"][T], got["H2"][T]])) and same_bits(got["cT"], np.stack([got["C1"][T], got["C2"][T]]))
    assert same_bits(got["XY"][0], p["x0"])
    for k, s_ in zip(("H1", "C1", "H2", "C2"), TT.STATES):                                   # row 0 is the initial state, bit for bit
        assert same_bits(got[k][0], np.zeros_like(got[k][0]) if p["st"][s_] is None else p["st"][s_]), k
    for k, res in (("C1", "RES1"), ("C2", "RES2")):                                          # the reserve's c is the tape's c
        assert same_bits(got[res][:, :, 0, 4], got[k][1:]), k


def sf2_check_backward(p, grads, tape, e_ref):
    ref = TT.selffed2_grads(p, tape)
    for k in TT.SF2_GRADS:
        held("%s %s" % (p["id"], k), family(p, "selffed2 backward"), grads[k], ref[k], GRAD, e_ref[k])


SF2_IDS = [c["id"] for c in TT.selffed2_cases()]


@pytest.mark.parametrize("cid", SF2_IDS)
def test_selffed2_on_guarded_views(cid):
    """Every table case: the ten outputs against fp64; each output pointer NULL on its own leaves the others the same bits and its
    buffer untouched; the other alignment of every operand gives the same bits.  At H = 32 the backward on these tapes, the same
    way: against fp64 on the same tapes, each of its five optional outputs NULL on its own, and all five."""
    p = TT.selffed2_case(cid)
    got = _sf2_gpu_forward("ordinary", cid)
    sf2_check_forward(p, got, e_refs(p, None)[0])
    for leave in TT.SF2_OUT:
        part = sf2_forward(p, absent=(leave,), repeat=False)
        for k in part:
            assert same_bits(part[k], got[k]), (cid, "without " + leave, k)
    part = sf2_forward(p, absent=TT.SF2_OUT[:7] + ("hT", "cT"), repeat=False)       # predict's call: y alone
    assert same_bits(part["y"], got["y"])
    other = sf2_forward(p, flip=1, repeat=False)
    for k in TT.SF2_OUT:
        assert same_bits(other[k], got[k]), (cid, "alignment", k)
    if p["H"] != 32:
        return
    tape = sf2_tape(got)
    grads = sf2_backward(p, tape)
    sf2_check_backward(p, grads, tape, e_refs(p, None)[1])
    for absent in [(k,) for k in TT.SF2_GRADS[3:]] + [TT.SF2_GRADS[3:]]:
        part = sf2_backward(p, tape, absent=absent, repeat=False)
        for k in part:
            assert same_bits(part[k], grads[k]), (cid, "without", absent, k)
    other = sf2_backward(p, tape, flip=1, repeat=False)
    for k in TT.SF2_GRADS:
        assert same_bits(other[k], grads[k]), (cid, "alignment", k)


@pytest.mark.parametrize("c", TT.SELFFED2_REGIME_CASES, ids=TT.selffed2_regime_id)
def test_selffed2_in_value_regimes(c):
    p = TT.selffed2_regime_case(c)
    regime, H = p["regime"], p["H"]
    e_fwd, e_bwd = e_refs(p, TT.selffed2_e_ref)
    got = _sf2_gpu_forward("regime", c)                  # made twice: the long runs repeat bit for bit
    sf2_check_forward(p, got, e_fwd)
    other = sf2_forward(p, flip=1, repeat=False)
    assert all(same_bits(other[k], got[k]) for k in TT.SF2_OUT), "alignment"
    assert np.abs(got["y"]).max() <= 1.0 and np.abs(got["H2"]).max() <= 1.0
    pre = np.swapaxes(p["ref"]["pre"], 0, 1)
    assert (got["y"][pre > 10.5] == 1.0).all() and (got["y"][pre < -10.5] == -1.0).all()      # 2 / (1 + e^21) is below half an ulp of 1
    if regime == "R4":
        assert float(np.abs(got["C1"]).max()) > 50 and float(np.abs(got["C2"]).max()) > 50
    if regime == "R3":          # the extreme rows' tile-mates do not see them
        calm = sf2_forward(dict(p, x0=p["x0_calm"], w=dict(p["w"], ctx=p["ctx_calm"])), repeat=False)
        mates = np.setdiff1d(np.arange(p["B"]), p["extreme"])
        for k in TT.SF2_TAPES:
            assert same_bits(calm[k][:, mates], got[k][:, mates]), k
        assert not same_bits(calm["y"][p["extreme"]], got["y"][p["extreme"]])
    if H != 32:
        return
    tape = sf2_tape(got)
    grads = sf2_backward(p, tape)
    sf2_check_backward(p, grads, tape, e_bwd)
    other = sf2_backward(p, tape, flip=1, repeat=False)
    assert all(same_bits(other[k], grads[k]) for k in TT.SF2_GRADS), "alignment"
    sat = np.abs(got["XY"][1:]) == 1.0                   # a head output of exactly +-1: 1 - y^2 is exactly zero
    assert sat.mean() >= 0.25 and (grads["DPRE"][sat] == 0.0).all() and (grads["DPRE"][~sat] != 0.0).any()
    if p["act"] == "hard_sigmoid":
        for res, dz in (("RES1", "DZ1"), ("RES2", "DZ2")):
            for q in (0, 1, 3):
                flat = (got[res][:, :, 0, q] == 0.0) | (got[res][:, :, 0, q] == 1.0)
                assert flat.any() and (grads[dz][:, :, q * H:(q + 1) * H][flat] == 0.0).all(), (p["id"], "a clamped gate with a gradient", q)
            assert float(np.abs(grads[dz]).max()) > 0


@pytest.mark.parametrize("cid", [SF2_IDS[2], SF2_IDS[5]])
def test_selffed2_without_a_step_or_a_sequence(cid):
    """T = 0: the forward writes nothing; the backward leaves exact zeros in dx0 and the four state gradients and touches nothing
    else.  B = 0: both calls return FOV_OK and touch nothing."""
    p = TT.selffed2_case(cid)
    B, H, n_out = p["B"], p["H"], p["O"]
    for flip in (0, 1):
        assert sf2_forward(p, T=0, flip=flip) is None
        assert sf2_forward(p, rows=slice(0, 0), flip=flip) is None
        empty = {"C1": np.zeros((1, B, H)), "C2": np.zeros((1, B, H)), "XY": np.zeros((1, B, n_out)), "RES1": np.zeros((0, B, 1, 5, H)),
                 "RES2": np.zeros((0, B, 1, 5, H))}
        for absent in ((), ("dh1_0", "dc2_0")):
            got = sf2_backward(p, empty, T=0, absent=absent, flip=flip)
            assert all((v == 0).all() and not np.signbit(v).any() for v in got.values()), cid
        none = {k: np.zeros((v.shape[0] + 2, 0) + v.shape[2:]) for k, v in empty.items()}
        assert sf2_backward(p, none, T=2, rows=slice(0, 0), flip=flip) is None


# ---------------------------------------------------------------------------------------------------------------------
# others-mixing decoder at a tile width
# ---------------------------------------------------------------------------------------------------------------------
def mt_forward(p, absent=(), flip=0, rows=None, repeat=True, T=None):
    """fov_mix_decoder_fwd on guarded views with the others' projection in the case's layout -> {name: numpy}."""
    T = p["T"] if T is None else T
    H, n_out = p["H"], p["O"]
    src = TT.mix_tile_operands(p)
    for k in ("dec0", "h1", "c1", "h2", "c2", "oth"):
        src[k] = rows_of(src[k], rows)
    src["oth"] = src["oth"][:, :T]
    B = src["dec0"].shape[0]
    sb, st = T * n_out, n_out
    if p["oth_form"] == "padded" and B and T:           # a step stride of O + 3: the three floats behind every row are NaN
        src["oth"] = np.concatenate([src["oth"], np.full((B, T, 3), np.nan, np.float32)], axis=2)
        sb, st = T * (n_out + 3), n_out + 3
    elif p["oth_form"] == "bcast" and B and T:          # one row for every sequence and step: both strides 0
        src["oth"], sb, st = src["oth"][0, 0], 0, 0
    off = {k: v ^ flip for k, v in offsets(p["id"], TT.MT_IN + TT.MT_OUT).items()}
    ins = {k: gv(src[k], off[k]) for k in TT.MT_IN}
    shapes = {"M": (T, B, n_out), "P": (T, B, n_out), "res1": (T, B, 5, H), "res2": (T, B, 5, H)}
    shapes.update({k: (B, H) for k in TT.MT_FINAL})
    outs = {k: ov(shapes.get(k, (T, B, H)), off[k]) for k in TT.MT_OUT}
    args = [addr(ins[k]) for k in TT.MT_IN[:6]] + [sb, st] + [addr(ins[k]) for k in TT.MT_IN[6:]] + \
        [None if k in absent else oaddr(outs[k]) for k in TT.MT_OUT] + [B, T, H, n_out, O.act_code(p["act"]), None, 0]
    call = lambda: launch(lib().fov_mix_decoder_fwd, *args)
    if B == 0 or T == 0:
        call()
        assert all(o.untouched() for o in outs.values()), "the forward wrote something without a step or a sequence"
        return None
    return run(outs, call, absent, repeat)


def mt_backward(p, tape, dloss, flip=0, repeat=True):
    """fov_mix_decoder_bwd with every tape a guarded view -> {name: numpy}."""
    H, n_out = p["H"], p["O"]
    src = dict(tape, dloss=dloss, mix_Wp=p["mix_Wp"], **{k: p["w"][k] for k in TT.MT_BWD_IN[7:12]})
    T, B = dloss.shape[:2]
    off = {k: v ^ flip for k, v in offsets(p["id"] + " bwd", TT.MT_BWD_IN + TT.MT_GRADS).items()}
    ins = {k: gv(src[k], off[k]) for k in TT.MT_BWD_IN}
    shapes = {"DZ1": (T, B, 4 * H), "DZ2": (T, B, 4 * H), "dpre_m": (T, B, n_out), "dpre_p": (T, B, n_out)}
    outs = {k: ov(shapes.get(k, (B, H)), off[k]) for k in TT.MT_GRADS}
    args = [addr(ins[k]) for k in TT.MT_BWD_IN] + [oaddr(outs[k]) for k in TT.MT_GRADS] + [B, T, H, n_out, O.act_code(p["act"]), None, 0]
    call = lambda: launch(lib().fov_mix_decoder_bwd, *args)
    if B == 0 or T == 0:
        call()
        assert all(o.untouched() for o in outs.values())
        return None
    return run(outs, call, (), repeat)


@functools.lru_cache(maxsize=None)
def _mt_gpu_forward(kind, key):
    p = TT.mix_tile_case(key) if kind == "ordinary" else TT.mix_tile_regime_case(key)
    got = mt_forward(p)
    for a in got.values():
        a.setflags(write=False)
    return got


def mt_check_forward(p, got, e_ref):
    T = p["T"]
    for k in TT.MT_OUT:
        held("%s %s" % (p["id"], k), family(p, "mix tile forward"), got[k], p["ref"][k], "f32", e_ref[k])
    for k in ("h1", "c1", "h2", "c2"):                   # the final states are the last tape rows
        assert same_bits(got[k + "T"], got[k.upper()][T - 1]), k
    for k, res in (("C1", "res1"), ("C2", "res2")):
        assert same_bits(got[res][:, :, 4], got[k]), k


def mt_check_backward(p, grads, tape, dloss, e_ref, entry="mix tile backward"):
    ref = TT.mix_tile_grads(p, tape, dloss)
    for k in TT.MT_GRADS:
        held("%s %s" % (p["id"], k), family(p, entry), grads[k], ref[k], GRAD, e_ref[k])


def mt_walk(p):
    """The step-wise walk of the trainer on the per-step entry points -> the forward's outputs (numpy), without the tile kernel."""
    from longterm360fov_amd import ops
    H, n_out, B, T, act = p["H"], p["O"], p["B"], p["T"], p["act"]
    dev = lambda a: torch.from_numpy(np.array(a, dtype=np.float32, order="C")).cuda()
    dw = {k: dev(v) for k, v in p["w"].items()}
    e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    H1, C1, H2, C2 = e(T + 1, B, H), e(T + 1, B, H), e(T + 1, B, H), e(T + 1, B, H)
    for buf, s in zip((H1, C1, H2, C2), p["st"]):
        buf[0].copy_(dev(s))
    XM, P, R1, R2 = e(T + 1, B, n_out), e(T, B, n_out), e(T, B, 1, 5, H), e(T, B, 1, 5, H)
    XM[0].copy_(dev(p["dec0"]))
    oth, Wp = dev(p["oth"]), dev(p["mix_Wp"])
    ws = ops.Workspace()
    for t in range(T):
        ops.lstm_seq_train(XM[t].view(B, 1, n_out), dw["dec1_K"], dw["dec1_R"], dw["dec1_b"], H1[t], C1[t], act=act, workspace=ws,
                           out=(H1[t + 1].view(B, 1, H), None, C1[t + 1], R1[t]))
        zx = ops.matmul(H1[t + 1], dw["dec2_K"]).reshape(B, 1, 4 * H)
        ops.lstm_seq_zx(zx, dw["dec2_R"], dw["dec2_b"], H2[t], C2[t], act=act, workspace=ws, reserve=R2[t],
                        out=(H2[t + 1].view(B, 1, H), None, C2[t + 1]))
        ops.mix_head_fwd(H2[t + 1], dw["dense_W"], dw["dense_b"], Wp, oth[:, t], P[t], XM[t + 1])
    ws.check()
    n = lambda a: a.cpu().numpy()
    return {"M": n(XM[1:]), "P": n(P), "H1": n(H1[1:]), "C1": n(C1[1:]), "H2": n(H2[1:]), "C2": n(C2[1:]), "res1": n(R1.view(T, B, 5, H)),
            "res2": n(R2.view(T, B, 5, H))}


MT_IDS = [c["id"] for c in TT.mix_tile_cases()]


@pytest.mark.parametrize("cid", MT_IDS)
def test_mix_tile_on_guarded_views(cid):
    """Every table case: M, the final states and the seven tapes against fp64; without the tapes (all or none), and with each final
    state NULL on its own, the rest keeps its bits; the other alignment gives the same bits.  At H = 32 the backward on the kernel's
    own tapes and on the step-wise walk's tapes."""
    p = TT.mix_tile_case(cid)
    got = _mt_gpu_forward("ordinary", cid)
    mt_check_forward(p, got, e_refs(p, None)[0])
    for absent in [TT.MT_TRAIN, TT.MT_TRAIN + TT.MT_FINAL] + [(k,) for k in TT.MT_FINAL]:
        part = mt_forward(p, absent=absent, repeat=False)
        for k in part:
            assert same_bits(part[k], got[k]), (cid, "without", absent, k)
    other = mt_forward(p, flip=1, repeat=False)
    for k in TT.MT_OUT:
        assert same_bits(other[k], got[k]), (cid, "alignment", k)
    if p["H"] != 32:
        return
    tape, dloss = TT.mix_tile_bwd_tape(p, got)
    grads = mt_backward(p, tape, dloss)
    mt_check_backward(p, grads, tape, dloss, e_refs(p, None)[1])
    other = mt_backward(p, tape, dloss, flip=1, repeat=False)
    for k in TT.MT_GRADS:
        assert same_bits(other[k], grads[k]), (cid, "alignment", k)
    tape, dloss = TT.mix_tile_bwd_tape(p, mt_walk(p))
    mt_check_backward(p, mt_backward(p, tape, dloss, repeat=False), tape, dloss, e_refs(p, None)[1], "mix tile backward, walk")


@pytest.mark.parametrize("c", TT.MIX_TILE_REGIME_CASES, ids=TT.mix_tile_regime_id)
def test_mix_tile_in_value_regimes(c):
    p = TT.mix_tile_regime_case(c)
    regime, H = p["regime"], p["H"]
    e_fwd, e_bwd = e_refs(p, TT.mix_tile_e_ref)
    got = _mt_gpu_forward("regime", c)
    mt_check_forward(p, got, e_fwd)
    other = mt_forward(p, flip=1, repeat=False)
    assert all(same_bits(other[k], got[k]) for k in TT.MT_OUT), "alignment"
    assert np.abs(got["M"]).max() <= 1.0 and np.abs(got["P"]).max() <= 1.0 and np.abs(got["H2"]).max() <= 1.0
    if regime == "R4":
        assert float(np.abs(got["C1"]).max()) > 50 and float(np.abs(got["C2"]).max()) > 50
    if regime == "R3":
        calm = mt_forward(dict(p, dec0=p["dec0_calm"], oth=p["oth_calm"]), repeat=False)
        mates = np.setdiff1d(np.arange(p["B"]), p["extreme"])
        for k in ("M",) + TT.MT_TRAIN:
            assert same_bits(calm[k][:, mates], got[k][:, mates]), k
        assert not same_bits(calm["M"][:, p["extreme"]], got["M"][:, p["extreme"]])
    if H != 32:
        return
    tape, dloss = TT.mix_tile_bwd_tape(p, got)
    grads = mt_backward(p, tape, dloss)
    mt_check_backward(p, grads, tape, dloss, e_bwd)
    other = mt_backward(p, tape, dloss, flip=1, repeat=False)
    assert all(same_bits(other[k], grads[k]) for k in TT.MT_GRADS), "alignment"
    sat = np.abs(got["P"]) == 1.0                        # a Dense output of exactly +-1: 1 - p^2 is exactly zero
    assert sat.mean() >= 0.25 and (grads["dpre_p"][sat] == 0.0).all() and (grads["dpre_p"][~sat] != 0.0).any()


def test_mix_tile_without_a_step_or_a_sequence():
    p = TT.mix_tile_case(MT_IDS[2])
    for flip in (0, 1):
        assert mt_forward(p, T=0, flip=flip) is None and mt_forward(p, rows=slice(0, 0), flip=flip) is None
        tape, dloss = TT.mix_tile_bwd_tape(p, p["tape32"])
        assert mt_backward(p, {k: v[:0] if k not in ("C1s", "C2s") else v[:1] for k, v in tape.items()}, dloss[:0], flip=flip) is None
        assert mt_backward(p, {k: v[:, :0] for k, v in tape.items()}, dloss[:, :0], flip=flip) is None


# ---------------------------------------------------------------------------------------------------------------------
# stacked training graph
# ---------------------------------------------------------------------------------------------------------------------
ST_OUT = ("enc_hs", "enc_res", "dec_hs", "dec_res", "dec_top", "hT", "cT")


def _ptr3(ins, side, part, L, first=0):
    from longterm360fov_amd import ops
    return ops._PTR3(*([addr(ins["%s%d_%s" % (side, l, part)]) if l >= first else None for l in range(L)] + [None] * (3 - L)))


def st_forward(p, absent=(), flip=0, rows=None, repeat=True):
    """fov_stacked_seq2seq_train_fwd on guarded views -> {name: numpy}."""
    L, H = p["L"], p["H"]
    src = TT.stacked_train_operands(p)
    src["enc"], src["dec_in"] = rows_of(src["enc"], rows), rows_of(src["dec_in"], rows)
    B, T_in, F_enc = src["enc"].shape
    T_out, F_dec = src["dec_in"].shape[1:]
    off = {k: v ^ flip for k, v in offsets(p["id"], list(src) + list(ST_OUT)).items()}
    ins = {k: gv(a, off[k]) for k, a in src.items()}
    shapes = {"enc_hs": (L, B, T_in, H), "enc_res": (L, B, T_in, 5, H), "dec_hs": (L, B, T_out, H), "dec_res": (L, B, T_out, 5, H),
              "dec_top": (B, T_out, H), "hT": (L, B, H), "cT": (L, B, H)}
    outs = {k: ov(shapes[k], off[k]) for k in ST_OUT}
    arrays = [_ptr3(ins, side, part, L) for side in ("enc", "dec") for part in "KRb"]
    args = [addr(ins["enc"]), addr(ins["dec_in"])] + arrays + [None if k in absent else oaddr(outs[k]) for k in ST_OUT] + \
        [B, T_in, T_out, F_enc, F_dec, H, L, O.act_code(p["act"])]
    call = lambda: launch(lib().fov_stacked_seq2seq_train_fwd, *args)
    if B == 0:
        call()
        assert all(o.untouched() for o in outs.values())
        return None
    return run(outs, call, absent, repeat)


def st_backward(p, tape, flip=0, rows=None, repeat=True):
    """fov_stacked_seq2seq_train_bwd with every tape a guarded view and the dx scratch between sentinels -> {name: numpy}."""
    L, H = p["L"], p["H"]
    src = {k: tape[k] for k in ("enc_res", "dec_res", "cT")}
    src["dhs_top"] = rows_of(p["dhs_top"], rows)
    src.update({k: v for k, v in p["w"].items() if k[-1] in "RK" and k[:3] in ("enc", "dec")})
    _, B, T_in = tape["enc_res"].shape[:3]
    T_out = tape["dec_res"].shape[2]
    off = {k: v ^ flip for k, v in offsets(p["id"] + " bwd", list(src) + list(TT.ST_GRADS)).items()}
    ins = {k: gv(a, off[k]) for k, a in src.items()}
    outs = {"enc_dz": ov((L, B, T_in, 4 * H), off["enc_dz"]), "dec_dz": ov((L, B, T_out, 4 * H), off["dec_dz"])}
    nbytes = int(lib().fov_stacked_seq2seq_train_bwd_scratch_bytes(B, T_in, T_out, H))
    scratch = ov((max(nbytes // 4, 1),))
    arrays = [_ptr3(ins, "enc", "R", L), _ptr3(ins, "enc", "K", L, 1), _ptr3(ins, "dec", "R", L), _ptr3(ins, "dec", "K", L, 1)]
    args = [addr(ins[k]) for k in ("enc_res", "dec_res", "cT", "dhs_top")] + arrays + [oaddr(outs["enc_dz"]), oaddr(outs["dec_dz"])] + \
        [B, T_in, T_out, H, L, O.act_code(p["act"]), oaddr(scratch), nbytes]
    call = lambda: launch(lib().fov_stacked_seq2seq_train_bwd, *args)
    if B == 0 or T_in + T_out == 0:
        call()
        assert all(o.untouched() for o in outs.values())
        return None
    got = run(outs, call, (), repeat)
    scratch._sentinels()          # the dx hand-off stays inside its bytes
    return got


@functools.lru_cache(maxsize=None)
def _st_gpu_forward(kind, key):
    p = TT.stacked_train_case(key) if kind == "ordinary" else TT.stacked_train_regime_case(key)
    got = st_forward(p)
    for a in got.values():
        a.setflags(write=False)
    return got


def st_check_forward(p, got, e_ref):
    L = p["L"]
    for k in TT.ST_TAPES:
        held("%s %s" % (p["id"], k), family(p, "stacked train forward"), got[k], p["ref"][k], "f32", e_ref[k])
    assert same_bits(got["dec_top"], got["dec_hs"][L - 1])
    if p["T_in"] == 0:
        assert not got["hT"].any() and not got["cT"].any()
    else:
        assert same_bits(got["hT"], got["enc_hs"][:, :, -1]) and same_bits(got["cT"], got["enc_res"][:, :, -1, 4])


def st_check_backward(p, grads, tape, e_ref):
    ref = TT.stacked_train_grads(p, tape)
    for k in TT.ST_GRADS:
        held("%s %s" % (p["id"], k), family(p, "stacked train backward"), grads[k], ref[k], GRAD, e_ref[k])


@pytest.mark.parametrize("cid", [c["id"] for c in TT.stacked_train_cases()])
def test_stacked_train_on_guarded_views(cid):
    """Every table case: the six tapes and dec_top against fp64; each of the seven output pointers NULL on its own, and all but
    dec_top (the inference forward), leave the rest the same bits; the other alignment gives the same bits; the backward on these
    tapes against fp64 on the same tapes.  An empty phase is a zero-length view passed by its address."""
    p = TT.stacked_train_case(cid)
    got = _st_gpu_forward("ordinary", cid)
    st_check_forward(p, got, e_refs(p, None)[0])
    for absent in [(k,) for k in ST_OUT] + [tuple(k for k in ST_OUT if k != "dec_top")]:
        part = st_forward(p, absent=absent, repeat=False)
        for k in part:
            assert same_bits(part[k], got[k]), (cid, "without", absent, k)
    other = st_forward(p, flip=1, repeat=False)
    for k in ST_OUT:
        assert same_bits(other[k], got[k]), (cid, "alignment", k)
    grads = st_backward(p, got)
    st_check_backward(p, grads, got, e_refs(p, None)[1])
    other = st_backward(p, got, flip=1, repeat=False)
    for k in TT.ST_GRADS:
        assert same_bits(other[k], grads[k]), (cid, "alignment", k)


@pytest.mark.parametrize("c", TT.STACKED_TRAIN_REGIME_CASES, ids=TT.stacked_train_regime_id)
def test_stacked_train_in_value_regimes(c):
    p = TT.stacked_train_regime_case(c)
    e_fwd, e_bwd = e_refs(p, TT.stacked_train_e_ref)
    got = _st_gpu_forward("regime", c)                   # made twice: the long runs repeat bit for bit
    st_check_forward(p, got, e_fwd)
    other = st_forward(p, flip=1, repeat=False)
    assert all(same_bits(other[k], got[k]) for k in ST_OUT), "alignment"
    assert np.abs(got["dec_hs"]).max() <= 1.0 and np.abs(got["enc_hs"]).max() <= 1.0
    if p["regime"] == "R3":      # the extreme rows' tile-mates do not see them
        calm = st_forward(dict(p, enc=p["enc_calm"]), repeat=False)
        mates = np.setdiff1d(np.arange(p["B"]), p["extreme"])
        for k in ST_OUT:
            axis = 0 if k == "dec_top" else 1
            assert same_bits(np.take(calm[k], mates, axis), np.take(got[k], mates, axis)), k
        assert not same_bits(calm["hT"][:, p["extreme"]], got["hT"][:, p["extreme"]])
    grads = st_backward(p, got)
    st_check_backward(p, grads, got, e_bwd)
    other = st_backward(p, got, flip=1, repeat=False)
    assert all(same_bits(other[k], grads[k]) for k in TT.ST_GRADS), "alignment"
    if p["act"] == "hard_sigmoid":
        H = p["H"]
        for res, dz in (("enc_res", "enc_dz"), ("dec_res", "dec_dz")):
            for q in (0, 1, 3):
                flat = (got[res][:, :, :, q] == 0.0) | (got[res][:, :, :, q] == 1.0)
                assert flat.any() and (grads[dz][..., q * H:(q + 1) * H][flat] == 0.0).all(), (p["id"], "a clamped gate with a gradient", q)


def test_stacked_train_without_a_sequence():
    p = TT.stacked_train_case(TT.stacked_train_cases()[1]["id"])
    for flip in (0, 1):
        assert st_forward(p, rows=slice(0, 0), flip=flip) is None
        tape = {k: p["tape32"][k][:, :0] for k in ("enc_res", "dec_res", "cT")}
        assert st_backward(p, tape, rows=slice(0, 0), flip=flip) is None


# ---------------------------------------------------------------------------------------------------------------------
# a sequence does not depend on its tile-mates: row 16 of B = 17 (alone in the ragged second tile) and the same row as a batch of one
# ---------------------------------------------------------------------------------------------------------------------
def _r2_b17(table, batch_at):
    return [c for c in table if c[0] == "R2" and c[batch_at] == 17]


@pytest.mark.parametrize("c", _r2_b17(TT.SELFFED2_REGIME_CASES, 3), ids=TT.selffed2_regime_id)
def test_selffed2_row_alone_in_R2(c):
    p = TT.selffed2_regime_case(c)
    got, one = _sf2_gpu_forward("regime", c), sf2_forward(p, rows=slice(16, 17), repeat=False)
    for k in TT.SF2_OUT:
        assert same_bits(one[k], got[k][16:17] if k == "y" else got[k][:, 16:17]), k
    if p["H"] == 32:
        full = sf2_backward(p, sf2_tape(got), repeat=False)
        alone = sf2_backward(p, sf2_tape(one), rows=slice(16, 17), repeat=False)
        for k in TT.SF2_GRADS:
            assert same_bits(alone[k], full[k][:, 16:17] if full[k].ndim == 3 else full[k][16:17]), k


@pytest.mark.parametrize("c", _r2_b17(TT.MIX_TILE_REGIME_CASES, 3), ids=TT.mix_tile_regime_id)
def test_mix_tile_row_alone_in_R2(c):
    p = TT.mix_tile_regime_case(c)
    got, one = _mt_gpu_forward("regime", c), mt_forward(p, rows=slice(16, 17), repeat=False)
    for k in TT.MT_OUT:
        assert same_bits(one[k], got[k][16:17] if k in TT.MT_FINAL else got[k][:, 16:17]), k
    if p["H"] == 32:
        tape, dloss = TT.mix_tile_bwd_tape(p, got)
        full = mt_backward(p, tape, dloss, repeat=False)
        alone = mt_backward(p, {k: v[:, 16:17] for k, v in tape.items()}, dloss[:, 16:17], repeat=False)
        for k in TT.MT_GRADS:
            assert same_bits(alone[k], full[k][:, 16:17] if full[k].ndim == 3 else full[k][16:17]), k


@pytest.mark.parametrize("c", _r2_b17(TT.STACKED_TRAIN_REGIME_CASES, 5), ids=TT.stacked_train_regime_id)
def test_stacked_train_row_alone_in_R2(c):
    p = TT.stacked_train_regime_case(c)
    got, one = _st_gpu_forward("regime", c), st_forward(p, rows=slice(16, 17), repeat=False)
    for k in ST_OUT:
        assert same_bits(one[k], got[k][16:17] if k == "dec_top" else got[k][:, 16:17]), k
    full, alone = st_backward(p, got, repeat=False), st_backward(p, one, rows=slice(16, 17), repeat=False)
    for k in TT.ST_GRADS:
        assert same_bits(alone[k], full[k][:, 16:17]), k
