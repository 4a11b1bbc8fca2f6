"""The 2- and 3-layer decode (fov_stacked_seq2seq_decode_fwd) and the self-fed decoder with its BPTT (fov_selffed_decoder_fwd /
_bwd) through the C ABI on GUARDED VIEWS and at their value edges.  tests/test_tile_decoders_host.py owns the case tables and
shows on the CPU what these checks can see (the regimes' shares, the yardstick, references that are wrong on purpose).

Every tensor input is a view inside a NaN buffer, every output a view inside a sentinel buffer, with margins of 16 operand rows and
1024 floats at least and with the alignment the case's table gives it (0 or 1 float behind a 16-byte boundary, both for every
operand over the table).  A read one row or one k-block past an operand - load_frag, the K_0 staging behind its descriptor, the
head's W^T, the R rows copied to LDS, a tape row of step t - 1 - makes a NaN where it is used; a write past a ragged tile breaks a
sentinel; an unwritten element stays NaN.  Every call is made twice into the same views and must give the same bits.  An operand
without elements (T_in = 0, T_out = 0, T = 0) is a zero-length view in the middle of such a buffer, passed by its address.

Bounds.  Values against fp64: the written 1e-3 |ref| + 1e-5 per element and 2e-5 (per unit of magnitude for a cell state beyond 1),
regime_error(., "f32") <= 1; in a value regime <= regime_bound(e_ref) = max(1, 8 e_ref), e_ref being the fp32 oracle against the
fp64 one.  Gradients: 1e-4 of the tensor's max |ref| + 1e-9 on the worst element, against selffed_backward in fp64 on the GPU
forward's OWN tapes: both sides take the same branch at every kink, no element is masked.  Each check prints its error in written
bounds before it asserts; when the module is through, the worst per entry point and regime is printed (a report, not a test)."""
import functools

import numpy as np
import pytest
import torch

import test_tile_decoders_host as TD
from oracle import fov_oracle as O
from test_guarded_views_host import OutView, same_bits
from test_tile_decoders_host import BWD_IN, GRAD, SF_GRADS, SF_IN, SF_OUT, SF_TAPES, STACKED_OUT, addr

pytestmark = pytest.mark.gpu

WORST = {}          # (entry point, regime) -> [checks, worst error in written bounds, worst e_ref]


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    """After the module's last test: the table that DESIGN.md quotes.  The bounds themselves are asserted check by check."""
    yield
    for (entry, regime), (n, err, e_ref) in sorted(WORST.items()):
        print("\n%-20s %-14s checks %4d   worst gpu error %.3f written bounds   worst e_ref %.3f" % (entry, regime, n, err, e_ref), end="")
    print()


def gv(a, off=0):
    return None if a is None else TD.view(np.array(a, dtype=np.float32), off, "cuda")


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


def twice(outs, call):
    """The call made twice into the same views -> the outputs (numpy), which must be the same bits."""
    call()
    first = {k: o.result() for k, o in outs.items()}
    for o in outs.values():
        o.reset()
    call()
    second = {k: o.result() for k, o in outs.items()}
    for k in first:
        assert same_bits(first[k], second[k]), k + ": two calls differ"
    return second


# ---------------------------------------------------------------------------------------------------------------------
# stacked decode
# ---------------------------------------------------------------------------------------------------------------------
def stacked_call(cid, w, enc, dec0, L, T_out, act, want=STACKED_OUT, flip=0):
    """One guarded call (made twice) -> (outputs {name: numpy}, views {name: OutView}).  flip: 1 swaps every alignment."""
    B, T_in, F_enc = enc.shape
    H, F_dec = w["enc0_R"].shape[0], w["dense_W"].shape[1]
    operands = TD.stacked_operands(w, enc, dec0, L)
    off = {k: v ^ flip for k, v in TD.offsets(cid, list(operands) + list(STACKED_OUT)).items()}
    ins = {n: gv(a, off[n]) for n, a in operands.items()}
    shapes = {"out": (B, T_out, F_dec), "hT": (L, B, H), "cT": (L, B, H)}
    outs = {k: ov(shapes[k], off[k]) for k in STACKED_OUT if k in want}
    layers = [addr(ins["%s%d_%s" % (side, l, k)]) if l < L else None for side in ("enc", "dec") for l in range(3) for k in "KRb"]
    args = [addr(ins["enc"]), addr(ins["dec0"])] + layers + [addr(ins["dense_W"]), addr(ins["dense_b"])] + \
        [oaddr(outs.get(k)) for k in STACKED_OUT] + [B, T_in, T_out, F_enc, F_dec, H, L, O.act_code(act)]
    got = twice(outs, lambda: launch(lib().fov_stacked_seq2seq_decode_fwd, *args))
    return got, outs


@pytest.mark.parametrize("cid", [c["id"] for c in TD.stacked_cases()])
def test_stacked_decode_on_guarded_views(cid):
    """Every table case: out, hT, cT against fp64 within the written bounds; without hT, without cT and without both the remaining
    outputs are the same bits; with T_out = 0 the zero-length `out` is passed by its address and nothing around it is written."""
    p = TD.stacked_case(cid)
    run = lambda **kw: stacked_call(cid, p["w"], p["enc"], p["dec0"], p["L"], p["T_out"], p["act"], **kw)
    full, views = run()
    assert full["out"].shape == (p["B"], p["T_out"], p["F_dec"])
    if p["T_out"] == 0:
        assert views["out"].untouched()
    for k in STACKED_OUT:
        held("%s %s" % (cid, k), ("stacked decode", "ordinary"), full[k], p["ref"][k])
    for want in (("out", "hT"), ("out", "cT"), ("out",)):
        part, _ = run(want=want)
        for k in want:
            assert same_bits(part[k], full[k]), (cid, want, k)
    other, _ = run(flip=1)          # the other alignment of every operand: the same bits
    for k in STACKED_OUT:
        assert same_bits(other[k], full[k]), (cid, "alignment", k)


@pytest.mark.parametrize("c", TD.STACKED_REGIME_CASES, ids=TD.stacked_regime_id)
def test_stacked_decode_in_value_regimes(c):
    p = TD.stacked_regime_case(c)
    cid, L, T_out, act, regime = p["id"], p["L"], p["T_out"], p["act"], p["regime"]
    got, _ = stacked_call(cid, p["w"], p["enc"], p["dec0"], L, T_out, act)          # twice: the long run repeats bit for bit
    for k in STACKED_OUT:
        held("%s %s" % (cid, k), ("stacked decode", regime), got[k], p["ref"][k], "f32", p["e_ref"][k])
    assert np.abs(got["out"]).max() <= 1.0 and np.abs(got["hT"]).max() <= 1.0
    pre = p["ref"]["pre"]
    hi, lo = pre > 10.5, pre < -10.5            # 2 / (1 + e^21) is far below half an ulp of 1
    assert (got["out"][hi] == 1.0).all() and (got["out"][lo] == -1.0).all()
    other, _ = stacked_call(cid, p["w"], p["enc"], p["dec0"], L, T_out, act, flip=1)          # every operand at the other alignment
    for k in STACKED_OUT:
        assert same_bits(other[k], got[k]), (cid, "alignment", k)
    if regime != "R3":
        return
    # the extreme rows' tile-mates do not see them
    calm, _ = stacked_call(cid, p["w"], p["enc_calm"], p["dec0"], L, T_out, act)
    mates = np.setdiff1d(np.arange(p["enc"].shape[0]), p["extreme"])
    assert same_bits(calm["out"][mates], got["out"][mates])
    assert same_bits(calm["hT"][:, mates], got["hT"][:, mates]) and same_bits(calm["cT"][:, mates], got["cT"][:, mates])
    assert not same_bits(calm["out"][p["extreme"]], got["out"][p["extreme"]])
    # zero LSTM biases, weights as given: the all-zero tile gives one result for all of its rows; the tile of 1e-6 inputs is held
    # to the absolute bound (tanh cancels)
    edge, _ = stacked_call(cid, p["w_edge"], p["enc_edge"], p["dec0_edge"], L, T_out, act)
    for k, rows in (("out", edge["out"][16:32]), ("hT", edge["hT"][:, 16:32].swapaxes(0, 1)), ("cT", edge["cT"][:, 16:32].swapaxes(0, 1))):
        assert all(same_bits(rows[i], rows[0]) for i in range(1, 16)), (cid, k, "rows of the all-zero tile differ")
    e64 = O.stacked_decode_reference(p["w_edge"], p["enc_edge"], p["dec0_edge"], L, T_out, act, np.float64)
    e32 = O.stacked_decode_reference(p["w_edge"], p["enc_edge"], p["dec0_edge"], L, T_out, act, np.float32)
    for k in STACKED_OUT:
        held("%s edge batch %s" % (cid, k), ("stacked decode", "R3 edge batch"), edge[k], e64[k], "abs", O.regime_error(e32[k], e64[k], "abs"))


@pytest.mark.parametrize("H,F_dec", [(20, 4), (40, 5), (20, 5), (40, 4)])
@pytest.mark.parametrize("L", [2, 3])
def test_padded_model_widths_at_other_feedback_widths(monkeypatch, L, H, F_dec):
    """StackedSeq2SeqLSTM.decode_sequence: latent_dim 20 runs at 32, 40 at 64, with 4 and 5 decoder tokens, against the oracle at the
    model's own width.  The model falls back to a launch per layer and step where the one-launch call is not supported: the call
    is counted, so that the case cannot pass on another kernel."""
    from longterm360fov_amd import ops
    from longterm360fov_amd.models import StackedSeq2SeqLSTM
    from longterm360fov_amd.training import stacked_weight_order
    B, T_in, T_out, F_enc, act = 17, 3, 3, 17, "hard_sigmoid" if L == 3 else "sigmoid"
    c = dict(id="model-H%d-L%d-O%d" % (H, L, F_dec), L=L, H=H, F_enc=F_enc, F_dec=F_dec)
    w = TD.stacked_weights(c)
    rng = np.random.default_rng(TD.seed_of(c["id"] + " inputs"))
    enc, dec0 = rng.uniform(-1, 1, (B, T_in, F_enc)).astype(np.float32), rng.uniform(-1, 1, (B, 1, F_dec)).astype(np.float32)
    m = StackedSeq2SeqLSTM(num_encoder_tokens=F_enc, num_decoder_tokens=F_dec, latent_dim=H, num_layers=L, recurrent_activation=act)
    m.set_weights([w[k] for k in stacked_weight_order(L)])
    Hp = 32 if H <= 32 else 64
    assert ops.stacked_seq2seq_decode_supported(B, T_in, T_out, F_enc, F_dec, Hp, L)
    calls, fused = [], ops.stacked_seq2seq_decode
    monkeypatch.setattr(ops, "stacked_seq2seq_decode", lambda e, x, fw, *a, **k: (calls.append(tuple(fw["enc0_R"].shape)), fused(e, x, fw, *a, **k))[1])
    got = m.decode_sequence(enc, dec0, predict_step=T_out)
    assert calls == [(Hp, 4 * Hp)], "decode_sequence did not take the one-launch call at the padded width"
    ref = O.stacked_decode_reference(w, enc, dec0, L, T_out, act)
    held("%s decode_sequence" % c["id"], ("stacked decode", "model path"), got, ref["out"])


# ---------------------------------------------------------------------------------------------------------------------
# self-fed decoder
# ---------------------------------------------------------------------------------------------------------------------
def _dact(name):
    return {"tanh": 1, "relu": 2}[name]


def sf_forward(p, T, want=SF_OUT, flip=0, B=None):
    """fov_selffed_decoder_fwd on guarded views, twice -> ({name: numpy}, {name: OutView})."""
    B = p["B"] if B is None else B
    H, n_out = p["H"], p["O"]
    off = {k: v ^ flip for k, v in TD.offsets(p["id"], SF_IN + SF_OUT).items()}
    ins = {k: gv(None if p[k] is None else p[k][:B] if k in ("x0", "h0", "c0", "r") else p[k], off[k]) for k in SF_IN}
    shapes = {"Hs": (T + 1, B, H), "Cs": (T + 1, B, H), "XA": (T + 1, B, n_out), "A": (T, B, n_out), "RES": (T, B, 1, 5, H), "y": (B, T, n_out)}
    outs = {k: ov(shapes[k], off[k]) for k in SF_OUT if k in want}
    args = [addr(ins[k]) for k in SF_IN] + [oaddr(outs.get(k)) for k in SF_OUT] + [B, T, n_out, H, O.act_code(p["act"]), _dact(p["dact"])]
    if B == 0 or T == 0:        # nothing is launched and nothing written: result() would find the NaN fill
        launch(lib().fov_selffed_decoder_fwd, *args)
        return None, outs
    return twice(outs, lambda: launch(lib().fov_selffed_decoder_fwd, *args)), outs


def sf_backward(p, tape, T, want=SF_GRADS, a_from_A=None, flip=0, B=None, null_tapes=False):
    """fov_selffed_decoder_bwd with every tape a guarded view, twice -> ({name: numpy}, {name: OutView}).  a_from_A None: 1 when
    the case has a residual term (XA[1:] is then a_t + r), else 0."""
    B = p["B"] if B is None else B
    H, n_out = p["H"], p["O"]
    a_from_A = int(p["r"] is not None) if a_from_A is None else a_from_A
    off = {k: v ^ flip for k, v in TD.offsets(p["id"] + " bwd", BWD_IN + SF_GRADS).items()}
    src = dict(tape, dloss=p["dloss"][:, :B], K=p["K"], R=p["R"], W=p["W"])
    ins = {k: gv(src[k], off[k]) for k in BWD_IN}
    shapes = {"DY": (T, B, n_out), "DPRE": (T, B, n_out), "DZ": (T, B, 4 * H), "dx0": (B, n_out), "dh0": (B, H), "dc0": (B, H)}
    outs = {k: ov(shapes[k], off[k]) for k in SF_GRADS if k in want}
    args = [addr(ins[k]) for k in BWD_IN] + [oaddr(outs.get(k)) for k in SF_GRADS] + \
        [B, T, n_out, H, O.act_code(p["act"]), _dact(p["dact"]), a_from_A]
    if null_tapes:
        args[:5] = [None] * 5
    if B == 0:
        launch(lib().fov_selffed_decoder_bwd, *args)
        return None, outs
    return twice(outs, lambda: launch(lib().fov_selffed_decoder_bwd, *args)), outs


@functools.lru_cache(maxsize=None)
def _gpu_forward(kind, key):
    p = TD.selffed_case(key) if kind == "ordinary" else TD.selffed_regime_case(key)
    got, _ = sf_forward(p, p["T"])
    for a in got.values():
        a.setflags(write=False)
    return got


def gpu_tape(got):
    return {k: got[k] for k in ("Cs", "XA", "A", "RES")}


def check_forward(p, got, family, e_ref=None):
    for k in SF_TAPES:
        held("%s %s" % (p["id"], k), family, got[k], p["ref"][k], "f32", 0.0 if e_ref is None else e_ref[k])
    assert same_bits(got["y"], np.ascontiguousarray(got["XA"][1:].swapaxes(0, 1)))          # y is XA[1:], batch-major
    if p["r"] is None:
        assert same_bits(got["A"], got["XA"][1:])
    else:                                                                                    # y_t = a_t + r is one fp32 addition
        assert same_bits(got["XA"][1:], got["A"] + p["r"][None])


def check_backward(p, grads, tape, family, e_ref=None):
    ref = TD.selffed_grads(p, tape)
    for k in SF_GRADS:
        held("%s %s" % (p["id"], k), family, grads[k], ref[k], GRAD, 0.0 if e_ref is None else e_ref[k])


SELFFED_IDS = [c["id"] for c in TD.selffed_cases()]


@pytest.mark.parametrize("cid", SELFFED_IDS)
def test_selffed_forward_on_guarded_views(cid):
    """y and all five tapes against fp64; each of the six output pointers NULL on its own leaves the others the same bits; A is
    written without a residual term too and is then XA[1:]."""
    p = TD.selffed_case(cid)
    got = _gpu_forward("ordinary", cid)
    check_forward(p, got, ("selffed forward", "ordinary"))
    for leave in SF_OUT:
        part, _ = sf_forward(p, p["T"], want=tuple(k for k in SF_OUT if k != leave))
        for k in part:
            assert same_bits(part[k], got[k]), (cid, "without " + leave, k)
    other, _ = sf_forward(p, p["T"], flip=1)
    for k in SF_OUT:
        assert same_bits(other[k], got[k]), (cid, "alignment", k)


@pytest.mark.parametrize("cid", SELFFED_IDS)
def test_selffed_backward_on_the_gpu_forwards_tapes(cid):
    """All six outputs against selffed_backward in fp64 on the same tapes; dh0 NULL, dc0 NULL and both NULL leave the rest the same
    bits; without a residual term a_t read from A and from XA[1:] gives the same bits."""
    p = TD.selffed_case(cid)
    tape = gpu_tape(_gpu_forward("ordinary", cid))
    grads, _ = sf_backward(p, tape, p["T"])
    check_backward(p, grads, tape, ("selffed backward", "ordinary"))
    for want in (tuple(k for k in SF_GRADS if k != "dh0"), tuple(k for k in SF_GRADS if k != "dc0"), SF_GRADS[:4]):
        part, _ = sf_backward(p, tape, p["T"], want=want)
        for k in want:
            assert same_bits(part[k], grads[k]), (cid, want, k)
    if p["r"] is None:
        both = [sf_backward(p, tape, p["T"], a_from_A=a)[0] for a in (0, 1)]
        for k in SF_GRADS:
            assert same_bits(both[0][k], both[1][k]) and same_bits(both[0][k], grads[k]), (cid, "a_from_A", k)
    other, _ = sf_backward(p, tape, p["T"], flip=1)
    for k in SF_GRADS:
        assert same_bits(other[k], grads[k]), (cid, "alignment", k)


@pytest.mark.parametrize("cid", [SELFFED_IDS[1], SELFFED_IDS[12]])
def test_selffed_without_a_step_or_a_sequence(cid):
    """T = 0: the forward writes nothing (no tape row 0 either); the backward leaves exact zeros in dx0, dh0, dc0, touches nothing
    else and needs none of the tapes.  B = 0: both calls return FOV_OK and touch nothing."""
    p = TD.selffed_case(cid)
    B, H, n_out = p["B"], p["H"], p["O"]
    for flip in (0, 1):          # both alignments of every operand and output
        _, outs = sf_forward(p, 0, flip=flip)
        assert all(o.untouched() for o in outs.values()), "the forward wrote something at T = 0"
        empty = {"Cs": np.zeros((1, B, H), np.float32), "XA": np.zeros((1, B, n_out), np.float32), "A": np.zeros((0, B, n_out), np.float32),
                 "RES": np.zeros((0, B, 1, 5, H), np.float32)}
        q = dict(p, dloss=np.zeros((0, B, n_out), np.float32))
        for null_tapes, want in ((False, SF_GRADS), (True, ("dx0", "dh0", "dc0")), (True, ("dx0",))):
            got, outs = sf_backward(q, empty, 0, want=want, null_tapes=null_tapes, flip=flip)
            for k in ("dx0", "dh0", "dc0"):
                assert k not in want or (got[k] == 0).all() and not np.signbit(got[k]).any(), (cid, k)
            assert all(outs[k].untouched() for k in ("DY", "DPRE", "DZ") if k in want)
        for T in (0, 2):
            _, outs = sf_forward(p, T, B=0, flip=flip)
            assert all(o.untouched() for o in outs.values())
            tape0 = {"Cs": np.zeros((T + 1, 0, H), np.float32), "XA": np.zeros((T + 1, 0, n_out), np.float32),
                     "A": np.zeros((T, 0, n_out), np.float32), "RES": np.zeros((T, 0, 1, 5, H), np.float32)}
            _, outs = sf_backward(dict(p, dloss=np.zeros((T, 0, n_out), np.float32)), tape0, T, B=0, flip=flip)
            assert all(o.untouched() for o in outs.values())


@pytest.mark.parametrize("state", [True, False])
def test_wrapper_returns_tape_row_zero_without_a_step(state):
    """ops.selffed_decoder_fwd(..., T=0, tape=True): the entry point writes nothing, the wrapper fills row 0 as it documents -
    Hs[0] = h0, Cs[0] = c0 (zeros without a state), XA[0] = x0 - exactly."""
    from longterm360fov_amd import ops
    p = TD.selffed_case(SELFFED_IDS[5])
    dev = lambda a: None if a is None else torch.from_numpy(np.array(a, dtype=np.float32)).cuda()
    B, H, n_out = p["B"], p["H"], p["O"]
    h0 = p["h0"] if p["h0"] is not None else np.full((B, H), 0.25, np.float32)
    c0 = p["c0"] if p["c0"] is not None else np.full((B, H), -0.5, np.float32)
    y, tp = ops.selffed_decoder_fwd(dev(p["x0"]), *(dev(p[k]) for k in ("K", "R", "b", "W", "bd")), 0, h0=dev(h0) if state else None,
                                    c0=dev(c0) if state else None, r=dev(p["r"]), act=p["act"], dense_activation=p["dact"], tape=True)
    torch.cuda.synchronize()
    assert tuple(y.shape) == (B, 0, n_out) and tuple(tp["Hs"].shape) == (1, B, H) and tuple(tp["RES"].shape) == (0, B, 1, 5, H)
    zero = np.zeros((B, H), np.float32)
    assert same_bits(tp["Hs"][0].cpu().numpy(), h0 if state else zero) and same_bits(tp["Cs"][0].cpu().numpy(), c0 if state else zero)
    assert same_bits(tp["XA"][0].cpu().numpy(), p["x0"])
    out = ops.selffed_decoder_bwd(tp, dev(np.zeros((0, B, n_out), np.float32)), *(dev(p[k]) for k in ("K", "R", "W")), act=p["act"],
                                  dense_activation=p["dact"])
    torch.cuda.synchronize()
    assert all(float(out[k].abs().max()) == 0.0 for k in ("dx0", "dh0", "dc0"))


@pytest.mark.parametrize("c", TD.SELFFED_REGIME_CASES, ids=TD.selffed_regime_id)
def test_selffed_decoder_in_value_regimes(c):
    p = TD.selffed_regime_case(c)
    regime, H = p["regime"], p["H"]
    e_fwd, e_bwd = TD.selffed_e_ref(p)
    got = _gpu_forward("regime", c)                   # made twice: the 64-step run repeats bit for bit
    check_forward(p, got, ("selffed forward", regime), dict(e_fwd, A=e_fwd.get("A", e_fwd["XA"])))
    tape = gpu_tape(got)
    grads, _ = sf_backward(p, tape, p["T"])
    check_backward(p, grads, tape, ("selffed backward", regime), e_bwd)
    flipped_f, flipped_b = sf_forward(p, p["T"], flip=1)[0], sf_backward(p, tape, p["T"], flip=1)[0]          # the other alignment
    assert all(same_bits(flipped_f[k], got[k]) for k in SF_OUT) and all(same_bits(flipped_b[k], grads[k]) for k in SF_GRADS)
    res = got["RES"][:, :, 0]
    if p["act"] == "hard_sigmoid":
        n = 0
        for q in (0, 1, 3):
            flat = (res[:, :, q] == 0.0) | (res[:, :, q] == 1.0)
            n += int(flat.sum())
            assert (grads["DZ"][:, :, q * H:(q + 1) * H][flat] == 0.0).all(), (p["id"], "a clamped gate with a gradient", q)
        assert n > 0.3 * 3 * res[:, :, 0].size and float(np.abs(grads["DZ"]).max()) > 0
    if p["dact"] == "relu":
        dead = got["A"] == 0.0
        assert dead.mean() >= 0.30 and (grads["DPRE"][dead] == 0.0).all() and (grads["DPRE"][~dead] != 0.0).any()
    if regime == "R4":
        assert float(np.abs(got["Cs"]).max()) > 50
