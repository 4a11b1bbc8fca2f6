"""The one-tile decoders - the 2- and 3-layer decode (fov_stacked_seq2seq_decode_fwd, lstm_stacked_s2s.hip) and the self-fed decoder
with its BPTT (fov_selffed_decoder_fwd / _bwd, lstm_selffed.hip) - on guarded views and at their value edges: the case tables of
tests/test_gpu_tile_decoders.py and everything that can be checked without a GPU.

Tables.  Shapes are the smallest at which each seam exists: B in {1, 16, 17, 30} (33 where a regime needs three tiles), step counts
in {0, 1, 2, 3} with both parities of T_in (the decoder's LDS parity is (T_in + s) & 1), one long run per kernel.  The stacked
decode runs every feedback width F_dec = 1 .. 8 and every encoder width of {1, 15, 16, 17, 32, 95, 96} in each of its four
instantiations (HP 32 / 64 x L 2 / 3); the self-fed decoder every output width 1 .. 8 at both widths, forward and backward.
Regime cases (oracle.fov_oracle: R1 clamped hard_sigmoid, R2 saturated sigmoid / tanh, R3 overflowing rows, R4 a growing cell
state) come from regime_stacked_seq2seq / regime_selffed.

Asserted here, in fp64, for every regime case: the shares of clamped / saturated pre-activations of EVERY layer in both phases, the
overflow of R3's extreme rows, max |c| of R4, the zero share of a relu head; that 8 e_ref (the oracle in fp32 against itself in
fp64, in written bounds) stays below REGIME_YARDSTICK_CAP, so that the written bounds themselves are what the GPU is held to; that
each reference that is WRONG ON PURPOSE (oracle.fov_oracle.STACKED_MISTAKES / SELFFED_MISTAKES) misses the GPU test's bound by
MARGIN = 10 at least on every case it applies to; selffed_backward against torch.autograd in fp64; and the guarded views of every
case (margins of 16 operand rows and 1024 floats, the alignment asked for, both alignments for every operand over the table)."""
import functools

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O
from test_guarded_views_host import MARGIN, TILE, OutView, f64, guarded, margin_floats, same_bits, seed_of

GRAD = 1e-4          # a gradient's written bound: this fraction of the tensor's max |ref| (+ 1e-9), no element left out
STACKED_OUT = ("out", "hT", "cT")
SF_TAPES = ("y", "Hs", "Cs", "XA", "A", "RES")
SF_GRADS = ("DY", "DPRE", "DZ", "dx0", "dh0", "dc0")
SF_IN = ("x0", "h0", "c0", "K", "R", "b", "W", "bd", "r")          # the self-fed forward's inputs, its output pointers and the
SF_OUT = ("Hs", "Cs", "XA", "A", "RES", "y")                        # backward's inputs, each in the C ABI's order
BWD_IN = ("Cs", "XA", "A", "RES", "dloss", "K", "R", "W")
BATCHES = (1, 16, 17, 30)
INSTANTIATIONS = ((32, 2), (32, 3), (64, 2), (64, 3))          # (HP, L) of stacked_s2s_kernel

# ---------------------------------------------------------------------------------------------------------------------
# stacked decode: the tables
# ---------------------------------------------------------------------------------------------------------------------
# The first eight rows run BOTH phases: every feedback width in front of a decoder (T_out > 0) and every encoder width behind an
# encoder (T_in > 0; 17, one column into a second k-block, twice), T_in of both parities in front of a decoder.  The last two rows
# are the empty phases, on widths that the rows above already run with that phase: T_out = 0 (the kernel skips the decoder block, so
# F_dec is not exercised) and T_in = 0 (it skips the encoder block, so F_enc is not).
_STACKED_ROWS = [  # F_dec, F_enc, T_in, T_out
    (1, 16, 1, 2), (2, 95, 2, 3), (3, 1, 3, 1), (4, 32, 1, 3), (5, 17, 3, 2), (6, 96, 2, 3), (7, 15, 1, 1), (8, 17, 2, 2),
    (6, 17, 2, 0), (5, 17, 0, 3)]


def stacked_cases():
    """-> [dict(id, L, H, F_enc, F_dec, B, T_in, T_out, act)]: 10 per instantiation, B and the activation rotating."""
    out = []
    for k, (H, L) in enumerate(INSTANTIATIONS):
        for i, (F_dec, F_enc, T_in, T_out) in enumerate(_STACKED_ROWS):
            B = BATCHES[(i + k) % 4]
            act = "hard_sigmoid" if (i + k) % 2 else "sigmoid"
            out.append(dict(id="stacked-H%d-L%d-O%d-F%d-B%d-T%d-%d" % (H, L, F_dec, F_enc, B, T_in, T_out), L=L, H=H, F_enc=F_enc,
                            F_dec=F_dec, B=B, T_in=T_in, T_out=T_out, act=act))
    return out


# (regime, HP, L, F_enc, F_dec, B, T_in, T_out): R3 needs three tiles (x_edge) and two encoder steps; its last row is the long run
STACKED_REGIME_CASES = [
    ("R1", 32, 2, 17, 5, 17, 2, 3), ("R1", 32, 3, 90, 8, 30, 3, 2), ("R1", 64, 2, 96, 4, 16, 3, 3), ("R1", 64, 3, 15, 7, 17, 2, 3),
    ("R2", 32, 2, 95, 7, 30, 3, 3), ("R2", 32, 3, 16, 4, 17, 2, 2), ("R2", 64, 2, 32, 5, 17, 3, 2), ("R2", 64, 3, 90, 6, 30, 2, 3),
    ("R3", 32, 2, 90, 6, 33, 4, 3), ("R3", 32, 3, 17, 3, 33, 3, 2), ("R3", 64, 2, 95, 8, 33, 2, 3), ("R3", 64, 3, 90, 6, 33, 4, 64)]


def stacked_regime_id(c):
    return "stacked-%s-H%d-L%d-F%d-O%d-B%d-T%d-%d" % c


def stacked_weights(c):
    """Glorot / orthogonal layers with a bias of 0.1 N(0, 1) and a small uniform head: ordinary data."""
    rng = np.random.default_rng(seed_of(c["id"]))
    L, H, w = c["L"], c["H"], {}
    for side, f0 in (("enc", c["F_enc"]), ("dec", c["F_dec"])):
        for l in range(L):
            K, R, b = O.init_lstm(rng, f0 if l == 0 else H, H)
            w["%s%d_K" % (side, l)], w["%s%d_R" % (side, l)] = K, R
            w["%s%d_b" % (side, l)] = (b + 0.1 * rng.standard_normal(4 * H)).astype(np.float32)
    w["dense_W"] = rng.uniform(-0.3, 0.3, (H, c["F_dec"])).astype(np.float32)
    w["dense_b"] = rng.uniform(-0.1, 0.1, c["F_dec"]).astype(np.float32)
    return w


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, dict):
            _frozen(*a.values())
        elif isinstance(a, (list, tuple)):
            _frozen(*a)
        elif isinstance(a, np.ndarray):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _stacked_case(cid):
    c = {x["id"]: x for x in stacked_cases()}[cid]
    w = stacked_weights(c)
    rng = np.random.default_rng(seed_of(cid + " inputs"))
    enc = rng.uniform(-1, 1, (c["B"], c["T_in"], c["F_enc"])).astype(np.float32)
    dec0 = rng.uniform(-1, 1, (c["B"], 1, c["F_dec"])).astype(np.float32)
    ref = O.stacked_decode_reference(w, enc, dec0, c["L"], c["T_out"], c["act"])
    _frozen(w, enc, dec0, ref)
    return dict(c, w=w, enc=enc, dec0=dec0, ref=ref)


def stacked_case(cid):
    """One ordinary case: weights, fp32 inputs and the fp64 reference, computed once and shared (nobody writes into them)."""
    return _stacked_case(cid)


@functools.lru_cache(maxsize=None)
def stacked_regime_case(c):
    """One regime case: regime_stacked_seq2seq's dict + L, T_out, ref (fp64), e_ref per output (fp32 oracle vs fp64, written bounds)."""
    regime, H, L, F_enc, F_dec, B, T_in, T_out = c
    p = O.regime_stacked_seq2seq(seed_of(stacked_regime_id(c)) % (1 << 31), regime, L, H, F_enc, F_dec, B, T_in)
    r64 = O.stacked_decode_reference(p["w"], p["enc"], p["dec0"], L, T_out, p["act"], np.float64)
    r32 = O.stacked_decode_reference(p["w"], p["enc"], p["dec0"], L, T_out, p["act"], np.float32)
    p.update(id=stacked_regime_id(c), L=L, H=H, T_out=T_out, ref=r64, e_ref={k: O.regime_error(r32[k], r64[k], "f32") for k in STACKED_OUT})
    _frozen(p)
    return p


def stacked_operands(w, enc, dec0, L):
    """The call's tensor inputs by name, in the C ABI's order."""
    ops = {"enc": enc, "dec0": dec0}
    for side in ("enc", "dec"):
        for l in range(L):
            for k in "KRb":
                ops["%s%d_%s" % (side, l, k)] = w["%s%d_%s" % (side, l, k)]
    ops["dense_W"], ops["dense_b"] = w["dense_W"], w["dense_b"]
    return ops


def view(a, off=0, device="cpu"):
    """guarded(a).  An operand without elements (no step to read) becomes a zero-length view in the middle of a NaN buffer with the
    margins its shape asks for; torch reports no address for such a view: addr() does."""
    a = np.array(a, dtype=np.float32)
    if a.size:
        return guarded(a, off, device)
    m = margin_floats(a.shape)
    g = guarded(np.full((2 * m + 8,), np.nan, np.float32), off, device)
    return g[m:m].view(a.shape)


def addr(t):
    """The address a view stands at, also where it has no elements (data_ptr() is 0 there); None for None."""
    if t is None:
        return None
    if t.numel() or t._base is None:
        return t.data_ptr()
    return t._base.data_ptr() + t._base.element_size() * t.storage_offset()


def offsets(cid, names):
    """0 or 1 float behind a 16-byte boundary for every operand (and output) of a case: alternating along the call, starting from
    the case's own bit, so that both appear for every operand over a table."""
    s = seed_of(cid)
    return {n: (s + i) & 1 for i, n in enumerate(names)}


# ---------------------------------------------------------------------------------------------------------------------
# self-fed decoder: the tables
# ---------------------------------------------------------------------------------------------------------------------
def selffed_cases():
    """-> [dict(id, H, O, B, T, act, dact, state, residual)]: every O = 1 .. 8 at both widths; every case runs forward and backward."""
    out = []
    for k, H in enumerate((32, 64)):
        for i in range(8):
            n_out = i + 1
            B, T = BATCHES[(i + k) % 4], (1, 2, 3)[(i + 2 * k) % 3]
            act = "hard_sigmoid" if (i + k) % 2 else "sigmoid"
            dact = "relu" if (i // 2 + k) % 2 else "tanh"
            state, residual = bool((i + k) % 3), bool((i // 2 + i + k) % 2)
            out.append(dict(id="selffed-H%d-O%d-B%d-T%d-%s-%s-s%d-r%d" % (H, n_out, B, T, act, dact, state, residual), H=H, O=n_out, B=B, T=T,
                            act=act, dact=dact, state=state, residual=residual))
    return out


# (regime, H, O, B, T, head, residual): both heads and both residual settings; R4 is the long run
SELFFED_REGIME_CASES = [("R1", 32, 5, 17, 3, "tanh", True), ("R1", 64, 7, 30, 3, "relu", False), ("R2", 64, 4, 17, 3, "relu", True),
                        ("R2", 32, 6, 30, 2, "tanh", False), ("R4", 64, 6, 17, 64, "tanh", False), ("R4", 32, 8, 17, 64, "relu", True)]


def selffed_regime_id(c):
    return "selffed-%s-H%d-O%d-B%d-T%d-%s-r%d" % c


def _selffed_finish(p, T):
    """Adds the fp64 forward, the fp32 oracle's tapes and (on those: one tape, the same branch at every kink) the fp64 backward."""
    args = [p[k] for k in ("x0", "h0", "c0", "r", "K", "R", "b", "W", "bd")]
    p["T"] = T
    p["ref"] = O.selffed_forward(*args, T, p["act"], p["dact"], np.float64)
    p["tape32"] = O.selffed_forward(*args, T, p["act"], p["dact"], np.float32)
    if p["r"] is None:
        p["tape32"]["A"] = None
    _frozen(p)
    return p


@functools.lru_cache(maxsize=None)
def _selffed_case(cid):
    c = {x["id"]: x for x in selffed_cases()}[cid]
    H, n_out, B, T = c["H"], c["O"], c["B"], c["T"]
    rng = np.random.default_rng(seed_of(cid))
    K, R, b = O.init_lstm(rng, n_out, H)
    p = dict(c, K=K, R=R, b=(b + 0.1 * rng.standard_normal(4 * H)).astype(np.float32),
             W=rng.uniform(-0.5, 0.5, (H, n_out)).astype(np.float32), bd=rng.uniform(-0.2, 0.2, n_out).astype(np.float32),
             x0=rng.uniform(-1, 1, (B, n_out)).astype(np.float32),
             h0=(0.3 * rng.standard_normal((B, H))).astype(np.float32) if c["state"] else None,
             c0=(0.3 * rng.standard_normal((B, H))).astype(np.float32) if c["state"] else None,
             r=rng.uniform(-0.5, 0.5, (B, n_out)).astype(np.float32) if c["residual"] else None,
             dloss=rng.standard_normal((T, B, n_out)).astype(np.float32))
    return _selffed_finish(p, T)


def selffed_case(cid):
    return _selffed_case(cid)


@functools.lru_cache(maxsize=None)
def selffed_regime_case(c):
    regime, H, n_out, B, T, dact, residual = c
    p = O.regime_selffed(seed_of(selffed_regime_id(c)) % (1 << 31), regime, H, n_out, B, T, dact, residual)
    p.update(id=selffed_regime_id(c), H=H, O=n_out, B=B)
    p = _selffed_finish(p, T)
    return p


def selffed_e_ref(p):
    """-> (forward, backward): per tape, the fp32 oracle against the fp64 one in written bounds; per gradient, selffed_backward on
    fp32 arrays against fp64, both on the fp32 oracle's tapes, in units of 1e-4 max |ref| + 1e-9."""
    fwd = {k: O.regime_error(p["tape32"][k], p["ref"][k], "f32") for k in SF_TAPES if p["tape32"][k] is not None}
    g64 = selffed_grads(p, p["tape32"], np.float64)
    g32 = selffed_grads(p, p["tape32"], np.float32)
    return fwd, {k: O.regime_error(g32[k], g64[k], GRAD) for k in SF_GRADS}


def selffed_grads(p, tape, dt=np.float64, mistake=None):
    """selffed_backward of case p on the given tapes (numpy; A None without a residual) in dtype dt."""
    c_ = lambda a: None if a is None else np.asarray(a, dt)
    t = {k: c_(tape.get(k)) for k in ("Cs", "XA", "A", "RES")}
    return O.selffed_backward(t, c_(p["dloss"]), p["K"], p["R"], p["W"], p["act"], p["dact"], mistake)


def selffed_operands(p):
    return {k: p[k] for k in SF_IN}


def worst(got, ref, keys, kind, e_ref=None):
    """max over `keys` of the error in ASSERTED bounds: written bounds over regime_bound(e_ref)."""
    return max(O.regime_error(got[k], ref[k], kind) / (1.0 if e_ref is None else O.regime_bound(e_ref[k])) for k in keys)


# ---------------------------------------------------------------------------------------------------------------------
# the tables cover what they say
# ---------------------------------------------------------------------------------------------------------------------
def test_stacked_table_covers_every_width_in_every_instantiation():
    cases = stacked_cases()
    assert len(cases) + len(STACKED_REGIME_CASES) >= 40
    for H, L in INSTANTIATIONS:
        mine = [c for c in cases if (c["H"], c["L"]) == (H, L)]
        # a width counts only where its phase runs: the kernel skips the decoder block at T_out = 0, the encoder block at T_in = 0
        assert {c["F_dec"] for c in mine if c["T_out"] > 0} == set(range(1, 9))
        assert {c["F_enc"] for c in mine if c["T_in"] > 0} == {1, 15, 16, 17, 32, 95, 96}
        assert [c for c in mine if c["T_out"] == 0 and c["T_in"] > 0] and [c for c in mine if c["T_in"] == 0 and c["T_out"] > 0]
        assert {c["B"] for c in mine} == set(BATCHES) and {c["act"] for c in mine} == {"sigmoid", "hard_sigmoid"}
        assert {c["T_in"] for c in mine} == {0, 1, 2, 3} and {c["T_out"] for c in mine} == {0, 1, 2, 3}
        assert {c["T_in"] % 2 for c in mine if c["T_out"]} == {0, 1}
        assert {r[0] for r in STACKED_REGIME_CASES if (r[1], r[2]) == (H, L)} == {"R1", "R2", "R3"}
    assert [r for r in STACKED_REGIME_CASES if r[6:] == (4, 64)] and all(r[5] > 2 * TILE for r in STACKED_REGIME_CASES if r[0] == "R3")


def test_selffed_table_covers_every_width_head_and_state():
    cases = selffed_cases()
    for H in (32, 64):
        mine = [c for c in cases if c["H"] == H]
        assert {c["O"] for c in mine} == set(range(1, 9)) and {c["B"] for c in mine} == set(BATCHES) and {c["T"] for c in mine} == {1, 2, 3}
        for k in ("act", "dact", "state", "residual"):
            assert len({c[k] for c in mine}) == 2, (H, k)
    assert {(c[5], c[6]) for c in SELFFED_REGIME_CASES} == {("tanh", True), ("tanh", False), ("relu", True), ("relu", False)}
    assert {c[0] for c in SELFFED_REGIME_CASES} == {"R1", "R2", "R4"} and {c[1] for c in SELFFED_REGIME_CASES} == {32, 64}
    assert all(c[4] == 64 for c in SELFFED_REGIME_CASES if c[0] == "R4")


# ---------------------------------------------------------------------------------------------------------------------
# shares and the yardstick
# ---------------------------------------------------------------------------------------------------------------------
def _gate_shares(z, H):
    gates = np.concatenate([z[..., :2 * H], z[..., 3 * H:]], axis=-1)
    g = z[..., 2 * H:3 * H]
    return float((np.abs(gates) > 2.5).mean()), float((np.abs(gates) > 17).mean()), float((np.abs(g) > 9).mean())


def _assert_shares(tag, regime, z, H):
    clamped, sat, g_sat = _gate_shares(z, H)
    print("%-56s beyond +-2.5: %.2f  beyond +-17: %.2f  g beyond +-9: %.2f" % (tag, clamped, sat, g_sat))
    if regime == "R1":
        assert clamped >= 0.30, (tag, clamped)
    if regime in ("R2", "R3"):
        assert sat >= 0.30 and g_sat >= 0.35, (tag, sat, g_sat)


@pytest.mark.parametrize("c", STACKED_REGIME_CASES, ids=stacked_regime_id)
def test_stacked_regime_shares_and_yardstick(c):
    p = stacked_regime_case(c)
    H, ref = p["H"], p["ref"]
    for phase in ("z_enc", "z_dec"):
        for l, z in enumerate(ref[phase]):
            assert z.shape[1] > 0
            _assert_shares("%s %s layer %d" % (p["id"], phase, l), p["regime"], z, H)
    if p["regime"] == "R3":
        z0 = ref["z_enc"][0]
        a, b = p["extreme"][:2]
        assert (z0[a] > 100).any() and (z0[a] < -100).any() and (z0[b] > 200).any() and (z0[b] < -200).any()
        assert (np.abs(z0[p["extreme"][2], :z0.shape[1] // 2]) < 100).all() and (np.abs(z0[p["extreme"][2], -1]) > 200).any()
    assert all(np.isfinite(ref[k]).all() for k in STACKED_OUT)
    print("%-56s e_ref %s" % (p["id"], {k: round(v, 3) for k, v in p["e_ref"].items()}))
    for k in STACKED_OUT:
        assert O.REGIME_YARDSTICK * p["e_ref"][k] < O.REGIME_YARDSTICK_CAP, (p["id"], k, p["e_ref"][k])


@pytest.mark.parametrize("c", SELFFED_REGIME_CASES, ids=selffed_regime_id)
def test_selffed_regime_shares_and_yardstick(c):
    p = selffed_regime_case(c)
    ref = p["ref"]
    _assert_shares(p["id"], p["regime"], ref["z"], p["H"])
    if p["regime"] == "R4":
        c_max = float(np.abs(ref["Cs"]).max())
        print("%-56s max |c| %.1f" % (p["id"], c_max))
        assert c_max > 50
    if p["dact"] == "relu":
        zero, pos = float((ref["A"] == 0).mean()), float((ref["A"] > 0).mean())
        print("%-56s relu head: %.2f exactly zero, %.2f positive" % (p["id"], zero, pos))
        assert zero >= 0.30 and pos >= 0.30
    fwd, bwd = selffed_e_ref(p)
    print("%-56s e_ref forward %.3f backward %.3f" % (p["id"], max(fwd.values()), max(bwd.values())))
    for k, v in list(fwd.items()) + list(bwd.items()):
        assert O.REGIME_YARDSTICK * v < O.REGIME_YARDSTICK_CAP, (p["id"], k, v)


@pytest.mark.parametrize("cid", [c["id"] for c in stacked_cases()])
def test_stacked_case_reference_is_finite(cid):
    p = stacked_case(cid)
    assert all(np.isfinite(p["ref"][k]).all() for k in STACKED_OUT)
    assert p["ref"]["out"].shape == (p["B"], p["T_out"], p["F_dec"]) and p["ref"]["hT"].shape == (p["L"], p["B"], p["H"])
    if p["T_out"] and p["T_in"]:      # the restatement against the oracle's own stacked model
        y = O.stacked_seq2seq_forward(f64(p["enc"]), f64(p["dec0"]), {k: f64(v) for k, v in p["w"].items()}, p["L"], p["act"], T_out=p["T_out"])
        np.testing.assert_allclose(p["ref"]["out"], y, rtol=0, atol=1e-13)


# ---------------------------------------------------------------------------------------------------------------------
# the references that are wrong on purpose
# ---------------------------------------------------------------------------------------------------------------------
def stacked_mistake_applies(mistake, F_enc, F_dec, T_in, T_out):
    return {"feedback rows 0..3": F_dec >= 5 and T_out > 0, "partial k-block dropped": F_enc % 16 != 0 and F_enc > 16 and T_in > 0,
            "layer below one step late": T_in + T_out > 0, "encoder state returned": T_out > 0,
            "head bias of outputs 0..3": F_dec >= 5 and T_out > 0}[mistake]


@pytest.mark.parametrize("mistake", O.STACKED_MISTAKES)
def test_wrong_stacked_references_miss_the_bound(mistake):
    seen = set()
    for c in stacked_cases():
        if stacked_mistake_applies(mistake, c["F_enc"], c["F_dec"], c["T_in"], c["T_out"]):
            p = stacked_case(c["id"])
            wrong = O.stacked_decode_reference(p["w"], p["enc"], p["dec0"], p["L"], p["T_out"], p["act"], mistake=mistake)
            r = worst(wrong, p["ref"], STACKED_OUT, "f32")
            assert all(np.isfinite(wrong[k]).all() for k in STACKED_OUT) and r >= MARGIN, (c["id"], mistake, r)
            seen.add((c["F_enc"], c["F_dec"]))
    for c in STACKED_REGIME_CASES:
        if stacked_mistake_applies(mistake, c[3], c[4], c[6], c[7]):
            p = stacked_regime_case(c)
            wrong = O.stacked_decode_reference(p["w"], p["enc"], p["dec0"], p["L"], p["T_out"], p["act"], mistake=mistake)
            r = worst(wrong, p["ref"], STACKED_OUT, "f32", p["e_ref"])
            assert all(np.isfinite(wrong[k]).all() for k in STACKED_OUT) and r >= MARGIN, (p["id"], mistake, r)
    if mistake == "feedback rows 0..3":
        assert {f for _, f in seen} == {5, 6, 7, 8}
    if mistake == "partial k-block dropped":
        assert {f for f, _ in seen} == {17, 95}


def selffed_mistake_applies(mistake, p):
    """A pinned forget gate (R4) has a derivative of exactly zero and the value exactly one: c_{t-1} reaches nothing through it and
    a multiplication by it changes nothing, so the two mistakes about it cannot be seen there (and are none)."""
    return {"feedback gradient dropped": p["T"] >= 2, "c_prev one step late": p.get("regime") != "R4",
            "tanh derivative from XA": p["dact"] == "tanh" and p["r"] is not None, "dc0 without f": p.get("regime") != "R4"}[mistake]


@pytest.mark.parametrize("mistake", O.SELFFED_MISTAKES)
def test_wrong_selffed_references_miss_the_bound(mistake):
    n = 0
    for p in [selffed_case(c["id"]) for c in selffed_cases()] + [selffed_regime_case(c) for c in SELFFED_REGIME_CASES]:
        if selffed_mistake_applies(mistake, p):
            ref, wrong = selffed_grads(p, p["tape32"]), selffed_grads(p, p["tape32"], mistake=mistake)
            e_ref = selffed_e_ref(p)[1] if "regime" in p else None
            r = worst(wrong, ref, SF_GRADS, GRAD, e_ref)
            assert all(np.isfinite(v).all() for v in wrong.values()) and r >= MARGIN, (p["id"], mistake, r)
            n += 1
    assert n >= 4


# ---------------------------------------------------------------------------------------------------------------------
# selffed_backward against torch.autograd, fp64, on an ordinary case away from the kinks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act,dact,residual", [("sigmoid", "tanh", True), ("hard_sigmoid", "relu", False)])
def test_selffed_backward_against_autograd(act, dact, residual):
    B, T, H, n_out = 5, 4, 32, 5
    rng = np.random.default_rng(seed_of("autograd " + act))
    K, R, b = (a.astype(np.float64) for a in O.init_lstm(rng, n_out, H))
    W, bd = rng.uniform(-0.5, 0.5, (H, n_out)), rng.uniform(0.05, 0.2, n_out) * np.where(np.arange(n_out) % 2, -1, 1)
    x0, h0, c0 = rng.uniform(-1, 1, (B, n_out)), 0.3 * rng.standard_normal((B, H)), 0.3 * rng.standard_normal((B, H))
    r = rng.uniform(-0.5, 0.5, (B, n_out)) if residual else None
    dloss = rng.standard_normal((T, B, n_out))
    tape = O.selffed_forward(x0, h0, c0, r, K, R, b, W, bd, T, act, dact)
    gates = np.concatenate([tape["z"][..., :2 * H], tape["z"][..., 3 * H:]], -1)
    assert act != "hard_sigmoid" or np.abs(np.abs(gates) - 2.5).min() > 1e-6
    assert dact != "relu" or (np.abs(tape["pre"]).min() > 1e-6 and (tape["A"] == 0).any() and (tape["A"] > 0).any())
    leaf = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    tK, tR, tW, tx, th, tc = leaf(K), leaf(R), leaf(W), leaf(x0), leaf(h0), leaf(c0)
    s = torch.sigmoid if act == "sigmoid" else (lambda v: torch.clamp(0.2 * v + 0.5, 0, 1))
    x, h, c, ys, pres, zs = tx, th, tc, [], [], []
    for _ in range(T):
        z = (torch.tensor(b) + x @ tK) + h @ tR
        c = s(z[:, H:2 * H]) * c + s(z[:, :H]) * torch.tanh(z[:, 2 * H:3 * H])
        h = s(z[:, 3 * H:]) * torch.tanh(c)
        pre = h @ tW + torch.tensor(bd)
        a = torch.tanh(pre) if dact == "tanh" else torch.relu(pre)
        x = a if r is None else a + torch.tensor(r)
        for v in (z, pre, x):
            v.retain_grad()
        ys.append(x); pres.append(pre); zs.append(z)
    np.testing.assert_allclose(torch.stack(ys).detach().numpy(), tape["XA"][1:], rtol=0, atol=1e-13)
    (torch.stack(ys) * torch.tensor(dloss)).sum().backward()
    want = {"DY": np.stack([v.grad.numpy() for v in ys]), "DPRE": np.stack([v.grad.numpy() for v in pres]),
            "DZ": np.stack([v.grad.numpy() for v in zs]), "dx0": tx.grad.numpy(), "dh0": th.grad.numpy(), "dc0": tc.grad.numpy()}
    for a_from_A in ([True, False] if r is None else [True]):
        got = O.selffed_backward(dict(tape, A=tape["A"] if a_from_A else None), dloss, K, R, W, act, dact)
        for k in SF_GRADS:
            np.testing.assert_allclose(got[k], want[k], rtol=1e-11, atol=1e-13, err_msg=k)
    # and the weight gradients that the trainer forms as products over these tapes
    DZ, DPRE = want["DZ"].reshape(T * B, 4 * H), want["DPRE"].reshape(T * B, n_out)
    np.testing.assert_allclose(tape["XA"][:-1].reshape(T * B, n_out).T @ DZ, tK.grad.numpy(), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(tape["Hs"][:-1].reshape(T * B, H).T @ DZ, tR.grad.numpy(), rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(tape["Hs"][1:].reshape(T * B, H).T @ DPRE, tW.grad.numpy(), rtol=1e-11, atol=1e-13)


# ---------------------------------------------------------------------------------------------------------------------
# the guarded views of every case
# ---------------------------------------------------------------------------------------------------------------------
def _check_view(tag, v, a, off):
    m = margin_floats(a.shape)
    row = int(np.prod(a.shape[1:])) if a.ndim > 1 else 1
    assert m >= 1024 and m >= TILE * row, tag
    base = v._base if v._base._base is None else v._base._base
    assert v.storage_offset() >= m and base.numel() - v.storage_offset() - v.numel() >= m, tag
    assert addr(v) == base.data_ptr() + 4 * v.storage_offset() and addr(v) % 16 == 4 * off, tag
    assert bool(torch.isnan(base[:v.storage_offset()]).all()) and bool(torch.isnan(base[v.storage_offset() + v.numel():]).all()), tag
    assert tuple(v.shape) == a.shape and same_bits(v.numpy(), a), tag


def test_guarded_inputs_of_every_case():
    seen = {}
    tables = [(p["id"], stacked_operands(p["w"], p["enc"], p["dec0"], p["L"]), list(STACKED_OUT)) for p in
              [stacked_case(c["id"]) for c in stacked_cases()] + [stacked_regime_case(c) for c in STACKED_REGIME_CASES]]
    for p in [selffed_case(c["id"]) for c in selffed_cases()] + [selffed_regime_case(c) for c in SELFFED_REGIME_CASES]:
        tables.append((p["id"], selffed_operands(p), list(SF_OUT)))
        tables.append((p["id"] + " bwd", {k: dict(p["tape32"], **p)[k] for k in BWD_IN}, list(SF_GRADS)))
    for cid, operands, outputs in tables:
        off = offsets(cid, list(operands) + outputs)          # as the GPU tests ask for them (which also run every case flipped)
        for name, a in operands.items():
            if a is None:
                continue
            cls = name if cid.startswith("selffed") else name.translate({ord(d): None for d in "012"})      # enc0_K, enc1_K: one class
            seen.setdefault((cid.split("-")[0], cls), set()).add(off[name])
            _check_view("%s %s" % (cid, name), view(a, off[name]), np.asarray(a, np.float32), off[name])
    assert all(v == {0, 1} for v in seen.values()), {k: v for k, v in seen.items() if v != {0, 1}}
    for shape in [(17, 0, 6), (3, 17, 64), (0, 17, 1, 5, 32)]:
        for off in ((0, 1) if np.prod(shape) else (0,)):      # a zero-length output stands on the boundary
            o = OutView(shape, off=off)
            m = margin_floats(shape)
            assert o.lo >= m and o.buf.numel() - o.hi >= m and m >= 1024 and o.untouched()
