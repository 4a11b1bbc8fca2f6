"""fov_lstm_stack2_bwd at H = 32 / 64: both layers' BPTT in one launch of stack2_tile_bwd_kernel (one workgroup per 16-sequence
tile; the upper layer's dx handed to the lower one through dz1 itself), then the weight gradients through lstm_seq_wgrad_layers.

Tapes come from ops.lstm_seq_train on seeded inputs.  Two references for dz1, dz2, the four state gradients and the six weight
gradients: an fp64 torch.autograd graph of the two layers on the CPU, and the two-call ops.lstm_seq_bwd path (upper layer first,
its dx as the lower layer's dhs).  Bounds, restated from where they are set:

    against fp64        1e-4 max|ref| + 1e-9 on the worst element    tests/test_gpu_stacked_train.py, every gradient and dz tape of
                                                                    stacked_seq2seq_train_bwd (the same bwd_layer arithmetic)
    against two calls   2e-5 max|ref| + 1e-9                         tests/test_gpu_train.py, the width-512 lstm_stack2_bwd test

Shapes: H in {32, 64}, both recurrent activations, B in {1, 16, 17, 35} (one row, a full tile, a ragged second tile, three tiles
with a ragged last one), T in {1, 2, 5} (no recurrence step, one, several), F in {6, 90}.

hard_sigmoid has kinks at +-2.5, where an fp32 pre-activation may fall on the other side than the fp64 one and the gate's derivative
is then 0.2 against 0: a case asserts on the CPU, in fp64, that no hard_sigmoid pre-activation of either layer lies within 1e-5 of a
kink, and a seed that violates that is passed over for the next one (no element is masked).  1e-5: an fp32 pre-activation of these
layers - a sum of at most 90 + 64 + 1 products of magnitude below one, near 2.5 where an ulp is 2.4e-7 - is within 2e-6 of the fp64
one."""
import contextlib
import functools
import itertools
import os
import re

import numpy as np
import pytest
import torch

import test_gpu_defer_order as DO
from oracle import fov_oracle as O
from test_guarded_views_host import OutView, guarded, same_bits

pytestmark = pytest.mark.gpu

UPS = ("dhs2", "dhT2", "dcT2", "dhT1", "dcT1")
STATES = ("dh0_1", "dc0_1", "dh0_2", "dc0_2")
WGRADS = ("dK1", "dR1", "db1", "dK2", "dR2", "db2")
LAUNCHED = re.compile(r"\[fov trace\] launched: (.+)")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def ptr(t):
    return None if t is None else t.data_ptr()


def wshapes(F, H):
    return {"dK1": (F, 4 * H), "dR1": (H, 4 * H), "db1": (4 * H,), "dK2": (H, 4 * H), "dR2": (H, 4 * H), "db2": (4 * H,)}


class Case:
    """Seeded weights, inputs, initial states, upstream gradients (numpy) and the device tapes with / without initial states."""

    def __init__(self, B, T, F, H, act, attempt=0):
        from longterm360fov_amd import ops
        self.B, self.T, self.F, self.H, self.act = B, T, F, H, act
        rng = np.random.default_rng(100003 * attempt + 1000 * H + 100 * B + 10 * T + F + (act == "hard_sigmoid"))
        self.K1, self.R1, self.b1 = O.init_lstm(rng, F, H, np.float32)
        self.K2, self.R2, self.b2 = O.init_lstm(rng, H, H, np.float32)
        self.b1 = (0.1 * rng.standard_normal(4 * H)).astype(np.float32)
        self.b2 = (0.1 * rng.standard_normal(4 * H)).astype(np.float32)
        self.x = rng.uniform(-1, 1, (B, T, F)).astype(np.float32)
        self.st = {k: (0.3 * rng.standard_normal((B, H))).astype(np.float32) for k in ("h0_1", "c0_1", "h0_2", "c0_2")}
        self.up = {"dhs2": (0.05 * rng.standard_normal((B, T, H))).astype(np.float32)}
        for k in UPS[1:]:
            self.up[k] = (0.1 * rng.standard_normal((B, H))).astype(np.float32)
        self.d = {k: dev(getattr(self, k)) for k in ("x", "K1", "R1", "b1", "K2", "R2", "b2")}
        self.dst = {k: dev(v) for k, v in self.st.items()}
        self.dup = {k: dev(v) for k, v in self.up.items()}
        self.tapes = {}
        for state in (False, True):
            s = self.dst if state else dict.fromkeys(self.st)
            if B and T:
                hs1, _, _, res1 = ops.lstm_seq_train(self.d["x"], self.d["K1"], self.d["R1"], self.d["b1"], s["h0_1"], s["c0_1"], act=act)
                hs2, _, _, res2 = ops.lstm_seq_train(hs1, self.d["K2"], self.d["R2"], self.d["b2"], s["h0_2"], s["c0_2"], act=act)
            else:
                hs1 = hs2 = torch.empty((B, T, H), device="cuda")
                res1 = res2 = torch.empty((B, T, 5, H), device="cuda")
            self.tapes[state] = (hs1, res1, hs2, res2)

    def rows(self, lo, hi):
        """The same problem restricted to the sequences lo .. hi - 1 (tapes sliced, not recomputed)."""
        c = object.__new__(Case)
        c.B, c.T, c.F, c.H, c.act = hi - lo, self.T, self.F, self.H, self.act
        c.d = dict(self.d, x=self.d["x"][lo:hi].contiguous())
        c.dst = {k: v[lo:hi].contiguous() for k, v in self.dst.items()}
        c.dup = {k: v[lo:hi].contiguous() for k, v in self.dup.items()}
        c.tapes = {s: tuple(t[lo:hi].contiguous() for t in tp) for s, tp in self.tapes.items()}
        return c


def entry(c, state, ups, out, accumulate=0, scratch=None, tapes=None):
    """fov_lstm_stack2_bwd through the library with caller-owned outputs: out = {name: tensor or None} over dz1, dz2, WGRADS, STATES."""
    from longterm360fov_amd import _lib, ops
    L = _lib.lib()
    hs1, res1, hs2, res2 = tapes or c.tapes[state]
    s = c.dst if state else dict.fromkeys(c.dst)
    u = {k: (c.dup[k] if k in ups else None) for k in UPS}
    buf = (scratch or ops.Scratch()).get(L.fov_lstm_stack2_bwd_workspace_bytes(c.B, c.T, c.F, c.H), torch.device("cuda", torch.cuda.current_device()))
    ops.check(L.fov_lstm_stack2_bwd(ptr(c.d["x"]), ptr(c.d["R1"]), ptr(c.d["K2"]), ptr(c.d["R2"]), ptr(s["h0_1"]), ptr(s["c0_1"]),
                                    ptr(s["h0_2"]), ptr(s["c0_2"]), ptr(hs1), ptr(res1), ptr(hs2), ptr(res2), *[ptr(u[k]) for k in UPS],
                                    ptr(out.get("dz1")), ptr(out.get("dz2")), *[ptr(out.get(k)) for k in WGRADS],
                                    *[ptr(out.get(k)) for k in STATES], c.B, c.T, c.F, c.H, ops.act_code(c.act), int(accumulate),
                                    buf.data_ptr(), buf.numel(), ops._stream()))
    return out


def fresh(c, wgrads=True, states=True, base=None):
    e = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    out = {"dz1": e(c.B, c.T, 4 * c.H), "dz2": e(c.B, c.T, 4 * c.H)}
    if wgrads:
        for k, s in wshapes(c.F, c.H).items():
            out[k] = e(*s) if base is None else base[k].clone()
    if states:
        for k in STATES:
            out[k] = e(c.B, c.H)
    return out


def two_calls(c, state, ups):
    from longterm360fov_amd import ops
    hs1, res1, hs2, res2 = c.tapes[state]
    s = c.dst if state else dict.fromkeys(c.dst)
    u = {k: (c.dup[k] if k in ups else None) for k in UPS}
    sc = ops.Scratch()
    e2 = ops.lstm_seq_bwd(hs1, c.d["K2"], c.d["R2"], hs2, res2, h0=s["h0_2"], c0=s["c0_2"], dhs=u["dhs2"], dhT=u["dhT2"], dcT=u["dcT2"],
                          need_dx=True, need_state_grads=True, act=c.act, scratch=sc)
    e1 = ops.lstm_seq_bwd(c.d["x"], c.d["K1"], c.d["R1"], hs1, res1, h0=s["h0_1"], c0=s["c0_1"], dhs=e2["dx"], dhT=u["dhT1"], dcT=u["dcT1"],
                          need_state_grads=True, act=c.act, scratch=sc)
    return {"dz1": e1["dz"], "dz2": e2["dz"], "dK1": e1["dK"], "dR1": e1["dR"], "db1": e1["db"], "dK2": e2["dK"], "dR2": e2["dR"],
            "db2": e2["db"], "dh0_1": e1["dh0"], "dc0_1": e1["dc0"], "dh0_2": e2["dh0"], "dc0_2": e2["dc0"]}


def graph64(c, state):
    """The two layers as an fp64 torch graph on the CPU -> (weights, initial states, pre-activations of both layers, what the
    upstream gradients multiply, distance of the nearest hard_sigmoid pre-activation from its kinks at +-2.5)."""
    t = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), requires_grad=g)
    B, T, H = c.B, c.T, c.H
    w = {k: t(getattr(c, k), True) for k in ("K1", "R1", "b1", "K2", "R2", "b2")}
    s0 = {k: t(c.st[k] if state else np.zeros((B, H)), True) for k in c.st}
    rec = (lambda z: torch.clamp(0.2 * z + 0.5, 0.0, 1.0)) if c.act == "hard_sigmoid" else torch.sigmoid

    def layer(xs, K, R, b, h, cc):
        hs, zs = [], []
        for step in range(T):
            z = xs[step] @ K + h @ R + b
            z.retain_grad()
            zs.append(z)
            i, f, g, o = rec(z[:, :H]), rec(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), rec(z[:, 3 * H:])
            cc = f * cc + i * g
            h = o * torch.tanh(cc)
            hs.append(h)
        return hs, zs, h, cc

    x = t(c.x)
    hs1, z1, hT1, cT1 = layer([x[:, i] for i in range(T)], w["K1"], w["R1"], w["b1"], s0["h0_1"], s0["c0_1"])
    hs2, z2, hT2, cT2 = layer(hs1, w["K2"], w["R2"], w["b2"], s0["h0_2"], s0["c0_2"])
    top = {"dhs2": torch.stack(hs2, 1), "dhT2": hT2, "dcT2": cT2, "dhT1": hT1, "dcT1": cT1}
    margin = np.inf
    if c.act == "hard_sigmoid":
        for z in z1 + z2:
            zz = z.detach().numpy()
            margin = min(margin, float(np.abs(np.abs(np.concatenate([zz[:, :2 * H], zz[:, 3 * H:]], 1)) - 2.5).min()))
    return w, s0, z1, z2, top, margin


def autograd64(c, state, ups):
    """torch.autograd through graph64 with the upstream gradients `ups`; dz is the gradient at the gates' pre-activations."""
    w, s0, z1, z2, top, _ = graph64(c, state)
    loss = sum((top[k] * torch.tensor(c.up[k].astype(np.float64))).sum() for k in ups)
    loss.backward()
    zero = lambda a: np.zeros(tuple(a.shape)) if a.grad is None else a.grad.numpy()
    r = {"dz1": np.stack([zero(z) for z in z1], 1), "dz2": np.stack([zero(z) for z in z2], 1)}
    for k in w:
        r["d" + k] = zero(w[k])
    for k in s0:
        r["d" + k] = zero(s0[k])
    return r


KINK_MARGIN = 1e-5


@functools.lru_cache(maxsize=8)
def case(B, T, F, H, act):
    """The first seed of the shape whose fp64 hard_sigmoid pre-activations, with and without initial states, keep KINK_MARGIN away
    from +-2.5 (the module's docstring); sigmoid: the first seed."""
    for attempt in range(16):
        c = Case(B, T, F, H, act, attempt)
        if min(graph64(c, s)[5] for s in (False, True)) > KINK_MARGIN:
            return c
    raise AssertionError("a hard_sigmoid pre-activation within %g of +-2.5 in 16 seeds" % KINK_MARGIN)


def near(got, ref, rel, tag):
    ref = f64(ref) if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    got = f64(got)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    print("%-60s max|ref| %.3e err %.3e bound %.3e" % (tag, scale, err, rel * scale + 1e-9))
    assert err <= rel * scale + 1e-9, (tag, err, scale)


VARIANTS = [(True, UPS), (False, UPS)] + [(True, (k,)) for k in UPS]


@pytest.mark.parametrize("H,act,B,T,F", list(itertools.product((32, 64), ("sigmoid", "hard_sigmoid"), (1, 16, 17, 35), (1, 2, 5), (6, 90))))
def test_one_launch_against_fp64_autograd_and_the_two_call_path(H, act, B, T, F):
    """With and without initial states, each upstream gradient alone and all five together (accumulate = 0); then accumulate = 1
    onto a random base, and the data path alone (no dK / dR / db, no state gradients: same dz bits)."""
    c = case(B, T, F, H, act)
    tag = "H%d %s B%d T%d F%d" % (H, act, B, T, F)
    for state, ups in VARIANTS:
        got = entry(c, state, ups, fresh(c))
        ref, two = autograd64(c, state, ups), two_calls(c, state, ups)
        for k in got:
            v = "%s state=%d ups=%s %s" % (tag, state, "+".join(ups), k)
            near(got[k], ref[k], 1e-4, v + " / fp64")
            near(got[k], two[k], 2e-5, v + " / two calls")
    state, ups = True, UPS
    first = entry(c, state, ups, fresh(c))
    rng = np.random.default_rng(5)
    base = {k: dev(rng.uniform(-1, 1, s)) for k, s in wshapes(F, H).items()}
    acc = entry(c, state, ups, fresh(c, base=base), accumulate=1)
    for k in WGRADS:
        ref = f64(base[k]) + f64(first[k])
        near(acc[k], ref, 2e-5, "%s accumulate %s" % (tag, k))
    for k in ("dz1", "dz2") + STATES:
        assert torch.equal(acc[k], first[k]), k
    data = entry(c, state, ups, fresh(c, wgrads=False, states=False))
    assert torch.equal(data["dz1"], first["dz1"]) and torch.equal(data["dz2"], first["dz2"])


@pytest.mark.parametrize("H,act,B,T,F,off", [(32, "sigmoid", 35, 5, 6, 0), (64, "hard_sigmoid", 17, 2, 90, 0), (32, "hard_sigmoid", 17, 1, 90, 0),
                                             (64, "sigmoid", 35, 5, 6, 1)])
def test_guarded_views_twice_and_the_weight_gradients_of_the_entrys_own_tapes(H, act, B, T, F, off):
    """Every operand inside a NaN buffer, every output inside a sentinel buffer (dz1, which carries the hand-off, included), the
    last tile ragged: nothing beyond B is read into a result or written, nothing is left unwritten; a second launch repeats the
    first bit for bit; dK / dR / db are the bits of ops.lstm_seq_wgrad_layers on the dz tapes the entry wrote.  off = 1: every view
    4 bytes off 16-byte alignment."""
    from longterm360fov_amd import ops
    c = case(B, T, F, H, act)
    g = lambda t: guarded(t.cpu().numpy(), off, device="cuda")
    v = object.__new__(Case)
    v.B, v.T, v.F, v.H, v.act = B, T, F, H, act
    v.d = {k: g(t) for k, t in c.d.items()}
    v.dst = {k: g(t) for k, t in c.dst.items()}
    v.dup = {k: g(t) for k, t in c.dup.items()}
    tapes = tuple(g(t) for t in c.tapes[True])
    views = {"dz1": OutView((B, T, 4 * H), None, off, device="cuda"), "dz2": OutView((B, T, 4 * H), None, off, device="cuda")}
    for k, s in wshapes(F, H).items():
        views[k] = OutView(s, None, off, device="cuda", row=s[-1])
    for k in STATES:
        views[k] = OutView((B, H), None, off, device="cuda")
    sc = ops.Scratch()
    runs = []
    for rep in range(2):
        for o in views.values():
            o.reset()
        entry(v, True, UPS, {k: o.v for k, o in views.items()}, scratch=sc, tapes=tapes)
        runs.append({k: o.result() for k, o in views.items()})
    for k in views:
        assert same_bits(runs[0][k], runs[1][k]), k
    plain = entry(c, True, UPS, fresh(c))
    for k in views:      # (misaligned gradients leave the rows form for the per-layer products: another summation order)
        if off == 0 or k not in WGRADS:
            assert same_bits(runs[0][k], plain[k].cpu().numpy()), k
        else:
            near(torch.from_numpy(runs[0][k]), plain[k], 2e-5, "guarded, misaligned %s / aligned" % k)
    ref = autograd64(c, True, UPS)
    for k in views:
        near(torch.from_numpy(runs[0][k]), ref[k], 1e-4, "guarded H%d B%d T%d %s" % (H, B, T, k))
    # the weight gradients from the entry's own tapes
    hs1, _, hs2, _ = c.tapes[True]
    w = {k: torch.full(s, float("nan"), device="cuda") for k, s in wshapes(F, H).items()}
    ops.lstm_seq_wgrad_layers([(c.d["x"], hs1, c.dst["h0_1"], plain["dz1"], w["dK1"], w["dR1"], w["db1"]),
                               (hs1, hs2, c.dst["h0_2"], plain["dz2"], w["dK2"], w["dR2"], w["db2"])], scratch=ops.Scratch())
    for k in WGRADS:
        assert torch.equal(w[k], plain[k]), k


@pytest.mark.parametrize("H,act", [(32, "sigmoid"), (64, "hard_sigmoid")])
def test_rows_of_the_second_tile_alone_give_the_same_bits(H, act):
    """Rows 16 .. 18 of the B = 35 case as a batch of three: dz and the state gradients of a sequence do not depend on its
    tile-mates or on its place in the batch."""
    c = case(35, 5, 6, H, act)
    full = entry(c, True, UPS, fresh(c, wgrads=False))
    part = entry(c.rows(16, 19), True, UPS, fresh(c.rows(16, 19), wgrads=False))
    for k in ("dz1", "dz2") + STATES:
        assert torch.equal(part[k], full[k][16:19]), k


@pytest.mark.parametrize("H,B,T", [(32, 17, 0), (64, 0, 3), (32, 0, 0)])
def test_empty_calls_zero_the_gradients_and_pass_the_state_gradients_through(H, B, T):
    """T = 0 or B = 0, as the header says: accumulate = 0 zeroes dK / dR / db, accumulate = 1 leaves them; dh0 / dc0 of each layer are
    its dhT / dcT, or zero where none is given."""
    F = 6
    c = Case(B, T, F, H, "sigmoid")
    base = {k: dev(np.full(s, 3.0, np.float32)) for k, s in wshapes(F, H).items()}
    out = entry(c, False, ("dhT2", "dcT1"), fresh(c, base=base), accumulate=1)
    for k in WGRADS:
        assert torch.equal(out[k], base[k]), k
    out = entry(c, False, ("dhT2", "dcT1"), fresh(c, base=base), accumulate=0)
    for k in WGRADS:
        assert float(out[k].abs().max()) == 0.0, k
    if B:
        assert torch.equal(out["dh0_2"], c.dup["dhT2"]) and torch.equal(out["dc0_1"], c.dup["dcT1"])
        assert float(out["dc0_2"].abs().max()) == 0.0 and float(out["dh0_1"].abs().max()) == 0.0


@contextlib.contextmanager
def trace_on():
    from longterm360fov_amd import ops
    before = os.environ.get("FOV_DBG_TRACE")
    os.environ["FOV_DBG_TRACE"] = "1"
    ops._sync_env()
    try:
        yield
        torch.cuda.synchronize()
    finally:
        os.environ.pop("FOV_DBG_TRACE", None) if before is None else os.environ.__setitem__("FOV_DBG_TRACE", before)
        ops._sync_env()


@pytest.mark.parametrize("H", [32, 64])
def test_the_launches_are_the_tile_kernel_and_the_planned_weight_gradient_form(capfd, H):
    """Few rows: one recurrence launch and one wgrad_rows launch for all six gradients.  B T beyond the rows form (640 rows): the
    tile launch, then each layer's products - no wgrad_rows, no host-stepped pointwise launch."""
    c = Case(17, 5, 6, H, "sigmoid")
    capfd.readouterr()
    with trace_on():
        entry(c, True, UPS, fresh(c))
    assert LAUNCHED.findall(capfd.readouterr().err) == ["two-layer tile BPTT", "wgrad_rows"]
    c = Case(130, 5, 6, H, "sigmoid")
    with trace_on():
        got = entry(c, True, UPS, fresh(c))
    names = LAUNCHED.findall(capfd.readouterr().err)
    assert names[0] == "two-layer tile BPTT" and names.count("two-layer tile BPTT") == 1 and len(names) > 1, names
    assert "wgrad_rows" not in names and "lstm_bwd_pointwise" not in names, names
    two = two_calls(c, True, UPS)
    for k in got:
        near(got[k], two[k], 2e-5, "H%d B130 %s / two calls" % (H, k))


arena = DO.arena


@pytest.mark.parametrize("H,acc", [(32, 1), (32, 0), (64, 1)])
def test_a_pending_split_product_stays_in_front_of_the_direct_writes(arena, capfd, H, acc):
    """Inside a reduce_defer region, after a pending split product over db of the lower layer and dR of the upper one, the entry's
    results are the bits of the run without a region (tests/test_gpu_defer_order.py's pattern)."""
    c = Case(17, 5, 6, H, "sigmoid")
    F = c.F
    layout = DO.Layout([wshapes(F, H)[k] for k in WGRADS])
    rng = np.random.default_rng(41 + acc)
    pending = {i: DO.Pending(rng, layout.shapes[i]) for i in (2, 4)}
    hs1, _, hs2, _ = c.tapes[True]

    def writer(v, a, sc):
        out = fresh(c, wgrads=False)
        out.update(zip(WGRADS, v))
        r = entry(c, True, UPS, out, accumulate=a)
        return [r["dz1"], r["dz2"]]

    ref = lambda out: (DO._lstm_wgrad_ref(c.x, f64(hs1), c.st["h0_1"], f64(out[0])) +
                       DO._lstm_wgrad_ref(f64(hs1), f64(hs2), c.st["h0_2"], f64(out[1])))
    DO._check(layout, pending, writer, ref, acc, arena, 2e-5, capfd, "two-layer tile BPTT")
