"""In-stream order inside a deferred-reduction region (fov_reduce_defer_begin / _flush / _end), for every weight-gradient writer.

Between _begin and _end a split product over the flat gradient buffer leaves its partial slices in the arena and its reduce is
pending.  include/fov360.h promises that a later write through the library over a pending range flushes first, so the results
are bit-identical to the same calls with no region open.  Each case below:
  1. lays the outputs of the writer under test, E, out as 16-byte-aligned views of one flat buffer (the few-row kernels take
     aligned outputs only);
  2. opens a region, issues a pending split product P over (part of) E's outputs and checks that the range still reads zero
     (the record really is pending);
  3. calls E with accumulate = 1 or 0, closes the region;
  4. asserts bit-for-bit equality with the same sequence run with no region open, and closeness to an fp64 reference:
     P + E for accumulate = 1, E for accumulate = 0.
A writer that stores without flushing loses its contribution (accumulate = 1) or is overwritten by P (accumulate = 0): an O(1)
relative error.  The optimizers are readers: they must see the reduced gradient.  The last test pins the empty-batch rule:
accumulate = 0 zeroes the weight gradients, accumulate = 1 leaves them unchanged."""
import os

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

pytestmark = pytest.mark.gpu

NP = 5120                 # rows of the pending product: long enough to split into slices
ARENA_FLOATS = 64 << 20   # 256 MiB


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def arena():
    return torch.empty(ARENA_FLOATS, dtype=torch.float32, device="cuda")


class Layout:
    """Views of one flat fp32 buffer, each at a 16-byte-aligned offset (plus `shift` floats: 4-byte misaligned)."""

    def __init__(self, shapes, shift=0):
        self.shapes = [tuple(s) for s in shapes]
        self.offs, o = [], 4 + shift
        for s in self.shapes:
            self.offs.append(o)
            o += (int(np.prod(s)) + 7) // 4 * 4          # a gap of at least one float between views
        self.total = o + 4

    def new(self):
        flat = torch.zeros(self.total, dtype=torch.float32, device="cuda")
        return flat, [flat[o:o + int(np.prod(s))].view(*s) for o, s in zip(self.offs, self.shapes)]


class Pending:
    """The split product P over one view: [x]^T dz (wgrad_fused) for a matrix view, column sums (colsum) for a vector."""

    def __init__(self, rng, shape):
        self.shape = shape
        cols = shape[-1]
        rows = int(np.prod(shape)) // cols
        self.dz = (0.1 * rng.uniform(-1, 1, (NP, cols))).astype(np.float32)
        self.x = None if len(shape) == 1 else (0.1 * rng.uniform(-1, 1, (NP, rows))).astype(np.float32)
        self.tdz, self.tx = dev(self.dz), None if self.x is None else dev(self.x)

    def issue(self, view, sc):
        from longterm360fov_amd import ops
        if self.x is None:
            ops.colsum(self.tdz, out=view, scratch=sc)
        else:
            ops.wgrad_fused(self.tx, None, self.tdz, view.view(self.x.shape[1], self.dz.shape[1]), bias=False, scratch=sc)

    def ref(self):
        if self.x is None:
            return self.dz.astype(np.float64).sum(0)
        return (self.x.astype(np.float64).T @ self.dz.astype(np.float64)).reshape(self.shape)


def _sequence(layout, pending, writer, acc, arena=None):
    """P over the views in `pending` ({index: Pending}), then E = writer(views, acc, scratch); in a region if `arena` is given."""
    from longterm360fov_amd import ops
    flat, views = layout.new()
    sc = ops.Scratch()
    if arena is not None:
        ops.reduce_defer_begin(flat, arena)
    try:
        for i, p in pending.items():
            p.issue(views[i], sc)
        if arena is not None:
            torch.cuda.synchronize()
            for i in pending:
                assert float(views[i].abs().max()) == 0.0, "the product over view %d was not deferred: the case tests nothing" % i
        out = writer(views, acc, sc)
    finally:
        if arena is not None:
            ops.reduce_defer_end(flat)
    torch.cuda.synchronize()
    return flat, views, out


def _check(layout, pending, writer, ref_fn, acc, arena, rel, capfd=None, trace=None, no_trace=()):
    """Region vs no region bit for bit; against fp64: P + E (acc) or E.  ref_fn(out) -> fp64 arrays of E's outputs, where `out`
    is what the no-region writer returned (its data-path outputs, e.g. the dz tape E's weight gradients are formed from)."""
    from longterm360fov_amd import ops
    flat0, views0, out0 = _sequence(layout, pending, writer, acc)
    if trace is not None or no_trace:
        capfd.readouterr()
        os.environ["FOV_DBG_TRACE"] = "1"
    try:
        flat1, views1, out1 = _sequence(layout, pending, writer, acc, arena)
    finally:
        if trace is not None or no_trace:
            del os.environ["FOV_DBG_TRACE"]
            ops.Scratch().get(256, flat0.device)       # (the library re-reads its knobs)
    err = capfd.readouterr().err if (trace is not None or no_trace) else ""
    if out0 is not None:
        for a, b in zip(out0, out1):
            assert torch.equal(a, b)
    refs = ref_fn(out0)
    for i, (got, r) in enumerate(zip(views1, refs)):
        want = r + (pending[i].ref() if (acc and i in pending) else 0.0)
        e = np.abs(f64(got) - want).max()
        assert e <= rel * np.abs(want).max() + 1e-5, (i, float(e), float(np.abs(want).max()))
    assert torch.equal(flat0, flat1), "a pending reduce and a direct write were reordered"
    if trace is not None:          # the form under test was the one taken
        assert trace in err, err
    for t in no_trace:
        assert t not in err, err


# ---------------------------------------------------------------------------------------------------------------------
# LSTM weight gradients: dK = x^T dz, dR = h_{t-1}^T dz (h_{-1} = h0 or 0), db = column sums of dz
# ---------------------------------------------------------------------------------------------------------------------
def _lstm_wgrad_ref(x, hs, h0, dz):
    x, hs, dz = (np.asarray(a, np.float64) for a in (x, hs, dz))
    B, H = hs.shape[0], hs.shape[-1]
    hp = np.concatenate([(np.zeros((B, H)) if h0 is None else np.asarray(h0, np.float64))[:, None], hs[:, :-1]], 1)
    return [np.einsum("btf,btn->fn", x, dz), np.einsum("bth,btn->hn", hp, dz), dz.sum((0, 1))]


# (B, T, F, H, views P covers, accumulate, misaligned, trace expected / traces that must be absent)
WGRAD_CASES = [
    pytest.param(32, 10, 90, 256, (0, 1, 2), 1, 0, "wgrad_rows: 2 problems", (), id="rows-acc1"),
    pytest.param(32, 10, 90, 256, (0, 1, 2), 0, 0, "wgrad_rows: 2 problems", (), id="rows-acc0"),
    pytest.param(32, 10, 90, 256, (1,), 1, 0, "wgrad_rows: 2 problems", (), id="rows-dR-only-acc1"),
    pytest.param(32, 10, 90, 256, (2,), 0, 0, "wgrad_rows: 2 problems", (), id="rows-bias-only-acc0"),
    pytest.param(32, 10, 90, 512, (0, 1, 2), 1, 0, "M tiles 2", (), id="rows-H512-acc1"),
    pytest.param(32, 10, 90, 512, (1,), 0, 0, "M tiles 2", (), id="rows-H512-dR-only-acc0"),
    pytest.param(48, 16, 90, 512, (0, 1, 2), 1, 0, "wgrad_group: 2 problems", ("wgrad_rows",), id="grouped-acc1"),
    pytest.param(48, 16, 90, 512, (0, 1, 2), 0, 0, "wgrad_group: 2 problems", ("wgrad_rows",), id="grouped-acc0"),
    pytest.param(48, 16, 90, 512, (2,), 1, 0, "wgrad_group: 2 problems", ("wgrad_rows",), id="grouped-bias-only-acc1"),
    pytest.param(64, 20, 90, 256, (0, 1, 2), 1, 0, None, ("wgrad_rows", "wgrad_group"), id="split-control-acc1"),
    pytest.param(64, 20, 90, 256, (0, 1, 2), 0, 0, None, ("wgrad_rows", "wgrad_group"), id="split-control-acc0"),
    pytest.param(32, 10, 90, 256, (0, 1, 2), 1, 1, None, ("wgrad_rows", "wgrad_group"), id="misaligned-control-acc1"),
    pytest.param(32, 10, 90, 256, (0, 1, 2), 0, 1, None, ("wgrad_rows", "wgrad_group"), id="misaligned-control-acc0"),
]


@pytest.mark.parametrize("B,T,F,H,cover,acc,shift,trace,no_trace", WGRAD_CASES)
def test_lstm_seq_wgrad_keeps_order(arena, capfd, B, T, F, H, cover, acc, shift, trace, no_trace):
    """fov_lstm_seq_wgrad in its few-row forms (wgrad_rows_kernel: 16 x 64 tiles, 32 x 64 at H = 512; wgrad_group_kernel) and,
    as controls, its split-product form (many rows, or outputs 4 bytes off 16-byte alignment)."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(B * 1000 + H + 7 * acc + len(cover))
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
    x, hs, dz, h0 = u(B, T, F), u(B, T, H), u(B, T, 4 * H), u(B, H)
    tx, ths, tdz, th0 = dev(x), dev(hs), dev(dz), dev(h0)
    layout = Layout([(F, 4 * H), (H, 4 * H), (4 * H,)], shift)
    pending = {i: Pending(rng, layout.shapes[i]) for i in cover}

    def writer(v, a, sc):
        ops.lstm_seq_wgrad(tx, ths, tdz, dK=v[0], dR=v[1], db=v[2], h0=th0, accumulate=bool(a), scratch=sc)

    _check(layout, pending, writer, lambda _: _lstm_wgrad_ref(x, hs, h0, dz), acc, arena, 2e-5, capfd, trace, no_trace)


@pytest.mark.parametrize("acc", [1, 0])
def test_lstm_seq_wgrad_pair_keeps_order(arena, capfd, acc):
    """fov_lstm_seq_wgrad_pair at the reference's batch: all six gradients of an encoder / decoder pair in one launch."""
    from longterm360fov_amd import ops
    B, T1, T2, F1, F2, H = 32, 10, 10, 90, 6, 256
    assert ops.lstm_seq_wgrad_pair_one_launch(B, T1, T2, H)
    rng = np.random.default_rng(11 + acc)
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
    x1, hs1, dz1 = u(B, T1, F1), u(B, T1, H), u(B, T1, 4 * H)
    x2, hs2, dz2, h02 = u(B, T2, F2), u(B, T2, H), u(B, T2, 4 * H), u(B, H)
    t1 = (dev(x1), dev(hs1), None, dev(dz1))
    t2 = (dev(x2), dev(hs2), dev(h02), dev(dz2))
    layout = Layout([(F1, 4 * H), (H, 4 * H), (4 * H,), (F2, 4 * H), (H, 4 * H), (4 * H,)])
    pending = {i: Pending(rng, layout.shapes[i]) for i in (1, 5)}      # dR of the encoder, db of the decoder

    def writer(v, a, sc):
        ops.lstm_seq_wgrad_pair(t1 + tuple(v[:3]), t2 + tuple(v[3:]), accumulate=bool(a), scratch=sc)

    ref = lambda _: _lstm_wgrad_ref(x1, hs1, None, dz1) + _lstm_wgrad_ref(x2, hs2, h02, dz2)
    _check(layout, pending, writer, ref, acc, arena, 2e-5, capfd, "wgrad_rows: 4 problems")


@pytest.mark.parametrize("cover,acc", [((0, 1, 2), 1), ((0, 1, 2), 0), ((0,), 1)])
def test_lstm_seq_bwd_keeps_order(arena, capfd, cover, acc):
    """fov_lstm_seq_bwd at the reference's batch: its weight gradients come from wgrad_rows_kernel behind the recurrence."""
    from longterm360fov_amd import ops
    B, T, F, H = 32, 10, 90, 256
    rng = np.random.default_rng(21 + acc + len(cover))
    K, R, b = O.init_lstm(rng, F, H, np.float32)
    x = rng.uniform(-1, 1, (B, T, F)).astype(np.float32)
    tx, tK, tR = dev(x), dev(K), dev(R)
    hs, _, _, res = ops.lstm_seq_train(tx, tK, tR, dev(b), act="sigmoid")
    dhs = dev((0.05 * rng.standard_normal((B, T, H))).astype(np.float32))
    dhT = dev((0.1 * rng.standard_normal((B, H))).astype(np.float32))
    layout = Layout([(F, 4 * H), (H, 4 * H), (4 * H,)])
    pending = {i: Pending(rng, layout.shapes[i]) for i in cover}

    def writer(v, a, sc):
        ws = ops.Scratch()          # (the BPTT kernel's workspace: its status word is checked)
        r = ops.lstm_seq_bwd(tx, tK, tR, hs, res, dhs=dhs, dhT=dhT, dK=v[0], dR=v[1], db=v[2], act="sigmoid", accumulate=bool(a),
                             scratch=ws)
        ws.check()
        return [r["dz"]]

    ref = lambda out: _lstm_wgrad_ref(x, f64(hs), None, f64(out[0]))
    _check(layout, pending, writer, ref, acc, arena, 2e-5, capfd, "wgrad_rows: 2 problems")


@pytest.mark.parametrize("acc", [1, 0])
def test_lstm_stack2_bwd_keeps_order(arena, capfd, acc):
    """fov_lstm_stack2_bwd (two width-512 layers in one BPTT launch): both layers' weight gradients from one wgrad_rows launch."""
    from longterm360fov_amd import ops
    B, T, F, H = 16, 8, 90, 512
    if not ops.lstm_stack2_bwd_supported(B, T, F, H):
        pytest.skip("needs 3 x 16 workgroups per tile resident")
    rng = np.random.default_rng(31 + acc)
    K1, R1, b1 = O.init_lstm(rng, F, H, np.float32)
    K2, R2, b2 = O.init_lstm(rng, H, H, np.float32)
    x = rng.uniform(-1, 1, (B, T, F)).astype(np.float32)
    tx, l1, l2 = dev(x), (dev(K1), dev(R1)), (dev(K2), dev(R2))
    hs1, _, _, res1 = ops.lstm_seq_train(tx, l1[0], l1[1], dev(b1), act="sigmoid")
    hs2, _, _, res2 = ops.lstm_seq_train(hs1, l2[0], l2[1], dev(b2), act="sigmoid")
    dhs2 = dev((0.05 * rng.standard_normal((B, T, H))).astype(np.float32))
    dhT2 = dev((0.1 * rng.standard_normal((B, H))).astype(np.float32))
    layout = Layout([(F, 4 * H), (H, 4 * H), (4 * H,), (H, 4 * H), (H, 4 * H), (4 * H,)])
    pending = {i: Pending(rng, layout.shapes[i]) for i in (2, 4)}      # db of the lower layer, dR of the upper one

    def writer(v, a, sc):
        ws = ops.Scratch()
        r = ops.lstm_stack2_bwd(tx, l1, l2, (hs1, res1, None, None), (hs2, res2, None, None), dhs2=dhs2, dhT2=dhT2,
                                grads1=tuple(v[:3]), grads2=tuple(v[3:]), act="sigmoid", accumulate=bool(a), scratch=ws)
        ws.check()
        return [r["dz1"], r["dz2"]]

    ref = lambda out: _lstm_wgrad_ref(x, f64(hs1), None, f64(out[0])) + _lstm_wgrad_ref(f64(hs1), f64(hs2), None, f64(out[1]))
    _check(layout, pending, writer, ref, acc, arena, 2e-5, capfd, "M tiles 2")


# ---------------------------------------------------------------------------------------------------------------------
# convolution weight gradients
# ---------------------------------------------------------------------------------------------------------------------
def _conv_wgrad_ref(x, dy, k, dil):
    """dw[u, v, c, n] = sum x[b, y + (u - k//2) dil, x + (v - k//2) dil, c] dy[b, y, x, n] ('same' padding, zeros outside)."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    B, H, W, C = x.shape
    r = k // 2
    pad = np.zeros((B, H + 2 * r * dil, W + 2 * r * dil, C))
    pad[:, r * dil:r * dil + H, r * dil:r * dil + W] = x
    dw = np.zeros((k, k, C, dy.shape[-1]))
    for a in range(k):
        for c in range(k):
            xs = pad[:, a * dil:a * dil + H, c * dil:c * dil + W]
            dw[a, c] = np.einsum("byxc,byxn->cn", xs, dy)
    return dw


@pytest.mark.parametrize("dil,acc", [(1, 0), (2, 0), (1, 1), (2, 1)], ids=["lines-acc0", "taps-acc0", "lines-acc1", "taps-acc1"])
def test_conv2d_wgrad_keeps_order(arena, dil, acc):
    """fov_conv2d_wgrad (conv_wgrad_lines form) and fov_conv2d_dilated_wgrad (tap-wise form): one map of 16 x 16 pixels leaves a
    single slice, so accumulate = 0 stores straight into dw.  accumulate = 1 goes through a reduce (control)."""
    from longterm360fov_amd import ops
    B, H, W, C, N, k = 1, 16, 16, 8, 16, 3
    rng = np.random.default_rng(41 + dil + 10 * acc)
    x, dy = rng.uniform(-1, 1, (B, H, W, C)).astype(np.float32), rng.uniform(-1, 1, (B, H, W, N)).astype(np.float32)
    tx, tdy = dev(x), dev(dy)
    layout = Layout([(k, k, C, N)])
    pending = {0: Pending(rng, layout.shapes[0])}

    def writer(v, a, sc):
        ops.conv2d_wgrad(tx, tdy, k, k, dw=v[0], accumulate=bool(a), scratch=sc, dilation=dil)

    _check(layout, pending, writer, lambda _: [_conv_wgrad_ref(x, dy, k, dil)], acc, arena, 2e-5)


# ---------------------------------------------------------------------------------------------------------------------
# the fused heads
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acc", [1, 0])
def test_mlp_head_bwd_keeps_order(arena, acc):
    """fov_mlp_head_bwd on lstm.py's mixture head (400 -> 64 -> 128 -> 256 -> 200, batch 32): gW / gb of four layers."""
    from longterm360fov_amd import ops
    B, dims = 32, [400, 64, 128, 256, 200]
    rng = np.random.default_rng(51 + acc)
    Ws = [(rng.standard_normal((dims[l], dims[l + 1])) / np.sqrt(dims[l])).astype(np.float32) for l in range(4)]
    bs = [(0.1 * rng.standard_normal(dims[l + 1])).astype(np.float32) for l in range(4)]
    h = rng.standard_normal((B, dims[0])).astype(np.float32)
    dlast = rng.standard_normal((B, dims[4])).astype(np.float32)
    layers = [(dev(Ws[l]), dev(bs[l]), "relu" if l < 3 else None) for l in range(4)]
    th, tdl = dev(h), dev(dlast)
    acts = ops.mlp_head_fwd(th, layers)
    shapes = []
    for l in range(4):
        shapes += [(dims[l], dims[l + 1]), (dims[l + 1],)]
    layout = Layout(shapes)
    pending = {i: Pending(rng, layout.shapes[i]) for i in (0, 7)}      # the first layer's W, the last layer's b

    def writer(v, a, sc):
        ops.mlp_head_bwd(th, layers, acts, tdl, v[0::2], v[1::2], need_dx=False, accumulate=bool(a), scratch=sc)

    def ref(_):
        tW = [torch.tensor(w.astype(np.float64), requires_grad=True) for w in Ws]
        tb = [torch.tensor(b.astype(np.float64), requires_grad=True) for b in bs]
        a = torch.tensor(h.astype(np.float64))
        for l in range(4):
            a = a @ tW[l] + tb[l]
            if l < 3:
                a = torch.relu(a)
        (a * torch.tensor(dlast.astype(np.float64))).sum().backward()
        return [t.grad.numpy() for pair in zip(tW, tb) for t in pair]

    _check(layout, pending, writer, ref, acc, arena, 2e-4)


TF_NAMES = ("mu_W1", "mu_b1", "mu_W2", "mu_b2", "var_W1", "var_b1", "var_W2", "var_b2")


@pytest.mark.parametrize("acc", [1, 0])
def test_tf_head_bwd_keeps_order(arena, acc):
    """fov_tf_head_bwd at lstm.py's shape (B = 32, H = 400, M = 32, O = 3): its eight gradients."""
    from longterm360fov_amd import ops
    B, H, M, Od = 32, 400, 32, 3
    rng = np.random.default_rng(61 + acc)
    shp = {"mu_W1": (H, M), "mu_b1": (M,), "mu_W2": (M, Od), "mu_b2": (Od,)}
    shp.update({k.replace("mu", "var"): s for k, s in shp.items()})
    w = {k: (0.1 * rng.standard_normal(shp[k])).astype(np.float32) for k in TF_NAMES}
    h = rng.uniform(-1, 1, (B, H)).astype(np.float32)
    dmu, dvar = rng.standard_normal((B, Od)).astype(np.float32), rng.standard_normal((B, Od)).astype(np.float32)
    tw = {k: dev(v) for k, v in w.items()}
    th, tdmu, tdvar = dev(h), dev(dmu), dev(dvar)
    head = ops.tf_head_fwd(th, tw)
    layout = Layout([shp[k] for k in TF_NAMES])
    pending = {i: Pending(rng, layout.shapes[i]) for i in (0, 7)}      # mu_W1, var_b2

    def writer(v, a, sc):
        ops.tf_head_bwd(th, tw, head, tdmu, tdvar, dict(zip(TF_NAMES, v)), accumulate=bool(a))

    def ref(_):
        t = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in w.items()}
        hh = torch.tensor(h.astype(np.float64))
        mu = torch.tanh(torch.relu(hh @ t["mu_W1"] + t["mu_b1"]) @ t["mu_W2"] + t["mu_b2"])
        var = torch.exp(torch.relu(hh @ t["var_W1"] + t["var_b1"]) @ t["var_W2"] + t["var_b2"])
        ((mu * torch.tensor(dmu.astype(np.float64))).sum() + (var * torch.tensor(dvar.astype(np.float64))).sum()).backward()
        return [t[k].grad.numpy() for k in TF_NAMES]

    _check(layout, pending, writer, ref, acc, arena, 2e-4)


# ---------------------------------------------------------------------------------------------------------------------
# controls: the writers that go through the deferral bookkeeping already
# ---------------------------------------------------------------------------------------------------------------------
def _control(kind, rng):
    """-> (shapes, writer, fp64 reference of E's outputs)"""
    from longterm360fov_amd import ops
    u = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)
    d = lambda a: np.asarray(a, np.float64)
    if kind == "dense_bwd":
        x, dp = u(300, 64), u(300, 32)
        tx, tdp, tW = dev(x), dev(dp), dev(u(64, 32))
        return ([(64, 32), (32,)], lambda v, a, sc: ops.dense_bwd(tx, tW, tdp, dW=v[0], db=v[1], need_dx=False, accumulate=bool(a), scratch=sc),
                [d(x).T @ d(dp), d(dp).sum(0)])
    if kind == "wgrad_fused":
        x, dp = u(300, 128), u(300, 64)
        tx, tdp = dev(x), dev(dp)
        return ([(129, 64)], lambda v, a, sc: ops.wgrad_fused(tx, None, tdp, v[0], accumulate=bool(a), scratch=sc),
                [np.concatenate([d(x), np.ones((300, 1))], 1).T @ d(dp)])
    if kind == "colsum":
        x = u(300, 64)
        tx = dev(x)
        return [(64,)], lambda v, a, sc: ops.colsum(tx, out=v[0], accumulate=bool(a), scratch=sc), [d(x).sum(0)]
    if kind == "mix_head_wgrad":
        T, B, H, Od, n = 5, 32, 64, 6, 12
        h2, dpp, oth, p, dpm = u(T, B, H), u(T, B, Od), u(B, T, n), u(T, B, Od), u(T, B, Od)
        t = [dev(a) for a in (h2, dpp, oth, p, dpm)]
        one = np.ones((T * B, 1))
        oth_tm = d(oth).transpose(1, 0, 2).reshape(T * B, n)
        ref = np.concatenate([np.concatenate([d(h2).reshape(T * B, H), one], 1).T @ d(dpp).reshape(T * B, Od),
                              np.concatenate([oth_tm, d(p).reshape(T * B, Od), one], 1).T @ d(dpm).reshape(T * B, Od)], 0)
        return ([((H + 1 + n + Od + 1) * Od,)], lambda v, a, sc: ops.mix_head_wgrad(*t, v[0], accumulate=bool(a), scratch=sc),
                [ref.reshape(-1)])
    if kind == "mse_dense_grad_db":
        N, Od = 300, 6
        y, tg = np.tanh(u(N, Od)), u(N, Od)
        ty, ttg = dev(y), dev(tg)
        dpre = 2.0 * (d(y) - d(tg)) / (N * Od) * (1 - d(y) ** 2)
        return [(Od,)], lambda v, a, sc: ops.mse_dense_grad(ty, ttg, "tanh", scratch=sc, db=v[0]), [dpre.sum(0)]
    assert kind == "dense_mse_head"
    N, H, Od = 300, 64, 6
    hs, W, b, tg = u(N, H), 0.2 * u(H, Od), 0.1 * u(Od), u(N, Od)
    ths, tW, tb, ttg = dev(hs), dev(W), dev(b), dev(tg)
    y = np.tanh(d(hs) @ d(W) + d(b))
    dpre = 2.0 * (y - d(tg)) / (N * Od) * (1 - y * y)
    return ([(H, Od), (Od,)], lambda v, a, sc: ops.dense_mse_head(ths, tW, tb, ttg, dW=v[0], db=v[1], need_dx=False, need_y=False, scratch=sc),
            [d(hs).T @ dpre, dpre.sum(0)])


@pytest.mark.parametrize("kind,acc", [("dense_bwd", 1), ("dense_bwd", 0), ("wgrad_fused", 1), ("colsum", 1), ("mix_head_wgrad", 1),
                                      ("dense_mse_head", 0), ("mse_dense_grad_db", 0)])
def test_deferring_writers_keep_order(arena, kind, acc):
    """Products whose reduce goes through the deferral table, and the loss launches that store a bias gradient from their last
    block (dense_mse_head; mse_dense_grad with db, whose fused form did not flush first): in-stream order is kept."""
    rng = np.random.default_rng(71 + len(kind) + acc)
    shapes, writer, refs = _control(kind, rng)
    layout = Layout(shapes)
    pending = {i: Pending(rng, s) for i, s in enumerate(layout.shapes)}
    def run(v, a, sc):
        writer(v, a, sc)

    _check(layout, pending, run, lambda _: refs, acc, arena, 2e-5)


# ---------------------------------------------------------------------------------------------------------------------
# readers: the optimizers must apply the reduced gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["adam", "rmsprop"])
def test_optimizer_reads_reduced_gradient(arena, opt):
    """fov_adam_step / fov_rmsprop_step issued on the flat gradient buffer while a split product into it is pending: the update
    uses the reduced gradient, bit for bit as with no region, and matches the fp64 Keras update of oracle/fov_oracle.py.
    (Step 3 from non-zero moments, so that the update depends on the gradient's value, not only its sign.)"""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(81 + len(opt))
    layout = Layout([(256, 1024)])
    pending = {0: Pending(rng, layout.shapes[0])}
    n = 256 * 1024
    p0 = rng.uniform(-1, 1, n).astype(np.float32)
    m0 = (0.1 * rng.standard_normal(n)).astype(np.float32)
    v0 = (0.01 + 0.05 * rng.random(n)).astype(np.float32)

    def writer(v, a, sc):
        st = [dev(p0), dev(m0), dev(v0)]
        if opt == "adam":
            ops.adam_step(st[0], v[0].view(-1), st[1], st[2], 3)
        else:
            ops.rmsprop_step(st[0], v[0].view(-1), st[2])
        return st

    flat0, views0, st0 = _sequence(layout, pending, writer, 0)
    flat1, _, st1 = _sequence(layout, pending, writer, 0, arena)
    assert torch.equal(flat0, flat1)
    for a, b in zip(st0, st1):
        assert torch.equal(a, b), "the optimizer read the gradient buffer before the pending reduce"
    g = pending[0].ref().reshape(-1)
    p, m, v = p0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
    if opt == "adam":
        O.adam_step(p, g, m, v, 3)
    else:
        O.rmsprop_step(p, g, v)
    assert np.abs(f64(st1[0]) - p).max() <= 2e-6
    assert np.abs(f64(st1[2]) - v).max() <= 1e-5 * np.abs(v).max()
    if opt == "adam":
        assert np.abs(f64(st1[1]) - m).max() <= 1e-5 * np.abs(m).max()


# ---------------------------------------------------------------------------------------------------------------------
# empty batch: accumulate = 0 writes the gradient of an empty sum (zero), accumulate = 1 leaves the buffer alone
# ---------------------------------------------------------------------------------------------------------------------
def _empty_calls():
    """-> [(name, [gradient shapes], call(grads, acc))] with B = 0 (and T = 0 where the entry point takes it)."""
    from longterm360fov_amd import ops
    e = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    F, H = 90, 256
    K, R = e(F, 4 * H), e(H, 4 * H)
    lstm = [(F, 4 * H), (H, 4 * H), (4 * H,)]
    calls = []
    for B, T in ((0, 10), (4, 0), (0, 0)):
        calls.append(("lstm_seq_wgrad B=%d T=%d" % (B, T), lstm,
                      lambda g, a, B=B, T=T: ops.lstm_seq_wgrad(e(B, T, F), e(B, T, H), e(B, T, 4 * H), *g, accumulate=bool(a))))
        calls.append(("lstm_seq_bwd B=%d T=%d" % (B, T), lstm,
                      lambda g, a, B=B, T=T: ops.lstm_seq_bwd(e(B, T, F), K, R, e(B, T, H), e(B, T, 5 * H), dK=g[0], dR=g[1], db=g[2],
                                                              accumulate=bool(a))))
    calls.append(("lstm_seq_wgrad_pair B=0", lstm + [(6, 4 * H), (H, 4 * H), (4 * H,)],
                  lambda g, a: ops.lstm_seq_wgrad_pair((e(0, 10, F), e(0, 10, H), None, e(0, 10, 4 * H)) + tuple(g[:3]),
                                                       (e(0, 10, 6), e(0, 10, H), None, e(0, 10, 4 * H)) + tuple(g[3:]),
                                                       accumulate=bool(a))))
    H2 = 512
    l1, l2 = (e(F, 4 * H2), e(H2, 4 * H2)), (e(H2, 4 * H2), e(H2, 4 * H2))
    for B, T in ((0, 8), (16, 0)):
        calls.append(("lstm_stack2_bwd B=%d T=%d" % (B, T), [(F, 4 * H2), (H2, 4 * H2), (4 * H2,), (H2, 4 * H2), (H2, 4 * H2), (4 * H2,)],
                      lambda g, a, B=B, T=T: ops.lstm_stack2_bwd(e(B, T, F), l1, l2, (e(B, T, H2), e(B, T, 5 * H2), None, None),
                                                                 (e(B, T, H2), e(B, T, 5 * H2), None, None), grads1=tuple(g[:3]),
                                                                 grads2=tuple(g[3:]), accumulate=bool(a))))
    for dil in (1, 2):
        calls.append(("conv2d_wgrad dilation=%d" % dil, [(3, 3, 8, 16)],
                      lambda g, a, dil=dil: ops.conv2d_wgrad(e(0, 16, 16, 8), e(0, 16, 16, 16), 3, 3, dw=g[0], accumulate=bool(a),
                                                             dilation=dil)))
    dims = [400, 64, 128, 256, 200]
    layers = [(e(dims[l], dims[l + 1]), e(dims[l + 1]), "relu" if l < 3 else None) for l in range(4)]
    mshapes = []
    for l in range(4):
        mshapes += [(dims[l], dims[l + 1]), (dims[l + 1],)]
    calls.append(("mlp_head_bwd B=0", mshapes,
                  lambda g, a: ops.mlp_head_bwd(e(0, 400), layers, [e(0, d) for d in dims[1:]], e(0, 200), g[0::2], g[1::2],
                                                need_dx=False, accumulate=bool(a))))
    w = {"mu_W1": e(400, 32), "mu_b1": e(32), "mu_W2": e(32, 3), "mu_b2": e(3)}
    w.update({k.replace("mu", "var"): v for k, v in w.items()})
    calls.append(("tf_head_bwd B=0", [tuple(w[k].shape) for k in TF_NAMES],
                  lambda g, a: ops.tf_head_bwd(e(0, 400), w, (e(0, 32), e(0, 3), e(0, 32), e(0, 3)), e(0, 3), e(0, 3),
                                               dict(zip(TF_NAMES, g)), accumulate=bool(a))))
    calls.append(("dense_bwd N=0", [(64, 32), (32,)],
                  lambda g, a: ops.dense_bwd(e(0, 64), e(64, 32), e(0, 32), dW=g[0], db=g[1], need_dx=False, accumulate=bool(a))))
    calls.append(("colsum rows=0", [(64,)], lambda g, a: ops.colsum(e(0, 64), out=g[0], accumulate=bool(a))))
    return calls


def test_empty_batch_zeroes_or_keeps_weight_gradients():
    """With no rows to sum over, accumulate = 0 writes zeros into every weight-gradient output and accumulate = 1 leaves it
    unchanged - for every entry point, including fov_lstm_seq_bwd at B = 0, fov_lstm_stack2_bwd at B = 0 or T = 0 and the fused
    heads, which returned without writing (a data-parallel rank with an empty shard kept a stale gradient)."""
    wrong = []
    for name, shapes, call in _empty_calls():
        for acc in (0, 1):
            g = [torch.full(s, 3.0 + i, dtype=torch.float32, device="cuda") for i, s in enumerate(shapes)]
            call(g, acc)
            torch.cuda.synchronize()
            wrong += ["%s accumulate=%d output %d" % (name, acc, i) for i, t in enumerate(g) if not bool((t == (0.0 if acc == 0 else 3.0 + i)).all())]
    assert not wrong, wrong


def test_stack2_bwd_without_steps_passes_state_gradients_through():
    """fov_lstm_stack2_bwd at T = 0 (as fov_lstm_seq_bwd at T = 0): dh0 / dc0 of each layer are its dhT / dcT, or zero."""
    from longterm360fov_amd import ops
    B, F, H = 4, 90, 512
    e = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(91)
    dhT2, dhT1 = dev(rng.standard_normal((B, H))), dev(rng.standard_normal((B, H)))
    tape = (e(B, 0, H), e(B, 0, 5 * H), None, None)
    r = ops.lstm_stack2_bwd(e(B, 0, F), (e(F, 4 * H), e(H, 4 * H)), (e(H, 4 * H), e(H, 4 * H)), tape, tape, dhT2=dhT2, dhT1=dhT1,
                            need_state_grads=True)
    torch.cuda.synchronize()
    assert torch.equal(r["dh0_2"], dhT2) and torch.equal(r["dh0_1"], dhT1)
    assert float(r["dc0_2"].abs().max()) == 0.0 and float(r["dc0_1"].abs().max()) == 0.0
