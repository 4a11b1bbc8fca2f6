"""The convolution path on GUARDED VIEWS at tile, halo and channel seams.

Every tensor operand - x as a channel slice of a wider NaN map or one time step of a NaN sequence, w, bias, add, c_prev, the
tapes - is a view inside a NaN buffer; every output a view inside a sentinel buffer (OutView; OutSlot where it is written with a
pixel stride).  tests/test_conv_guarded_host.py owns the helpers, the margin rule and the case tables, and shows on the CPU that
the harness catches a read of the neighbour channel / time step / pixel and a write beside a slot, that every margin holds a
whole 256-pixel block plus the farthest tap (a stray access is a wrong value or a broken sentinel, never a fault), and that a
reference with one mask lost - padding that wraps, a tap into the next map, channels past C from the neighbour - misses every
bound asserted here by a factor of ten.

The conv kernels do not clamp, they mask: a missed mask here reads NaN (a neighbour's data in the model) and the output has a NaN;
a store past the last pixel or beside a slot breaks a sentinel.  Every call is made twice into the same views and must give the
same bits, and the FORM that ran is asserted from the `form:` line of FOV_DBG_TRACE - the tile shape, the staging modes, the
segments, the patch form's geometry, the slices: a heuristic that moves fails the case instead of silently testing another kernel.

Map independence: every forward and cell case runs once more with unrelated maps appended, enough to fill the last pixel block;
the trace must name the same form and the first B maps must be the same bits.

References are fp64: conv_reference / cell_reference of the host file (O.conv2d_same and O.convlstm2d_step where those apply -
asserted equal there), the einsum of the existing weight-gradient test, torch fp64 autograd for the gates' backward.  Bounds,
imported or restated under names by the host file: `close` of tests/test_gpu_convlstm.py; the weight-gradient bound of
test_conv2d_weight_gradient_all_taps_per_workgroup; the literals of test_convlstm_gates_backward_softmax_relu_colsum and
test_convlstm_cell_and_softmax.  Every check prints its error over its bound; the last test prints the worst per family."""
import numpy as np
import pytest
import torch

import test_conv_guarded_host as H
import test_guarded_views_host as G
from oracle import fov_oracle as O
from test_gpu_convlstm import close
from test_gpu_ragged_guarded import launches, traced, twice
from test_guarded_views_host import OutView, f64, same_bits

pytestmark = pytest.mark.gpu

WORST = {}          # family -> [cases, worst error over bound]


def forms(trace):
    return [l.split("[fov trace] ", 1)[1] for l in trace.splitlines() if " form: " in l and l.startswith("[fov trace] ")]


def note(family, ratio):
    w = WORST.setdefault(family, [0, 0.0])
    w[0] += 1
    w[1] = max(w[1], ratio)


def checked(tag, family, got, ref, tol=H.CLOSE_TOL):
    """close() with its error over its bound on record."""
    r = H.close_ratio(got, ref, tol)
    print("%-56s error / bound %.3f" % (tag, r))
    note(family, r)
    close(got, f64(ref), tag, tol)


@pytest.fixture(scope="module")
def scratch():
    """One Scratch for the weight gradients, large enough for 512 slices of every case (the lines kernel then splits over
    min(B, 512, 1024 / tiles) maps, as it does on the model's layers)."""
    from longterm360fov_amd import ops
    s = ops.Scratch()
    s.get(64 << 20, torch.device("cuda", torch.cuda.current_device()))
    return s


# ---------------------------------------------------------------------------------------------------------------------
# forward: conv2d / conv2d_cat / dilated on the implicit GEMM, the map-resident form, the address-routed cases
# ---------------------------------------------------------------------------------------------------------------------
def run_forward(capfd, c, extra=0):
    """-> (output of the first B maps + extra, reference inputs).  Asserts the form of both calls and equal bits."""
    from longterm360fov_amd import ops
    p = H.forward_inputs(c, extra)
    t, out = H.forward_operands(c, p, "cuda")
    add = out.v if c["add"] == "alias" else t.get("add")

    def call():
        if c["C2"]:
            ops.conv2d_cat(t["x"], t["x2"], t["w"], t.get("b"), c["act"], out=out.v)
        else:
            ops.conv2d(t["x"], t["w"], t.get("b"), add=add, activation=c["act"], out=out.v, dilation=c["dil"])
    res, trace = traced(capfd, lambda: twice(call, {"out": out}, lambda: None), {})
    assert forms(trace) == [c["form"]] * 2, (c["name"], forms(trace))
    assert launches(trace) == ["conv2d_patch" if " patch " in c["form"] else "conv2d_igemm"] * 2
    for k, v in t.items():          # no operand was written
        assert not bool(torch.isnan(v).any()), k
    return res["out"], p


@pytest.mark.parametrize("c", H.all_forward_cases(), ids=H._ids(H.all_forward_cases()))
def test_conv2d_forward_on_guarded_views(capfd, c):
    got, p = run_forward(capfd, c)
    checked(c["name"], c["family"], got, H.forward_reference(c, p))
    more, _ = run_forward(capfd, c, H.extra_maps(c))
    assert same_bits(more[:c["B"]], got), "the first B maps depend on the maps behind them"


# ---------------------------------------------------------------------------------------------------------------------
# ConvLSTM2D cell in one launch: implicit GEMM (three tile shapes), patch form, dilated
# ---------------------------------------------------------------------------------------------------------------------
def run_cell(capfd, c, extra=0):
    from longterm360fov_amd import ops
    p = H.cell_inputs(c, extra)
    t, outs = H.cell_operands(c, p, "cuda")
    alias = c["alias"] and "c" in p
    act = H.act_of(c["name"])

    def call():
        ops.convlstm_cell(t["x"], t.get("h"), t["w"], t["b"], outs["c_out"].v if alias else t.get("c"), outs["h_out"].v, act,
                          c_new=None if alias else outs["c_out"].v, gates=outs["gates"].v if c["gates"] else None, dilation=c["dil"])
    res, trace = traced(capfd, lambda: twice(call, outs, lambda: None), {})
    assert forms(trace) == [c["form"]] * 2, (c["name"], forms(trace))
    assert launches(trace) == ["convlstm_cell_patch" if " patch " in c["form"] else "convlstm_cell"] * 2
    return res, p, act


@pytest.mark.parametrize("c", H.all_cell_cases(), ids=H._ids(H.all_cell_cases()))
def test_convlstm_cell_on_guarded_views(capfd, c):
    got, p, act = run_cell(capfd, c)
    h, cn, gates, _ = H.cell_reference(p["x"], p.get("h"), p.get("c"), p["w"], p["b"], act, c["dil"])
    checked(c["name"] + " h", "cell " + c["family"], got["h_out"], h)
    checked(c["name"] + " c", "cell " + c["family"], got["c_out"], cn)
    if c["gates"]:
        checked(c["name"] + " gates", "cell " + c["family"], got["gates"], gates)
    more, _, _ = run_cell(capfd, c, H.extra_maps(c))
    for k in got:
        assert same_bits(more[k][:c["B"]], got[k]), "%s: the first B maps depend on the maps behind them" % k


# ---------------------------------------------------------------------------------------------------------------------
# weight gradients: the lines form (six tile shapes, rows / columns, a short last slice) and the tap-wise form (four variants)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", H.all_wgrad_cases(), ids=H._ids(H.all_wgrad_cases()))
def test_conv2d_weight_gradient_on_guarded_views(capfd, scratch, c):
    from longterm360fov_amd import ops
    p = H.wgrad_inputs(c)
    t, out = H.wgrad_operands(c, p, "cuda")

    def call():
        ops.conv2d_wgrad(t["x"], t["dy"], c["kh"], c["kw"], dw=out.v, accumulate=c["accumulate"], scratch=scratch, dilation=c["dil"])
    res, trace = traced(capfd, lambda: twice(call, {"dw": out}, lambda: None), c["env"])
    assert forms(trace) == [c["form"]] * 2, (c["name"], forms(trace))
    assert [l for l in launches(trace) if l.startswith("conv_wgrad")] == ["conv_wgrad_lines" if " lines " in c["form"] else "conv_wgrad"] * 2
    ref = H.wgrad_reference(p["x"], p["dy"], c["kh"], c["kw"], c["dil"])
    px = c["B"] * c["H"] * c["W"]
    got = f64(res["dw"]) - (f64(p["base"]) if c["accumulate"] else 0.0)
    r = H.wgrad_ratio(got, ref, px)
    print("%-56s error / bound %.3f" % (c["name"], r))
    note("wgrad " + c["family"], r)
    assert np.abs(got - ref).max() <= H.wgrad_bound(ref, px), c["name"]


# ---------------------------------------------------------------------------------------------------------------------
# pointwise and small kernels
# ---------------------------------------------------------------------------------------------------------------------
def _rows(name, what, rows, n, scale=1.0):
    return H.maps(name, what, 1, (1, rows, n), scale)         # (1, 1, rows, n)


def _gates_reference(z, cp, act, dh=None, dc=None):
    """torch fp64: h, c_new, gates and - with the upstream gradients - dz, dc_prev by autograd."""
    F = z.shape[-1] // 4
    s = torch.sigmoid if act == "sigmoid" else (lambda v: torch.clamp(0.2 * v + 0.5, 0, 1))
    tz = torch.tensor(f64(z), requires_grad=True)
    tc = torch.tensor(f64(cp) if cp is not None else np.zeros(z.shape[:-1] + (F,)), requires_grad=True)
    i, f, g, o = s(tz[..., :F]), s(tz[..., F:2 * F]), torch.tanh(tz[..., 2 * F:3 * F]), s(tz[..., 3 * F:])
    cn = f * tc + i * g
    hn = o * torch.tanh(cn)
    out = dict(h=hn.detach().numpy(), c=cn.detach().numpy(), gates=torch.cat([i, f, g, o], -1).detach().numpy())
    if dh is not None:
        ((hn * torch.tensor(f64(dh))).sum() + (cn * torch.tensor(f64(dc))).sum()).backward()
        out.update(dz=tz.grad.numpy(), dc=tc.grad.numpy())
    return out


@pytest.mark.parametrize("rows,F", H.GATE_CASES)
def test_gate_kernels_on_guarded_views(capfd, rows, F):
    """convlstm_gates, convlstm_gates_train (gates apart, and gates aliasing z; zero state) and convlstm_gates_bwd (dz apart, and dz
    aliasing gates): h / dh in slots of a wider map, c and dc updated in place."""
    from longterm360fov_amd import ops
    name = "gates-%dx%d" % (rows, F)
    act = H.act_of(name)
    z, cp = _rows(name, "z", rows, 4 * F, 2.0), _rows(name, "c", rows, F)
    dh, dc = _rows(name, "dh", rows, F), _rows(name, "dc", rows, F)
    ref = _gates_reference(z, cp, act, dh, dc)
    shape = (1, 1, rows, F)
    lead, trail = (4, 3) if rows % 2 else (1, 2)

    # inference: c in place
    outs = dict(h=H.OutSlot(shape, lead, trail, device="cuda"), c=H.pixel_out(shape, cp, "cuda"))
    zv = H.view_of(z, None, "cuda")
    res, trace = traced(capfd, lambda: twice(lambda: ops.convlstm_gates(zv, outs["c"].v, outs["h"].v, act), outs, lambda: None), {})
    assert launches(trace) == ["convlstm_gates"] * 2
    checked(name + " gates h", "gates", res["h"], ref["h"])
    checked(name + " gates c", "gates", res["c"], ref["c"])

    # training forward: gates apart, then gates aliasing z; then from the zero state
    tapes = {}
    for alias in (False, True):
        outs = dict(h=H.OutSlot(shape, lead, trail, device="cuda"), c=H.pixel_out(shape, None, "cuda"),
                    gates=H.pixel_out((1, 1, rows, 4 * F), z if alias else None, "cuda"))
        zz, cv = (outs["gates"].v if alias else zv), H.view_of(cp, None, "cuda")
        res, trace = traced(capfd, lambda: twice(lambda: ops.convlstm_gates_train(zz, cv, outs["h"].v, act, gates=None if alias else outs["gates"].v,
                                                                                  c_new=outs["c"].v), outs, lambda: None), {})
        assert launches(trace) == ["convlstm_gates_train"] * 2
        for k in ("h", "c", "gates"):
            checked("%s train %s%s" % (name, k, " (gates = z)" if alias else ""), "gates", res[k], ref[k])
        tapes[alias] = res
    assert all(same_bits(tapes[True][k], tapes[False][k]) for k in tapes[True])
    zero = _gates_reference(z, None, act)
    outs = dict(h=H.OutSlot(shape, lead, trail, device="cuda"), c=H.pixel_out(shape, None, "cuda"), gates=H.pixel_out((1, 1, rows, 4 * F), None, "cuda"))
    res, _ = traced(capfd, lambda: twice(lambda: ops.convlstm_gates_train(zv, None, outs["h"].v, act, gates=outs["gates"].v, c_new=outs["c"].v),
                                         outs, lambda: None), {})
    checked(name + " train c from the zero state", "gates", res["c"], zero["c"])
    checked(name + " train h from the zero state", "gates", res["h"], zero["h"])

    # backward on the GPU's own tape: dz apart, then dz aliasing gates
    tape = tapes[False]
    bwd = {}
    for alias in (False, True):
        outs = dict(dz=H.pixel_out((1, 1, rows, 4 * F), tape["gates"] if alias else None, "cuda"), dc=H.pixel_out(shape, dc, "cuda"))
        gv = outs["dz"].v if alias else H.view_of(tape["gates"], None, "cuda")
        dhv, cpv, cnv = H.guarded_nhwc(dh, lead, trail, device="cuda"), H.view_of(cp, None, "cuda"), H.view_of(tape["c"], None, "cuda")
        res, trace = traced(capfd, lambda: twice(lambda: ops.convlstm_gates_bwd(dhv, outs["dc"].v, gv, cpv, cnv, act, dz=outs["dz"].v), outs, lambda: None), {})
        assert launches(trace) == ["convlstm_gates_bwd"] * 2
        checked("%s bwd dz%s" % (name, " (dz = gates)" if alias else ""), "gates bwd", res["dz"], ref["dz"], H.GATES_BWD_TOL)
        checked("%s bwd dc_prev" % name, "gates bwd", res["dc"], ref["dc"], H.GATES_BWD_TOL)
        bwd[alias] = res
    assert all(same_bits(bwd[True][k], bwd[False][k]) for k in bwd[True])


@pytest.mark.parametrize("rows,n", H.SOFTMAX_CASES)
def test_softmax_on_guarded_views(capfd, rows, n):
    from longterm360fov_amd import ops
    name = "softmax-%dx%d" % (rows, n)
    x, dp = H.maps(name, "x", rows, (n,), 3.0), H.maps(name, "dp", rows, (n,))
    xv, out = G.guarded(x, device="cuda"), H.pixel_out((rows, n), None, "cuda")
    res, trace = traced(capfd, lambda: twice(lambda: ops.softmax_lastdim(xv, out=out.v), {"p": out}, lambda: None), {})
    assert launches(trace) == ["softmax_lastdim"] * 2
    checked(name, "softmax", res["p"], O.softmax_last(f64(x)), H.SOFTMAX_TOL)
    p = res["p"]
    ref = f64(p) * (f64(dp) - (f64(dp) * f64(p)).sum(-1, keepdims=True))
    dpv, pv, out = G.guarded(dp, device="cuda"), G.guarded(p, device="cuda"), H.pixel_out((rows, n), None, "cuda")
    res, trace = traced(capfd, lambda: twice(lambda: ops.softmax_lastdim_bwd(dpv, pv, out=out.v), {"dx": out}, lambda: None), {})
    assert launches(trace) == ["softmax_bwd"] * 2
    checked(name + " bwd", "softmax bwd", res["dx"], ref, H.SOFTMAX_BWD_TOL)


@pytest.mark.parametrize("kh,kw,C,N", H.TRANSPOSE_CASES)
def test_weight_transpose_on_guarded_views(capfd, kh, kw, C, N):
    from longterm360fov_amd import ops
    w = H.weights("transpose-%d-%d-%d-%d" % (kh, kw, C, N), kh, kw, C, N)
    wv, out = G.guarded(w, device="cuda"), OutView((kh, kw, N, C), device="cuda")
    res, trace = traced(capfd, lambda: twice(lambda: ops.conv2d_weight_transpose(wv, out=out.v), {"wt": out}, lambda: None), {})
    assert launches(trace) == ["conv_weight_transpose"] * 2
    assert same_bits(res["wt"], np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2)))
    note("weight transpose", 0.0)


@pytest.mark.parametrize("rows,cols", H.COLSUM_CASES)
def test_colsum_on_guarded_views(capfd, scratch, rows, cols):
    """Every branch of colsum(): the narrow kernels (cols <= 8 / <= 16 from 4096 rows), the partial kernel below and beside them,
    a second column block; overwrite and accumulate."""
    from longterm360fov_amd import ops
    name = "colsum-%dx%d" % (rows, cols)
    x = H.maps(name, "x", rows, (cols,))
    base = H.vector(name, "base", cols)
    xv = G.guarded(x, device="cuda")
    ref = f64(x).sum(0)
    for acc in (False, True):
        out = OutView((cols,), base if acc else None, device="cuda")
        res, trace = traced(capfd, lambda: twice(lambda: ops.colsum(xv, out=out.v, accumulate=acc, scratch=scratch), {"s": out}, lambda: None), {})
        assert launches(trace)[0] == "colsum_partial"
        got = f64(res["s"]) - (f64(base) if acc else 0.0)
        # close() on the sum itself; under accumulate the base's own rounding (half an ulp of base + sum) is inside the bound's floor
        checked(name + (" accumulate" if acc else ""), "colsum", got, ref, H.COLSUM_TOL)


# ---------------------------------------------------------------------------------------------------------------------
# the 2 GiB refusals of the fp32 entry points: host decisions that touch no memory
# ---------------------------------------------------------------------------------------------------------------------
def test_operands_past_2_gib_are_refused_before_any_launch(capfd):
    """a_pix of conv2d_igemm_kernel is a 32-bit byte offset: right only because operand_fits_31bit refuses B ldb 4 >= 2^31 - for x and
    for the second segment.  Each refusal returns the unsupported code with its message, launches nothing and leaves the output
    untouched; just under the limit (B = 1: no batch stride is read) the call runs and is right."""
    from longterm360fov_amd import _lib, ops
    L = _lib.lib()
    B, Hh, W, C, F, k = 2, 3, 5, 4, 8, 3
    name = "refusal"
    x, h = H.maps(name, "x", B, (Hh, W, C)), H.maps(name, "h", B, (Hh, W, F), 0.5)
    w, wc, b = H.weights(name, k, k, C, 4 * F), H.weights(name, k, k, C + F, 4 * F, "wc"), H.vector(name, "b", 4 * F)
    halo = H.halo_pixels(W, k, k)
    xv, hv = H.guarded_nhwc(x, device="cuda", halo=halo), H.guarded_nhwc(h, device="cuda", halo=halo)
    wv, wcv, bv = G.guarded(w, device="cuda"), G.guarded(wc, device="cuda"), G.guarded(b, device="cuda")
    big = 1 << 28                       # B ldb 4 = 2^31 at B = 2
    y = H.pixel_out((B, Hh, W, 4 * F), None, "cuda")
    hs, cs = H.OutSlot((B, Hh, W, F), 3, 2, device="cuda"), H.pixel_out((B, Hh, W, F), None, "cuda")
    dense = Hh * W * C

    def conv(Bc, ldb):
        return L.fov_conv2d_fwd(xv.data_ptr(), C, ldb, wv.data_ptr(), bv.data_ptr(), None, y.v.data_ptr(), Bc, Hh, W, C, 4 * F, k, k, 0, ops._stream())

    def cell(Bc, ldb, ldb2):
        return L.fov_convlstm_cell_fwd(xv.data_ptr(), C, ldb, C, hv.data_ptr(), F, ldb2, wcv.data_ptr(), bv.data_ptr(), None, cs.v.data_ptr(),
                                       hs.v.data_ptr(), hs.v.stride(2), None, Bc, Hh, W, F, k, k, ops.act_code("hard_sigmoid"), ops._stream())
    for what, fn, msg in (("conv2d x", lambda: conv(B, big), "conv2d: operand larger than 2 GiB"),
                          ("cell x", lambda: cell(B, big, Hh * W * F), "convlstm_cell: operand larger than 2 GiB"),
                          ("cell h_prev", lambda: cell(B, dense, big), "convlstm_cell: operand larger than 2 GiB")):
        rc, trace = traced(capfd, fn, {})
        assert rc == _lib.ERR_UNSUPPORTED and L.fov_last_error().decode() == msg, (what, rc, L.fov_last_error())
        assert launches(trace) == [] and forms(trace) == [], (what, trace)
        assert y.untouched() and hs.untouched() and cs.untouched(), what
    rc, trace = traced(capfd, lambda: L.fov_conv2d_fwd2(xv.data_ptr(), C, dense, C, hv.data_ptr(), F, big, F, wcv.data_ptr(), bv.data_ptr(), None,
                                                        y.v.data_ptr(), B, Hh, W, 4 * F, k, k, 0, ops._stream()), {})
    assert rc == _lib.ERR_UNSUPPORTED and L.fov_last_error().decode() == "conv2d: operand larger than 2 GiB"         # the second segment's stride
    assert launches(trace) == [] and y.untouched()
    # just under the limit in the arithmetic sense only: one map, whose batch stride no kernel reads
    under = (1 << 29) - 4
    y1 = H.pixel_out((1, Hh, W, 4 * F), None, "cuda")
    rc, trace = traced(capfd, lambda: L.fov_conv2d_fwd(xv.data_ptr(), C, under, wv.data_ptr(), bv.data_ptr(), None, y1.v.data_ptr(), 1, Hh, W, C, 4 * F,
                                                       k, k, 0, ops._stream()), {})
    assert rc == 0 and launches(trace) == ["conv2d_igemm"]
    checked("conv2d, one map, batch stride 2^29 - 4", "refusals", y1.result(), H.conv_reference([(x[:1], 1)], w, b))
    h1, c1 = H.OutSlot((1, Hh, W, F), 3, 2, device="cuda"), H.pixel_out((1, Hh, W, F), None, "cuda")
    rc, trace = traced(capfd, lambda: L.fov_convlstm_cell_fwd(xv.data_ptr(), C, under, C, hv.data_ptr(), F, under, wcv.data_ptr(), bv.data_ptr(), None,
                                                              c1.v.data_ptr(), h1.v.data_ptr(), h1.v.stride(2), None, 1, Hh, W, F, k, k,
                                                              ops.act_code("hard_sigmoid"), ops._stream()), {})
    assert rc == 0 and launches(trace) == ["convlstm_cell_patch"]
    href, cref, _, _ = H.cell_reference(x[:1], h[:1], None, wc, b, "hard_sigmoid")
    checked("cell, one map, batch strides 2^29 - 4: h", "refusals", h1.result(), href)
    checked("cell, one map, batch strides 2^29 - 4: c", "refusals", c1.result(), cref)


# ---------------------------------------------------------------------------------------------------------------------
# bf16 forms, one tier smaller: both forms of each entry point, against the rounded-operand restatements of the bf16 host files
# ---------------------------------------------------------------------------------------------------------------------
def bf16_checked(tag, family, got, ref, op_close):
    r = float(np.abs(f64(got) - ref).max() / (H.BF16_OP_TOL * np.abs(ref).max()))
    print("%-56s error / bound %.3f" % (tag, r))
    note(family, r)
    op_close(torch.from_numpy(np.ascontiguousarray(got)), ref, tag)


@pytest.mark.parametrize("c", H.BF16_FORWARD_CASES, ids=H._ids(H.BF16_FORWARD_CASES))
def test_conv2d_bf16_on_guarded_views(capfd, c):
    import test_gpu_convlstm_bf16 as BF
    from longterm360fov_amd import ops
    from test_convlstm_bf16_host import conv2d_bf16_ref
    x, w, b = BF.op_inputs(G.seed_of(c["name"]) % (1 << 31), c["B"], c["H"], c["W"], c["C"], c["N"], c["kh"], c["kw"])
    p = dict(x=x, w=w, **({"b": b} if c["bias"] else {}))
    t, out = H.forward_operands(c, p, "cuda")
    packed = ops.conv2d_pack_bf16(t["w"])
    res, trace = traced(capfd, lambda: twice(lambda: ops.conv2d_bf16(t["x"], t["w"], t.get("b"), c["act"], out=out.v, packed=packed),
                                             {"out": out}, lambda: None), {})
    assert launches(trace) == [c["form"]] * 2, (c["name"], launches(trace))
    ref = conv2d_bf16_ref(f64(x), f64(w), f64(b) if c["bias"] else None)
    bf16_checked(c["name"], "bf16 conv2d", res["out"], np.maximum(ref, 0) if c["act"] == "relu" else ref, BF.op_close)


@pytest.mark.parametrize("c", H.BF16_CELL_CASES, ids=H._ids(H.BF16_CELL_CASES))
def test_convlstm_cell_bf16_on_guarded_views(capfd, c):
    import test_convlstm_cell_bf16_host as CB
    import test_gpu_convlstm_cell_bf16 as CG
    from longterm360fov_amd import ops
    assert c["kh"] == c["kw"]
    q = CB.cell_inputs(G.seed_of(c["name"]) % (1 << 31), c["B"], c["H"], c["W"], c["C"], c["F"], c["kh"])
    state = c["hview"] is not None
    p = dict(x=q["x"], w=np.concatenate([q["K"], q["R"]], 2) if state else q["K"], b=q["b"])
    if state:
        p["h"] = q["h"]
    if c["c"]:
        p["c"] = q["c"]
    t, outs = H.cell_operands(c, p, "cuda")
    alias, act = c["alias"] and c["c"], H.act_of(c["name"])

    def call():
        ops.convlstm_cell_bf16(t["x"], t.get("h"), t["w"], t["b"], outs["c_out"].v if alias else t.get("c"), outs["h_out"].v, act,
                               c_new=None if alias else outs["c_out"].v, gates=outs["gates"].v if c["gates"] else None)
    res, trace = traced(capfd, lambda: twice(call, outs, lambda: None), {})
    assert [l for l in launches(trace) if "pack" not in l] == [c["form"]] * 2, (c["name"], launches(trace))
    r = CB.cell_bf16_ref(f64(q["x"]), f64(q["h"]) if state else None, f64(q["c"]) if c["c"] else None, f64(q["K"]), f64(q["R"]), f64(q["b"]), act)
    for k, n in (("h_out", "h"), ("c_out", "c")) + ((("gates", "gates"),) if c["gates"] else ()):
        bf16_checked("%s %s" % (c["name"], n), "bf16 cell", res[k], r[n], CG.op_close)


@pytest.mark.parametrize("c", H.BF16_WGRAD_CASES, ids=H._ids(H.BF16_WGRAD_CASES))
def test_conv2d_wgrad_bf16_on_guarded_views(capfd, scratch, c):
    """The bound of test_wgrad_bf16_against_the_rounded_operand_reference: max(1, 8 e_ref) units of 1e-5 max|ref|, e_ref the fp32
    restatement's own distance from the fp64 one."""
    from longterm360fov_amd import ops
    from test_convlstm_train_bf16_host import wgrad_bf16_ref
    from test_gpu_conv_wgrad_bf16 import units
    p = H.wgrad_inputs(c)
    t, out = H.wgrad_operands(c, p, "cuda")
    res, trace = traced(capfd, lambda: twice(lambda: ops.conv2d_wgrad_bf16(t["x"], t["dy"], c["kh"], c["kw"], dw=out.v, accumulate=c["accumulate"],
                                                                           scratch=scratch), {"dw": out}, lambda: None), {})
    plans = [l.split("conv2d_wgrad_bf16: ")[1].split(" form")[0] for l in trace.splitlines() if "conv2d_wgrad_bf16: " in l]
    assert plans == [c["form"]] * 2, (c["name"], plans)
    assert [l for l in launches(trace) if l.startswith("conv_wgrad")] == ["conv_wgrad_bf16" if c["form"] == "tuned" else "conv_wgrad_plain_bf16"] * 2
    ref = wgrad_bf16_ref(f64(p["x"]), f64(p["dy"]), c["kh"], c["kw"])
    bound = max(1.0, 8.0 * units(f64(wgrad_bf16_ref(p["x"], p["dy"], c["kh"], c["kw"])), ref))
    u = units(f64(res["dw"]) - (f64(p["base"]) if c["accumulate"] else 0.0), ref)
    print("%-56s %.3f units, bound %.2f" % (c["name"], u, bound))
    note("bf16 wgrad", u / bound)
    assert u <= bound, c["name"]


def test_print_the_worst_error_over_bound_per_family():
    """Last in the file: the table of DESIGN.md (checks and worst error over bound per family)."""
    print("\n%-24s %6s %s" % ("family", "checks", "worst error / bound"))
    for k in sorted(WORST):
        print("%-24s %6d %.3f" % (k, WORST[k][0], WORST[k][1]))
        assert WORST[k][1] <= 1.0
