"""The recurrent kernels, the few-row weight gradients and the small heads on GUARDED VIEWS at ragged tile edges.

Every tensor operand is a view inside a NaN buffer (guarded), every output a view inside a sentinel buffer (OutView), both with
margins of 16 operand rows and 1024 floats at least (tests/test_guarded_views_host.py owns the helpers and the case tables, and
shows on the CPU that the harness catches a write in front of / behind a view, an unwritten element and a read past an operand).
So: a write past row B of a ragged 16-row tile breaks a sentinel; an unwritten element stays NaN; a read past an operand's end -
rows B .. of the tile, the rows of K between F and the next k-block, step t - 2 of a prefetch at T = 1 - makes a NaN where it is
used; padded rows that leak into a sum over rows (db, dK, dR, dW) miss the bound by a factor of ten at least (shown on the CPU for
every case).  Every call is made twice into the same views and must give the same bits, and the form that ran is asserted from
FOV_DBG_TRACE: a heuristic that moves fails the case instead of silently testing another kernel.

Row independence: every ragged case runs once more with the batch filled up to the next multiple of 16 by unrelated rows; the
trace must name the same form and the first B rows of every per-row output must be the same bits.

References: the fp64 oracle (lstm_layer_train; lstm_layer_backward on the GPU's own tape; dense), for the bf16 kernels on
bf16-rounded operands.  Bounds, imported: assert_parity (tests/test_gpu_parity.py) for fp32 forward values, check_grads
(tests/test_gpu_train.py) for fp32 gradients, TIGHT of tests/test_gpu_bf16.py and near / PER_KERNEL / STATE of
tests/test_gpu_bf16_backward.py for the bf16 kernels; the heads' bounds are inline literals in tests/test_gpu_lstm_py_heads.py and
are restated under names.  Every check prints its error over its bound; the last test prints the worst per kernel family.

Covered: the layer forward with its tape in every form (generic, cluster 64 / 128 / 256, lstm_wide at F 256 and at width 512 with
and without the projection, lstm_wide16 128 / 256 / 512, the bf16 layer with vector and scalar x staging, fov_lstm_seq_fwd_zx); the
two-layer launches and the two-layer BPTT; the fused decodes, the decoder alone and the teacher-forced graph; the mixing decoder and
its BPTT in fp32 and bf16; every row of BACKWARD_FORMS in four variants (the last one with FOV_NO_WGRAD_GROUP=1: only then is db the
sum a BPTT kernel formed over its own rows - at these row counts wgrad_rows takes db otherwise, and a kernel without its padded-row
mask passes every other variant); the few-row weight gradients alone, in pairs and for the mixing head; the Dense, mixing, TF,
mixture and raw heads and the Dense + MSE head; and one case per launcher branch on an operand's address, with only that operand
misaligned.  The four kernels behind launch_dense and the three x stagings of the bf16 layer and decode kernels have trace names of
their own, and the wgrad_group line says how many of its problems take the 16-byte stores: all asserted."""
import contextlib
import os
import re
import sys

import numpy as np
import pytest
import torch

import test_guarded_views_host as G
from oracle import fov_oracle as O
from test_gpu_bf16 import TIGHT as BF16_TIGHT
from test_gpu_bf16_backward import PER_KERNEL, STATE, near
from test_gpu_parity import ATOL_FLOOR, RTOL, TIGHT, assert_parity
from test_guarded_views_host import OutView, f64, same_bits

pytestmark = pytest.mark.gpu

LAUNCHED = re.compile(r"\[fov trace\] launched: (.+)")
BWD_LINE = re.compile(r"\[fov trace\] lstm_seq_bwd B=(\d+) T=(\d+) F=(\d+) H=(\d+) wide16=(\d) fuse_kr=(\d) fuse_r=(\d) grouped=(\d) acc=(\d)")
RECURRENT = {"generic", "cluster", "wide LSTM", "wide16 LSTM", "bf16 LSTM layer (narrow x)", "bf16 LSTM layer (vector x)", "bf16 LSTM layer (scalar x)", "bwd cluster", "8-group BPTT", "16-unit BPTT",
             "lstm_bwd_pointwise", "two-layer width-512", "bf16 two-layer", "two-layer BPTT"}
WORST = {}          # kernel family -> [cases, worst error over bound]: printed by the last test of the file


def gv(a, off=0):
    return None if a is None else G.guarded(a, off, device="cuda")


def out_view(shape, base=None, off=0, row=None, dtype=torch.float32):
    return OutView(shape, base, off, dtype, "cuda", row)


def ptr(t):
    return None if t is None else t.data_ptr()


@pytest.fixture(scope="module")
def bufs():
    """An ordinary Workspace, the Scratch of the BPTT calls (stateful like the workspace: the persistent kernels keep their header
    and granule area at its head), a plain Scratch for the calls that put split partials there and the Workspace of the fused
    decoder's backward, shared by this file's cases."""
    from longterm360fov_amd import ops
    return ops.Workspace(), ops.Scratch(), ops.Scratch(), ops.Workspace()


@contextlib.contextmanager
def knobs(env):
    before = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in before.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def traced(capfd, fn, env):
    """fn() under the case's knobs and FOV_DBG_TRACE=1 -> (result, trace).  The library re-reads its environment at the next
    workspace / scratch fetch; calls that fetch none need the reload made here."""
    before = capfd.readouterr()
    with knobs(dict(env, FOV_DBG_TRACE="1")):
        reload_env()
        r = fn()
        torch.cuda.synchronize()
    reload_env()
    trace = capfd.readouterr().err
    sys.stdout.write(before.out)        # what the test has printed so far stays in its captured output
    sys.stderr.write(before.err)
    return r, trace


def reload_env():
    from longterm360fov_amd import ops
    ops._sync_env()


def launches(trace):
    return LAUNCHED.findall(trace)


def recurrent_launches(trace):
    return sorted(set(launches(trace)) & RECURRENT)


def note(family, ratio):
    w = WORST.setdefault(family, [0, 0.0])
    w[0] += 1
    w[1] = max(w[1], ratio)


def parity(tag, family, got, ref):
    """assert_parity, and its error over its bound (the tighter of the per-element 1e-3 |ref| + 1e-5 and 2e-5) for the table."""
    ref = f64(ref)
    r = float((np.abs(f64(got) - ref) / np.minimum(RTOL * np.abs(ref) + ATOL_FLOOR, TIGHT)).max()) if ref.size else 0.0
    print("%-64s error / bound %.3f" % (tag, r))
    note(family, r)
    assert_parity(got, ref, tag)


def grads(tag, family, got, ref):
    """check_grads over the keys of ref (got: numpy), and the worst error over its bound."""
    r = max(G.grad_bounds(got[k], ref[k]) for k in ref)
    print("%-64s error / bound %.3f" % (tag, r))
    note(family, r)
    G.check_grads({k: torch.from_numpy(np.ascontiguousarray(got[k])) for k in ref}, ref, tag)


def bf16_grads(tag, family, got, ref):
    for k in ref:
        bound = STATE if k == "dh0" else PER_KERNEL
        note(family, near("%s %s" % (tag, k), got[k], ref[k], bound) / bound)


def twice(call, outs, check):
    """call() twice into the same OutViews (reset in between); check() after each; -> the results of the second, which
    must equal the first bit for bit."""
    call()
    check()
    first = {k: o.result() for k, o in outs.items()}
    for o in outs.values():
        o.reset()
    call()
    check()
    second = {k: o.result() for k, o in outs.items()}
    for k in first:
        assert same_bits(first[k], second[k]), "%s: two calls differ" % k
    return second


# ---------------------------------------------------------------------------------------------------------------------
# one layer, forward with the reserve tape: fov_lstm_seq_fwd_train / fov_lstm_seq_fwd_bf16
# ---------------------------------------------------------------------------------------------------------------------
def layer_forward(ops, capfd, bufs, form, inp, B, T, F, act, state, with_hs=True):
    """-> (dict of numpy outputs, the recurrent launches of the trace).  Every operand guarded, every output an OutView."""
    name, launched, dtype, impl, H, env = form[:6]
    ws = bufs[0]
    x, K, R, b = gv(inp["x"][:B]), gv(inp["K"]), gv(inp["R"]), gv(inp["b"])
    h0, c0 = (gv(inp["h0"][:B]), gv(inp["c0"][:B])) if state else (None, None)
    outs = {"hT": out_view((B, H)), "cT": out_view((B, H)), "res": out_view((B, T, 5, H))}
    if with_hs:
        outs["hs"] = out_view((B, T, H))
    views = (outs["hs"].v if with_hs else None, outs["hT"].v, outs["cT"].v, outs["res"].v)

    def call():
        if dtype == "bf16":
            ops.lstm_seq_bf16(x, K, R, b, h0, c0, act=act, workspace=ws, out=views)
        else:
            ops.lstm_seq_train(x, K, R, b, h0, c0, act=act, impl=impl, workspace=ws, out=views)
    got, trace = traced(capfd, lambda: twice(call, outs, ws.check), env)
    return got, recurrent_launches(trace)


@pytest.mark.parametrize("cid,form,B,F,T", G.layer_cases(), ids=[c[0] for c in G.layer_cases()])
def test_layer_forward_on_guarded_views(capfd, bufs, cid, form, B, F, T):
    from longterm360fov_amd import ops
    name, launched, dtype, impl, H, env = form[:6]
    bf, act = dtype == "bf16", G.act_of(cid)
    rows = G.round_up(B)
    inp = G.layer_inputs(cid, B, T, F, H, rows=rows)
    live = {k: (v[:B] if k not in ("K", "R", "b") else v) for k, v in inp.items()}
    for state in (True, False):
        tag = "%s F%d T%d %s state=%d" % (cid, F, T, act, state)
        got, ran = layer_forward(ops, capfd, bufs, form, inp, B, T, F, act, state)
        assert ran == [launched], (tag, ran)
        ref = dict(zip(("hs", "hT", "cT", "res"), G.layer_reference(live, act, state, bf)))
        for k in ("hs", "hT", "cT", "res"):
            if bf:
                r = O.regime_error(got[k], ref[k], "bf16") if k == "res" else float(np.abs(got[k] - ref[k]).max()) / BF16_TIGHT
                print("%-64s error / bound %.3f" % (tag + " " + k, r))
                note(launched, r)
                assert r <= 1.0, (tag, k, r)
            else:
                parity(tag + " " + k, launched, got[k], ref[k])
        assert same_bits(got["res"][:, -1, 4], got["cT"]) and same_bits(got["hs"][:, -1], got["hT"])
        if state:       # return_sequences=False: hs NULL, everything else the same bits
            no_hs, ran2 = layer_forward(ops, capfd, bufs, form, inp, B, T, F, act, state, with_hs=False)
            assert ran2 == [launched] and all(same_bits(no_hs[k], got[k]) for k in no_hs), tag
        if rows != B:   # the tile filled up with unrelated rows: same form, the first B rows the same bits
            full, ran3 = layer_forward(ops, capfd, bufs, form, inp, rows, T, F, act, state)
            assert ran3 == [launched], (tag, ran3)
            for k in got:
                assert same_bits(full[k][:B], got[k]), "%s %s: a live row depends on the rows behind it" % (tag, k)


# ---------------------------------------------------------------------------------------------------------------------
# one layer, backward: fov_lstm_seq_bwd / _bf16 through the C ABI, all seven outputs OutViews
# ---------------------------------------------------------------------------------------------------------------------
def layer_backward(ops, capfd, bufs, form, inp, tape, B, T, F, act, variant, cid, env_extra=None, offs=None):
    """One variant of one backward case on the tape (hs, res as numpy, B rows) -> (outputs, base, trace).  offs: operand -> off of
    its guarded view (the alignment cases)."""
    from longterm360fov_amd import _lib
    name, launched, dtype, H, env = form[:5]
    sc = bufs[1]
    st, ups = variant["state"], variant["ups"]
    offs = offs or {}
    x, K, R = gv(inp["x"][:B]), gv(inp["K"], offs.get("K", 0)), gv(inp["R"], offs.get("R", 0))
    h0, c0 = (gv(inp["h0"][:B]), gv(inp["c0"][:B])) if st else (None, None)
    hs, res = gv(tape[0]), gv(tape[1])
    dhs = gv(inp["dhs"][:B]) if "s" in ups else None
    dhT = gv(inp["dhT"][:B]) if "h" in ups else None
    dcT = gv(inp["dcT"][:B]) if "c" in ups else None
    N4 = 4 * H
    shapes = {"dK": (F, N4), "dR": (H, N4), "db": (N4,)}
    base = {k: G.accumulate_base("%s %s" % (cid, k), s) for k, s in shapes.items()} if variant["base"] else {}
    outs = {"dz": out_view((B, T, N4)), "dx": out_view((B, T, F), off=offs.get("dx", 0)), "dh0": out_view((B, H)), "dc0": out_view((B, H))}
    if variant["adjacent"]:
        flat = np.concatenate([base[k].reshape(-1) for k in ("dK", "dR", "db")]) if base else None
        outs["flat"] = out_view(((F + H + 1) * N4,), flat, row=N4)
        w = {"dK": outs["flat"].part(0, (F, N4)), "dR": outs["flat"].part(F * N4, (H, N4)), "db": outs["flat"].part((F + H) * N4, (N4,))}
    else:
        for k, s in shapes.items():
            outs[k] = out_view(s, base.get(k), row=N4)
        w = {k: outs[k].v for k in shapes}
    L = _lib.lib()
    fn = L.fov_lstm_seq_bwd_bf16 if dtype == "bf16" else L.fov_lstm_seq_bwd

    def call():
        buf = sc.get(L.fov_lstm_seq_bwd_workspace_bytes(B, T, F, H), x.device)
        ops.check(fn(ptr(x), ptr(K), ptr(R), ptr(h0), ptr(c0), ptr(hs), ptr(res), ptr(dhs), ptr(dhT), ptr(dcT), ptr(outs["dz"].v),
                     ptr(outs["dx"].v), ptr(w["dK"]), ptr(w["dR"]), ptr(w["db"]), ptr(outs["dh0"].v), ptr(outs["dc0"].v), B, T, F, H,
                     ops.act_code(act), 1 if base else 0, buf.data_ptr(), buf.numel(), ops._stream()))
    got, trace = traced(capfd, lambda: twice(call, outs, sc.check), dict(env, **(env_extra or {})))
    if variant["adjacent"]:
        flat = got.pop("flat")
        got.update(dK=flat[:F * N4].reshape(F, N4), dR=flat[F * N4:(F + H) * N4].reshape(H, N4), db=flat[(F + H) * N4:])
    return got, base, trace


def backward_tape(ops, bufs, form, inp, B, F, T, act, state):
    """The GPU's own forward tape of the first B rows (plain tensors: the forward has its own test) -> (hs, res) numpy."""
    dtype, H = form[2], form[3]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    h0, c0 = (dev(inp["h0"][:B]), dev(inp["c0"][:B])) if state else (None, None)
    hs, _, _, res = ops.lstm_seq_train(dev(inp["x"][:B]), dev(inp["K"]), dev(inp["R"]), dev(inp["b"]), h0, c0, act=act, workspace=bufs[0], dtype=dtype)
    bufs[0].check()
    return hs.cpu().numpy(), res.cpu().numpy()


@pytest.mark.parametrize("cid,form,B,F,T", G.backward_cases(), ids=[c[0] for c in G.backward_cases()])
def test_layer_backward_on_guarded_views(capfd, bufs, cid, form, B, F, T):
    """Every variant of BACKWARD_VARIANTS: overwrite with all upstream gradients and an initial state; accumulate onto a
    non-zero base into adjacent dK | dR | db from dhs alone without a state; dhT / dcT alone; and FOV_NO_WGRAD_GROUP=1 with
    separate outputs, where db is the sum the BPTT kernel formed over its own rows (grouped=0, no wgrad_rows launch).  The trace line of lstm_seq_bwd
    is asserted (wide16, grouped), and so is the weight-gradient launch: at these row counts wgrad_rows takes the fp32 weight
    gradients of the persistent forms whether dK | dR | db are adjacent or not (fuse_kr and fuse_r stay 0:
    test_fused_weight_gradients_into_adjacent_outputs below)."""
    from longterm360fov_amd import ops
    name, launched, dtype, H, env = form[:5]
    bf, act = dtype == "bf16", G.act_of(cid)
    rows = G.round_up(B)
    inp = G.layer_inputs(cid, B, T, F, H, rows=rows)
    live = {k: (v[:B] if k not in ("K", "R", "b") else v) for k, v in inp.items()}
    for variant in G.BACKWARD_VARIANTS:
        tag = "%s F%d T%d %s %s" % (cid, F, T, act, variant["name"])
        tape = backward_tape(ops, bufs, form, inp, B, F, T, act, variant["state"])
        venv = variant.get("env", {})
        few_rows = not bf and not venv and launched != "lstm_bwd_pointwise"      # (the stepped form leaves the weight gradients to the products)
        got, base, trace = layer_backward(ops, capfd, bufs, form, inp, tape, B, T, F, act, variant, cid, venv)
        assert recurrent_launches(trace) == [launched], (tag, launches(trace))
        if launched != "lstm_bwd_pointwise":
            line = BWD_LINE.search(trace)
            assert line, (tag, trace)
            v = [int(g) for g in line.groups()]
            assert v[:4] == [B, T, F, H] and v[4] == (launched == "16-unit BPTT") and v[8] == (1 if base else 0), (tag, line.group(0))
            assert v[7] == (1 if few_rows else 0) and (bf or v[5] == v[6] == 0), (tag, line.group(0))
        assert ("wgrad_rows" in launches(trace)) == few_rows, (tag, launches(trace))
        if bf and F == 256:
            assert "gemm_bf16_nt" not in launches(trace), (tag, "dx was not formed in the kernel")
        if launched == "8-group BPTT" and not bf and F == 256:
            assert not re.search(r"gemm_f32 next: M=%d N=%d " % (B * T, F), trace), (tag, "dx was not formed in the kernel")
        ref = G.backward_reference(live, tape[0], tape[1], variant, act, bf)
        for k, b_ in base.items():
            ref[k] = ref[k] + b_
        (bf16_grads if bf else grads)(tag, launched + (" bf16" if bf else ""), got, ref)
        if rows != B:
            tape_full = backward_tape(ops, bufs, form, inp, rows, F, T, act, variant["state"])
            assert same_bits(tape_full[0][:B], tape[0]) and same_bits(tape_full[1][:B], tape[1])
            full, _, trace2 = layer_backward(ops, capfd, bufs, form, inp, tape_full, rows, T, F, act, variant, cid, venv)
            assert recurrent_launches(trace2) == [launched], (tag, launches(trace2))
            for k in ("dz", "dx", "dh0", "dc0"):
                assert same_bits(full[k][:B], got[k]), "%s %s: a live row depends on the rows behind it" % (tag, k)


@pytest.mark.parametrize("B", [17, 30])
def test_bwd8_dx_in_the_kernel_and_by_the_product(capfd, bufs, B):
    """lstm_bwd8 at F = 256 forms dx in the kernel (eight partial tapes and one reduce); FOV_NO_DX_FUSION=1 takes the NT product
    behind the recurrence.  Both on guarded views, both within check_grads of the fp64 reference."""
    from longterm360fov_amd import ops
    form = [f for f in G.BACKWARD_FORMS if f[0] == "bwd8-256"][0]
    cid, T, F, H = "bwd8-dx-B%d" % B, 3, 256, 256
    act, variant = G.act_of(cid), G.BACKWARD_VARIANTS[0]
    inp = G.layer_inputs(cid, B, T, F, H)
    tape = backward_tape(ops, bufs, form, inp, B, F, T, act, True)
    ref = G.backward_reference(inp, tape[0], tape[1], variant, act)
    dx_product = r"gemm_f32 next: M=%d N=%d " % (B * T, F)
    fused, _, t1 = layer_backward(ops, capfd, bufs, form, inp, tape, B, T, F, act, variant, cid)
    plain, _, t2 = layer_backward(ops, capfd, bufs, form, inp, tape, B, T, F, act, variant, cid, {"FOV_NO_DX_FUSION": "1"})
    assert recurrent_launches(t1) == recurrent_launches(t2) == ["8-group BPTT"]
    assert not re.search(dx_product, t1) and re.search(dx_product, t2), (t1, t2)
    grads(cid + " dx in the kernel", "8-group BPTT", fused, ref)
    grads(cid + " dx by the product", "8-group BPTT", plain, ref)
    assert all(same_bits(fused[k], plain[k]) for k in ("dz", "dh0", "dc0", "dK", "dR", "db"))


@pytest.mark.parametrize("fname,B,F,T,kr,r", [("bwd_cluster-256", 17, 256, 3, 1, 0), ("bwd16-256", 30, 256, 2, 1, 0), ("bwd16-512", 17, 256, 2, 1, 0),
                                              ("bwd8-256-bf16", 30, 256, 3, 1, 0), ("bwd16-128", 17, 90, 3, 0, 1), ("bwd8-256", 1, 96, 2, 0, 1)])
def test_fused_weight_gradients_into_adjacent_outputs(capfd, bufs, fname, B, F, T, kr, r):
    """dK | dR | db adjacent and FOV_NO_WGRAD_GROUP=1 (without it the few-row kernels take every fp32 case of this file).  The
    trace line shows fuse_kr=1 where F is a multiple of 128 (one product [x | h_prev | 1]^T dz writes all three), else fuse_r=1
    ([h_prev | 1]^T dz writes dR and db, x^T dz is its own product); T > 1 in both."""
    from longterm360fov_amd import ops
    form = [f for f in G.BACKWARD_FORMS if f[0] == fname][0]
    H, bf = form[3], form[2] == "bf16"
    cid = "fused-wgrad-%s-B%d" % (fname, B)
    act, variant = G.act_of(cid), G.BACKWARD_VARIANTS[1]
    inp = G.layer_inputs(cid, B, T, F, H)
    tape = backward_tape(ops, bufs, form, inp, B, F, T, act, False)
    got, base, trace = layer_backward(ops, capfd, bufs, form, inp, tape, B, T, F, act, variant, cid, {"FOV_NO_WGRAD_GROUP": "1"})
    line = BWD_LINE.search(trace)
    assert line and [int(line.group(i)) for i in (6, 7, 8)] == [kr, r, 0], trace
    assert recurrent_launches(trace) == [form[1]] and not {"wgrad_rows", "wgrad_group"} & set(launches(trace))
    ref = G.backward_reference(inp, tape[0], tape[1], variant, act, bf)
    for k, b_ in base.items():
        ref[k] = ref[k] + b_
    (bf16_grads if bf else grads)(cid, "fused weight gradients", got, ref)


# ---------------------------------------------------------------------------------------------------------------------
# few-row weight gradients: fov_lstm_seq_wgrad, fov_lstm_seq_wgrad_pair (wgrad_rows, wgrad_group), fov_mix_head_wgrad
# ---------------------------------------------------------------------------------------------------------------------
def wgrad_inputs(name, B, T, F, H):
    rng = np.random.default_rng(G.seed_of(name))
    p = dict(x=rng.uniform(-1, 1, (B, T, F)), hs=rng.uniform(-1, 1, (B, T, H)), h0=0.5 * rng.standard_normal((B, H)),
             dz=0.2 * rng.standard_normal((B, T, 4 * H)))
    p["dz"][B - 1] *= 5.0
    return {k: v.astype(np.float32) for k, v in p.items()}


def wgrad_reference(p, with_h0):
    x, hs, h0, dz = (f64(p[k]) for k in ("x", "hs", "h0", "dz"))
    B, T, F = x.shape
    H = hs.shape[-1]
    hprev = np.concatenate([(h0 if with_h0 else np.zeros_like(h0))[:, None], hs[:, :-1]], axis=1)
    d2 = dz.reshape(B * T, 4 * H)
    return {"dK": x.reshape(B * T, F).T @ d2, "dR": hprev.reshape(B * T, H).T @ d2, "db": d2.sum(0)}


def wgrad_outs(name, F, H, accumulate):
    shapes = {"dK": (F, 4 * H), "dR": (H, 4 * H), "db": (4 * H,)}
    base = {k: G.accumulate_base("%s %s" % (name, k), s) for k, s in shapes.items()} if accumulate else {}
    return {k: out_view(s, base.get(k), row=4 * H) for k, s in shapes.items()}, base


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("name,kernel,H,F,B,T,with_h0", G.WGRAD_CASES)
def test_few_row_weight_gradients_on_guarded_views(capfd, bufs, name, kernel, H, F, B, T, with_h0, accumulate):
    from longterm360fov_amd import ops
    p = wgrad_inputs(name, B, T, F, H)
    x, hs, dz, h0 = gv(p["x"]), gv(p["hs"]), gv(p["dz"]), gv(p["h0"]) if with_h0 else None
    outs, base = wgrad_outs(name, F, H, accumulate)
    call = lambda: ops.lstm_seq_wgrad(x, hs, dz, outs["dK"].v, outs["dR"].v, outs["db"].v, h0=h0, accumulate=accumulate, scratch=bufs[2])
    got, trace = traced(capfd, lambda: twice(call, outs, torch.cuda.synchronize), {})
    assert launches(trace) == [kernel] * 2, launches(trace)
    assert kernel != "wgrad_group" or trace.count(" vector_stores 2\n") == 2, trace       # aligned outputs: the 16-byte stores
    ref = wgrad_reference(p, with_h0)
    for k, b_ in base.items():
        ref[k] = ref[k] + b_
    grads("%s B%d T%d F%d acc=%d" % (name, B, T, F, accumulate), kernel, got, ref)


@pytest.mark.parametrize("name,H,F1,T1,F2,T2,B", G.WGRAD_PAIR_CASES)
def test_weight_gradients_of_a_layer_pair_on_guarded_views(capfd, bufs, name, H, F1, T1, F2, T2, B):
    """fov_lstm_seq_wgrad_pair: an encoder over T1 steps and a decoder over T2 != T1 steps in one wgrad_rows launch; the
    decoder's h0 is given, the encoder's is not."""
    from longterm360fov_amd import ops
    assert ops.lstm_seq_wgrad_pair_one_launch(B, T1, T2, H)
    p1, p2 = wgrad_inputs(name + " enc", B, T1, F1, H), wgrad_inputs(name + " dec", B, T2, F2, H)
    o1, _ = wgrad_outs(name + " enc", F1, H, False)
    o2, _ = wgrad_outs(name + " dec", F2, H, False)
    l1 = (gv(p1["x"]), gv(p1["hs"]), None, gv(p1["dz"]), o1["dK"].v, o1["dR"].v, o1["db"].v)
    l2 = (gv(p2["x"]), gv(p2["hs"]), gv(p2["h0"]), gv(p2["dz"]), o2["dK"].v, o2["dR"].v, o2["db"].v)
    outs = dict([("1" + k, v) for k, v in o1.items()] + [("2" + k, v) for k, v in o2.items()])
    got, trace = traced(capfd, lambda: twice(lambda: ops.lstm_seq_wgrad_pair(l1, l2, scratch=bufs[2]), outs, torch.cuda.synchronize), {})
    assert launches(trace) == ["wgrad_rows"] * 2, launches(trace)
    r1, r2 = wgrad_reference(p1, False), wgrad_reference(p2, True)
    grads(name + " encoder", "wgrad_rows", {k: got["1" + k] for k in r1}, r1)
    grads(name + " decoder", "wgrad_rows", {k: got["2" + k] for k in r2}, r2)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("B,T,H,O_,n_oth", G.MIX_HEAD_WGRAD_CASES)
def test_mix_head_weight_gradients_on_guarded_views(capfd, bufs, B, T, H, O_, n_oth, accumulate):
    """fov_mix_head_wgrad: [dense_W ; dense_b ; mix_W ; mix_b] = [h2 | 1]^T dpre_p, [others | p | 1]^T dpre_m over the T * B rows
    (time-major tapes, batch-major others), one flat output."""
    from longterm360fov_amd import ops
    name = "mix-head-wgrad B%d T%d" % (B, T)
    q = G.mix_head_wgrad_inputs(B, T, H, O_, n_oth)
    ncol = H + 1 + n_oth + O_ + 1
    base = G.accumulate_base(name, (ncol, O_)) if accumulate else None
    outs = {"out": out_view((ncol, O_), base)}
    ops_in = [gv(q[k]) for k in ("h2", "dp", "oth", "p", "dm")]
    call = lambda: ops.mix_head_wgrad(*ops_in, outs["out"].v, accumulate=accumulate, scratch=bufs[2])
    got, trace = traced(capfd, lambda: twice(call, outs, torch.cuda.synchronize), {})
    assert "mix_head_wgrad" in launches(trace)
    ref = G.mix_head_wgrad_reference(q) + (0 if base is None else base)
    rows = G.mix_head_wgrad_rows(H, n_oth, O_)
    grads(name + " acc=%d" % accumulate, "mix_head_wgrad", {k: got["out"][r] for k, r in rows.items()}, {k: ref[r] for k, r in rows.items()})


# ---------------------------------------------------------------------------------------------------------------------
# heads: fov_dense_fwd, fov_dense_add_fwd, fov_mix_head_fwd / _bwd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kernel,N,In,Out,activation", G.DENSE_CASES)
def test_dense_forward_on_guarded_views(capfd, name, kernel, N, In, Out, activation):
    """Each of the four kernels behind launch_dense, asserted from its own trace name: a threshold that moves fails the case."""
    from longterm360fov_amd import ops
    rows = G.round_up(N)
    p = G.dense_inputs(name, N, In, Out, rows=rows)
    W, b = gv(p["W"]), gv(p["b"])

    def run(n):
        x, outs = gv(p["x"][:n]), {"y": out_view((n, Out))}
        got, trace = traced(capfd, lambda: twice(lambda: ops.dense(x, W, b, activation, out=outs["y"].v), outs, lambda: None), {})
        assert launches(trace) == [kernel] * 2, launches(trace)
        return got["y"]
    y = run(N)
    parity(name, kernel, y, O.dense(f64(p["x"][:N]), f64(p["W"]), f64(p["b"]), activation))
    if rows != N:
        assert same_bits(run(rows)[:N], y), name + ": a live row depends on the rows behind it"


@pytest.mark.parametrize("name,kernel,N,In,Out,stride", G.DENSE_ADD_CASES)
def test_dense_add_forward_on_guarded_views(capfd, name, kernel, N, In, Out, stride):
    """act(x W + b + add[row * stride + :]): `add` a strided row view inside its NaN buffer - the floats between Out and the
    stride are NaN too, as are the rows behind row N."""
    from longterm360fov_amd import ops
    p = G.dense_inputs(name, N, In, Out)
    add = np.random.default_rng(G.seed_of(name + " add")).uniform(-1, 1, (N, Out)).astype(np.float32)
    wide = np.full((N, stride), np.nan, np.float32)
    wide[:, :Out] = add
    addv = gv(wide)[:, :Out]
    assert addv.stride(0) == stride
    x, W, b, outs = gv(p["x"]), gv(p["W"]), gv(p["b"]), {"y": out_view((N, Out))}
    got, trace = traced(capfd, lambda: twice(lambda: ops.dense_add(x, W, b, addv, "tanh", out=outs["y"].v), outs, lambda: None), {})
    assert launches(trace) == [kernel] * 2, launches(trace)
    parity(name, "dense_add, " + kernel, got["y"], np.tanh(f64(p["x"]) @ f64(p["W"]) + f64(p["b"]) + f64(add)))


@pytest.mark.parametrize("name,N,H,O_", G.MIX_HEAD_CASES)
def test_mix_head_forward_and_backward_on_guarded_views(capfd, name, N, H, O_):
    """p = tanh(h dense_W + dense_b), m = tanh(p mix_Wp + add) and the backward of that step (with and without the feedback
    gradient); rows filled up to the tile: the first N the same bits."""
    from longterm360fov_amd import ops
    rows = G.round_up(N)
    rng = np.random.default_rng(G.seed_of(name))
    Wd = (rng.standard_normal((H, O_)) / np.sqrt(H)).astype(np.float32)
    bd = (0.1 * rng.standard_normal(O_)).astype(np.float32)
    Wp = (rng.standard_normal((O_, O_)) / np.sqrt(O_)).astype(np.float32)
    h, add, dl, dfb = (rng.uniform(-1, 1, s).astype(np.float32) for s in ((rows, H), (rows, O_ + 5), (rows, O_), (rows, O_)))
    dWd, dbd, dWp = gv(Wd), gv(bd), gv(Wp)

    def run(n, feedback):
        addw = np.full((n, O_ + 5), np.nan, np.float32)
        addw[:, :O_] = add[:n, :O_]
        hv, addv = gv(h[:n]), gv(addw)[:, :O_]
        fw = {"p": out_view((n, O_)), "m": out_view((n, O_))}
        got, trace = traced(capfd, lambda: twice(lambda: ops.mix_head_fwd(hv, dWd, dbd, dWp, addv, fw["p"].v, fw["m"].v), fw, lambda: None), {})
        assert launches(trace) == ["mix_head_fwd"] * 2
        bw = {"dpre_m": out_view((n, O_)), "dpre_p": out_view((n, O_)), "dh": out_view((n, H))}
        ins = [gv(dl[:n]), gv(dfb[:n]) if feedback else None, gv(got["m"]), gv(got["p"])]
        g2, trace = traced(capfd, lambda: twice(lambda: ops.mix_head_bwd(*ins, dWp, dWd, bw["dpre_m"].v, bw["dpre_p"].v, bw["dh"].v), bw, lambda: None), {})
        assert launches(trace) == ["mix_head_bwd"] * 2
        return dict(got, **g2)
    for feedback in (True, False):
        got = run(N, feedback)
        p_ref = np.tanh(f64(h[:N]) @ f64(Wd) + f64(bd))
        m_ref = np.tanh(p_ref @ f64(Wp) + f64(add[:N, :O_]))
        parity(name + " p", "mix_head", got["p"], p_ref)
        parity(name + " m", "mix_head", got["m"], m_ref)
        # the backward on the GPU's own p, m (include/fov360.h: dm_loss is the gradient at m's pre-activation, dm_feedback at m)
        m, p = f64(got["m"]), f64(got["p"])
        dpre_m = f64(dl[:N]) + (f64(dfb[:N]) * (1 - m * m) if feedback else 0)
        dpre_p = (dpre_m @ f64(Wp).T) * (1 - p * p)
        grads("%s backward feedback=%d" % (name, feedback), "mix_head", got, {"dpre_m": dpre_m, "dpre_p": dpre_p, "dh": dpre_p @ f64(Wd).T})
        if rows != N:
            full = run(rows, feedback)
            assert all(same_bits(full[k][:N], got[k]) for k in got), name + ": a live row depends on the rows behind it"


# ---------------------------------------------------------------------------------------------------------------------
# decode: fov_seq2seq_decode_fwd / _bf16, fov_seq2seq_decoder_fwd, fov_seq2seq_tf_fwd - out, hT and cT all OutViews
# ---------------------------------------------------------------------------------------------------------------------
def forward_checks(tag, family, got, ref, bf):
    for k in ref:
        if bf:
            r = O.regime_error(got[k], ref[k], "bf16") if k == "res" else float(np.abs(got[k] - ref[k]).max()) / BF16_TIGHT
            print("%-64s error / bound %.3f" % (tag + " " + k, r))
            note(family, r)
            assert r <= 1.0, (tag, k, r)
        else:
            parity(tag + " " + k, family, got[k], ref[k])


def decode_run(ops, capfd, bufs, form, p, B, T_out, act):
    name, launched, dtype, impl, H = form[:5]
    w = {k: gv(v) for k, v in p["w"].items()}
    enc, dec0 = gv(p["enc"][:B]), gv(p["dec0"][:B])
    outs = {"out": out_view((B, T_out, G.F_DEC)), "hT": out_view((B, H)), "cT": out_view((B, H))}
    kw = {"dtype": "bf16"} if dtype == "bf16" else {"impl": impl}
    call = lambda: ops.seq2seq_decode(enc, dec0, w, T_out, act=act, workspace=bufs[0], out=outs["out"].v, hT=outs["hT"].v, cT=outs["cT"].v, **kw)
    got, trace = traced(capfd, lambda: twice(call, outs, bufs[0].check), {})
    return got, launches(trace)


@pytest.mark.parametrize("cid,form,B,F_enc,T_in,T_out", G.decode_cases(), ids=[c[0] for c in G.decode_cases()])
def test_seq2seq_decode_on_guarded_views(capfd, bufs, cid, form, B, F_enc, T_in, T_out):
    from longterm360fov_amd import ops
    launched, bf, H = form[1], form[2] == "bf16", form[4]
    act, rows = G.act_of(cid), G.round_up(B)
    p = G.decode_inputs(cid, B, T_in, T_out, F_enc, H, rows=rows)
    got, ran = decode_run(ops, capfd, bufs, form, p, B, T_out, act)
    assert ran == [launched] * 2, (cid, ran)
    ref = O.regime_decode(p["enc"][:B], p["dec0"][:B], p["w"], T_out, act, bf)
    forward_checks(cid, launched, got, {k: ref[k] for k in ("out", "hT", "cT")}, bf)
    if rows != B:
        full, ran2 = decode_run(ops, capfd, bufs, form, p, rows, T_out, act)
        assert ran2 == [launched] * 2, (cid, ran2)
        for k in got:
            assert same_bits(full[k][:B], got[k]), "%s %s: a live row depends on the rows behind it" % (cid, k)


@pytest.mark.parametrize("cid,form,B,T_out", G.decoder_cases(), ids=[c[0] for c in G.decoder_cases()])
def test_seq2seq_decoder_from_a_given_state_on_guarded_views(capfd, bufs, cid, form, B, T_out):
    from longterm360fov_amd import _lib, ops
    name, launched, impl, H = form[:4]
    act, rows = G.act_of(cid), G.round_up(B)
    p = G.decode_inputs(cid, B, 1, 1, 6, H, rows=rows)
    w = [gv(p["w"][k]) for k in ("dec_K", "dec_R", "dec_b", "dense_W", "dense_b")]
    L = _lib.lib()

    def run(n):
        dec0, h0, c0 = gv(p["dec0"][:n]), gv(p["h0"][:n]), gv(p["c0"][:n])
        outs = {"out": out_view((n, T_out, G.F_DEC)), "hT": out_view((n, H)), "cT": out_view((n, H))}

        def call():
            buf = bufs[0].get(L.fov_seq2seq_decode_workspace_bytes(n, 0, T_out, 1, G.F_DEC, H, ops.impl_code(impl)), dec0.device)
            ops.check(L.fov_seq2seq_decoder_fwd(ptr(dec0), ptr(h0), ptr(c0), *[ptr(t) for t in w], ptr(outs["out"].v), ptr(outs["hT"].v),
                                                ptr(outs["cT"].v), n, T_out, G.F_DEC, H, ops.act_code(act), ops.impl_code(impl), buf.data_ptr(),
                                                buf.numel(), ops._stream()))
        got, trace = traced(capfd, lambda: twice(call, outs, bufs[0].check), {})
        assert launches(trace) == [launched] * 2, (cid, launches(trace))
        return got
    got = run(B)
    forward_checks(cid, launched + " (decoder)", got, G.decoder_reference(p, B, T_out, act), False)
    if rows != B:
        full = run(rows)
        assert all(same_bits(full[k][:B], got[k]) for k in got), cid + ": a live row depends on the rows behind it"


@pytest.mark.parametrize("name,layer_launches,impl,H,B,F_enc,T_in,T_out", G.TF_CASES)
def test_teacher_forced_graph_on_guarded_views(capfd, bufs, name, layer_launches, impl, H, B, F_enc, T_in, T_out):
    from longterm360fov_amd import _lib, ops
    act = G.act_of(name)
    p = G.decode_inputs(name, B, T_in, T_out, F_enc, H)
    w = [gv(p["w"][k]) for k in ("enc_K", "enc_R", "enc_b", "dec_K", "dec_R", "dec_b", "dense_W", "dense_b")]
    enc, dec_in, outs = gv(p["enc"]), gv(p["dec_in"]), {"out": out_view((B, T_out, G.F_DEC))}
    L = _lib.lib()

    def call():
        buf = bufs[0].get(L.fov_seq2seq_tf_workspace_bytes(B, T_in, T_out, F_enc, G.F_DEC, H, ops.impl_code(impl)), enc.device)
        ops.check(L.fov_seq2seq_tf_fwd(ptr(enc), ptr(dec_in), *[ptr(t) for t in w], ptr(outs["out"].v), B, T_in, T_out, F_enc, G.F_DEC, H,
                                       ops.act_code(act), ops.impl_code(impl), buf.data_ptr(), buf.numel(), ops._stream()))
    got, trace = traced(capfd, lambda: twice(call, outs, bufs[0].check), {})
    assert launches(trace) == (layer_launches * 2 + [G.DENSE_WAVE]) * 2, launches(trace)
    parity(name, "teacher-forced graph", got["out"], O.seq2seq_teacher_forced(f64(p["enc"]), f64(p["dec_in"]), {k: f64(v) for k, v in p["w"].items()}, act))


# ---------------------------------------------------------------------------------------------------------------------
# fov_lstm_seq_fwd_zx, and the two-layer launches fov_lstm_stack2_fwd / _bf16
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,form,B,T", G.zx_cases(), ids=[c[0] for c in G.zx_cases()])
def test_layer_from_an_input_projection_on_guarded_views(capfd, bufs, cid, form, B, T):
    from longterm360fov_amd import ops
    name, launched, impl, H = form[:4]
    act, rows = G.act_of(cid), G.round_up(B)
    p = G.layer_inputs(cid, B, T, 90, H, rows=rows)
    zx_all = (f64(p["x"]) @ f64(p["K"])).astype(np.float32)
    R, b = gv(p["R"]), gv(p["b"])

    def run(n, state):
        zx = gv(zx_all[:n])
        h0, c0 = (gv(p["h0"][:n]), gv(p["c0"][:n])) if state else (None, None)
        outs = {"hs": out_view((n, T, H)), "hT": out_view((n, H)), "cT": out_view((n, H)), "res": out_view((n, T, 5, H))}
        call = lambda: ops.lstm_seq_zx(zx, R, b, h0, c0, act=act, impl=impl, workspace=bufs[0], reserve=outs["res"].v,
                                       out=(outs["hs"].v, outs["hT"].v, outs["cT"].v))
        got, trace = traced(capfd, lambda: twice(call, outs, bufs[0].check), {})
        assert launches(trace) == [launched] * 2, (cid, launches(trace))
        return got
    for state in (True, False):
        got = run(B, state)
        ref = G.zx_reference(zx_all[:B], p["R"], p["b"], p["h0"][:B] if state else None, p["c0"][:B] if state else None, act)
        forward_checks("%s state=%d" % (cid, state), launched + " (zx)", got, dict(zip(("hs", "hT", "cT", "res"), ref)), False)
    if rows != B:
        full = run(rows, False)
        assert all(same_bits(full[k][:B], got[k]) for k in got), cid + ": a live row depends on the rows behind it"


def stack2_run(ops, capfd, bufs, form, a, b, n, T, F, act, state, reserve):
    from longterm360fov_amd import _lib
    launched, bf, H = form[1], form[2] == "bf16", form[3]
    x = gv(a["x"][:n])
    l1, l2 = [gv(a[k]) for k in ("K", "R", "b")], [gv(b[k]) for k in ("K", "R", "b")]
    st = [gv(q[k][:n]) if state else None for q in (a, b) for k in ("h0", "c0")]
    outs = {}
    for l in ("1", "2"):
        outs.update({"hs" + l: out_view((n, T, H)), "hT" + l: out_view((n, H)), "cT" + l: out_view((n, H))})
        if reserve:
            outs["res" + l] = out_view((n, T, 5, H))
    v = lambda k: outs[k].v if k in outs else None
    o1, o2 = [tuple(v(k + l) for k in ("hs", "hT", "cT", "res")) for l in ("1", "2")]
    L = _lib.lib()

    def call():
        if bf:
            ops.lstm_stack2_bf16(x, l1, l2, act=act, workspace=bufs[0], out1=o1, out2=o2)
        else:
            buf = bufs[0].get(L.fov_lstm_seq_workspace_bytes(n, T, F, H, ops.IMPL_AUTO), x.device)
            ops.check(L.fov_lstm_stack2_fwd(ptr(x), *[ptr(t) for t in l1], ptr(st[0]), ptr(st[1]), *[ptr(t) for t in l2], ptr(st[2]), ptr(st[3]),
                                            *[ptr(t) for t in o1], *[ptr(t) for t in o2], n, T, F, H, ops.act_code(act), buf.data_ptr(),
                                            buf.numel(), ops._stream()))
    got, trace = traced(capfd, lambda: twice(call, outs, bufs[0].check), {})
    assert launches(trace) == [launched] * 2, launches(trace)
    return got


@pytest.mark.parametrize("cid,form,B,F,T", G.stack2_cases(), ids=[c[0] for c in G.stack2_cases()])
def test_two_layer_launches_on_guarded_views(capfd, bufs, cid, form, B, F, T):
    """fov_lstm_stack2_fwd (with and without the reserve, with and without initial states) and fov_lstm_stack2_fwd_bf16 (zero
    initial states by its signature)."""
    from longterm360fov_amd import ops
    launched, bf, H = form[1], form[2] == "bf16", form[3]
    act, rows = G.act_of(cid), G.round_up(B)
    a, b = G.stack2_inputs(cid, B, T, F, H, rows=rows)
    supported = ops.lstm_stack2_bf16_supported if bf else ops.lstm_stack2_supported
    assert supported(B, T, F, H) and supported(rows, T, F, H)
    for state in ((False,) if bf else (True, False)):
        ref = G.stack2_reference(a, b, B, act, state, bf)
        got = stack2_run(ops, capfd, bufs, form, a, b, B, T, F, act, state, True)
        for l, layer in zip(("1", "2"), ref):
            forward_checks("%s state=%d layer %s" % (cid, state, l), launched, {k: got[k + l] for k in ("hs", "hT", "cT", "res")},
                           dict(zip(("hs", "hT", "cT", "res"), layer)), bf)
        bare = stack2_run(ops, capfd, bufs, form, a, b, B, T, F, act, state, False)
        assert all(same_bits(bare[k], got[k]) for k in bare), cid + ": the launch without the reserve differs"
        if rows != B:
            full = stack2_run(ops, capfd, bufs, form, a, b, rows, T, F, act, state, True)
            assert all(same_bits(full[k][:B], got[k]) for k in got), cid + ": a live row depends on the rows behind it"


def stack2_tape(ops, bufs, a, b, n, act, state):
    """The GPU's own tapes of the two-layer forward on plain tensors -> [(hs1, res1), (hs2, res2)] numpy."""
    dev = lambda t: torch.from_numpy(np.ascontiguousarray(t)).cuda()
    st = lambda q: (dev(q["h0"][:n]), dev(q["c0"][:n])) if state else None
    o1, o2 = ops.lstm_stack2(dev(a["x"][:n]), [dev(a[k]) for k in ("K", "R", "b")], [dev(b[k]) for k in ("K", "R", "b")], st(a), st(b), act=act,
                             workspace=bufs[0], reserve=True)
    bufs[0].check()
    return [(o[0].cpu().numpy(), o[3].cpu().numpy()) for o in (o1, o2)]


def stack2_backward(ops, capfd, bufs, a, b, tapes, n, T, F, H, act, state, accumulate, cid, env):
    from longterm360fov_amd import _lib
    N4 = 4 * H
    x, R1, K2, R2 = gv(a["x"][:n]), gv(a["R"]), gv(b["K"]), gv(b["R"])
    st = [gv(q[k][:n]) if state else None for q in (a, b) for k in ("h0", "c0")]
    tp = [gv(t) for pair in tapes for t in pair]
    ups = [gv(b["dhs"][:n]), gv(b["dhT"][:n]), gv(b["dcT"][:n]), gv(a["dhT"][:n]), gv(a["dcT"][:n])]
    shapes = {"dK1": (F, N4), "dR1": (H, N4), "db1": (N4,), "dK2": (H, N4), "dR2": (H, N4), "db2": (N4,)}
    base = {k: G.accumulate_base("%s %s" % (cid, k), s) for k, s in shapes.items()} if accumulate else {}
    outs = {"dz1": out_view((n, T, N4)), "dz2": out_view((n, T, N4))}
    outs.update({k: out_view(s, base.get(k), row=N4) for k, s in shapes.items()})
    outs.update({k: out_view((n, H)) for k in ("dh0_1", "dc0_1", "dh0_2", "dc0_2")})
    L = _lib.lib()
    order = ("dz1", "dz2", "dK1", "dR1", "db1", "dK2", "dR2", "db2", "dh0_1", "dc0_1", "dh0_2", "dc0_2")

    def call():
        buf = bufs[1].get(L.fov_lstm_stack2_bwd_workspace_bytes(n, T, F, H), x.device)
        ops.check(L.fov_lstm_stack2_bwd(ptr(x), ptr(R1), ptr(K2), ptr(R2), *[ptr(t) for t in st], *[ptr(t) for t in tp], *[ptr(t) for t in ups],
                                        *[ptr(outs[k].v) for k in order], n, T, F, H, ops.act_code(act), 1 if accumulate else 0, buf.data_ptr(),
                                        buf.numel(), ops._stream()))
    got, trace = traced(capfd, lambda: twice(call, outs, bufs[1].check), env)
    assert recurrent_launches(trace) == ["two-layer BPTT"] and ("wgrad_rows" in launches(trace)) == (not env), launches(trace)
    return got, base


@pytest.mark.parametrize("cid,form,B,F,T", [c for c in G.stack2_cases() if c[1][2] == "f32"], ids=[c[0] for c in G.stack2_cases() if c[1][2] == "f32"])
def test_two_layer_bptt_on_guarded_views(capfd, bufs, cid, form, B, F, T):
    """fov_lstm_stack2_bwd on the GPU's own tapes: both layers' dz, weight and state gradients; overwrite with initial states,
    accumulate without; and with FOV_NO_WGRAD_GROUP=1, where db1 and db2 are the sums the kernel formed over its own rows."""
    from longterm360fov_amd import ops
    H = form[3]
    act, rows = G.act_of(cid), G.round_up(B)
    assert ops.lstm_stack2_bwd_supported(B, T, F, H) and ops.lstm_stack2_bwd_supported(rows, T, F, H)
    a, b = G.stack2_inputs(cid, B, T, F, H, rows=rows)
    for state, accumulate, env in ((True, False, {}), (False, True, {}), (True, True, {"FOV_NO_WGRAD_GROUP": "1"})):
        tapes = stack2_tape(ops, bufs, a, b, B, act, state)
        got, base = stack2_backward(ops, capfd, bufs, a, b, tapes, B, T, F, H, act, state, accumulate, cid, env)
        st = lambda q: (q["h0"][:B], q["c0"][:B]) if state else None
        ups = (b["dhs"][:B], b["dhT"][:B], b["dcT"][:B], a["dhT"][:B], a["dcT"][:B])
        ref = O.regime_stack2_backward([(a["K"], a["R"], a["b"]), (b["K"], b["R"], b["b"])], a["x"][:B], [st(a), st(b)], tapes, ups, act)
        for k, v in base.items():
            ref[k] = ref[k] + v
        grads("%s state=%d acc=%d %s" % (cid, state, accumulate, " ".join(env)), "two-layer BPTT", got, ref)
        if rows != B:
            tapes_full = stack2_tape(ops, bufs, a, b, rows, act, state)
            full, _ = stack2_backward(ops, capfd, bufs, a, b, tapes_full, rows, T, F, H, act, state, accumulate, cid, env)
            for k in ("dz1", "dz2", "dh0_1", "dc0_1", "dh0_2", "dc0_2"):
                assert same_bits(full[k][:B], got[k]), "%s %s: a live row depends on the rows behind it" % (cid, k)


# ---------------------------------------------------------------------------------------------------------------------
# the fused others-mixing decoder: fov_mix_decoder_fwd / _bwd and their bf16 forms, every tape an OutView
# ---------------------------------------------------------------------------------------------------------------------
MIX_TAPES = ("P", "H1", "C1", "H2", "C2", "res1", "res2")
MIX_GRADS = ("DZ1", "DZ2", "dpre_m", "dpre_p", "dh1_0", "dc1_0", "dh2_0", "dc2_0")


def mix_run(ops, capfd, bufs, p, n, T, act, dtype):
    """Forward with tapes and final states, then the backward on those tapes -> (forward outputs, backward outputs)."""
    H, O_ = G.MIX_H, G.MIX_O
    bf = dtype == "bf16"
    w, Wp = {k: gv(v) for k, v in p["w"].items()}, gv(p["Wp"])
    ins = [gv(p[k][:n]) for k in ("dec0", "h1", "c1", "h2", "c2", "oth")]
    outs = {"M": out_view((T, n, O_)), "P": out_view((T, n, O_)), "res1": out_view((T, n, 5, H)), "res2": out_view((T, n, 5, H))}
    outs.update({k: out_view((T, n, H)) for k in ("H1", "C1", "H2", "C2")})
    outs.update({k: out_view((n, H)) for k in ("h1T", "c1T", "h2T", "c2T")})
    call = lambda: ops.mix_decoder(*ins, w, Wp, T, act=act, workspace=bufs[0], out=outs["M"].v, train={k: outs[k].v for k in MIX_TAPES},
                                   final_state=[outs[k].v for k in ("h1T", "c1T", "h2T", "c2T")], dtype=dtype)
    fw, trace = traced(capfd, lambda: twice(call, outs, bufs[0].check), {})
    name = "mix_decoder_bf16" if bf else "mix_decoder"
    assert [l for l in launches(trace) if "prepack" not in l] == [name] * 2, launches(trace)
    for a_, b_ in (("H1", "h1T"), ("C1", "c1T"), ("H2", "h2T"), ("C2", "c2T")):
        assert same_bits(fw[a_][-1], fw[b_])
    dloss = (np.transpose(p["G"][:n], (1, 0, 2)) * (1 - fw["M"] * fw["M"])).astype(np.float32)
    C1f, C2f = np.concatenate([p["c1"][:n][None], fw["C1"]]), np.concatenate([p["c2"][:n][None], fw["C2"]])
    bins = [gv(a) for a in (fw["M"], fw["P"], dloss, fw["res1"], fw["res2"], C1f, C2f)]
    bouts = {"DZ1": out_view((T, n, 4 * H)), "DZ2": out_view((T, n, 4 * H)), "dpre_m": out_view((T, n, O_)), "dpre_p": out_view((T, n, O_))}
    bouts.update({k: out_view((n, H)) for k in MIX_GRADS[4:]})
    bcall = lambda: ops.mix_decoder_bwd(*bins, w, Wp, {k: o.v for k, o in bouts.items()}, act=act, workspace=bufs[3], dtype=dtype)
    bw, trace = traced(capfd, lambda: twice(bcall, bouts, bufs[3].check), {})
    name = "mix_decoder_bwd_bf16" if bf else "mix_decoder_bwd"
    assert [l for l in launches(trace) if "prepack" not in l] == [name] * 2, launches(trace)
    return fw, bw, dloss


@pytest.mark.parametrize("cid,form,B,T", G.mix_cases(), ids=[c[0] for c in G.mix_cases()])
def test_mix_decoder_forward_and_backward_on_guarded_views(capfd, bufs, cid, form, B, T):
    from longterm360fov_amd import ops
    dtype = form[1]
    bf, act, rows = dtype == "bf16", G.act_of(cid), G.round_up(B)
    assert ops.mix_decoder_supported(G.MIX_H, G.MIX_O)
    p = G.mix_inputs(cid, B, T, rows=rows)
    fw, bw, dloss = mix_run(ops, capfd, bufs, p, B, T, act, dtype)
    ref = G.mix_forward_reference(p, B, T, act, bf)
    family = "mix_decoder" + ("_bf16" if bf else "")
    for k in ("M",) + MIX_TAPES:
        if bf:
            r = O.regime_error(fw[k], ref[k], "bf16") if k.startswith("res") else float(np.abs(fw[k] - ref[k]).max()) / BF16_TIGHT
            print("%-64s error / bound %.3f" % (cid + " " + k, r))
            note(family, r)
            assert r <= 1.0, (cid, k, r)
        else:
            parity("%s %s" % (cid, k), family, fw[k], ref[k])
    bref = G.mix_backward_reference(p, B, {k: fw[k] for k in ("M",) + MIX_TAPES}, dloss, act, bf)
    if bf:
        for k in MIX_GRADS:
            bound = STATE if k in ("dh1_0", "dh2_0") else PER_KERNEL
            note(family + " backward", near("%s %s" % (cid, k), bw[k], bref[k], bound) / bound)
    else:
        grads(cid + " backward", family + " backward", bw, {k: bref[k] for k in MIX_GRADS})
    if rows != B:
        fw2, bw2, _ = mix_run(ops, capfd, bufs, p, rows, T, act, dtype)
        for k in ("M",) + MIX_TAPES:
            assert same_bits(fw2[k][:, :B], fw[k]), "%s %s: a live row depends on the rows behind it" % (cid, k)
        for k in MIX_GRADS:
            part = bw2[k][:, :B] if bw[k].ndim == 3 else bw2[k][:B]
            assert same_bits(part, bw[k]), "%s %s: a live row depends on the rows behind it" % (cid, k)


# ---------------------------------------------------------------------------------------------------------------------
# heads: fov_tf_head_fwd / _bwd, fov_mlp_head_fwd / _bwd, fov_dense_mse_head.  tests/test_gpu_lstm_py_heads.py states its bounds
# inline (outputs 1e-3 |ref| + 2e-5; gradients 2e-4 of the tensor's max + 1e-6); they are restated here under names.
# ---------------------------------------------------------------------------------------------------------------------
from test_guarded_views_host import HEAD_GRAD, HEAD_GRAD_FLOOR, HEAD_OUT_ATOL, HEAD_OUT_RTOL  # noqa: E402


def head_out(tag, family, got, ref):
    ref = f64(ref)
    r = float((np.abs(f64(got) - ref) / (HEAD_OUT_RTOL * np.abs(ref) + HEAD_OUT_ATOL)).max())
    print("%-64s error / bound %.3f" % (tag, r))
    note(family, r)
    assert r <= 1.0, (tag, r)


def head_grad(tag, family, got, ref):
    ref = f64(ref)
    r = G.head_grad_bounds(got, ref)
    assert HEAD_GRAD == 2e-4 and HEAD_GRAD_FLOOR == 1e-6
    print("%-64s error / bound %.3f" % (tag, r))
    note(family, r)
    assert r <= 1.0, (tag, r)


@pytest.mark.parametrize("shape,accumulate", G.TF_HEAD_CASES)
def test_tf_head_on_guarded_views(capfd, shape, accumulate):
    from longterm360fov_amd import _lib, ops
    B, H, M, O_ = shape
    name, rows = "tf head B%d" % B, G.round_up(B)
    assert ops.tf_head_supported(B, H, M, O_) and ops.tf_head_supported(rows, H, M, O_)
    w, h_all, dmu_all, dvar_all = G.tf_head_inputs(name, B, H, M, O_, rows=rows)
    wv = {k: gv(v) for k, v in w.items()}
    L = _lib.lib()

    def run(n):
        h = gv(h_all[:n])
        fo = {"a1": out_view((n, M)), "mu": out_view((n, O_)), "a3": out_view((n, M)), "var": out_view((n, O_))}
        fcall = lambda: ops.check(L.fov_tf_head_fwd(ptr(h), *[ptr(wv[k]) for k in G.TF_NAMES], *[ptr(fo[k].v) for k in ("a1", "mu", "a3", "var")],
                                                    n, H, M, O_, ops._stream()))
        fw, trace = traced(capfd, lambda: twice(fcall, fo, lambda: None), {})
        assert set(launches(trace)) == {"tf head forward"}, launches(trace)
        base = {k: G.accumulate_base("%s %s" % (name, k), w[k].shape) for k in G.TF_NAMES} if accumulate else {}
        bo = {k: out_view(w[k].shape, base.get(k)) for k in G.TF_NAMES}
        bo["dh"] = out_view((n, H))
        tape = [gv(fw[k]) for k in ("a1", "mu", "a3", "var")]
        dmu, dvar = gv(dmu_all[:n]), gv(dvar_all[:n])
        bcall = lambda: ops.check(L.fov_tf_head_bwd(ptr(h), ptr(wv["mu_W1"]), ptr(wv["mu_W2"]), ptr(wv["var_W1"]), ptr(wv["var_W2"]), *[ptr(t) for t in tape],
                                                    ptr(dmu), ptr(dvar), *[ptr(bo[k].v) for k in G.TF_NAMES], ptr(bo["dh"].v), n, H, M, O_,
                                                    1 if accumulate else 0, ops._stream()))
        bw, trace = traced(capfd, lambda: twice(bcall, bo, lambda: None), {})
        assert "tf head backward" in launches(trace), launches(trace)
        return fw, bw, base
    fw, bw, base = run(B)
    w64 = {k: f64(v) for k, v in w.items()}
    mu, var = O.tf_mean_var_head(f64(h_all[:B]), w64)
    head_out(name + " mu", "tf head", fw["mu"], mu)
    head_out(name + " var", "tf head", fw["var"], var)
    head_out(name + " a1", "tf head", fw["a1"], np.maximum(f64(h_all[:B]) @ w64["mu_W1"] + w64["mu_b1"], 0))
    head_out(name + " a3", "tf head", fw["a3"], np.maximum(f64(h_all[:B]) @ w64["var_W1"] + w64["var_b1"], 0))
    ref = G.tf_head_backward_reference(h_all[:B], w, fw["a1"], fw["mu"], fw["a3"], fw["var"], dmu_all[:B], dvar_all[:B])
    for k in G.TF_NAMES + ("dh",):
        head_grad("%s %s" % (name, k), "tf head backward", bw[k], ref[k] + base.get(k, 0))
    fw2, bw2, _ = run(rows)
    assert all(same_bits(fw2[k][:B], fw[k]) for k in fw) and same_bits(bw2["dh"][:B], bw["dh"]), name + ": a live row depends on the rows behind it"


@pytest.mark.parametrize("kind,B,H,n_mix,with_masks,accumulate", G.MLP_HEAD_CASES)
def test_mlp_head_on_guarded_views(capfd, bufs, kind, B, H, n_mix, with_masks, accumulate):
    """fov_mlp_head_fwd / _bwd on the mixture head and the raw head: every layer's output, every weight and bias gradient, dx."""
    from longterm360fov_amd import _lib, ops
    name, rows = "mlp %s B%d H%d" % (kind, B, H), G.round_up(B)
    head, layers, h_all, masks_all, dlast_all = G.mlp_head_inputs(kind, B, H, n_mix, with_masks, rows=rows)
    nl = len(layers)
    lv = [(gv(W), gv(b), a) for W, b, a in layers]
    lib = _lib.lib()
    P4 = ops._PTR4

    def run(n):
        assert ops.mlp_head_supported(n, [H] + [W.shape[1] for W, _, _ in layers])
        x = gv(h_all[:n])
        dims, codes, Wp, bp = ops._mlp_tables(lv, H)
        mv = None if masks_all is None else [gv(m[:n]) for m in masks_all]
        mp = None if mv is None else P4(*([ptr(m) for m in mv] + [None] * (4 - len(mv))))
        fo = {"act%d" % l: out_view((n, layers[l][0].shape[1])) for l in range(nl)}
        ap = P4(*([fo["act%d" % l].v.data_ptr() for l in range(nl)] + [None] * (4 - nl)))
        fcall = lambda: ops.check(lib.fov_mlp_head_fwd(ptr(x), Wp, bp, mp, ap, dims, codes, nl, 1 if n_mix else 0, int(n_mix), n, ops._stream()))
        fw, trace = traced(capfd, lambda: twice(fcall, fo, lambda: None), {})
        assert set(launches(trace)) == {"mlp head forward"}, launches(trace)
        base = {}
        if accumulate:
            for l, (W, b, _) in enumerate(layers):
                base["gW%d" % l], base["gb%d" % l] = G.accumulate_base("%s gW%d" % (name, l), W.shape), G.accumulate_base("%s gb%d" % (name, l), b.shape)
        bo = {"dx": out_view((n, H))}
        for l, (W, b, _) in enumerate(layers):
            bo["gW%d" % l], bo["gb%d" % l] = out_view(W.shape, base.get("gW%d" % l)), out_view(b.shape, base.get("gb%d" % l))
        tape = [gv(fw["act%d" % l]) for l in range(nl)]
        tp = P4(*([ptr(t) for t in tape] + [None] * (4 - nl)))
        gWp = P4(*([bo["gW%d" % l].v.data_ptr() for l in range(nl)] + [None] * (4 - nl)))
        gbp = P4(*([bo["gb%d" % l].v.data_ptr() for l in range(nl)] + [None] * (4 - nl)))
        dl = gv(dlast_all[:n])

        def bcall():
            buf = bufs[2].get(lib.fov_mlp_head_bwd_workspace_bytes(n, nl, dims), x.device)
            ops.check(lib.fov_mlp_head_bwd(ptr(x), Wp, mp, tp, ptr(dl), gWp, gbp, ptr(bo["dx"].v), dims, codes, nl, n, 1 if accumulate else 0,
                                           buf.data_ptr(), buf.numel(), ops._stream()))
        bw, trace = traced(capfd, lambda: twice(bcall, bo, lambda: None), {})
        assert "mlp head weight gradients" in launches(trace), launches(trace)
        return fw, bw, base
    fw, bw, base = run(B)
    masks = None if masks_all is None else [m[:B] for m in masks_all]
    out_ref, hidden = G.mlp_head_forward_reference(kind, h_all[:B], head, masks, n_mix)
    head_out(name + " output", "mlp head", fw["act%d" % (nl - 1)], out_ref)
    for l, a in enumerate(hidden or ()):
        head_out("%s layer %d" % (name, l), "mlp head", fw["act%d" % l], a)
    gW, gb, dx = G.mlp_head_backward_reference(h_all[:B], layers, [fw["act%d" % l] for l in range(nl)], masks, dlast_all[:B])
    for l in range(nl):
        head_grad("%s gW%d" % (name, l), "mlp head backward", bw["gW%d" % l], gW[l] + base.get("gW%d" % l, 0))
        head_grad("%s gb%d" % (name, l), "mlp head backward", bw["gb%d" % l], gb[l] + base.get("gb%d" % l, 0))
    head_grad(name + " dx", "mlp head backward", bw["dx"], dx)
    fw2, bw2, _ = run(rows)
    assert all(same_bits(fw2[k][:B], fw[k]) for k in fw) and same_bits(bw2["dx"][:B], bw["dx"]), name + ": a live row depends on the rows behind it"


@pytest.mark.parametrize("N,H,O_,activation", G.DENSE_MSE_CASES)
def test_dense_mse_head_on_guarded_views(capfd, bufs, N, H, O_, activation):
    """Dense + mean squared error, forward and backward in one launch: y, the loss, dX, dW, db."""
    from longterm360fov_amd import ops
    name = "dense-mse-%d" % N
    assert ops.dense_mse_head_supported(N, H, O_)
    p, target = G.dense_mse_inputs(N, H, O_)
    hs, W, b, tg = gv(p["x"]), gv(p["W"]), gv(p["b"]), gv(target)
    outs = {"y": out_view((N, O_)), "dX": out_view((N, H)), "dW": out_view((H, O_)), "db": out_view((O_,)), "loss": out_view((1,))}
    call = lambda: ops.dense_mse_head(hs, W, b, tg, activation, dW=outs["dW"].v, db=outs["db"].v, loss=outs["loss"].v, weight=0.5, scratch=bufs[2],
                                      dx=outs["dX"].v, y=outs["y"].v)
    got, trace = traced(capfd, lambda: twice(call, outs, lambda: None), {})
    assert launches(trace) == ["dense_mse_head"] * 2, launches(trace)
    ref = G.dense_mse_reference(p["x"], p["W"], p["b"], target, activation, 0.5)
    parity(name + " y", "dense_mse_head", got["y"], ref["y"])
    assert abs(float(got["loss"][0]) - float(ref["loss"][0])) <= 1e-5 * float(ref["loss"][0]) + 1e-9
    grads(name, "dense_mse_head", got, {k: ref[k] for k in ("dX", "dW", "db")})


# ---------------------------------------------------------------------------------------------------------------------
# alignment-routed forms: only the operand the launcher branches on is misaligned (off = 1: four bytes behind a 16-byte boundary)
# ---------------------------------------------------------------------------------------------------------------------
def test_mix_head_forward_refuses_a_misaligned_h():
    """fov_mix_head_fwd reads h with 16-byte loads and says so: a misaligned h is refused, nothing is written."""
    from longterm360fov_amd import ops
    N, H, O_ = 17, 256, 6
    z = lambda *s: gv(np.zeros(s, np.float32))
    p, m = out_view((N, O_)), out_view((N, O_))
    with pytest.raises(ops.FovError, match="16-byte aligned"):
        ops.mix_head_fwd(gv(np.zeros((N, H), np.float32), off=1), z(H, O_), z(O_), z(O_, O_), z(N, O_), p.v, m.v)
    assert p.untouched() and m.untouched()


@pytest.mark.parametrize("H,F,aligned_form,impl,env", [(256, 256, "wide LSTM", "auto", {"FOV_NO_WIDE16": "1"}), (128, 128, "wide16 LSTM", "auto", {}),
                                                       (256, 256, "wide16 LSTM", "auto", {})])
def test_layer_forward_with_a_misaligned_x_takes_the_generic_kernel(capfd, bufs, H, F, aligned_form, impl, env):
    """lstm_wide.hip (F > 96 at H = 256) and lstm_wide16.hip's F = H form stage x with 16-byte loads; the launcher routes an x
    that is not 16-byte aligned to the generic kernel instead.  Same bound as the aligned twin, which runs first."""
    from longterm360fov_amd import ops
    B, T = 17, 2
    cid = "misaligned-x-%s-H%d" % (aligned_form, H)
    act = G.act_of(cid)
    inp = G.layer_inputs(cid, B, T, F, H)
    ref = dict(zip(("hs", "hT", "cT", "res"), G.layer_reference(inp, act, True)))
    K, R, b, h0, c0 = (gv(inp[k]) for k in ("K", "R", "b", "h0", "c0"))
    for off, want in ((0, aligned_form), (1, "generic")):
        x = gv(inp["x"], off)
        outs = {"hs": out_view((B, T, H)), "hT": out_view((B, H)), "cT": out_view((B, H)), "res": out_view((B, T, 5, H))}
        call = lambda: ops.lstm_seq_train(x, K, R, b, h0, c0, act=act, impl=impl, workspace=bufs[0],
                                          out=(outs["hs"].v, outs["hT"].v, outs["cT"].v, outs["res"].v))
        got, trace = traced(capfd, lambda: twice(call, outs, bufs[0].check), env)
        assert recurrent_launches(trace) == [want], launches(trace)
        for k in ref:
            parity("%s x off=%d %s" % (cid, off, k), "alignment-routed", got[k], ref[k])


@pytest.mark.parametrize("H,other", [(512, "lstm_bwd_pointwise"), (128, "bwd cluster")])
def test_layer_backward_with_a_misaligned_R_leaves_the_16_unit_kernel(capfd, bufs, H, other):
    """lstm_bwd16.hip loads R with 16-byte loads; lstm_seq_bwd takes it only for an aligned R.  Width 512 then walks the steps
    (pointwise + product), width 128 takes lstm_bwd_cluster.hip."""
    from longterm360fov_amd import ops
    form = [f for f in G.BACKWARD_FORMS if f[0] == "bwd16-%d" % H][0]
    B, T, F = 17, 2, 90
    cid = "misaligned-R-H%d" % H
    act, variant = G.act_of(cid), G.BACKWARD_VARIANTS[0]
    inp = G.layer_inputs(cid, B, T, F, H)
    tape = backward_tape(ops, bufs, form, inp, B, F, T, act, True)
    ref = G.backward_reference(inp, tape[0], tape[1], variant, act)
    for off, want in ((0, "16-unit BPTT"), (1, other)):
        got, _, trace = layer_backward(ops, capfd, bufs, form, inp, tape, B, T, F, act, variant, cid, offs={"R": off})
        assert recurrent_launches(trace) == [want], launches(trace)
        grads("%s R off=%d" % (cid, off), "alignment-routed", got, ref)


@pytest.mark.parametrize("operand", ["K", "dx"])
def test_bwd8_with_a_misaligned_K_or_dx_forms_dx_by_the_product(capfd, bufs, operand):
    """lstm_bwd8's in-kernel dx reads K with 16-byte loads and its reduce stores dx 16 bytes at a time; lstm_seq_bwd asks for it only
    when both are 16-byte aligned, else the NT product behind the recurrence."""
    from longterm360fov_amd import ops
    form = [f for f in G.BACKWARD_FORMS if f[0] == "bwd8-256"][0]
    cid, B, T, F, H = "misaligned-" + operand, 17, 2, 256, 256
    act, variant = G.act_of(cid), G.BACKWARD_VARIANTS[0]
    inp = G.layer_inputs(cid, B, T, F, H)
    tape = backward_tape(ops, bufs, form, inp, B, F, T, act, True)
    ref = G.backward_reference(inp, tape[0], tape[1], variant, act)
    for off in (0, 1):
        got, _, trace = layer_backward(ops, capfd, bufs, form, inp, tape, B, T, F, act, variant, cid, offs={operand: off})
        assert recurrent_launches(trace) == ["8-group BPTT"]
        assert bool(re.search(r"gemm_f32 next: M=%d N=%d " % (B * T, F), trace)) == (off == 1), trace
        grads("%s off=%d" % (cid, off), "alignment-routed", got, ref)


def test_bf16_bptt_with_a_misaligned_K_forms_dx_in_fp32(capfd, bufs):
    """fov_lstm_seq_bwd_bf16 forms dx = dz K^T on bf16 operands (in the kernel at F = 256) only for a 16-byte aligned K; a K four
    bytes off takes the fp32 NT product, and the reference then leaves that product unrounded."""
    from longterm360fov_amd import ops
    form = [f for f in G.BACKWARD_FORMS if f[0] == "bwd8-256-bf16"][0]
    cid, B, T, F, H = "misaligned-K-bf16", 17, 2, 256, 256
    act, variant = G.act_of(cid), G.BACKWARD_VARIANTS[0]
    inp = G.layer_inputs(cid, B, T, F, H)
    tape = backward_tape(ops, bufs, form, inp, B, F, T, act, True)
    for off in (0, 1):
        got, _, trace = layer_backward(ops, capfd, bufs, form, inp, tape, B, T, F, act, variant, cid, offs={"K": off})
        assert recurrent_launches(trace) == ["8-group BPTT"] and "gemm_bf16_nt" not in launches(trace)
        assert bool(re.search(r"gemm_f32 next: M=%d N=%d " % (B * T, F), trace)) == (off == 1), trace
        ref = O.lstm_layer_backward(*[f64(inp[k]) for k in ("x", "K", "R", "h0", "c0")], f64(tape[0]), f64(tape[1]), f64(inp["dhs"]), f64(inp["dhT"]),
                                    f64(inp["dcT"]), act=act, round_rec=True, round_dx=(off == 0), round_wgrad=True)
        bf16_grads("%s K off=%d" % (cid, off), "alignment-routed", got, ref)


@pytest.mark.parametrize("H,F,B,T,kernel", [(64, 90, 17, 3, "wgrad_rows"), (512, 90, 30, 23, "wgrad_group")])
def test_few_row_weight_gradients_with_a_misaligned_dz_take_the_products(capfd, bufs, H, F, B, T, kernel):
    """wgrad_rows and wgrad_group read dz with 16-byte loads; fov_lstm_seq_wgrad takes them only for a 16-byte aligned dz.  A dz
    four bytes off goes to the GEMMs (their own alignment forms: tests/test_gpu_gemm_forms.py)."""
    from longterm360fov_amd import ops
    name = "misaligned-dz-%d" % H
    p = wgrad_inputs(name, B, T, F, H)
    ref = wgrad_reference(p, True)
    x, hs, h0 = gv(p["x"]), gv(p["hs"]), gv(p["h0"])
    for off in (0, 1):
        dz = gv(p["dz"], off)
        outs, _ = wgrad_outs(name, F, H, False)
        call = lambda: ops.lstm_seq_wgrad(x, hs, dz, outs["dK"].v, outs["dR"].v, outs["db"].v, h0=h0, scratch=bufs[2])
        got, trace = traced(capfd, lambda: twice(call, outs, torch.cuda.synchronize), {})
        assert (kernel in launches(trace)) == (off == 0) and ("gemm_f32" in launches(trace)) == (off == 1), launches(trace)
        assert not {"wgrad_rows", "wgrad_group"} - {kernel} & set(launches(trace))
        grads("%s off=%d" % (name, off), "alignment-routed", got, ref)


def test_few_row_weight_gradients_into_misaligned_outputs_take_wgrad_group(capfd, bufs):
    """wgrad_rows stores 16 bytes at a time and is taken only for 16-byte aligned dK, dR, db; at H = 512 outputs four bytes off go
    to wgrad_group, whose result tile falls back to scalar stores (its own branch on the output's address)."""
    from longterm360fov_amd import ops
    name, H, F, B, T = "misaligned-dK", 512, 96, 17, 2
    p = wgrad_inputs(name, B, T, F, H)
    ref = wgrad_reference(p, False)
    x, hs, dz = gv(p["x"]), gv(p["hs"]), gv(p["dz"])
    for off, kernel in ((0, "wgrad_rows"), (1, "wgrad_group")):
        outs = {k: out_view(s_, off=off, row=4 * H) for k, s_ in (("dK", (F, 4 * H)), ("dR", (H, 4 * H)), ("db", (4 * H,)))}
        call = lambda: ops.lstm_seq_wgrad(x, hs, dz, outs["dK"].v, outs["dR"].v, outs["db"].v, scratch=bufs[2])
        got, trace = traced(capfd, lambda: twice(call, outs, torch.cuda.synchronize), {})
        assert launches(trace) == [kernel] * 2, launches(trace)
        assert off == 0 or trace.count("wgrad_group: 2 problems, ") == trace.count(" vector_stores 0\n") == 2, trace
        grads("%s off=%d" % (name, off), "alignment-routed", got, ref)


def test_bf16_kernels_stage_a_misaligned_wide_x_by_scalar_loads(capfd, bufs):
    """lstm_layer_bf16.hip and lstm_s2s_bf16.hip stage a 256-wide x with 16-byte loads only when it is 16-byte aligned; a misaligned
    x takes the scalar staging, which the trace names.  Same bound as the aligned twin; and since the staging only copies, the two
    runs give the same bits."""
    from longterm360fov_amd import ops
    B, T, F, H = 17, 2, 256, 256
    cid = "misaligned-x-bf16"
    act = G.act_of(cid)
    inp = G.layer_inputs(cid, B, T, F, H)
    ref = dict(zip(("hs", "hT", "cT", "res"), G.layer_reference(inp, act, True, True)))
    K, R, b, h0, c0 = (gv(inp[k]) for k in ("K", "R", "b", "h0", "c0"))
    runs = []
    for off in (0, 1):
        x = gv(inp["x"], off)
        outs = {"hs": out_view((B, T, H)), "hT": out_view((B, H)), "cT": out_view((B, H)), "res": out_view((B, T, 5, H))}
        call = lambda: ops.lstm_seq_bf16(x, K, R, b, h0, c0, act=act, workspace=bufs[0], out=(outs["hs"].v, outs["hT"].v, outs["cT"].v, outs["res"].v))
        got, trace = traced(capfd, lambda: twice(call, outs, bufs[0].check), {})
        assert launches(trace) == ["bf16 LSTM layer (%s x)" % ("scalar" if off else "vector")] * 2, launches(trace)
        forward_checks("%s layer x off=%d" % (cid, off), "alignment-routed", got, ref, True)
        runs.append(got)
    assert all(same_bits(runs[0][k], runs[1][k]) for k in runs[0]), "bf16 layer: the vector and the scalar x staging differ"
    p = G.decode_inputs(cid, B, 2, 2, 256, H)
    w = {k: gv(v) for k, v in p["w"].items()}
    dref = O.regime_decode(p["enc"], p["dec0"], p["w"], 2, act, True)
    runs = []
    for off in (0, 1):
        enc, dec0 = gv(p["enc"], off), gv(p["dec0"])
        outs = {"out": out_view((B, 2, G.F_DEC)), "hT": out_view((B, H)), "cT": out_view((B, H))}
        call = lambda: ops.seq2seq_decode(enc, dec0, w, 2, act=act, workspace=bufs[0], out=outs["out"].v, hT=outs["hT"].v, cT=outs["cT"].v, dtype="bf16")
        got, trace = traced(capfd, lambda: twice(call, outs, bufs[0].check), {})
        assert launches(trace) == ["bf16 seq2seq decode (%s x)" % ("scalar" if off else "vector")] * 2, launches(trace)
        forward_checks("%s decode enc_in off=%d" % (cid, off), "alignment-routed", got, {k: dref[k] for k in ("out", "hT", "cT")}, True)
        runs.append(got)
    assert all(same_bits(runs[0][k], runs[1][k]) for k in runs[0]), "bf16 decode: the vector and the scalar x staging differ"


def test_dense_forward_with_a_misaligned_x_takes_the_scalar_staging(capfd):
    """dense_small_kernel<4> stages x with 16-byte loads and is taken for In % 4 == 0 and an aligned x only; a misaligned x takes
    dense_small_kernel<1>, which the trace names."""
    from longterm360fov_amd import ops
    name, N, In, Out = "misaligned-x-dense", 85, 256, 6
    p = G.dense_inputs(name, N, In, Out)
    W, b = gv(p["W"]), gv(p["b"])
    ref = O.dense(f64(p["x"]), f64(p["W"]), f64(p["b"]), "tanh")
    for off in (0, 1):
        x, outs = gv(p["x"], off), {"y": out_view((N, Out))}
        got, trace = traced(capfd, lambda: twice(lambda: ops.dense(x, W, b, "tanh", out=outs["y"].v), outs, lambda: None), {})
        assert launches(trace) == [G.DENSE_16S if off else G.DENSE_16V] * 2, launches(trace)
        parity("%s off=%d" % (name, off), "alignment-routed", got["y"], ref)


def test_zz_worst_error_over_bound_per_family():
    """Prints the table of DESIGN.md (Tests): cases and worst error over bound per kernel family of this file's run."""
    for fam in sorted(WORST):
        print("%-28s %4d checks   worst error / bound %.3f" % (fam, WORST[fam][0], WORST[fam][1]))
    assert all(w[1] <= 1.0 for w in WORST.values())
