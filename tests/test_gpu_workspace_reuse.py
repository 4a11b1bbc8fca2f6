"""Exchange kernels on a REUSED workspace: other data, other shapes and other kernels on one workspace, tile rounds, epoch bases,
the tags themselves, and the area behind the granules.  tests/test_workspace_reuse_host.py owns the case table (one row per
exchanging launch, from the guarded-view tables), tag_report and the rule which outputs are bit-identical across group counts.

Every call goes through ops on ONE workspace that is pre-sized for the largest case (Workspace.get hands out a new buffer when
a call asks for more, and nothing would be reused: data_ptr is asserted unchanged around every launch).  Around every launch the
granule area [256, 256 + 64 MB) is cloned on the device and the header read; tag_report must be empty, ST_TIMEOUT 0, ST_LAUNCHES
grown by the exchange launches the trace shows, and the trace must name the row's form.  ws.check() follows every launch.

A  X (B 30, T 3), Y (B 17, T 2), Z (B 30, T 3, other data) on one workspace: each the same bits as on a fresh workspace; Z within
   its fp64 bound (the references and bounds of tests/test_gpu_ragged_guarded.py).
C  all rows one after the other on one workspace, then in reverse order on a second one.
D  B = 33 (three tiles, one live row in the last) under FOV_DBG_RESIDENT_LIMIT = G and 2 G against the unlimited run.
E  four epoch bases set by fov_debug_set_epoch, the last one crossed by the first launch (re-zero in front of it).
F  fov_mix_decoder_prepack's mark on a workspace whose tail another call writes before the fused decoder runs."""
import contextlib
import os
import re
import sys

import numpy as np
import pytest
import torch

import test_guarded_views_host as G
import test_workspace_reuse_host as W
from oracle import fov_oracle as O
from test_gpu_bf16 import TIGHT as BF16_TIGHT
from test_gpu_bf16_backward import PER_KERNEL, STATE, near
from test_gpu_parity import assert_parity
from test_guarded_views_host import f64

pytestmark = pytest.mark.gpu

LAUNCHED = re.compile(r"\[fov trace\] launched: (.+)")
EXCHANGE = {"cluster", "fused cluster", "wide LSTM", "wide16 LSTM", "seq2seq decode (wide16)", "two-layer width-512", "bf16 two-layer",
            "bf16 LSTM layer (narrow x)", "bf16 LSTM layer (vector x)", "bf16 LSTM layer (scalar x)", "bf16 seq2seq decode (narrow x)",
            "bf16 seq2seq decode (vector x)", "bf16 seq2seq decode (scalar x)", "bwd cluster", "8-group BPTT", "16-unit BPTT", "two-layer BPTT",
            "mix_decoder", "mix_decoder_bf16", "mix_decoder_bwd", "mix_decoder_bwd_bf16"}
MIX_TAPES = ("P", "H1", "C1", "H2", "C2", "res1", "res2")
MIX_GRADS = ("DZ1", "DZ2", "dpre_m", "dpre_p", "dh1_0", "dc1_0", "dh2_0", "dc2_0")
BWD_VARIANT = dict(state=True, ups="shc")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def apart(*shapes):
    """Tensors of the given shapes in ONE buffer, 64 floats apart.  The weight-gradient plan of lstm_seq_bwd looks at the addresses:
    db directly behind dR (and dR behind dK) selects the fused products (plan_products, lstm_train.hip), which form db themselves
    and sum in another order.  Separate torch allocations end up adjacent or not as the caching allocator pleases, so the same call
    would take one form on the reused workspace and the other on the fresh one; with a gap every run takes the separate products
    and db is the BPTT kernel's own sum."""
    sizes = [int(np.prod(s)) for s in shapes]
    buf = torch.empty(sum(sizes) + 64 * len(sizes), dtype=torch.float32, device="cuda")
    out, at = [], 0
    for s, n in zip(shapes, sizes):
        out.append(buf[at:at + n].view(s))
        at += n + 64
    return out


def host(t):
    return t.detach().cpu().numpy()


@contextlib.contextmanager
def knobs(env):
    """The row's knobs and FOV_DBG_TRACE=1; the library re-reads its environment now and once the caller's is back."""
    from longterm360fov_amd import _lib, ops
    env = dict(env, FOV_DBG_TRACE="1")
    before = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        _lib.lib().fov_reload_env()
        ops._sync_env()
        yield
    finally:
        for k, v in before.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        _lib.lib().fov_reload_env()
        ops._sync_env()


def traced(capfd, fn, env):
    before = capfd.readouterr()
    with knobs(env):
        r = fn()
        torch.cuda.synchronize()
    trace = capfd.readouterr().err
    sys.stdout.write(before.out)
    sys.stderr.write(before.err)
    return r, trace


# ---------------------------------------------------------------------------------------------------------------------
# one call of a row: inputs on the device, run(ws) -> its outputs, check(outputs) against the row's fp64 reference
# ---------------------------------------------------------------------------------------------------------------------
def aux_ws():
    """The workspace of the forward passes that make a backward case's tape (not under test)."""
    from longterm360fov_amd import ops
    if "aux" not in _CACHE:
        _CACHE["aux"] = ops.Workspace()
    return _CACHE["aux"]


_CACHE = {}


def need_bytes(row, B, T):
    from longterm360fov_amd import _lib, ops
    L = _lib.lib()
    kind, H, F, bf = row["kind"], row["H"], row["F"], row["dtype"] == "bf16"
    impl = ops.impl_code(row["impl"] or "auto")
    if kind == "backward":
        return L.fov_lstm_seq_bwd_workspace_bytes(B, T, F, H)
    if kind == "stack2_bwd":
        return L.fov_lstm_stack2_bwd_workspace_bytes(B, T, F, H)
    if kind == "mix_fwd":
        return L.fov_mix_decoder_workspace_bytes(B, H)
    if kind == "mix_bwd":
        return L.fov_mix_decoder_bwd_workspace_bytes(B, H)
    if bf:
        return L.fov_lstm_seq_workspace_bytes(B, T, 128, 256, ops.IMPL_CLUSTER)
    if kind == "decode":
        return L.fov_seq2seq_decode_workspace_bytes(B, T, T, F, G.F_DEC, H, impl)
    if kind == "decoder":
        return L.fov_seq2seq_decode_workspace_bytes(B, 0, T, 1, G.F_DEC, H, impl)
    if kind == "zx":
        return L.fov_lstm_seq_workspace_bytes(B, T, 1, H, impl)
    return L.fov_lstm_seq_workspace_bytes(B, T, F, H, ops.IMPL_AUTO if kind == "stack2" else impl)


def max_need():
    if "need" not in _CACHE:
        shapes = set(W.SHAPES) | {(W.ROUNDS_B, 3)}
        _CACHE["need"] = max(need_bytes(r, B, T) for r in W.ROWS for B, T in shapes)
    return _CACHE["need"]


def new_ws():
    """A fresh workspace of the size every case fits."""
    from longterm360fov_amd import ops
    ws = ops.Workspace()
    ws.get(max_need(), torch.device("cuda", torch.cuda.current_device()))
    return ws


class Call:
    def __init__(self, row, B, T, seed):
        from longterm360fov_amd import ops
        self.row, self.B, self.T = row, B, T
        self.cid = "%s reuse %s B%d T%d" % (row["name"], seed, B, T)
        self.act = G.act_of(self.cid)
        self.bf = row["dtype"] == "bf16"
        self.env = row["knobs"]
        getattr(self, "_make_" + row["kind"])(ops)

    # -- one layer -----------------------------------------------------------------------------------------------------
    def _make_layer(self, ops):
        r = self.row
        self.inp = inp = G.layer_inputs(self.cid, self.B, self.T, r["F"], r["H"])
        t = {k: dev(inp[k]) for k in ("x", "K", "R", "b", "h0", "c0")}

        def run(ws):
            if self.bf:
                o = ops.lstm_seq_bf16(t["x"], t["K"], t["R"], t["b"], t["h0"], t["c0"], act=self.act, workspace=ws)
            else:
                o = ops.lstm_seq_train(t["x"], t["K"], t["R"], t["b"], t["h0"], t["c0"], act=self.act, impl=r["impl"], workspace=ws)
            return dict(zip(("hs", "hT", "cT", "res"), o))
        self.run = run
        self.reference = lambda outs: dict(zip(("hs", "hT", "cT", "res"), G.layer_reference(inp, self.act, True, self.bf)))
        self.kindcheck = "forward"

    def _make_zx(self, ops):
        r = self.row
        H = r["H"]
        inp = G.layer_inputs(self.cid, self.B, self.T, 90, H)
        zx = (f64(inp["x"]) @ f64(inp["K"])).astype(np.float32)
        t = {k: dev(inp[k]) for k in ("R", "b", "h0", "c0")}
        zxd = dev(zx)

        def run(ws):
            res = torch.empty((self.B, self.T, 5, H), dtype=torch.float32, device="cuda")
            hs, hT, cT = ops.lstm_seq_zx(zxd, t["R"], t["b"], t["h0"], t["c0"], act=self.act, impl=r["impl"], workspace=ws, reserve=res)
            return {"hs": hs, "hT": hT, "cT": cT, "res": res}
        self.run = run
        self.reference = lambda outs: dict(zip(("hs", "hT", "cT", "res"), G.zx_reference(zx, inp["R"], inp["b"], inp["h0"], inp["c0"], self.act)))
        self.kindcheck = "forward"

    # -- decode --------------------------------------------------------------------------------------------------------
    def _make_decode(self, ops):
        r = self.row
        H, B, T = r["H"], self.B, self.T
        p = G.decode_inputs(self.cid, B, T, T, r["F"], H)
        w = {k: dev(v) for k, v in p["w"].items()}
        enc, dec0 = dev(p["enc"]), dev(p["dec0"])
        kw = {"dtype": "bf16"} if self.bf else {"impl": r["impl"]}

        def run(ws):
            hT, cT = (torch.empty((B, H), dtype=torch.float32, device="cuda") for _ in range(2))
            out = ops.seq2seq_decode(enc, dec0, w, T, act=self.act, workspace=ws, hT=hT, cT=cT, **kw)
            return {"out": out, "hT": hT, "cT": cT}
        self.run = run

        def reference(outs):
            ref = O.regime_decode(p["enc"], p["dec0"], p["w"], T, self.act, self.bf)
            return {k: ref[k] for k in ("out", "hT", "cT")}
        self.reference = reference
        self.kindcheck = "forward"

    def _make_decoder(self, ops):
        r = self.row
        H, B, T = r["H"], self.B, self.T
        p = G.decode_inputs(self.cid, B, 1, 1, 6, H)
        w = {k: dev(v) for k, v in p["w"].items()}
        dec0, h0, c0 = dev(p["dec0"]), dev(p["h0"]), dev(p["c0"])
        self.run = lambda ws: {"out": ops.seq2seq_decoder(dec0, h0, c0, w, T, act=self.act, impl=r["impl"], workspace=ws)}
        self.reference = lambda outs: {"out": G.decoder_reference(p, B, T, self.act)["out"]}
        self.kindcheck = "forward"

    # -- two layers in one launch --------------------------------------------------------------------------------------
    def _stack2_inputs(self):
        r = self.row
        a, b = G.stack2_inputs(self.cid, self.B, self.T, r["F"], r["H"])
        return a, b, {k: dev(a[k]) for k in a}, {k: dev(b[k]) for k in b}

    def _make_stack2(self, ops):
        r = self.row
        a, b, ta, tb = self._stack2_inputs()
        supported = ops.lstm_stack2_bf16_supported if self.bf else ops.lstm_stack2_supported
        assert supported(self.B, self.T, r["F"], r["H"])
        l1, l2 = [ta[k] for k in ("K", "R", "b")], [tb[k] for k in ("K", "R", "b")]

        def run(ws):
            if self.bf:
                o1, o2 = ops.lstm_stack2_bf16(ta["x"], l1, l2, act=self.act, workspace=ws)
            else:
                o1, o2 = ops.lstm_stack2(ta["x"], l1, l2, (ta["h0"], ta["c0"]), (tb["h0"], tb["c0"]), act=self.act, workspace=ws, reserve=True)
            return {k + n: v for n, o in (("1", o1), ("2", o2)) for k, v in zip(("hs", "hT", "cT", "res"), o)}
        self.run = run

        def reference(outs):
            ref = G.stack2_reference(a, b, self.B, self.act, not self.bf, self.bf)
            return {k + n: v for n, layer in zip(("1", "2"), ref) for k, v in zip(("hs", "hT", "cT", "res"), layer)}
        self.reference = reference
        self.kindcheck = "forward"

    def _make_stack2_bwd(self, ops):
        r = self.row
        B, T, F, H = self.B, self.T, r["F"], r["H"]
        a, b, ta, tb = self._stack2_inputs()
        assert ops.lstm_stack2_bwd_supported(B, T, F, H)
        o1, o2 = ops.lstm_stack2(ta["x"], [ta[k] for k in ("K", "R", "b")], [tb[k] for k in ("K", "R", "b")], (ta["h0"], ta["c0"]), (tb["h0"], tb["c0"]),
                                 act=self.act, workspace=aux_ws(), reserve=True)
        aux_ws().check()
        tapes = [(host(o[0]), host(o[3])) for o in (o1, o2)]

        def run(ws):
            e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
            g = apart((F, 4 * H), (H, 4 * H), (4 * H,), (H, 4 * H), (H, 4 * H), (4 * H,))
            g1, g2 = g[:3], g[3:]
            o = ops.lstm_stack2_bwd(ta["x"], (ta["K"], ta["R"]), (tb["K"], tb["R"]), (o1[0], o1[3], ta["h0"], ta["c0"]), (o2[0], o2[3], tb["h0"], tb["c0"]),
                                    dhs2=tb["dhs"], dhT2=tb["dhT"], dcT2=tb["dcT"], dhT1=ta["dhT"], dcT1=ta["dcT"], grads1=g1, grads2=g2,
                                    need_state_grads=True, act=self.act, scratch=ws)
            o.update(dK1=g1[0], dR1=g1[1], db1=g1[2], dK2=g2[0], dR2=g2[1], db2=g2[2])
            return o
        self.run = run
        self.reference = lambda outs: O.regime_stack2_backward([(a["K"], a["R"], a["b"]), (b["K"], b["R"], b["b"])], a["x"], [(a["h0"], a["c0"]), (b["h0"], b["c0"])],
                                                               tapes, (b["dhs"], b["dhT"], b["dcT"], a["dhT"], a["dcT"]), self.act)
        self.kindcheck = "grads"

    # -- one layer, backward on the GPU's own tape ---------------------------------------------------------------------
    def _make_backward(self, ops):
        r = self.row
        inp = G.layer_inputs(self.cid, self.B, self.T, r["F"], r["H"])
        t = {k: dev(inp[k]) for k in ("x", "K", "R", "b", "h0", "c0", "dhs", "dhT", "dcT")}
        hs, _, _, res = ops.lstm_seq_train(t["x"], t["K"], t["R"], t["b"], t["h0"], t["c0"], act=self.act, workspace=aux_ws(), dtype=r["dtype"])
        aux_ws().check()
        F, H = r["F"], r["H"]

        def run(ws):
            dK, dR, db = apart((F, 4 * H), (H, 4 * H), (4 * H,))
            return ops.lstm_seq_bwd(t["x"], t["K"], t["R"], hs, res, t["h0"], t["c0"], t["dhs"], t["dhT"], t["dcT"], dK=dK, dR=dR, db=db, need_dx=True,
                                    need_state_grads=True, act=self.act, scratch=ws, dtype=r["dtype"])
        self.run = run
        self.reference = lambda outs: G.backward_reference(inp, host(hs), host(res), BWD_VARIANT, self.act, self.bf)
        self.kindcheck = "grads"

    # -- the fused others-mixing decoder -------------------------------------------------------------------------------
    def _mix_inputs(self):
        p = G.mix_inputs(self.cid, self.B, self.T)
        self.p = p
        self.w = {k: dev(v) for k, v in p["w"].items()}
        self.Wp = dev(p["Wp"])
        self.ins = [dev(p[k]) for k in ("dec0", "h1", "c1", "h2", "c2", "oth")]

    def _mix_forward(self, ops, ws):
        B, T, H, O_ = self.B, self.T, G.MIX_H, G.MIX_O
        e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
        outs = {"M": e(T, B, O_), "P": e(T, B, O_), "res1": e(T, B, 5, H), "res2": e(T, B, 5, H)}
        outs.update({k: e(T, B, H) for k in ("H1", "C1", "H2", "C2")})
        ops.mix_decoder(*self.ins, self.w, self.Wp, T, act=self.act, workspace=ws, out=outs["M"], train={k: outs[k] for k in MIX_TAPES}, dtype=self.row["dtype"])
        return outs

    def _make_mix_fwd(self, ops):
        self._mix_inputs()
        self.run = lambda ws: self._mix_forward(ops, ws)
        self.reference = lambda outs: G.mix_forward_reference(self.p, self.B, self.T, self.act, self.bf)
        self.kindcheck = "forward"

    def _make_mix_bwd(self, ops):
        self._mix_inputs()
        B, T, H, O_, p = self.B, self.T, G.MIX_H, G.MIX_O, self.p
        fw = self._mix_forward(ops, aux_ws())
        aux_ws().check()
        tape = {k: host(v) for k, v in fw.items()}
        dloss = (np.transpose(p["G"], (1, 0, 2)) * (1 - tape["M"] * tape["M"])).astype(np.float32)
        C1f, C2f = np.concatenate([p["c1"][None], tape["C1"]]), np.concatenate([p["c2"][None], tape["C2"]])
        bins = [fw["M"], fw["P"], dev(dloss), fw["res1"], fw["res2"], dev(C1f), dev(C2f)]

        def run(ws):
            e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
            outs = {"DZ1": e(T, B, 4 * H), "DZ2": e(T, B, 4 * H), "dpre_m": e(T, B, O_), "dpre_p": e(T, B, O_)}
            outs.update({k: e(B, H) for k in MIX_GRADS[4:]})
            return ops.mix_decoder_bwd(*bins, self.w, self.Wp, outs, act=self.act, workspace=ws, dtype=self.row["dtype"])
        self.run = run

        def reference(outs):
            ref = G.mix_backward_reference(p, B, tape, dloss, self.act, self.bf)
            return {k: ref[k] for k in MIX_GRADS}
        self.reference = reference
        self.kindcheck = "grads"

    # -- the row's bound ---------------------------------------------------------------------------------------------------
    def check(self, outs, only=None):
        """The outputs (all, or those named) against the fp64 reference at the bound tests/test_gpu_ragged_guarded.py uses for the form."""
        ref = self.reference(outs)
        keys = [k for k in ref if k in outs and outs[k] is not None and (only is None or k in only)]
        got = {k: host(outs[k]) for k in keys}
        if self.kindcheck == "forward":
            for k in keys:
                tag = "%s %s" % (self.cid, k)
                if self.bf:
                    err = O.regime_error(got[k], ref[k], "bf16") if k.startswith("res") else float(np.abs(got[k] - ref[k]).max()) / BF16_TIGHT
                    print("%-72s error / bound %.3f" % (tag, err))
                    assert err <= 1.0, (tag, err)
                else:
                    assert_parity(got[k], ref[k], tag)
        elif self.bf:
            for k in keys:
                near("%s %s" % (self.cid, k), got[k], ref[k], STATE if k in ("dh0", "dh1_0", "dh2_0") else PER_KERNEL)
        else:
            print("%-72s error / bound %.3f" % (self.cid, max(G.grad_bounds(got[k], ref[k]) for k in keys)))
            G.check_grads({k: torch.from_numpy(np.ascontiguousarray(got[k])) for k in keys}, {k: ref[k] for k in keys}, self.cid)


# ---------------------------------------------------------------------------------------------------------------------
# a launch with check B around it
# ---------------------------------------------------------------------------------------------------------------------
def snapshot(ws):
    """-> (the words of the granule area, cloned on the device and brought to the host; the header's 64 words)."""
    torch.cuda.synchronize()
    area = ws.buf[W.STATUS_BYTES:W.STATUS_BYTES + W.XCH_BYTES].view(torch.int32).clone()
    header = ws.buf[:W.STATUS_BYTES].view(torch.int32).cpu().numpy().view(np.uint32).copy()
    return area.cpu().numpy().view(np.uint32), header


def launch(capfd, call, ws, before=None, rezeroed=False, env=None, launched=None):
    """call.run(ws) under the row's knobs with check B around it -> (outputs, snapshot behind the launch, epochs consumed).
    before: the snapshot in front of it if the caller has one; rezeroed: the launch crosses the re-zero threshold, so header and
    granules count as zero in front of it."""
    ptr0 = ws.buf.data_ptr()
    words0, hdr0 = before if before is not None else snapshot(ws)
    outs, trace = traced(capfd, lambda: call.run(ws), dict(call.env, **(env or {})))
    words1, hdr1 = snapshot(ws)
    assert ws.buf.data_ptr() == ptr0, "%s: the workspace was reallocated - nothing is reused" % call.cid
    assert hdr1[W.ST_TIMEOUT] == 0, "%s: a bounded wait gave up" % call.cid
    ws.check()
    ran = [l for l in LAUNCHED.findall(trace) if l in EXCHANGE]
    assert ran == (call.row["launched"] if launched is None else launched), (call.cid, LAUNCHED.findall(trace))
    if call.row["kind"] == "backward":      # the separate products: db is the kernel's own sum in every run (apart)
        assert "fuse_kr=0 fuse_r=0 grouped=0" in trace, (call.cid, trace)
    base0, n0 = (0, 0) if rezeroed else (int(hdr0[W.ST_EPOCH]), int(hdr0[W.ST_LAUNCHES]))
    base1 = int(hdr1[W.ST_EPOCH])
    settles = call.row["settles"]            # (width 64 on the cluster kernels: one workgroup per group, header and granules untouched)
    assert int(hdr1[W.ST_LAUNCHES]) - n0 == settles, (call.cid, n0, int(hdr1[W.ST_LAUNCHES]), ran)
    assert (base1 > base0) if settles else (base1 == base0), (call.cid, base0, base1)
    if rezeroed:
        words0 = np.zeros_like(words0)
    report = W.tag_report(words0, words1, base0, base1)
    assert report == [], (call.cid, report)
    return {k: v for k, v in outs.items() if v is not None}, (words1, hdr1), base1 - base0


def fresh(capfd, call, key=None):
    """The call on a fresh workspace (cached under `key`: C runs every row's call twice)."""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    ws = new_ws()
    outs, _ = traced(capfd, lambda: call.run(ws), call.env)
    ws.check()
    outs = {k: v for k, v in outs.items() if v is not None}
    if key is not None:
        _CACHE[key] = outs
    return outs


def same(tag, got, want, keys=None):
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    for k in (got if keys is None else keys):
        if k not in got:
            continue
        a, b = got[k].contiguous().view(torch.int32), want[k].contiguous().view(torch.int32)
        assert a.shape == b.shape and torch.equal(a, b), "%s %s: %d of %d elements differ from the fresh workspace's" % (
            tag, k, int((a != b).sum()), a.numel())


# ---------------------------------------------------------------------------------------------------------------------
# A, B: other data and other shapes on one workspace
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", W.ROWS, ids=W.ROW_IDS)
def test_other_data_on_the_same_workspace(capfd, row):
    ws, snap = new_ws(), None
    for i, ((B, T), seed) in enumerate(zip(W.SHAPES, "XYZ")):
        call = Call(row, B, T, seed)
        outs, snap, _ = launch(capfd, call, ws, snap)
        same("%s %s" % (row["name"], seed), outs, fresh(capfd, call))
        if seed == "Z":
            call.check(outs)


# ---------------------------------------------------------------------------------------------------------------------
# C: a chain of different kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_a_chain_of_different_kernels(capfd, order):
    rows = W.ROWS if order == "forward" else W.ROWS[::-1]
    ws, snap = new_ws(), None
    B, T = W.SHAPES[0]
    for row in rows:
        if ("chain-call", row["name"]) not in _CACHE:
            _CACHE["chain-call", row["name"]] = Call(row, B, T, "chain")
        call = _CACHE["chain-call", row["name"]]
        outs, snap, _ = launch(capfd, call, ws, snap)
        same("chain (%s) %s" % (order, row["name"]), outs, fresh(capfd, call, ("chain-fresh", row["name"])))
    if order == "reverse":
        for k in [k for k in _CACHE if isinstance(k, tuple) and k[0].startswith("chain")]:
            del _CACHE[k]


# ---------------------------------------------------------------------------------------------------------------------
# D: tile rounds
# ---------------------------------------------------------------------------------------------------------------------
_ROUNDS = W.rounds_cases()


@pytest.mark.parametrize("row,limit,groups", _ROUNDS, ids=["%s-limit%d" % (r["name"], l) for r, l, _ in _ROUNDS])
def test_tile_rounds(capfd, row, limit, groups):
    """B = 33 on `groups` groups (FOV_DBG_RESIDENT_LIMIT = groups * G) against the unlimited run on three groups: the same form
    by its trace name, more epochs consumed, the bit-identical set of the host table the same bits and the rest within the bound."""
    call = Call(row, W.ROUNDS_B, 3, "rounds")
    free, _, span_free = launch(capfd, call, new_ws())
    outs, _, span = launch(capfd, call, new_ws(), env={"FOV_DBG_RESIDENT_LIMIT": str(limit)})
    assert span > span_free or not row["settles"], (row["name"], limit, span, span_free)         # the groups made more than one round
    bits, bound = W.identity(row)
    assert set(outs) <= set(bits) | set(bound), sorted(outs)
    same("%s limit %d" % (row["name"], limit), outs, free, keys=bits)
    call.check(outs)


# ---------------------------------------------------------------------------------------------------------------------
# E: epoch bases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", W.ROWS, ids=W.ROW_IDS)
def test_epoch_bases(capfd, row):
    from longterm360fov_amd import _lib, ops
    L = _lib.lib()
    (B, T), (B2, T2) = W.SHAPES[0], W.SHAPES[1]
    call, other = Call(row, B, T, "epoch"), Call(row, B2, T2, "epoch-other")
    want, _, span0 = launch(capfd, call, new_ws())             # base 0: a fresh workspace
    want_other = fresh(capfd, other)
    for base in W.EPOCH_BASES:
        ws = new_ws()
        ops.check(L.fov_debug_set_epoch(ws.buf.data_ptr(), ws.buf.numel(), base, ops._stream()))
        crosses = base == W.EPOCH_BASES[3]
        outs, snap, span = launch(capfd, call, ws, rezeroed=crosses)
        same("%s from base 0x%x" % (row["name"], base), outs, want)
        epoch = int(snap[1][W.ST_EPOCH])
        assert span == span0, (row["name"], base, span, span0)         # the launch consumes the epochs it consumes from base 0
        if crosses:
            assert epoch == span0 < 64, (row["name"], epoch, span0)    # header and granules were re-zeroed in front of the launch
        outs2, _, _ = launch(capfd, other, ws, snap)
        same("%s second launch from base 0x%x" % (row["name"], base), outs2, want_other)


# ---------------------------------------------------------------------------------------------------------------------
# F: the area behind the granules
# ---------------------------------------------------------------------------------------------------------------------
def _row(name):
    return [r for r in W.ROWS if r["name"] == name][0]


@pytest.mark.parametrize("between", ["another call", "nothing"])
@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_prepack_mark_and_the_shared_tail(capfd, direction, between):
    """fov_mix_decoder_prepack leaves a packed dec2_K behind the granule area and a mark for the next fused-decoder launch.  The
    two-launch cluster decode keeps its carried state there, fov_lstm_seq_bwd its carries and scratch: behind such a call the mark
    must be gone (the launch packs again), or the decoder computes from a pack whose first rows are the other call's state.  With
    nothing in between the mark is consumed: the launch then uses the pack as it was made, even of weights changed in place since
    (include/fov360.h: the mark is keyed by pointer)."""
    from longterm360fov_amd import ops
    B, T = W.SHAPES[0]
    mix = Call(_row("mix-decoder" if direction == "forward" else "mix-decoder-bwd"), B, T, "tail")
    other = Call(_row("decode-two-launches-256" if direction == "forward" else "bwd8-256"), B, T, "tail-between")
    want = fresh(capfd, mix)
    ws = new_ws()
    K2 = mix.w["dec2_K"]
    prepack = lambda: ops.mix_decoder_prepack(K2, B, G.MIX_H, **({"workspace": ws} if direction == "forward" else {"workspace_bwd": ws}))
    prepack()
    if between == "another call":
        _, snap, _ = launch(capfd, other, ws)
        outs, _, _ = launch(capfd, mix, ws, snap)
        same("%s behind %s" % (mix.row["name"], other.row["name"]), outs, want)
        mix.check(outs)
        return
    outs, snap, _ = launch(capfd, mix, ws)
    same(mix.row["name"] + " behind its prepack", outs, want)
    # the mark was consumed, not ignored: a pack of the old weights is what a marked launch uses
    kept = K2.clone()
    prepack()
    K2.mul_(0.5)
    try:
        stale, snap, _ = launch(capfd, mix, ws, snap)
        same(mix.row["name"] + " from the marked pack", stale, want)
        again, _, _ = launch(capfd, mix, ws, snap)          # the mark is for one launch: this one packs the halved weights
        changed = [k for k in again if not torch.equal(again[k].view(torch.int32), want[k].view(torch.int32))]
        assert changed, "halving dec2_K changed no output: the control proves nothing"
    finally:
        K2.copy_(kept)
