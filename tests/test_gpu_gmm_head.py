"""The mixture-density head's three device pieces - fov_gmm3d_loss_grad, fov_gmm3d_sample and the split at the end of
mlp_head_fwd_kernel - at their chunk, tie and value edges, on GUARDED VIEWS.

tests/test_gmm_head_host.py owns the references, the case tables and the proof that the cases are sharp: on the CPU, every
wrong-on-purpose reference (the sums restarted per chunk, the LDS entries restarted, 256 rows of the loss, a row stride of 3 P, no
repair gradient, no floor in the weight, a softmax backward without its dot; for the sampler >= for >, a double running sum, no clamp)
misses the bounds asserted here by a factor of ten at least.

Loss and gradient: through the C ABI, params and y inside NaN buffers at offsets 0 and 1, dpre, the loss and the workspace (ticket
word and the rows' parts) inside sentinel buffers.  dpre per element within 2^-23 |ref| + 16 spread(case) + 1e-12 max|ref| of the fp64
reference on the same fp32 parameters; the loss within 2^-23 (|scale| sum |part| + |loss|).  Four calls on one workspace: two with
the loss (same bits), one without (same dpre bits, the loss left alone), one with it again (same loss bits: the ticket was left at
zero).  Sampler: the chosen component is read back from the draw (means 8 apart) and must be the reference's on EVERY frame - at
u = 0, one ulp below, at and above cumulative weights, at cum[n - 1], 1 - 2^-24, 1 and 2.  Every check prints its error over its
bound; the last test prints the worst per family."""
import numpy as np
import pytest
import torch

import test_gmm_head_host as H
import test_guarded_views_host as G
from test_guarded_views_host import OutView, f64, same_bits, seed_of

pytestmark = pytest.mark.gpu

WORST = {}          # family -> [checks, worst error over bound]: printed by the last test of the file
WS_HEAD = 64        # floats of the workspace in front of the rows' parts (256 bytes: the ticket word first)


def gv(a, off=0):
    return G.guarded(a, off, device="cuda")


def out_view(shape, base=None, off=0):
    return OutView(shape, base, off, torch.float32, "cuda")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def note(tag, family, ratio):
    print("%-64s error / bound %.3f" % (tag, ratio))
    w = WORST.setdefault(family, [0, 0.0])
    w[0] += 1
    w[1] = max(w[1], ratio)


def workspace(B):
    """Exactly the bytes fov_gmm3d_loss_grad asks for, zero (the ticket's resting state), inside sentinels."""
    return out_view((WS_HEAD + B,), base=np.zeros(WS_HEAD + B, np.float32))


def last_error(lib):
    return lib.fov_last_error().decode("utf-8", "replace")


# ---------------------------------------------------------------------------------------------------------------------
# fov_gmm3d_loss_grad
# ---------------------------------------------------------------------------------------------------------------------
def offsets(name):
    """(params, y, dpre) start 0 or 1 float behind a 16-byte boundary: a function of the case name, every combination in the table."""
    s = seed_of(name)
    return s & 1, (s >> 1) & 1, (s >> 2) & 1


def test_every_offset_combination_is_in_the_table():
    assert {offsets(name) for name in H.all_cases()} == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}


@pytest.mark.parametrize("name", H.all_cases())
def test_loss_and_gradient(name):
    from longterm360fov_amd import _lib, ops
    lib = _lib.lib()
    c = H.case(name)
    ref, spread = H.reference(name)
    B, n, P = c["B"], c["n"], c["P"]
    op, oy, od = offsets(name)
    params, y = gv(c["params"], op), gv(c["y"], oy)
    dpre, loss, ws = out_view((B, 10 * n), off=od), out_view((1,)), workspace(B)

    def call(with_loss=True):
        ops.check(lib.fov_gmm3d_loss_grad(ptr(params), ptr(y), c["ldy"], ptr(loss.v) if with_loss else None, ptr(dpre.v), B, n, P, c["scale"],
                                          1 if c["weight_by_pi"] else 0, ptr(ws.v), 4 * ws.v.numel(), ops._stream()))
        torch.cuda.synchronize()
    call()
    g, l = dpre.result(), loss.result()
    dpre.reset(), loss.reset()
    call()
    assert same_bits(dpre.result(), g) and same_bits(loss.result(), l), name + ": two calls on one workspace differ"
    dpre.reset(), loss.reset()
    call(with_loss=False)
    assert same_bits(dpre.result(), g), name + ": dpre depends on the loss pointer"
    assert loss.untouched(), name + ": a call without a loss pointer wrote the loss"
    dpre.reset()
    call()
    assert same_bits(loss.result(), l) and same_bits(dpre.result(), g), name + ": the call without a loss left the ticket off zero"
    w = ws.result()
    assert int(ws.v.view(torch.int32)[0].item()) == 0 and (w[1:WS_HEAD] == 0).all(), name + ": the ticket is not back at zero"
    if not c["weight_by_pi"]:
        assert (g[:, :n] == 0).all()
    family = "loss+grad " + ("shapes" if name in H.shape_cases() else name.rsplit("-pi", 1)[0])
    r = H.over_bound(g, ref["dpre"], spread)
    note(name + " dpre", family, r)
    rl = abs(float(l[0]) - ref["loss"]) / H.loss_bound(ref["part"], ref["loss"], c["scale"])
    note(name + " loss", "loss value", rl)
    print("   loss gpu %.9e ref %.9e   max|dpre| %.3e   spread %.3e" % (float(l[0]), ref["loss"], np.abs(ref["dpre"]).max(), spread))
    assert r <= 1.0, (name, r)
    assert rl <= 1.0, (name, rl)
    assert np.abs(f64(g) - ref["dpre"]).max() <= 2e-4 * np.abs(ref["dpre"]).max()          # the heads' existing bound, never looser


def test_an_empty_batch_writes_nothing():
    from longterm360fov_amd import _lib, ops
    lib = _lib.lib()
    c = H.case("n2-P3-B1-pi1-ld0")
    params, y, dpre, loss, ws = gv(c["params"]), gv(c["y"]), out_view((1, 20)), out_view((1,)), workspace(1)
    assert lib.fov_gmm3d_loss_grad(ptr(params), ptr(y), c["ldy"], ptr(loss.v), ptr(dpre.v), 0, 2, 3, c["scale"], 1, ptr(ws.v), 4 * ws.v.numel(),
                                   ops._stream()) == 0
    out = out_view((1, 9))
    assert lib.fov_gmm3d_sample(ptr(params), ptr(gv(np.zeros((1, 3)))), ptr(gv(np.zeros((1, 3, 3)))), ptr(out.v), 9, 0, 2, 3, ops._stream()) == 0
    torch.cuda.synchronize()
    assert dpre.untouched() and loss.untouched() and ws.untouched() and out.untouched()


@pytest.mark.parametrize("what", ["n_mix = 33", "n_pts = 257", "ldy = 3 P - 1", "workspace one byte short"])
def test_loss_refusals(what):
    from longterm360fov_amd import _lib, ops
    lib = _lib.lib()
    B, n, P = 2, (33 if what == "n_mix = 33" else 2), (257 if what == "n_pts = 257" else 3)
    ldy = 3 * P - (1 if what == "ldy = 3 P - 1" else 0)
    params, y = gv(np.full((B, 10 * n), 0.5, np.float32)), gv(np.zeros((B, 3 * P), np.float32))
    dpre, loss, ws = out_view((B, 10 * n)), out_view((1,)), workspace(B)
    short = what == "workspace one byte short"
    rc = lib.fov_gmm3d_loss_grad(ptr(params), ptr(y), ldy, ptr(loss.v), ptr(dpre.v), B, n, P, 1.0, 0, ptr(ws.v), 4 * ws.v.numel() - (1 if short else 0),
                                 ops._stream())
    torch.cuda.synchronize()
    assert rc == (_lib.ERR_WORKSPACE if short else _lib.ERR_UNSUPPORTED), (what, rc)
    assert "fov_gmm3d_loss_grad" in last_error(lib)
    assert dpre.untouched() and loss.untouched() and ws.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# fov_gmm3d_sample
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.sampler_cases())
def test_sampler(name):
    """The component on every frame - nothing is skipped at a tie - and mu + L z within 2^-22 |ref| + 1e-7; two calls, the same bits.
    `window`: out is a slot of wider rows, the floats between the rows' slots stay as they were."""
    from longterm360fov_amd import _lib, ops
    lib = _lib.lib()
    s = H.sampler_case(name)
    B, P = s["u"].shape
    n = s["params"].shape[1] // 10
    off = seed_of(name) & 1
    params, u, z = gv(s["params"], off), gv(s["u"], 1 - off), gv(s["z"], off)
    ldo, col = (3 * P + 5, 2) if name == "window" else (3 * P, 0)
    base = np.random.default_rng(seed_of(name + " base")).standard_normal((B, ldo)).astype(np.float32) if name == "window" else None
    out = out_view((B, ldo), base=base, off=1 - off)

    def call():
        ops.check(lib.fov_gmm3d_sample(ptr(params), ptr(u), ptr(z), ptr(out.v) + 4 * col, ldo, B, n, P, ops._stream()))
        torch.cuda.synchronize()
    call()
    first = out.result()
    out.reset()
    call()
    got = out.result()
    assert same_bits(first, got), name + ": two calls differ"
    flat = got.reshape(-1)
    draw = np.stack([flat[col + b * ldo:col + b * ldo + 3 * P] for b in range(B)]).reshape(B, P, 3)
    if name == "window":
        gap = np.ones(B * ldo, bool)
        for b in range(B):
            gap[col + b * ldo:col + b * ldo + 3 * P] = False
        assert same_bits(flat[gap], base.reshape(-1)[gap]), "a write between the rows' slots"
    comp, ref = H.sample_reference(s["params"], s["u"], s["z"])
    chosen = np.rint(f64(draw[..., 0]) / H.MEAN_STEP).astype(np.int64)
    wrong = np.argwhere(chosen != comp)
    assert wrong.size == 0, "%s: frame (row, frame) %s: component %d, reference %d at u = %r" % (
        name, wrong[0], chosen[tuple(wrong[0])], comp[tuple(wrong[0])], s["u"][tuple(wrong[0])])
    r = float((np.abs(f64(draw) - ref) / H.sample_bound(ref)).max())
    note(name, "sampler", r)
    assert r <= 1.0, (name, r)


@pytest.mark.parametrize("what", ["n_mix = 0", "ldo = 3 P - 1"])
def test_sampler_refusals(what):
    from longterm360fov_amd import _lib, ops
    lib = _lib.lib()
    B, n, P = 2, 2, 3
    params, u, z, out = gv(np.full((B, 10 * n), 0.5, np.float32)), gv(np.zeros((B, P))), gv(np.zeros((B, P, 3))), out_view((B, 3 * P))
    rc = lib.fov_gmm3d_sample(ptr(params), ptr(u), ptr(z), ptr(out.v), 3 * P - (1 if what.startswith("ldo") else 0), B, 0 if what.startswith("n_mix") else n,
                              P, ops._stream())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_UNSUPPORTED and "fov_gmm3d_sample" in last_error(lib) and out.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# the split at the end of mlp_head_fwd_kernel
# ---------------------------------------------------------------------------------------------------------------------
def _layers(head):
    return [(dev(head["fc%d_W" % l]), dev(head["fc%d_b" % l]), "relu" if l < 4 else None) for l in (1, 2, 3, 4)]


def _split_checks(tag, out, ref):
    """pi and sigma relative 1e-3 with NO absolute floor (pi: 1e-37, below fp32's normal range); mu 1e-3 |ref| + 2e-5; rho 2e-5."""
    n = H.SPLIT_N
    pi, us, sg, rh = ref
    out = f64(out)
    for k, got, want, rtol, atol in (("pi", out[:, :n], pi, 1e-3, 1e-37), ("mu", out[:, n:4 * n], us, 1e-3, 2e-5), ("sigma", out[:, 4 * n:7 * n], sg, 1e-3, 0.0),
                                     ("rho", out[:, 7 * n:], rh, 0.0, 2e-5)):
        r = float((np.abs(got - want) / (rtol * np.abs(want) + atol)).max())
        note("%s %s" % (tag, k), "split", r)
        assert r <= 1.0, (tag, k, r)
    assert np.abs(out[:, 7 * n:]).max() <= 1.0
    assert np.abs(out[:, :n].sum(1) - 1.0).max() <= 1e-5


def test_split_over_wide_spans():
    """Logits over +-40 (pi down to e^-80), log sigma over -12 .. 6, rho pre-activations of +-15 and +-1e-4, against O.tf_gmm3d_head in fp64."""
    from longterm360fov_amd import ops
    head, h = H.split_head_inputs()
    acts = ops.mlp_head_fwd(dev(h), _layers(head), n_mix=H.SPLIT_N)
    torch.cuda.synchronize()
    _split_checks("split", acts[-1].cpu().numpy(), H.split_reference(head, h)[0])


def test_split_and_backward_behind_a_dead_layer():
    """fc3_b = -1e3: the third layer is off in every row, so every row's parameters are the split of fc4_b, and the backward chain
    passes nothing below the last layer: gW1 .. gW3, gb1 .. gb3, dx and gW4 exactly zero, gb4 the column sums of dlast."""
    from longterm360fov_amd import ops
    head, h = H.split_head_inputs(dead_layer=True)
    layers = _layers(head)
    x = dev(h)
    acts = ops.mlp_head_fwd(x, layers, n_mix=H.SPLIT_N)
    out = acts[-1].cpu().numpy()
    assert (acts[2].cpu().numpy() == 0).all()
    assert all(same_bits(out[b], out[0]) for b in range(1, H.SPLIT_B))
    _split_checks("dead layer", out, H.split_reference(head, h)[0])
    dlast = np.random.default_rng(seed_of("gmm dead layer dlast")).standard_normal(out.shape).astype(np.float32)
    gW, gb = [torch.full_like(W, 7.0) for W, _, _ in layers], [torch.full_like(b, 7.0) for _, b, _ in layers]
    dx = ops.mlp_head_bwd(x, layers, acts, dev(dlast), gW, gb, need_dx=True, accumulate=False)
    torch.cuda.synchronize()
    for l in range(3):
        assert (gW[l].cpu().numpy() == 0).all() and (gb[l].cpu().numpy() == 0).all(), "layer %d" % (l + 1)
    assert (dx.cpu().numpy() == 0).all() and (gW[3].cpu().numpy() == 0).all()
    r = G.head_grad_bounds(gb[3].cpu().numpy(), f64(dlast).sum(0))
    note("dead layer gb4", "split", r)
    assert r <= 1.0, r


def test_zz_worst_error_over_bound_per_family():
    """Prints cases and worst error over bound per family of this file's run."""
    for fam in sorted(WORST):
        print("%-28s %4d checks   worst error / bound %.3f" % (fam, WORST[fam][0], WORST[fam][1]))
    assert all(w[1] <= 1.0 for w in WORST.values())
