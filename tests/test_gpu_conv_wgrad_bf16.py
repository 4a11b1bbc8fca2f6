"""fov_conv2d_wgrad_bf16 (ops.conv2d_wgrad_bf16) against the NumPy restatement of its contract in fp64
(test_convlstm_train_bf16_host.wgrad_bf16_ref: both operands rounded to bf16 round-to-nearest-even, exact sums).

Bound per case: max(1, 8 * e_ref) units of 1e-5 * max|ref|, e_ref the restatement's own fp32-vs-fp64 error
(test_convlstm_train_bf16_host.test_operator_yardstick checks 8 * e_ref <= 10 without a GPU).  Every case runs on the form
the shape selects and on the plain form (FOV_NO_WGRAD_BF16_TILES=1).  Then: ties round to even on both operands, accumulate
and bit-for-bit determinism, the same bits inside a deferred-reduction region behind a pending product over the output,
the empty-batch rule and the error returns."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_convlstm_train_bf16_host import OP_CASES, op_bound_units, op_inputs, op_reference, wgrad_bf16_ref  # noqa: E402

pytestmark = pytest.mark.gpu

KNOB = "FOV_NO_WGRAD_BF16_TILES"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def units(got, ref):
    """max |got - ref| in units of 1e-5 * max|ref|"""
    return float(np.abs(got - ref).max() / (1e-5 * np.abs(ref).max()))


def x_view(x, extra):
    """x on the device, as the channel slice [extra/2, extra/2 + C) of a map `extra` channels wider (pixel stride > C)."""
    if not extra:
        return dev(x)
    wide = torch.randn(x.shape[:-1] + (x.shape[-1] + extra,), device="cuda")
    lo = extra // 2
    wide[..., lo:lo + x.shape[-1]] = dev(x)
    return wide[..., lo:lo + x.shape[-1]]


# the form each operator case must take: dense odd strides, unaligned slices and 1 x 1 maps are the plain kernel's
EXPECT_FORM = ["plain", "tuned", "tuned", "plain", "tuned", "plain", "plain"]


class traced:
    """FOV_DBG_TRACE=1 around a call: the library names the form and the slices it chose on stderr (read through capfd)."""

    def __init__(self, capfd):
        self.capfd = capfd

    def __enter__(self):
        os.environ["FOV_DBG_TRACE"] = "1"
        self.capfd.readouterr()
        return self

    def __exit__(self, *exc):
        del os.environ["FOV_DBG_TRACE"]
        torch.cuda.synchronize()
        err = self.capfd.readouterr().err
        self.plans = [ln.split("conv2d_wgrad_bf16: ")[1] for ln in err.splitlines() if "conv2d_wgrad_bf16: " in ln]
        return False

    def form(self, i=0):
        return self.plans[i].split(" form")[0]

    def slices(self, i=0):
        return int(self.plans[i].split(", ")[1].split(" slices")[0])


class plain_form:
    def __enter__(self):
        os.environ[KNOB] = "1"

    def __exit__(self, *exc):
        del os.environ[KNOB]
        return False


@pytest.mark.parametrize("idx", range(len(OP_CASES)), ids=[c[0] for c in OP_CASES])
def test_wgrad_bf16_against_the_rounded_operand_reference(idx, capfd):
    from longterm360fov_amd import ops
    name, B, H, W, C, N, kh, kw, extra = OP_CASES[idx]
    x, dy = op_inputs(OP_CASES[idx])
    ref, _ = op_reference(idx)
    bound = op_bound_units(idx)
    xd, dyd = x_view(x, extra), dev(dy)
    sc = ops.Scratch()
    with traced(capfd) as tr:
        got = f64(ops.conv2d_wgrad_bf16(xd, dyd, kh, kw, scratch=sc))
        with plain_form():
            plain = f64(ops.conv2d_wgrad_bf16(xd, dyd, kh, kw, scratch=sc))
    assert [tr.form(0), tr.form(1)] == [EXPECT_FORM[idx], "plain"], tr.plans
    assert idx != 2 or tr.slices(0) >= 2, tr.plans
    e, ep = units(got, ref), units(plain, ref)
    print("%s: %.3f units (plain form %.3f), bound %.2f" % (name, e, ep, bound))
    assert got.shape == (kh, kw, C, N)
    assert e <= bound and ep <= bound


@pytest.mark.parametrize("C,N,wide", [(64, 30, 32), (64, 28, 32), (30, 64, 32)])
def test_wgrad_bf16_ragged_channels_in_an_aligned_buffer_take_the_tuned_form(C, N, wide, capfd):
    """dy (or x) as the leading channels of a buffer padded to a multiple of 4 - what the trainer keeps for the last head
    layer's 30-channel dy: the tuned kernel, addressing with the row stride and zeroing the tail of the last quad (the pad
    holds NaN here: a value that leaked would poison the result)."""
    from longterm360fov_amd import ops
    B, H, W, k = 2, 36, 18, 5
    rng = np.random.default_rng(8)
    x, dy = rng.standard_normal((B, H, W, C)).astype(np.float32), rng.standard_normal((B, H, W, N)).astype(np.float32)
    ref = wgrad_bf16_ref(x.astype(np.float64), dy.astype(np.float64), k, k)

    def padded(a):
        if a.shape[-1] == 64:
            return dev(a)
        buf = torch.full(a.shape[:-1] + (wide,), float("nan"), device="cuda")
        buf[..., :a.shape[-1]] = dev(a)
        return buf[..., :a.shape[-1]]
    with traced(capfd) as tr:
        got = ops.conv2d_wgrad_bf16(padded(x), padded(dy), k, k)
        dense = ops.conv2d_wgrad_bf16(dev(x), dev(dy), k, k)
    assert tr.form(0) == "tuned" and tr.form(1) == ("tuned" if (C % 4, N % 4) == (0, 0) else "plain"), tr.plans
    assert units(f64(got), ref) <= 1.0 and units(f64(dense), ref) <= 1.0


def test_wgrad_bf16_operands_beyond_2_gib_are_cut_into_slices(capfd):
    """The trainer forms a head layer's weight gradient as ONE product over the maps of all steps: at configs[3] that is up to
    6.8 GB of dy.  Here dy is 2.2 GB (830 maps x 648 pixels x 1024 outputs): the call must take the tuned form with at least two
    slices, each addressed from its own base, and equal the sum of two calls over halves of the maps (each under 2 GiB, added with
    accumulate) - and the fp64 restatement on a corner of the output."""
    from longterm360fov_amd import ops
    B, H, W, C, N, k = 830, 36, 18, 8, 1024, 5
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    x = torch.randn((B, H, W, C), device="cuda", generator=g)
    dy = torch.randn((B, H, W, N), device="cuda", generator=g)
    assert dy.numel() * 4 > 2 ** 31
    with traced(capfd) as tr:
        whole = ops.conv2d_wgrad_bf16(x, dy, k, k)
        halves = ops.conv2d_wgrad_bf16(x[:B // 2], dy[:B // 2], k, k)
        ops.conv2d_wgrad_bf16(x[B // 2:], dy[B // 2:], k, k, dw=halves, accumulate=True)
    assert tr.form(0) == "tuned" and tr.slices(0) >= 2, tr.plans
    scale = float(whole.abs().max())
    assert float((whole - halves).abs().max()) <= 1e-5 * scale
    n = 16          # fp64 restatement of 16 output columns: the last maps decide whether the far slices were read where they lie
    ref = wgrad_bf16_ref(x.cpu().numpy().astype(np.float64), dy[..., N - n:].cpu().numpy().astype(np.float64), k, k)
    assert units(f64(whole[..., N - n:]), ref) <= 1.0


@pytest.mark.parametrize("pad", [0, 2])
def test_data_gradient_on_the_packed_transposed_kernel(pad):
    """dx = conv2d_bf16(dy, *conv2d_bwd_data_pack_bf16(w)) = the data gradient of y = conv2d_same(x, w) with both operands
    rounded; with pad zero channels behind dy's 30 and as many zero rows in the transposed kernel it is the same numbers."""
    from longterm360fov_amd import ops
    B, H, W, C, N, k = 2, 9, 6, 8, 30, 3
    rng = np.random.default_rng(4)
    w = rng.standard_normal((k, k, C, N)).astype(np.float32)
    dy = rng.standard_normal((B, H, W, N)).astype(np.float32)
    wt_ref = np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2)).astype(np.float64)
    ref = O.conv2d_same(O.round_bf16(dy.astype(np.float64)), O.round_bf16(wt_ref))
    wt, packed = ops.conv2d_bwd_data_pack_bf16(dev(w), pad)
    assert wt.shape == (k, k, N + pad, C) and np.array_equal(f64(wt[:, :, :N]), wt_ref) and float(wt[:, :, N:].abs().sum()) == 0
    dyd = torch.zeros((B, H, W, N + pad), device="cuda")
    dyd[..., :N] = dev(dy)
    assert units(f64(ops.conv2d_bf16(dyd, wt, packed=packed)), ref) <= 1.0


def test_wgrad_bf16_ties_round_to_even_on_both_operands():
    """Every input sits exactly half way between two bf16 neighbours: round-to-nearest-even decides all of them.  Against the
    restatement with ties rounded away from zero, or truncated, on either operand the kernel is far OUTSIDE the bound."""
    from longterm360fov_amd import ops
    B, H, W, C, N, k = 2, 9, 6, 16, 20, 3
    rng = np.random.default_rng(21)

    def ties(shape):
        a = rng.standard_normal(shape).astype(np.float32)
        u = (a.view(np.uint32) & 0xFFFF0000) | 0x8000          # bf16 value + half an ulp: exactly representable in fp32
        return u.astype(np.uint32).view(np.float32)
    x, dy = ties((B, H, W, C)), ties((B, H, W, N))
    assert not np.array_equal(O.round_bf16(x), x)
    up = lambda a: ((a.view(np.uint32).astype(np.uint64) + 0x8000) & 0xFFFF0000).astype(np.uint32).view(np.float32).astype(np.float64)
    trunc = lambda a: (a.view(np.uint32) & 0xFFFF0000).view(np.float32).astype(np.float64)
    rne = lambda a: O.round_bf16(a).astype(np.float64)

    def product(xr, dr):       # the exact sum over operands already rounded (bf16 values pass O.round_bf16 unchanged)
        return wgrad_bf16_ref(xr, dr, k, k)
    ref = product(rne(x), rne(dy))
    for form in (None, "plain"):
        if form:
            with plain_form():
                got = f64(ops.conv2d_wgrad_bf16(dev(x), dev(dy), k, k))
        else:
            got = f64(ops.conv2d_wgrad_bf16(dev(x), dev(dy), k, k))
        assert units(got, ref) <= 1.0, form
        for name, wrong in {"x ties away": product(up(x), rne(dy)), "dy ties away": product(rne(x), up(dy)),
                            "x truncated": product(trunc(x), rne(dy)), "dy truncated": product(rne(x), trunc(dy))}.items():
            e = units(got, wrong)
            print("%s (%s): %.1f units" % (name, form or "selected form", e))
            assert e > 10, (form, name)


@pytest.mark.parametrize("idx", [0, 2], ids=["plain form", "tuned form, split"])
def test_wgrad_bf16_accumulates_and_is_deterministic(idx):
    from longterm360fov_amd import ops
    name, B, H, W, C, N, kh, kw, extra = OP_CASES[idx]
    x, dy = op_inputs(OP_CASES[idx])
    ref, _ = op_reference(idx)
    xd, dyd = x_view(x, extra), dev(dy)
    one = ops.conv2d_wgrad_bf16(xd, dyd, kh, kw)
    two = ops.conv2d_wgrad_bf16(xd, dyd, kh, kw)
    assert torch.equal(one, two)
    base = np.random.default_rng(2).standard_normal(ref.shape).astype(np.float32)
    acc = dev(base)
    ops.conv2d_wgrad_bf16(xd, dyd, kh, kw, dw=acc, accumulate=True)
    assert units(f64(acc) - base.astype(np.float64), ref) <= op_bound_units(idx) + 1.0    # + the fp32 add onto |base| <= 5
    acc2 = dev(base)
    ops.conv2d_wgrad_bf16(xd, dyd, kh, kw, dw=acc2, accumulate=True)
    assert torch.equal(acc, acc2)


@pytest.mark.parametrize("accumulate", [True, False])
@pytest.mark.parametrize("idx", [0, 2], ids=["plain form", "tuned form, split"])
def test_wgrad_bf16_inside_a_deferred_region_equals_outside_bit_for_bit(idx, accumulate):
    """A pending split product P (a column-sum-free [x]^T dz over the same output) first, then the weight gradient: in a region
    P's reduce is pending when the call arrives, so the call must flush it before it adds to / replaces the range."""
    from longterm360fov_amd import ops
    name, B, H, W, C, N, kh, kw, extra = OP_CASES[idx]
    x, dy = op_inputs(OP_CASES[idx])
    ref, _ = op_reference(idx)
    xd, dyd = x_view(x, extra), dev(dy)
    rng = np.random.default_rng(5)
    rows = 5120
    pa, pb = rng.standard_normal((rows, kh * kw * C)).astype(np.float32) / 8, rng.standard_normal((rows, N)).astype(np.float32) / 8
    pad, pbd = dev(pa), dev(pb)
    n = kh * kw * C * N
    arena = torch.empty(64 << 20, dtype=torch.float32, device="cuda")

    def run(region):
        flat = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
        out = flat[4:4 + n]
        sc = ops.Scratch()
        if region:
            ops.reduce_defer_begin(flat, arena)
        ops.wgrad_fused(pad, None, pbd, out.view(kh * kw * C, N), bias=False, scratch=sc)
        pending = region and float(out.abs().max()) == 0.0
        ops.conv2d_wgrad_bf16(xd, dyd, kh, kw, dw=out.view(kh, kw, C, N), accumulate=accumulate, scratch=sc)
        if region:
            ops.reduce_defer_end(flat)
        return out.clone(), pending
    inside, pending = run(True)
    outside, _ = run(False)
    assert pending, "the product in front was not pending: the case does not test the order"
    assert torch.equal(inside, outside)
    want = ref + (pa.astype(np.float64).T @ pb.astype(np.float64)).reshape(ref.shape) if accumulate else ref
    assert np.abs(f64(inside).reshape(ref.shape) - want).max() <= 1e-3 * np.abs(want).max()


def test_wgrad_bf16_empty_batch_and_errors():
    from longterm360fov_amd import ops, _lib
    C, N, k = 8, 12, 3
    base = torch.randn((k, k, C, N), device="cuda")
    x0, dy0 = torch.empty((0, 9, 6, C), device="cuda"), torch.empty((0, 9, 6, N), device="cuda")
    dw = base.clone()
    ops.conv2d_wgrad_bf16(x0, dy0, k, k, dw=dw, accumulate=True)
    assert torch.equal(dw, base)                      # accumulate: the buffer is left alone
    ops.conv2d_wgrad_bf16(x0, dy0, k, k, dw=dw, accumulate=False)
    assert float(dw.abs().max()) == 0.0               # the gradient of an empty sum
    L = _lib.lib()
    need = L.fov_conv2d_wgrad_bf16_workspace_bytes(C, N, k, k)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    x, dy = torch.randn((2, 9, 6, C), device="cuda"), torch.randn((2, 9, 6, N), device="cuda")
    args = lambda **kw: [x.data_ptr(), kw.get("ldx", C), dy.data_ptr(), kw.get("ldy", N), dw.data_ptr(), 2, 9, 6, C, N, kw.get("kh", k), k, 0,
                         ws.data_ptr(), kw.get("bytes", need), None]
    assert L.fov_conv2d_wgrad_bf16(*args()) == 0
    assert L.fov_conv2d_wgrad_bf16(*args(kh=2)) == _lib.ERR_INVALID                 # even kernel
    assert b"fov_conv2d_wgrad_bf16" in L.fov_last_error()
    assert L.fov_conv2d_wgrad_bf16(*args(ldx=C - 1)) == _lib.ERR_INVALID
    assert L.fov_conv2d_wgrad_bf16(*args(ldy=N - 1)) == _lib.ERR_INVALID
    assert L.fov_conv2d_wgrad_bf16(*args(bytes=need - 16)) == _lib.ERR_WORKSPACE    # workspace too small
    torch.cuda.synchronize()
