"""Guarded views for the convolution path: strided helpers on top of tests/test_guarded_views_host.py, the case tables of
tests/test_gpu_conv_guarded.py, and what can be checked without a GPU.

guarded_nhwc(a)  the (B,H,W,C) array `a` as the channel slice [lead : lead + C] of a NaN map (B, steps, H, W, lead + C + trail), at
                 time step `step`: the neighbour channels, the other time steps and the margins are all NaN.  lead a multiple of 4
                 keeps the pixels 16-byte aligned; lead = 1, or an odd total width, takes the kernels' scalar staging.
OutSlot          an OutView for an output written with a pixel stride (h_out of a cell, h of the gate kernels): the slice
                 [lead : lead + F] of a wider map; the channels around it and the margins hold the sentinel.

THE MARGIN RULE.  The convolution kernels do not clamp, they mask: an out-of-image tap, a channel past C, a pixel past B H W is an
offset the kernel must declare out of range.  One that loses a mask runs further than a 16-row tile - a whole pixel block at the
farthest tap.  So on each side of every view the margin is at least margin_floats of the enclosing map (16 of its batch rows, 1024
floats) AND at least (256 + (kh // 2) dil W + (kw // 2) dil) pixels x the pixel stride: one whole 256-pixel block plus the farthest
tap.  A stray access then gives a wrong value (NaN) or a broken sentinel and NEVER a fault.  test_margins_cover_a_block_and_the_
farthest_tap checks it for every operand and output of every case of the tables.

The references that are WRONG ON PURPOSE (MARGIN = 10, the rule of tests/test_guarded_views_host.py) state what the value checks
can see on finite data:
  (a) "wrap"      'same' padding that wraps into the neighbouring image row instead of reading zero;
  (b) "next map"  a tap that leaves its map by a row and reads the neighbouring map of the batch;
  (c) "neighbour" channels C .. round_up(C, 16) of a slice taken from the neighbour (finite data here, NaN on the GPU) against the
                  rows that follow in the flat weight matrix (forward), or stored into them (weight gradient).
Each is finite and misses the bound its GPU test asserts by a factor of ten at least.  Exemptions, where a mistake cannot differ
from the truth, are stated by exempt(): (a) needs kw > 1 and more than one image row, (b) needs kh > 1 and more than one map, (c) needs a
neighbour (slice cases only) and C % 16 != 0; a single one-pixel map is exempt from (a) and (b), a 1 x 1 filter too.

Bounds (no new tolerance): `close` of tests/test_gpu_convlstm.py for fp32 forward values; the weight-gradient bound of
test_conv2d_weight_gradient_all_taps_per_workgroup and the literals of test_convlstm_gates_backward_softmax_relu_colsum /
test_convlstm_cell_and_softmax, inline there, restated here under names."""
import numpy as np
import pytest
import torch

import test_guarded_views_host as G
from oracle import fov_oracle as O
from test_guarded_views_host import MARGIN, SENTINEL, OutView, _aligned_start, f64, margin_floats, round_up, same_bits, seed_of

BLOCK_PIXELS = 256                  # the largest pixel block of any conv kernel

# ---------------------------------------------------------------------------------------------------------------------
# the bounds of the existing conv tests, under names
# ---------------------------------------------------------------------------------------------------------------------
CLOSE_RTOL, CLOSE_FLOOR, CLOSE_TOL = 1e-3, 1e-5, 2e-5          # close(): per element 1e-3 |ref| + 1e-5 max|ref|; worst 2e-5 max|ref|
WGRAD_TOL = 3e-6                    # test_conv2d_weight_gradient_all_taps_per_workgroup: 3e-6 max|ref| max(1, sqrt(pixels / 1000))
GATES_BWD_TOL = 5e-5                # close(..., tol=5e-5) on dz and dc_prev of convlstm_gates_bwd
SOFTMAX_TOL, SOFTMAX_BWD_TOL = 1e-6, 1e-5
COLSUM_TOL = CLOSE_TOL              # close() with its default


def close_ratio(got, ref, tol=CLOSE_TOL):
    """Worst error in units of close()'s bound (<= 1 passes): the tighter of the per-element and the worst-element bound."""
    got, ref = f64(got), f64(ref)
    scale = max(np.abs(ref).max(), 1e-6) if ref.size else 1.0
    bound = np.minimum(CLOSE_RTOL * np.abs(ref) + CLOSE_FLOOR * scale, tol * scale)
    return float((np.abs(got - ref) / bound).max()) if ref.size else 0.0


def wgrad_bound(ref, pixels):
    return WGRAD_TOL * np.abs(ref).max() * max(1.0, np.sqrt(pixels / 1000.0))


def wgrad_ratio(got, ref, pixels):
    return float(np.abs(f64(got) - f64(ref)).max() / wgrad_bound(f64(ref), pixels))


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def halo_pixels(W, kh=1, kw=1, dil=1):
    """Pixels from a pixel to its farthest tap."""
    return (kh // 2) * dil * W + (kw // 2) * dil


def conv_margin(shape, ld, halo=0):
    """The margin rule: margin_floats of the enclosing map, and a 256-pixel block plus the farthest tap at pixel stride ld."""
    return (max(margin_floats(shape), (BLOCK_PIXELS + halo) * ld) + 3) // 4 * 4


def guarded_nhwc(a, lead=0, trail=0, steps=1, step=0, off=0, device="cpu", halo=0):
    """`a` (B,H,W,C) as the channel slice [lead : lead + C] of time step `step` of a NaN map (B, steps, H, W, lead + C + trail).
    halo: halo_pixels of the filter the view is read with.  The view carries .guard = (first, behind, margin) of the enclosing
    map in its buffer."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    B, H, W, C = a.shape
    wd = lead + C + trail
    shape = (B, steps, H, W, wd)
    n = int(np.prod(shape))
    m = conv_margin(shape, wd, halo)
    buf = torch.full((2 * m + n + 8,), float("nan"), dtype=torch.float32, device=device)
    lo = _aligned_start(buf, m, off)
    v = buf[lo:lo + n].view(shape)[:, step, :, :, lead:lead + C]
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == (4 * (off + lead)) % 16 and v.stride(2) == wd and v.stride(3) == 1
    v.guard = (lo, lo + n, m)
    return v


class OutSlot:
    """An output written with a pixel stride: the channels [lead : lead + F] of a sentinel map (..., lead + F + trail) inside
    sentinel margins.  base None: the call overwrites (the slot is pre-filled with NaN); else it updates `base` in place."""

    def __init__(self, shape, lead=0, trail=0, base=None, off=0, device="cpu", halo=0):
        self.shape, self.lead = tuple(shape), lead
        F = self.shape[-1]
        self.full_shape = self.shape[:-1] + (lead + F + trail,)
        n = int(np.prod(self.full_shape))
        self.m = conv_margin(self.full_shape, lead + F + trail, halo)
        self.buf = torch.full((2 * self.m + n + 8,), SENTINEL, dtype=torch.float32, device=device)
        self.lo = _aligned_start(self.buf, self.m, off)
        self.hi = self.lo + n
        self.full = self.buf[self.lo:self.hi].view(self.full_shape)
        self.v = self.full[..., lead:lead + F]
        self.base = None if base is None else np.ascontiguousarray(base, dtype=np.float32)
        self.inside = torch.zeros(self.buf.shape, dtype=torch.bool, device=device)
        self.inside[self.lo:self.hi].view(self.full_shape)[..., lead:lead + F] = True
        assert self.v.data_ptr() % 16 == (4 * (off + lead)) % 16
        self.v.guard = (self.lo, self.hi, self.m)
        self.reset()

    def reset(self):
        if self.base is None:
            self.v.fill_(float("nan"))
        else:
            self.v.copy_(torch.from_numpy(self.base))

    def _sentinels(self):
        if self.buf.is_cuda:
            torch.cuda.synchronize()
        want = torch.tensor([SENTINEL], dtype=torch.float32).view(torch.int32).item()
        bad = (self.buf.view(torch.int32) != want) & ~self.inside
        assert not bool(bad[:self.lo].any()), "a write in front of the output"
        assert not bool(bad[self.hi:].any()), "a write behind the output"
        assert not bool(bad[self.lo:self.hi].any()), "a write into the channels beside the slot"

    def untouched(self):
        self._sentinels()
        want = OutSlot(self.shape, self.lead, self.full_shape[-1] - self.lead - self.shape[-1], self.base).v
        return same_bits(self.v.cpu().numpy().copy(), want.numpy().copy())

    def result(self):
        self._sentinels()
        out = self.v.cpu().numpy().copy()
        assert not np.isnan(out).any(), "%d of %d output elements are NaN (not written, or computed from a read outside an operand)" % (
            int(np.isnan(out).sum()), out.size)
        return out


def guard_ok(v, ld, halo, block=BLOCK_PIXELS):
    """The margin rule on a view made by guarded_nhwc / OutSlot (.guard) or by guarded / OutView (contiguous: from the view).
    block: rows a kernel's tile spans - 256 pixels of a map; 16 rows (a k-tile) of a weight matrix."""
    base = v._base if v._base is not None else v
    if hasattr(v, "guard"):
        lo, hi, _ = v.guard
    else:
        lo, hi = v.storage_offset(), v.storage_offset() + v.numel()
    need = (block + halo) * ld
    return lo >= need and base.numel() - hi >= need and lo >= 1024 and base.numel() - hi >= 1024


# ---------------------------------------------------------------------------------------------------------------------
# fp64 references, and the same with one mask lost
# ---------------------------------------------------------------------------------------------------------------------
MISTAKES = ("wrap", "next map", "neighbour")


def gather(x, oy, ox, mistake=None):
    """out[b, y, x] = x[b, y + oy, x + ox], zero where the source is outside the image; "wrap": the row test holds, the column test is
    lost (zero only where the flat pixel index leaves the map); "next map": the column test holds, the flat index may run into the neighbouring map of the batch."""
    B, H, W, C = x.shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    sy, sx = yy + oy, xx + ox
    q = (sy * W + sx).reshape(-1)
    if mistake == "wrap":
        ok = ((sy >= 0) & (sy < H)).reshape(-1) & (q >= 0) & (q < H * W)
        src = x.reshape(B, H * W, C)[:, np.clip(q, 0, H * W - 1)]
        return np.where(ok[None, :, None], src, 0.0).reshape(B, H, W, C)
    if mistake == "next map":
        Q = np.arange(B)[:, None] * H * W + q[None]
        ok = ((sx >= 0) & (sx < W)).reshape(-1)[None] & (Q >= 0) & (Q < B * H * W)
        src = x.reshape(B * H * W, C)[np.clip(Q, 0, B * H * W - 1)]
        return np.where(ok[..., None], src, 0.0).reshape(B, H, W, C)
    ok = ((sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)).reshape(-1)
    src = x.reshape(B, H * W, C)[:, np.clip(q, 0, H * W - 1)]
    return np.where(ok[None, :, None], src, 0.0).reshape(B, H, W, C)


def conv_reference(segs, w, b=None, mistake=None, neighbour=None):
    """sum over the segments [(x, dilation)] of conv2d_same(x, the segment's rows of w) (+ b), fp64.  mistake: one of MISTAKES;
    "neighbour": `neighbour` (B,H,W,p) holds the p = round_up(C, 16) - C channels behind the FIRST segment in its wide map; they
    meet the rows that follow the segment's in the flat (kh kw Ctot, N) weight matrix (zero past its end)."""
    w = f64(w)
    kh, kw, Ctot, N = w.shape
    wflat = np.concatenate([w.reshape(kh * kw * Ctot, N), np.zeros((16, N))])
    B, H, W, _ = segs[0][0].shape
    out = np.zeros((B, H, W, N))
    spatial = mistake if mistake in ("wrap", "next map") else None
    c0 = 0
    for si, (x, d) in enumerate(segs):
        x = f64(x)
        C = x.shape[-1]
        for dy in range(kh):
            for dx in range(kw):
                oy, ox = (dy - kh // 2) * d, (dx - kw // 2) * d
                out += gather(x, oy, ox, spatial) @ w[dy, dx, c0:c0 + C]
                if mistake == "neighbour" and si == 0:
                    row = (dy * kw + dx) * Ctot + c0 + C
                    out += gather(f64(neighbour), oy, ox) @ wflat[row:row + neighbour.shape[-1]]
        c0 += C
    return out if b is None else out + f64(b)


def wgrad_reference(x, dy_, kh, kw, dil=1, mistake=None, neighbour=None):
    """dw (kh,kw,C,N) = sum over the pixels of x[pixel + tap] dy[pixel]: the einsum of the existing weight-gradient test, fp64.
    "neighbour": rows C .. of a tap's tile are the neighbour channels' products, stored behind the tap's rows in the flat dw."""
    x, dy_ = f64(x), f64(dy_)
    C, N = x.shape[-1], dy_.shape[-1]
    dw = np.zeros((kh * kw * C + 16, N))
    spatial = mistake if mistake in ("wrap", "next map") else None
    for i in range(kh):
        for j in range(kw):
            oy, ox = (i - kh // 2) * dil, (j - kw // 2) * dil
            t = (i * kw + j) * C
            dw[t:t + C] += np.einsum("bhwc,bhwn->cn", gather(x, oy, ox, spatial), dy_)
            if mistake == "neighbour":
                dw[t + C:t + C + neighbour.shape[-1]] += np.einsum("bhwc,bhwn->cn", gather(f64(neighbour), oy, ox), dy_)
    return dw[:kh * kw * C].reshape(kh, kw, C, N)


def cell_reference(x, h, c, w, b, act, dil=1, mistake=None, neighbour=None):
    """One ConvLSTM2D step from the stacked kernel w = [K ; R] -> h, c, gates (i|f|g|o), z; fp64.  Without a mistake it is
    O.convlstm2d_step (asserted by test_cell_reference_is_the_oracle)."""
    F = w.shape[-1] // 4
    z = conv_reference([(x, dil)] + ([(h, 1)] if h is not None else []), w, b, mistake, neighbour)
    s = O.hard_sigmoid if act == "hard_sigmoid" else O.sigmoid
    i, f, g, o = s(z[..., :F]), s(z[..., F:2 * F]), np.tanh(z[..., 2 * F:3 * F]), s(z[..., 3 * F:])
    cn = i * g if c is None else f * f64(c) + i * g
    return o * np.tanh(cn), cn, np.concatenate([i, f, g, o], -1), z


def exempt(mistake, B, H, W, kh, kw, C, sliced):
    """Where a mistake cannot differ from the truth (see the module docstring)."""
    if mistake == "wrap":
        return kw == 1 or H == 1
    if mistake == "next map":
        return kh == 1 or B == 1
    return not sliced or C % 16 == 0


# ---------------------------------------------------------------------------------------------------------------------
# inputs: every map a function of (case name, map index), so unrelated maps can be appended without touching the first B
# ---------------------------------------------------------------------------------------------------------------------
def maps(name, what, B, shape, scale=1.0):
    return np.stack([scale * np.random.default_rng([seed_of(name + " " + what), b + 1]).standard_normal(shape) for b in range(B)]).astype(np.float32)


def weights(name, kh, kw, C, N, what="w"):
    rng = np.random.default_rng(seed_of(name + " " + what))
    return (rng.standard_normal((kh, kw, C, N)) / np.sqrt(kh * kw * C)).astype(np.float32)


def vector(name, what, n, scale=1.0):
    return (scale * np.random.default_rng(seed_of(name + " " + what)).standard_normal(n)).astype(np.float32)


def view_of(a, v, device, halo=0):
    """`a` through the view description v = (lead, trail, steps, step, off) (None: a dense guarded view)."""
    if v is None:
        v = (0, 0, 1, 0, 0)
    lead, trail, steps, step, off = v
    return guarded_nhwc(a, lead, trail, steps, step, off, device, halo)


DENSE = (0, 0, 1, 0, 0)


def is_slice(v):
    return v is not None and v[1] > 0


# ---------------------------------------------------------------------------------------------------------------------
# case tables.  Pixel counts of the implicit GEMM: 1 (a 1 x 1 map: every tap but the centre is outside), 105 (3 maps of 5 x 7),
# 258 (2 maps of 3 x 43: a block that straddles two maps, two live pixels in the last 256- and the last 128-block), 256 (4 maps of
# 8 x 8, the aligned control).  The values are spread over the families as LAYER_FORMS spreads its own; no cross product.
# ---------------------------------------------------------------------------------------------------------------------
PIXELS = {1: (1, 1, 1), 105: (3, 5, 7), 258: (2, 3, 43), 256: (4, 8, 8)}
FWD_C, FWD_N = (1, 3, 17, 20, 36), (1, 30, 33, 64, 65, 130, 132)
FWD_FILTERS = ((5, 5), (3, 3), (1, 7), (5, 3), (1, 1))
CAT_C1, CAT_C2 = (3, 17, 32), (8, 30)


def igemm(tile, avec, bvec, seg=1, dil=1, ep16=0):
    return "conv2d form: igemm tile %s avec %d bvec %d segments %d dil %d epilogue16 %d" % (tile, avec, bvec, seg, dil, ep16)


def patch(waves_n, step, cvec):
    return "conv2d form: patch waves_n %d step %s cvec %d" % (waves_n, step, cvec)


def fwd(name, family, pix, C, view, N, k, form, dil=1, bias=True, add=None, act=None, C2=0, view2=None, B=None, offs=None):
    B_, H, W = pix if isinstance(pix, tuple) else PIXELS[pix]
    return dict(name=name, family=family, B=B or B_, H=H, W=W, C=C, view=view, N=N, kh=k[0], kw=k[1], dil=dil, bias=bias, add=add, act=act,
                C2=C2, view2=view2, form=form, offs=offs or {})


# view: (lead, trail, steps, step, off).  add: None, "own" (a guarded operand) or "alias" (add is the output, updated in place)
FORWARD_CASES = [
    # conv2d, one segment, no dilation: every N (all three tile shapes, ragged column blocks, N % 4 != 0, N % 4 == 0 with a ragged block)
    fwd("conv-N1", "conv2d", 1, 1, DENSE, 1, (5, 5), igemm("N<=32", 0, 0)),
    fwd("conv-N30", "conv2d", 105, 3, (1, 2, 1, 0, 0), 30, (3, 3), igemm("N<=32", 0, 0), bias=False, add="own", act="relu"),
    fwd("conv-N33", "conv2d", 258, 17, (4, 3, 1, 0, 0), 33, (1, 7), igemm("N<=64", 0, 0)),
    fwd("conv-N64", "conv2d", 256, 20, (4, 8, 1, 0, 0), 64, (5, 3), igemm("N<=64", 1, 1, ep16=1), add="alias"),
    fwd("conv-N65", "conv2d", 105, 36, (0, 0, 2, 1, 0), 65, (1, 1), igemm("N>64", 1, 0)),
    fwd("conv-N130", "conv2d", 258, 20, (8, 4, 1, 0, 0), 130, (5, 5), igemm("N>64", 1, 0), bias=False),
    fwd("conv-N132", "conv2d", 1, 36, DENSE, 132, (3, 3), igemm("N>64", 1, 1, ep16=1), add="own"),
    # dilation 2 and 3; a 1 x 1 map and a 5 x 7 map under a reach of 6 are smaller than the dilated filter
    fwd("dil-N1", "dilated", 105, 3, DENSE, 1, (5, 5), igemm("N<=32", 0, 0, dil=3), dil=3),
    fwd("dil-N30", "dilated", 1, 17, (4, 3, 1, 0, 0), 30, (3, 3), igemm("N<=32", 0, 0, dil=2), dil=2),
    fwd("dil-N33", "dilated", 256, 1, (1, 0, 1, 0, 0), 33, (5, 3), igemm("N<=64", 0, 0, dil=2), dil=2, bias=False),
    fwd("dil-N64", "dilated", 258, 36, (0, 0, 2, 0, 0), 64, (1, 7), igemm("N<=64", 1, 1, dil=3, ep16=1), dil=3),
    fwd("dil-N65", "dilated", 256, 20, (4, 0, 1, 0, 0), 65, (3, 3), igemm("N>64", 1, 0, dil=3), dil=3, add="alias"),
    fwd("dil-N130", "dilated", 105, 36, DENSE, 130, (5, 5), igemm("N>64", 1, 0, dil=2), dil=2, act="relu"),
    fwd("dil-N132", "dilated", 258, 3, (0, 1, 1, 0, 0), 132, (5, 5), igemm("N>64", 0, 1, dil=2, ep16=1), dil=2, add="own"),
    # two segments, the seam inside a k-tile; each segment is its own slice view
    fwd("cat-N1", "cat", 1, 3, (1, 2, 1, 0, 0), 1, (5, 5), igemm("N<=32", 0, 0, 2), C2=8, view2=(4, 4, 1, 0, 0)),
    fwd("cat-N30", "cat", 105, 17, (4, 3, 1, 0, 0), 30, (3, 3), igemm("N<=32", 0, 0, 2), C2=30, view2=(0, 2, 1, 0, 0)),
    fwd("cat-N33", "cat", 258, 32, (4, 4, 1, 0, 0), 33, (1, 7), igemm("N<=64", 1, 0, 2), C2=8, view2=(8, 4, 1, 0, 0)),
    fwd("cat-N64", "cat", 256, 3, (0, 1, 2, 1, 0), 64, (5, 3), igemm("N<=64", 0, 1, 2, ep16=1), C2=30, view2=(1, 1, 1, 0, 0)),
    fwd("cat-N65", "cat", 105, 17, DENSE, 65, (1, 1), igemm("N>64", 0, 0, 2), C2=8, view2=(0, 0, 2, 0, 0), bias=False),
    fwd("cat-N130", "cat", 258, 32, (0, 0, 2, 1, 0), 130, (3, 3), igemm("N>64", 0, 0, 2), C2=30, view2=(4, 2, 1, 0, 0)),
    fwd("cat-N132", "cat", 256, 32, (4, 4, 1, 0, 0), 132, (5, 5), igemm("N>64", 1, 1, 2, ep16=1), C2=8, view2=(8, 4, 1, 0, 0), act="relu"),
]

# the map-resident form (conv_patch.hip) and both sides of conv_patch_shape_ok.  step: "fixed" where rs (W + kw - 1) 24 == 4224
# (W = 18 under a 5-wide filter; W = 9 under a 3-wide one is the same number), else "run-time"
PATCH_MAPS = ((8, 9), (4, 18), (2, 36), (36, 18), (18, 36))
PATCH_C, PATCH_N, PATCH_FILTERS = (32, 36, 48, 33), (1, 30, 33, 65, 130), ((5, 5), (3, 3), (7, 7), (1, 1))
PATCH_CASES = [
    # C = 33 as a slice of a 36- and a 48-wide map: the scalar-channel path (cvec 0), never run before
    fwd("patch-8x9-C33of36", "patch", (2, 8, 9), 33, (0, 3, 1, 0, 0), 30, (3, 3), patch(1, "fixed", 0)),
    fwd("patch-4x18-C33of48", "patch", (2, 4, 18), 33, (8, 7, 1, 0, 0), 65, (5, 5), patch(2, "fixed", 0), add="own", act="relu"),
    fwd("patch-2x36", "patch", (3, 2, 36), 36, (4, 8, 1, 0, 0), 1, (3, 3), patch(1, "run-time", 1), bias=False),
    fwd("patch-36x18", "patch", (1, 36, 18), 32, DENSE, 130, (5, 5), patch(2, "fixed", 1), add="alias", act="relu"),
    fwd("patch-18x36", "patch", (2, 18, 36), 48, (0, 0, 2, 1, 0), 33, (1, 1), patch(2, "run-time", 1), bias=False),
    fwd("patch-8x9-7x7", "patch", (2, 8, 9), 36, DENSE, 33, (7, 7), patch(2, "run-time", 1)),
    fwd("patch-4x18-7x7", "patch", (2, 4, 18), 48, (4, 4, 1, 0, 0), 130, (7, 7), patch(2, "run-time", 1), add="own"),
    fwd("patch-2x36-C33", "patch", (2, 2, 36), 33, (4, 11, 1, 0, 0), 1, (5, 5), patch(1, "run-time", 0)),
    fwd("patch-36x18-C36", "patch", (2, 36, 18), 36, (0, 0, 2, 0, 0), 30, (3, 3), patch(1, "run-time", 1)),
    fwd("patch-18x36-C32", "patch", (1, 18, 36), 32, (8, 8, 1, 0, 0), 65, (5, 5), patch(2, "run-time", 1), act="relu"),
    # the boundaries of the shape check, both sides: 63 | 64 pixels (7 x 9 | 8 x 9 above), 648 | 657, the staging limit
    fwd("edge-7x9", "patch-edge", (2, 7, 9), 48, DENSE, 30, (3, 3), igemm("N<=32", 1, 0)),
    fwd("edge-72x9", "patch-edge", (1, 72, 9), 32, DENSE, 30, (3, 3), patch(1, "fixed", 1)),
    fwd("edge-73x9", "patch-edge", (1, 73, 9), 32, DENSE, 30, (3, 3), igemm("N<=32", 1, 0)),
    fwd("edge-9x72-3x3", "patch-edge", (1, 9, 72), 32, DENSE, 65, (3, 3), patch(2, "run-time", 1)),
    fwd("edge-9x72-5x5", "patch-edge", (1, 9, 72), 32, DENSE, 65, (5, 5), igemm("N>64", 1, 0)),
]


# one case per launcher branch on an operand's address, only that operand four bytes off (or, for x, a pixel stride that is no
# multiple of 4): the patch forms are left, the implicit GEMM takes its scalar staging / scalar epilogue.  The map-resident form
# reads w, bias, add and writes y by elements: it looks at no address but x's, stays, and must be right (the last case)
ADDRESS_FORWARD_CASES = [
    fwd("addr-x-off", "address", (2, 8, 9), 32, (0, 0, 1, 0, 1), 64, (3, 3), igemm("N<=64", 0, 1, ep16=1)),
    fwd("addr-x-stride33", "address", (2, 8, 9), 32, (0, 1, 1, 0, 0), 64, (3, 3), igemm("N<=64", 0, 1, ep16=1)),
    fwd("addr-w-off", "address", 105, 20, (4, 0, 1, 0, 0), 64, (3, 3), igemm("N<=64", 1, 0, ep16=1), offs={"w": 1}),
    fwd("addr-out-off", "address", 105, 20, (4, 0, 1, 0, 0), 64, (3, 3), igemm("N<=64", 1, 1, ep16=0), offs={"out": 1}),
    fwd("addr-add-off", "address", 105, 20, (4, 0, 1, 0, 0), 64, (3, 3), igemm("N<=64", 1, 1, ep16=0), add="own", offs={"add": 1}),
    fwd("addr-bias-off", "address", 105, 20, (4, 0, 1, 0, 0), 64, (3, 3), igemm("N<=64", 1, 1, ep16=0), offs={"b": 1}),
    fwd("addr-patch-others-off", "address", (2, 8, 9), 32, DENSE, 64, (3, 3), patch(2, "fixed", 1), add="own", offs={"w": 1, "b": 1, "add": 1, "out": 1}),
]


def lines(mi, ni, ks, mode, avec, bvec, slices, mps):
    return "conv2d_wgrad form: lines %dx%d ks %d %s avec %d bvec %d slices %d maps_per_slice %d" % (mi, ni, ks, mode, avec, bvec, slices, mps)


def tapwise(variant, split, tps, avec, bvec):
    return "conv2d_wgrad form: tap-wise variant %d split %d tiles_per_split %d avec %d bvec %d" % (variant, split, tps, avec, bvec)


def wg(name, family, B, H, W, C, view, N, k, form, dil=1, accumulate=False, env=None, offs=None, dyview=None):
    return dict(name=name, family=family, B=B, H=H, W=W, C=C, view=view, N=N, kh=k[0], kw=k[1], dil=dil, accumulate=accumulate,
                env=env or {}, form=form, offs=offs or {}, dyview=dyview)


LINES_MAPS = ((1, 1), (3, 5), (4, 6), (36, 18), (5, 64), (64, 3))
LINES_C, LINES_N, LINES_B = (1, 16, 17, 32, 33, 100), (1, 16, 17, 30, 33), (1, 2, 7, 513)
NO_LINES = {"FOV_NO_WGRAD_LINES": "1"}
# the shared scratch holds 512 slices of every case: the lines kernel then splits over min(B, 512, 1024 / tiles) slices
WGRAD_CASES = [
    # lines form: MI x NI in all six shapes, both filter sizes, rows and columns.  513 one-pixel maps: 257 slices of 2, the last has 1
    wg("lines-513x1x1", "lines", 513, 1, 1, 17, (4, 3, 1, 0, 0), 17, (3, 3), lines(2, 2, 3, "rows", 1, 0, 257, 2)),
    wg("lines-3x5", "lines", 2, 3, 5, 1, DENSE, 1, (5, 5), lines(1, 1, 5, "rows", 0, 0, 2, 1)),
    wg("lines-4x6", "lines", 7, 4, 6, 16, (4, 4, 1, 0, 0), 16, (3, 3), lines(1, 1, 3, "columns", 1, 1, 7, 1), accumulate=True),
    wg("lines-36x18", "lines", 1, 36, 18, 33, (4, 3, 1, 0, 0), 30, (5, 5), lines(4, 2, 5, "columns", 1, 0, 1, 1)),
    wg("lines-5x64", "lines", 2, 5, 64, 32, DENSE, 33, (3, 3), lines(2, 2, 3, "rows", 1, 0, 2, 1), accumulate=True),
    wg("lines-64x3", "lines", 1, 64, 3, 100, (0, 4, 1, 0, 0), 16, (5, 5), lines(4, 1, 5, "columns", 1, 1, 1, 1)),
    wg("lines-C17-N1", "lines", 7, 3, 5, 17, (1, 0, 1, 0, 0), 1, (5, 5), lines(2, 1, 5, "rows", 0, 0, 7, 1)),
    wg("lines-C1-N33", "lines", 2, 4, 6, 1, (0, 3, 1, 0, 0), 33, (3, 3), lines(1, 2, 3, "columns", 1, 0, 2, 1)),
    wg("lines-C33-N16", "lines", 2, 1, 1, 33, DENSE, 16, (3, 3), lines(4, 1, 3, "rows", 0, 1, 2, 1)),
    wg("lines-C100-N30", "lines", 1, 3, 5, 100, DENSE, 30, (3, 3), lines(4, 2, 3, "rows", 1, 0, 1, 1)),
    # tap-wise form, all four variants: 1 pixel, 500 pixels (split > 1 with a last k-tile of 4 pixels), 512 (aligned), and maps smaller
    # than 16 pixels (the a_x / a_y trackers wrap more than once per tile)
    wg("taps-v0-1px", "tap-wise", 1, 1, 1, 17, DENSE, 30, (1, 7), tapwise(0, 1, 1, 0, 0)),
    wg("taps-v0-500px", "tap-wise", 100, 1, 5, 32, (4, 4, 1, 0, 0), 33, (5, 5), tapwise(0, 4, 8, 1, 0), env=NO_LINES, accumulate=True),
    wg("taps-v1-500px", "tap-wise", 4, 5, 25, 36, DENSE, 16, (5, 3), tapwise(1, 4, 8, 1, 1)),
    wg("taps-v1-dil", "tap-wise", 8, 8, 8, 33, (4, 3, 1, 0, 0), 17, (3, 3), tapwise(1, 4, 8, 0, 0), dil=2),
    wg("taps-v2-3x5", "tap-wise", 7, 3, 5, 100, (0, 4, 1, 0, 0), 33, (3, 3), tapwise(2, 1, 7, 1, 0)),
    wg("taps-v2-512px", "tap-wise", 8, 8, 8, 97, DENSE, 64, (3, 3), tapwise(2, 4, 8, 0, 1), accumulate=True),
    wg("taps-v3-500px", "tap-wise", 20, 5, 5, 100, (4, 0, 1, 0, 0), 30, (5, 5), tapwise(3, 4, 8, 1, 0), env=NO_LINES),
    wg("taps-v3-dil3", "tap-wise", 2, 3, 5, 132, DENSE, 1, (3, 3), tapwise(3, 1, 2, 1, 0), dil=3),
]


ADDRESS_WGRAD_CASES = [
    wg("addr-lines-x-off", "address", 2, 3, 5, 16, (0, 0, 1, 0, 1), 16, (3, 3), lines(1, 1, 3, "rows", 0, 1, 2, 1)),
    wg("addr-lines-dz-off", "address", 2, 3, 5, 16, DENSE, 16, (3, 3), lines(1, 1, 3, "rows", 1, 0, 2, 1), offs={"dy": 1}),
    wg("addr-taps-x-off", "address", 2, 3, 5, 16, (0, 0, 1, 0, 1), 16, (1, 7), tapwise(0, 1, 2, 0, 1)),
    wg("addr-taps-dz-off", "address", 2, 3, 5, 16, DENSE, 16, (1, 7), tapwise(0, 1, 2, 1, 0), offs={"dy": 1}),
    # dw four bytes off: the slices' reduce (splitk_reduce checks the address itself) leaves its 16-byte form; no trace names that
    wg("addr-lines-dw-off", "address", 2, 3, 5, 16, DENSE, 16, (3, 3), lines(1, 1, 3, "rows", 1, 1, 2, 1), offs={"dw": 1}, accumulate=True),
]


def cellf(kind, *a):
    if kind == "patch":
        return "convlstm_cell form: patch F %d CB %d rows %d groups %d" % a
    tile, avec, bvec, seg, dil = a
    return "convlstm_cell form: igemm tile %s avec %d bvec %d segments %d dil %d" % (tile, avec, bvec, seg, dil)


def cell(name, family, pix, C, view, F, k, form, dil=1, h=DENSE, c=True, gates=True, alias=False, slot=(3, 2), offs=None):
    B, H, W = pix if isinstance(pix, tuple) else PIXELS[pix]
    return dict(name=name, family=family, B=B, H=H, W=W, C=C, view=view, F=F, kh=k[0], kw=k[1], dil=dil, hview=h, c=c, gates=gates,
                alias=alias, slot=slot, form=form, offs=offs or {})


CELL_F = (1, 5, 8, 9, 12, 16, 17, 20, 33)
CELL_PATCH_F, CELL_PATCH_CTOT = (8, 16, 32), (12, 20, 36, 52, 64)
# h: the view of h_prev (None: zero state, w is K alone); c: c_prev given; alias: c_new is c_prev; slot: (lead, trail) of h_out
CELL_CASES = [
    cell("cell-F1", "igemm", 1, 3, (1, 0, 1, 0, 0), 1, (5, 5), cellf("igemm", "F<=8", 0, 0, 2, 1), h=(1, 2, 1, 0, 0), alias=True),
    cell("cell-F5", "igemm", 105, 17, DENSE, 5, (3, 3), cellf("igemm", "F<=8", 0, 0, 1, 1), h=None, c=False),
    cell("cell-F8", "igemm", 258, 3, (0, 1, 1, 0, 0), 8, (3, 3), cellf("igemm", "F<=8", 0, 1, 2, 1), h=(4, 4, 1, 0, 0), gates=False, alias=True),
    cell("cell-F9", "igemm", 256, 20, (4, 4, 1, 0, 0), 9, (5, 5), cellf("igemm", "F<=16", 0, 0, 2, 1), h=(0, 3, 1, 0, 0)),
    cell("cell-F12", "igemm", 105, 36, (0, 0, 2, 1, 0), 12, (3, 3), cellf("igemm", "F<=16", 1, 1, 2, 1), h=(4, 0, 2, 0, 0), c=False, slot=(4, 4)),
    cell("cell-F16", "igemm", 1, 1, DENSE, 16, (5, 5), cellf("igemm", "F<=16", 0, 1, 1, 1), h=None, alias=True),
    cell("cell-F17", "igemm", 258, 3, DENSE, 17, (3, 3), cellf("igemm", "F>16", 0, 0, 2, 1), h=DENSE, gates=False),
    cell("cell-F20", "igemm", 256, 20, (4, 0, 1, 0, 0), 20, (3, 3), cellf("igemm", "F>16", 1, 1, 2, 1), h=(8, 4, 1, 0, 0), alias=True, slot=(0, 1)),
    cell("cell-F33", "igemm", 105, 17, (4, 3, 1, 0, 0), 33, (5, 5), cellf("igemm", "F>16", 0, 0, 1, 1), h=None, c=False),
    # dilated (x only): leaves the patch form
    cell("cell-dil2-F8", "dilated", 105, 20, (4, 0, 1, 0, 0), 8, (5, 5), cellf("igemm", "F<=8", 1, 1, 2, 2), dil=2, h=(4, 4, 1, 0, 0)),
    cell("cell-dil3-F16", "dilated", 258, 3, DENSE, 16, (3, 3), cellf("igemm", "F<=16", 0, 1, 2, 3), dil=3, alias=True),
    cell("cell-dil2-F20", "dilated", 1, 36, DENSE, 20, (5, 5), cellf("igemm", "F>16", 1, 1, 1, 2), dil=2, h=None, gates=False),
    # patch form: CB 1 .. 4 with a short last channel block; 3 x 5 (less than one row tile), 20 x 18 (rows 6, 6, 6, 2), 2 x 112 (one row
    # per group), 1 x W; W = 113 leaves it
    cell("cellp-F8-Ctot12", "patch", (3, 3, 5), 4, (4, 4, 1, 0, 0), 8, (3, 3), cellf("patch", 8, 1, 3, 1), h=(0, 4, 1, 0, 0)),
    cell("cellp-F16-Ctot20", "patch", (2, 20, 18), 4, DENSE, 16, (5, 5), cellf("patch", 16, 2, 6, 4), h=(4, 0, 2, 1, 0), alias=True),
    cell("cellp-F32-Ctot36", "patch", (1, 2, 112), 4, (0, 0, 2, 0, 0), 32, (3, 3), cellf("patch", 32, 3, 1, 2), h=DENSE, gates=False),
    cell("cellp-F32-Ctot52", "patch", (2, 1, 30), 20, (4, 8, 1, 0, 0), 32, (5, 5), cellf("patch", 32, 4, 1, 1), h=(8, 0, 1, 0, 0), c=False),
    cell("cellp-F32-Ctot64", "patch", (2, 3, 5), 32, DENSE, 32, (3, 3), cellf("patch", 32, 4, 3, 1), h=(0, 4, 1, 0, 0), alias=True, slot=(4, 0)),
    cell("cellp-F16-zero-state", "patch", (2, 1, 30), 12, (0, 4, 1, 0, 0), 16, (5, 5), cellf("patch", 16, 1, 1, 1), h=None, c=False),
    cell("cellp-F8-Ctot20", "patch", (1, 20, 18), 12, (4, 0, 1, 0, 0), 8, (3, 3), cellf("patch", 8, 2, 6, 4), h=DENSE, gates=False),
    cell("cellp-W113-leaves", "patch-edge", (1, 1, 113), 4, DENSE, 8, (3, 3), cellf("igemm", "F<=8", 1, 1, 2, 1)),
]

ADDRESS_CELL_CASES = [
    cell("addr-cell-x-off", "address", (2, 3, 5), 4, (0, 0, 1, 0, 1), 8, (3, 3), cellf("igemm", "F<=8", 0, 1, 2, 1)),
    cell("addr-cell-h-off", "address", (2, 3, 5), 4, DENSE, 8, (3, 3), cellf("igemm", "F<=8", 0, 1, 2, 1), h=(0, 0, 1, 0, 1)),
    cell("addr-cell-h-stride9", "address", (2, 3, 5), 4, DENSE, 8, (3, 3), cellf("igemm", "F<=8", 0, 1, 2, 1), h=(0, 1, 1, 0, 0)),
    cell("addr-cell-w-off", "address", (2, 3, 5), 3, DENSE, 8, (3, 3), cellf("igemm", "F<=8", 0, 0, 2, 1), offs={"w": 1}),
    cell("addr-cellp-w-off", "address", (2, 3, 5), 4, DENSE, 8, (3, 3), cellf("patch", 8, 1, 3, 1), offs={"w": 1}),
]

# bf16 forms, one tier smaller: both forms of each entry point on guarded slice and time-step views, a ragged N, C % 16 != 0, a
# one-map batch.  `form` is the launch name (conv2d_wgrad_bf16: the form word of its own trace line).  The map-resident bf16 form
# needs (H + 5) W >= 16 x 44 on top of the fp32 form's rules: 5 x 72 is the smallest map that passes, 4 x 72 the largest that does not
BF16_OP_TOL = 1e-5                  # OP_TOL of tests/test_gpu_convlstm_bf16.py and tests/test_convlstm_cell_bf16_host.py: of max|ref| per tensor
BF16_FORWARD_CASES = [
    fwd("bf16-patch-5x72", "bf16", (1, 5, 72), 36, (4, 8, 1, 0, 0), 33, (3, 3), "conv2d_patch_bf16"),
    fwd("bf16-patch-15x36", "bf16", (2, 15, 36), 48, (0, 0, 2, 1, 0), 30, (5, 5), "conv2d_patch_bf16", bias=False, act="relu"),
    fwd("bf16-edge-4x72", "bf16", (1, 4, 72), 36, (4, 8, 1, 0, 0), 33, (3, 3), "conv2d_plain_bf16"),
    fwd("bf16-plain-5x7", "bf16", 105, 17, (1, 2, 1, 0, 0), 33, (3, 3), "conv2d_plain_bf16", act="relu"),
    fwd("bf16-plain-1x1", "bf16", 1, 36, DENSE, 65, (5, 5), "conv2d_plain_bf16"),
]
BF16_CELL_CASES = [
    cell("bf16-cellp-F8", "bf16", (1, 3, 5), 4, (4, 4, 1, 0, 0), 8, (3, 3), "convlstm_cell_patch_bf16", h=(0, 4, 1, 0, 0)),
    cell("bf16-cellp-F16", "bf16", (1, 20, 18), 12, (0, 0, 2, 1, 0), 16, (5, 5), "convlstm_cell_patch_bf16", alias=True, gates=False),
    cell("bf16-cell-plain-F5", "bf16", 105, 17, (1, 2, 1, 0, 0), 5, (3, 3), "convlstm_cell_plain_bf16", h=(1, 0, 1, 0, 0)),
    cell("bf16-cell-plain-F12", "bf16", 1, 36, DENSE, 12, (5, 5), "convlstm_cell_plain_bf16", h=None, c=False),
]
BF16_WGRAD_CASES = [
    wg("bf16-wgrad-tuned", "bf16", 1, 3, 5, 20, (4, 4, 1, 0, 0), 30, (3, 3), "tuned", dyview=(0, 2, 1, 0, 0)),
    wg("bf16-wgrad-plain", "bf16", 2, 3, 5, 17, DENSE, 33, (3, 3), "plain", accumulate=True),
]

# pointwise and small kernels
GATE_CASES = [(1, 1), (51, 5), (255, 1), (256, 1), (257, 1), (7, 33), (1, 5), (8, 33)]        # (rows, F): rows F in {1, 255, 256, 257}, more than one block
GATE_ROWSF, GATE_F = (1, 255, 256, 257), (1, 5, 33)
SOFTMAX_CASES = [(1, 1), (1, 30), (256, 33), (257, 30), (257, 1), (256, 30), (1, 33)]          # (rows, n)
TRANSPOSE_CASES = [(1, 1, 1, 1), (1, 5, 3, 17), (1, 1, 1, 255), (1, 1, 257, 1), (5, 3, 3, 2)]   # (kh, kw, C, N)
COLSUM_ROWS, COLSUM_COLS = (1, 127, 129, 4095, 4096, 4097), (1, 8, 9, 16, 17)
COLSUM_CASES = [(1, 1), (127, 8), (129, 9), (4095, 16), (4096, 17), (4097, 1), (4096, 8), (4097, 9), (4096, 16), (4095, 17), (129, 1),
                (127, 16), (1, 17), (4097, 8), (4095, 9), (4097, 16), (4096, 1), (4096, 9), (4095, 8), (4095, 1), (4097, 17), (127, 255), (129, 256), (4097, 257)]


# ---------------------------------------------------------------------------------------------------------------------
# operands of a case on a device: the SAME code builds the views the GPU tests run on and the ones the margin test inspects
# ---------------------------------------------------------------------------------------------------------------------
def forward_inputs(c, extra=0):
    """numpy inputs of a forward case (maps B .. B + extra - 1 are the unrelated ones of the map-independence run)."""
    B, n = c["B"] + extra, c["name"]
    p = dict(x=maps(n, "x", B, (c["H"], c["W"], c["C"])), w=weights(n, c["kh"], c["kw"], c["C"] + c["C2"], c["N"]))
    if c["C2"]:
        p["x2"] = maps(n, "x2", B, (c["H"], c["W"], c["C2"]))
    if c["bias"]:
        p["b"] = vector(n, "b", c["N"])
    if c["add"]:
        p["add"] = maps(n, "add", B, (c["H"], c["W"], c["N"]))
    return p


def forward_reference(c, p, mistake=None, neighbour=None):
    segs = [(p["x"], c["dil"])] + ([(p["x2"], 1)] if c["C2"] else [])
    ref = conv_reference(segs, p["w"], p.get("b"), mistake, neighbour)
    if c["add"]:
        ref = ref + f64(p["add"])
    return np.maximum(ref, 0) if c["act"] == "relu" else ref


def forward_operands(c, p, device):
    """-> (dict of guarded operand views, the output OutView).  add "alias": the output's base is `add`."""
    halo = halo_pixels(c["W"], c["kh"], c["kw"], c["dil"])
    B = p["x"].shape[0]
    o = c["offs"]
    t = dict(x=view_of(p["x"], c["view"], device, halo), w=G.guarded(p["w"], o.get("w", 0), device))
    if c["C2"]:
        t["x2"] = view_of(p["x2"], c["view2"], device, halo)
    if c["bias"]:
        t["b"] = G.guarded(p["b"], o.get("b", 0), device)
    if c["add"] == "own":
        t["add"] = view_of(p["add"], (0, 0, 1, 0, o.get("add", 0)), device)
    out = pixel_out((B, c["H"], c["W"], c["N"]), p["add"] if c["add"] == "alias" else None, device, o.get("out", 0))
    return t, out


def wgrad_inputs(c):
    n = c["name"]
    p = dict(x=maps(n, "x", c["B"], (c["H"], c["W"], c["C"])), dy=maps(n, "dy", c["B"], (c["H"], c["W"], c["N"])))
    if c["accumulate"]:
        p["base"] = G.accumulate_base(n, (c["kh"], c["kw"], c["C"], c["N"]))
    return p


def wgrad_operands(c, p, device):
    halo = halo_pixels(c["W"], c["kh"], c["kw"], c["dil"])
    t = dict(x=view_of(p["x"], c["view"], device, halo), dy=view_of(p["dy"], c["dyview"] or (0, 0, 1, 0, c["offs"].get("dy", 0)), device, halo))
    return t, OutView((c["kh"], c["kw"], c["C"], c["N"]), p.get("base"), c["offs"].get("dw", 0), device=device, row=max(c["C"], 16) * c["N"])


def cell_inputs(c, extra=0):
    B, n, F = c["B"] + extra, c["name"], c["F"]
    Ctot = c["C"] + (F if c["hview"] is not None else 0)
    p = dict(x=maps(n, "x", B, (c["H"], c["W"], c["C"])), w=weights(n, c["kh"], c["kw"], Ctot, 4 * F), b=vector(n, "b", 4 * F, 0.5))
    p["w"] = (2.0 * p["w"]).astype(np.float32)          # pre-activations of order 1: the gates leave their linear range
    if c["hview"] is not None:
        p["h"] = maps(n, "h", B, (c["H"], c["W"], F), 0.5)
    if c["c"]:
        p["c"] = maps(n, "c", B, (c["H"], c["W"], F), 0.5)
    return p


def cell_operands(c, p, device):
    """-> (operands, outputs {h_out, c_out, gates}).  alias: c_new is c_prev - an OutView whose base is c_prev."""
    halo = halo_pixels(c["W"], c["kh"], c["kw"], c["dil"])
    B, F = p["x"].shape[0], c["F"]
    shape = (B, c["H"], c["W"], F)
    t = dict(x=view_of(p["x"], c["view"], device, halo), w=G.guarded(p["w"], c["offs"].get("w", 0), device), b=G.guarded(p["b"], device=device))
    if "h" in p:
        t["h"] = view_of(p["h"], c["hview"], device, halo_pixels(c["W"], c["kh"], c["kw"]))
    alias = c["alias"] and "c" in p
    if "c" in p and not alias:
        t["c"] = view_of(p["c"], None, device)
    outs = dict(h_out=OutSlot(shape, c["slot"][0], c["slot"][1], device=device), c_out=pixel_out(shape, p["c"] if alias else None, device))
    if c["gates"]:
        outs["gates"] = pixel_out(shape[:3] + (4 * F,), device=device)
    return t, outs


def pixel_out(shape, base=None, device="cpu", off=0):
    """An OutView over (pixels..., n) whose margins obey the rule: 256 pixels of n floats at least."""
    return OutView(shape, base, off, device=device, row=max(int(np.prod(shape[1:])), 16 * shape[-1]))


def act_of(name):
    return "hard_sigmoid" if seed_of(name) % 2 else "sigmoid"


def extra_maps(c, block=BLOCK_PIXELS):
    """Unrelated maps that fill the case's last pixel block (one more where it is full already)."""
    px, hw = c["B"] * c["H"] * c["W"], c["H"] * c["W"]
    return max(1, (round_up(px, block) - px + hw - 1) // hw)


# ---------------------------------------------------------------------------------------------------------------------
# the harness catches what it is for
# ---------------------------------------------------------------------------------------------------------------------
def _fake_conv(out, x, mistake=None):
    """out (B,H,W,F) = 2 x[..., :F] through the storage underneath the views, with the mistakes of a kernel that lost a mask."""
    F = out.v.shape[-1]
    wd, shift = x.stride(2), {"neighbour channel": 1, "neighbouring time step": x.shape[1] * x.shape[2] * x.stride(2),
                              "pixel before": -x.stride(2), "pixel behind": x.stride(2)}.get(mistake, 0)
    assert wd >= F
    src = torch.as_strided(x, x.shape, x.stride(), x.storage_offset() + shift)
    out.v.copy_(2 * src[..., x.shape[-1] - F:])
    if mistake == "write beside":
        out.full[0, 1, 1, out.lead + F] = 1.0
    if mistake == "write beside in front":
        out.full[-1, -1, -1, out.lead - 1] = 1.0
    if mistake == "unwritten pixel":
        out.v[-1, -1, -1, :] = float("nan")


@pytest.mark.parametrize("mistake,caught", [(None, None), ("neighbour channel", "NaN"), ("neighbouring time step", "NaN"),
                                            ("pixel before", "NaN"), ("pixel behind", "NaN"), ("write beside", "beside the slot"),
                                            ("write beside in front", "beside the slot"), ("unwritten pixel", "NaN")])
@pytest.mark.parametrize("lead,off", [(4, 0), (1, 0), (4, 1)])
def test_the_strided_harness_catches_each_mistake(mistake, caught, lead, off):
    B, H, W, C, F = 2, 3, 5, 6, 4
    x = np.random.default_rng(2).standard_normal((B, H, W, C)).astype(np.float32)
    xv = guarded_nhwc(x, lead, 3, steps=2, step=0, off=off)
    out = OutSlot((B, H, W, F), lead, 2, off=off)
    _fake_conv(out, xv, mistake)
    if caught is None:
        assert same_bits(out.result(), 2 * x[..., C - F:])
    else:
        with pytest.raises(AssertionError, match=caught):
            out.result()


def test_outslot_margins_base_and_untouched():
    base = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    s = OutSlot((2, 3, 4), 2, 3, base=base)
    assert s.untouched() and same_bits(s.result(), base)
    s.v.add_(1.0)
    assert not s.untouched() and same_bits(s.result(), base + 1)
    s.reset()
    assert s.untouched()
    for where, msg in ((s.lo - 1, "in front of"), (s.hi, "behind")):
        t = OutSlot((2, 3, 4), 2, 3, base=base)
        t.buf[where] = 1.0
        with pytest.raises(AssertionError, match=msg):
            t.result()
    fresh = OutSlot((5, 7), 1, 0)
    assert fresh.untouched()
    with pytest.raises(AssertionError, match="NaN"):
        fresh.result()


def test_guarded_nhwc_is_where_it_says():
    a = np.random.default_rng(3).standard_normal((2, 3, 4, 5)).astype(np.float32)
    for lead, trail, steps, step, off in [(0, 0, 1, 0, 0), (4, 3, 1, 0, 0), (1, 0, 3, 1, 0), (0, 2, 2, 1, 1)]:
        v = guarded_nhwc(a, lead, trail, steps, step, off, halo=halo_pixels(4, 5, 5, 3))
        wd = lead + 5 + trail
        assert same_bits(v.numpy().copy(), a) and v.stride() == (steps * 12 * wd, 4 * wd, wd, 1)
        lo, hi, m = v.guard
        assert m >= (256 + halo_pixels(4, 5, 5, 3)) * wd and m >= margin_floats((2, steps, 3, 4, wd)) and guard_ok(v, wd, halo_pixels(4, 5, 5, 3))
        base = v._base
        assert int(torch.isnan(base).sum()) == base.numel() - a.size          # everything but the slice is NaN


# ---------------------------------------------------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------------------------------------------------
def all_forward_cases():
    return FORWARD_CASES + PATCH_CASES + ADDRESS_FORWARD_CASES


def all_wgrad_cases():
    return WGRAD_CASES + ADDRESS_WGRAD_CASES


def all_cell_cases():
    return CELL_CASES + ADDRESS_CELL_CASES


def _ids(cases):
    return [c["name"] for c in cases]


def test_case_names_are_unique_and_every_listed_value_appears_for_every_family_that_can_take_it():
    names = _ids(all_forward_cases() + all_wgrad_cases() + all_cell_cases() + BF16_FORWARD_CASES + BF16_CELL_CASES + BF16_WGRAD_CASES)
    assert len(set(names)) == len(names)
    by = lambda cases, fam: [c for c in cases if c["family"] == fam]
    px = lambda c: c["B"] * c["H"] * c["W"]
    for fam in ("conv2d", "dilated", "cat"):
        cs = by(FORWARD_CASES, fam)
        assert {c["N"] for c in cs} == set(FWD_N) and {px(c) for c in cs} == set(PIXELS), fam
        filters = {(c["kh"], c["kw"]) for c in cs}
        assert filters >= set(FWD_FILTERS) - ({(1, 1)} if fam == "dilated" else set()), fam        # a 1 x 1 filter has nothing to dilate
        if fam == "cat":
            assert {c["C"] for c in cs} == set(CAT_C1) and {c["C2"] for c in cs} == set(CAT_C2)
            assert all(c["view"] is not DENSE or c["view2"] is not DENSE for c in cs)
        else:
            assert {c["C"] for c in cs} == set(FWD_C), fam
        assert {c["add"] for c in cs} >= ({None, "own", "alias"} if fam != "cat" else {None}) and {c["bias"] for c in cs} == {True, False}
    assert {c["dil"] for c in by(FORWARD_CASES, "dilated")} == {2, 3}
    assert any(c["dil"] * (c["kh"] // 2) >= c["H"] and c["H"] > 1 for c in by(FORWARD_CASES, "dilated"))      # a map smaller than the reach
    ps = by(PATCH_CASES, "patch")
    assert {(c["H"], c["W"]) for c in ps} == set(PATCH_MAPS) and {c["C"] for c in ps} == set(PATCH_C) and {c["N"] for c in ps} == set(PATCH_N)
    assert {(c["kh"], c["kw"]) for c in ps} == set(PATCH_FILTERS)
    assert {c["view"][0] + c["C"] + c["view"][1] for c in ps if c["C"] == 33} == {36, 48}
    assert all("cvec 0" in c["form"] for c in ps if c["C"] == 33) and {c["add"] for c in ps} == {None, "own", "alias"}
    assert {c["act"] for c in ps} == {None, "relu"} and {c["bias"] for c in ps} == {True, False}
    assert {(c["H"], c["W"], c["kh"]) for c in by(PATCH_CASES, "patch-edge")} == {(7, 9, 3), (72, 9, 3), (73, 9, 3), (9, 72, 3), (9, 72, 5)}
    ls = by(WGRAD_CASES, "lines")
    assert {(c["H"], c["W"]) for c in ls} == set(LINES_MAPS) and {c["C"] for c in ls} == set(LINES_C) and {c["N"] for c in ls} == set(LINES_N)
    assert {c["B"] for c in ls} == set(LINES_B) and {c["kh"] for c in ls} == {3, 5} and {c["accumulate"] for c in ls} == {True, False}
    assert {c["form"].split(" ks ")[0][-3:] for c in ls} == {"1x1", "1x2", "2x1", "2x2", "4x1", "4x2"}
    assert all(c["N"] <= 32 for c in ls if c["C"] > 96) and any(is_slice(c["view"]) and c["C"] % 4 and "avec 1" in c["form"] for c in ls)
    ts = by(WGRAD_CASES, "tap-wise")
    assert {c["form"].split("variant ")[1][0] for c in ts} == set("0123") and {px(c) for c in ts} >= {1, 500, 512}
    assert any(c["H"] * c["W"] < 16 and px(c) > 16 for c in ts) and any(c["dil"] > 1 for c in ts) and any(c["env"] for c in ts)
    assert any((c["kh"], c["kw"]) == (1, 7) for c in ts) and any((c["kh"], c["kw"]) == (5, 3) for c in ts)
    ig = by(CELL_CASES, "igemm")
    assert {c["F"] for c in ig} == set(CELL_F)
    for cs in (ig, by(CELL_CASES, "patch")):
        assert {c["hview"] is None for c in cs} == {True, False} and {c["c"] for c in cs} == {True, False}
        assert {c["gates"] for c in cs} == {True, False} and any(c["alias"] and c["c"] for c in cs)
    cp = by(CELL_CASES, "patch")
    assert {c["F"] for c in cp} == set(CELL_PATCH_F) and {c["C"] + (c["F"] if c["hview"] is not None else 0) for c in cp} == set(CELL_PATCH_CTOT)
    assert {(c["H"], c["W"]) for c in cp} >= {(3, 5), (20, 18), (2, 112), (1, 30)}
    assert {c["dil"] for c in by(CELL_CASES, "dilated")} == {2, 3}
    for cs in (BF16_FORWARD_CASES, BF16_CELL_CASES, BF16_WGRAD_CASES):
        assert len({c["form"] for c in cs}) == 2 and any(c["B"] == 1 for c in cs) and any(c["C"] % 16 for c in cs)
        assert any(is_slice(c["view"]) for c in cs) and any(c.get("N", 1) % 16 or c.get("F", 16) % 16 for c in cs)
    assert any(c["view"][2] > 1 for c in BF16_FORWARD_CASES) and any(c["view"][2] > 1 for c in BF16_CELL_CASES)
    assert {r * F for r, F in GATE_CASES} >= set(GATE_ROWSF) and {F for _, F in GATE_CASES} == set(GATE_F)
    assert {r for r, _ in SOFTMAX_CASES} == {1, 256, 257} and {n for _, n in SOFTMAX_CASES} == {1, 30, 33}
    assert {kh * kw * C * N for kh, kw, C, N in TRANSPOSE_CASES} >= {1, 255, 257} and any(kh != kw and C != N for kh, kw, C, N in TRANSPOSE_CASES)
    assert {(r, c) for r, c in COLSUM_CASES if r >= 4095} >= {(r, c) for r in (4095, 4096, 4097) for c in COLSUM_COLS}
    assert {r for r, _ in COLSUM_CASES} == set(COLSUM_ROWS) and {c for _, c in COLSUM_CASES} == set(COLSUM_COLS) | {255, 256, 257}


def _views_of(t, outs):
    for k, v in t.items():
        yield k, v
    for k, o in (outs.items() if isinstance(outs, dict) else [("out", outs)]):
        yield k, o.v


def test_margins_cover_a_block_and_the_farthest_tap():
    """Every operand and output of every case: a whole 256-pixel block plus the farthest tap, at the view's pixel stride, lies
    inside the margin on both sides (and 1024 floats at least)."""
    for c in all_forward_cases() + BF16_FORWARD_CASES:
        t, out = forward_operands(c, forward_inputs(c), "cpu")
        halo = halo_pixels(c["W"], c["kh"], c["kw"], c["dil"])
        for k, v in _views_of(t, out):
            ld = v.stride(2) if k in ("x", "x2") else 1 if k == "b" else c["N"]          # (a bias: 256 columns, two column blocks)
            assert guard_ok(v, ld, halo if k in ("x", "x2") else 0, 16 if k == "w" else BLOCK_PIXELS), (c["name"], k)
    for c in all_wgrad_cases() + BF16_WGRAD_CASES:
        t, out = wgrad_operands(c, wgrad_inputs(c), "cpu")
        halo = halo_pixels(c["W"], c["kh"], c["kw"], c["dil"])
        assert guard_ok(t["x"], t["x"].stride(2), halo) and guard_ok(t["dy"], t["dy"].stride(2), halo) and guard_ok(out.v, c["N"], 0), c["name"]
        assert out.m >= 16 * c["C"] * c["N"]          # sixteen taps' rows of the (taps C, N) gradient, and a 256-channel tile (above)
    for c in all_cell_cases() + BF16_CELL_CASES:
        t, outs = cell_operands(c, cell_inputs(c), "cpu")
        halo = halo_pixels(c["W"], c["kh"], c["kw"], c["dil"])
        for k, v in _views_of(t, outs):
            ld = v.stride(2) if k in ("x", "h", "h_out") else 1 if k == "b" else (4 * c["F"] if k in ("w", "gates") else c["F"])
            assert guard_ok(v, ld, halo if k in ("x", "h") else 0, 16 if k == "w" else BLOCK_PIXELS), (c["name"], k)


def _neighbour(c, p, seg="x"):
    """Finite stand-ins for the channels behind a slice, up to the end of its last 16-channel k-tile."""
    C = p[seg].shape[-1]
    return maps(c["name"], "neighbour", p[seg].shape[0], (c["H"], c["W"], round_up(C) - C))


@pytest.mark.parametrize("c", all_forward_cases(), ids=_ids(all_forward_cases()))
def test_forward_reference_is_finite_and_every_lost_mask_misses_the_bound(c):
    p = forward_inputs(c)
    ref = forward_reference(c, p)
    assert np.isfinite(ref).all() and ref.shape == (c["B"], c["H"], c["W"], c["N"])
    if c["dil"] == 1 and not c["C2"] and not c["add"] and c["act"] is None:
        assert np.abs(ref - O.conv2d_same(f64(p["x"]), f64(p["w"]), f64(p["b"]) if c["bias"] else None)).max() < 1e-12
    more = forward_inputs(c, extra_maps(c))
    assert all(same_bits(more[k][:c["B"]] if k in ("x", "x2", "add") else more[k], p[k]) for k in p)
    for m in MISTAKES:
        if exempt(m, c["B"], c["H"], c["W"], c["kh"], c["kw"], c["C"], is_slice(c["view"])):
            continue
        wrong = forward_reference(c, p, m, _neighbour(c, p) if m == "neighbour" else None)
        assert np.isfinite(wrong).all()
        assert close_ratio(wrong, ref) >= MARGIN, (c["name"], m, close_ratio(wrong, ref))


@pytest.mark.parametrize("c", all_wgrad_cases(), ids=_ids(all_wgrad_cases()))
def test_weight_gradient_reference_is_finite_and_every_lost_mask_misses_the_bound(c):
    p = wgrad_inputs(c)
    ref = wgrad_reference(p["x"], p["dy"], c["kh"], c["kw"], c["dil"])
    px = c["B"] * c["H"] * c["W"]
    assert np.isfinite(ref).all()
    for m in MISTAKES:
        if exempt(m, c["B"], c["H"], c["W"], c["kh"], c["kw"], c["C"], is_slice(c["view"])):
            continue
        wrong = wgrad_reference(p["x"], p["dy"], c["kh"], c["kw"], c["dil"], m, _neighbour(c, p) if m == "neighbour" else None)
        assert np.isfinite(wrong).all()
        assert wgrad_ratio(wrong, ref, px) >= MARGIN, (c["name"], m, wgrad_ratio(wrong, ref, px))


@pytest.mark.parametrize("c", all_cell_cases(), ids=_ids(all_cell_cases()))
def test_cell_reference_is_the_oracle_and_every_lost_mask_misses_the_bound(c):
    p, act, F = cell_inputs(c), act_of(c["name"]), c["F"]
    h, cn, gates, z = cell_reference(p["x"], p.get("h"), p.get("c"), p["w"], p["b"], act, c["dil"])
    assert all(np.isfinite(a).all() for a in (h, cn, gates))
    zero = np.zeros((c["B"], c["H"], c["W"], F))
    K, R = f64(p["w"][:, :, :c["C"]]), f64(p["w"][:, :, c["C"]:]) if "h" in p else np.zeros((c["kh"], c["kw"], F, 4 * F))
    ho, co = O.convlstm2d_step(f64(p["x"]), f64(p["h"]) if "h" in p else zero, f64(p["c"]) if "c" in p else zero, K, R, f64(p["b"]), act, c["dil"])
    assert np.abs(h - ho).max() < 1e-12 and np.abs(cn - co).max() < 1e-12
    assert 0.3 < np.sqrt((z ** 2).mean()) < 5.0                 # the gates are neither all linear nor all saturated
    for m in MISTAKES:
        if exempt(m, c["B"], c["H"], c["W"], c["kh"], c["kw"], c["C"], is_slice(c["view"])):
            continue
        wrong = cell_reference(p["x"], p.get("h"), p.get("c"), p["w"], p["b"], act, c["dil"], m, _neighbour(c, p) if m == "neighbour" else None)
        assert all(np.isfinite(a).all() for a in wrong)
        assert max(close_ratio(wrong[0], h), close_ratio(wrong[1], cn)) >= MARGIN, (c["name"], m)


def test_the_wrong_references_differ_only_where_they_should():
    """wrap and next map agree with the truth on a single one-pixel map and for a 1 x 1 filter (the exemptions are real), and differ
    on a batch of 4 x 5 maps under a 3 x 3 filter."""
    x = maps("exempt", "x", 1, (1, 1, 4))
    w = weights("exempt", 3, 3, 4, 5)
    assert all(np.array_equal(conv_reference([(x, 1)], w, None, m), conv_reference([(x, 1)], w)) for m in ("wrap", "next map"))
    x = maps("exempt", "x", 3, (4, 5, 4))
    w1 = weights("exempt", 1, 1, 4, 5)
    assert all(np.array_equal(conv_reference([(x, 1)], w1, None, m), conv_reference([(x, 1)], w1)) for m in ("wrap", "next map"))
    w = weights("exempt", 3, 3, 4, 5)
    assert all(not np.array_equal(conv_reference([(x, 1)], w, None, m), conv_reference([(x, 1)], w)) for m in ("wrap", "next map"))


def test_bf16_cases_every_lost_mask_misses_the_bf16_bound():
    """The bf16 entry points are asserted to BF16_OP_TOL of max|ref| (weight gradient: units of the same 1e-5): a lost mask misses
    that by MARGIN on the fp64 references too (the rounding of the operands moves a value by 2^-9 of itself, not by a tap)."""
    for c in BF16_FORWARD_CASES:
        p = forward_inputs(c)
        ref = forward_reference(c, p)
        for m in MISTAKES:
            if not exempt(m, c["B"], c["H"], c["W"], c["kh"], c["kw"], c["C"], is_slice(c["view"])):
                wrong = forward_reference(c, p, m, _neighbour(c, p) if m == "neighbour" else None)
                assert np.isfinite(wrong).all() and np.abs(wrong - ref).max() >= MARGIN * BF16_OP_TOL * np.abs(ref).max(), (c["name"], m)
    for c in BF16_WGRAD_CASES:
        p = wgrad_inputs(c)
        ref = wgrad_reference(p["x"], p["dy"], c["kh"], c["kw"])
        for m in MISTAKES:
            if not exempt(m, c["B"], c["H"], c["W"], c["kh"], c["kw"], c["C"], is_slice(c["view"])):
                wrong = wgrad_reference(p["x"], p["dy"], c["kh"], c["kw"], 1, m, _neighbour(c, p) if m == "neighbour" else None)
                assert np.isfinite(wrong).all() and np.abs(wrong - ref).max() >= MARGIN * 10 * BF16_OP_TOL * np.abs(ref).max(), (c["name"], m)
