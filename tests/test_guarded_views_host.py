"""Guarded views for the recurrent kernels, the few-row weight gradients and the small heads: the helpers, the case tables of
tests/test_gpu_ragged_guarded.py, and what can be checked without a GPU.

guarded(a)   a contiguous view of `a` inside a NaN buffer.  The margin on each side is at least 16 rows of the operand (a row
             is everything behind the batch index: T*F floats of x, T*5*H of the reserve) and at least 1024 floats, so a kernel
             that reads a whole padded 16-row tile, or a k-block past the operand's last row, gets a NaN and a wrong value -
             never a fault.  off = 1 starts the view one float behind a 16-byte boundary.
OutView      an output view inside a sentinel buffer with the same margins: pre-filled with NaN where the call overwrites
             (int32: UNWRITTEN_I32), with `base` where it accumulates.  result() asserts that every sentinel survives bit for
             bit and that no NaN is left inside.
Both take a device, so the harness itself is tested here: fake kernels that write one element in front of / behind the view,
leave one unwritten or read one row past an operand are caught, one that stays in bounds passes.

The references that are WRONG ON PURPOSE state what the GPU checks can see: db, dK, dR of a layer and dW, db of a Dense head
with the padding rows of the ragged 16-row tile filled by copies of row B - 1 - what a kernel returns that clamps its row
index into the tensor but does not mask the padded rows out of the sum over rows.  They are finite and plausible; each must
miss the bound of the GPU test (check_grads of tests/test_gpu_train.py: 1e-4 of the tensor's max |ref| on the worst element; for
the TF, mixture and raw heads the heads' own 2e-4 of max + 1e-6, every layer) by MARGIN = 10 at least, or the case's inputs are too tame.  The upstream gradient of the last live row is of order 1
(layer_inputs) for that reason.  B = 16, the aligned control, has no padding and is left out.

The case tables are walked here: every case's fp64 reference is finite and every ragged row count is ragged."""
import zlib

import numpy as np
import pytest
import torch

import test_gpu_train as TR
from oracle import fov_oracle as O

SENTINEL = -12345.5
SENTINEL_I32 = -1234567
UNWRITTEN_I32 = 0x7FC00000          # the bits of a quiet NaN: an int32 output's "not written yet"
MARGIN = 10.0                       # a wrong-on-purpose reference misses its bound by this factor at least
TILE = 16


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
def margin_floats(shape):
    """>= 16 rows of the operand and >= 1024 elements, a multiple of four."""
    row = int(np.prod(shape[1:])) if len(shape) > 1 else 1
    return (max(1024, TILE * row) + 3) // 4 * 4


def _aligned_start(buf, m, off):
    """Index of the element `off` behind the first 16-byte boundary at or after element m of `buf`."""
    assert buf.element_size() == 4
    skew = (-(buf.data_ptr() // 4 + m)) % 4
    return m + skew + off


def guarded(a, off=0, device="cpu"):
    """A contiguous view of `a` (float32) inside a NaN buffer on `device`."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    m = margin_floats(a.shape)
    buf = torch.full((2 * m + a.size + 8,), float("nan"), dtype=torch.float32, device=device)
    lo = _aligned_start(buf, m, off)
    v = buf[lo:lo + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return v


class OutView:
    """An output view inside a sentinel buffer.  base None: the call overwrites (pre-filled with NaN / UNWRITTEN_I32); else
    the call accumulates onto `base`.  `row`: elements per row where the shape's leading axis is not the batch (a flat
    gradient buffer)."""

    def __init__(self, shape, base=None, off=0, dtype=torch.float32, device="cpu", row=None):
        self.shape, self.dtype = tuple(shape), dtype
        n = int(np.prod(shape))
        self.m = m = margin_floats((0, row) if row else self.shape)
        self.sentinel = SENTINEL if dtype == torch.float32 else SENTINEL_I32
        self.buf = torch.full((2 * m + n + 8,), self.sentinel, dtype=dtype, device=device)
        self.lo = _aligned_start(self.buf, m, off)
        self.hi = self.lo + n
        self.flat = self.buf[self.lo:self.hi]
        self.base = None if base is None else np.ascontiguousarray(base, dtype=np.float32 if dtype == torch.float32 else np.int32).reshape(-1)
        self.v = self.flat.view(self.shape)
        assert self.v.data_ptr() % 16 == 4 * off
        self.reset()

    def reset(self):
        """Back to the state before the call (for the second of two calls that must give the same bits)."""
        if self.base is not None:
            self.flat.copy_(torch.from_numpy(self.base))
        elif self.dtype == torch.float32:
            self.flat.fill_(float("nan"))
        else:
            self.flat.fill_(UNWRITTEN_I32)

    def part(self, start, shape):
        n = int(np.prod(shape))
        assert 0 <= start and start + n <= self.hi - self.lo
        return self.flat[start:start + n].view(shape)

    def untouched(self):
        """True when the view still holds what reset() put there (a refused call wrote nothing) and the sentinels stand."""
        self._sentinels()
        bits = self.flat.view(torch.int32).cpu()
        want = OutView(self.shape, self.base, dtype=self.dtype).flat.view(torch.int32)
        return bool((bits == want).all())

    def _sentinels(self):
        if self.buf.is_cuda:
            torch.cuda.synchronize()
        bits = self.buf.view(torch.int32)
        want = torch.tensor([self.sentinel], dtype=self.dtype).view(torch.int32).item()
        assert bool((bits[:self.lo] == want).all()), "a write in front of the output"
        assert bool((bits[self.hi:] == want).all()), "a write behind the output"

    def result(self):
        self._sentinels()
        out = self.v.cpu().numpy().copy()
        if self.dtype == torch.float32:
            assert not np.isnan(out).any(), "%d of %d output elements are NaN (not written, or computed from a read outside an operand)" % (
                int(np.isnan(out).sum()), out.size)
        else:
            assert not (out == UNWRITTEN_I32).any(), "an output element was not written"
        return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(np.int32) == b.view(np.int32)).all())


def seed_of(name):
    return zlib.crc32(name.encode())


def round_up(n, k=TILE):
    return (n + k - 1) // k * k


# ---------------------------------------------------------------------------------------------------------------------
# case tables.  Shapes: the smallest at which each seam exists.  B: 1 (one live row), 17 (a second tile with one live row of
# its first quad), 30 (a second tile whose last quad has two live rows), 16 (the aligned control).  T in {1, 2, 3} (the
# two-deep reserve / dhs prefetch clamps t - 2 and t - 1); F in {6, 90, 96, 256} where the form allows.
# ---------------------------------------------------------------------------------------------------------------------
BATCHES = (1, 17, 30, 16)

# (name, launched, dtype, impl, H, knobs, [(F, T) for B = 1, 17, 30, 16])        `launched`: the recurrent launch's trace name
LAYER_FORMS = [
    ("generic-32", "generic", "f32", "generic", 32, {}, [(6, 1), (90, 2), (96, 3), (11, 2)]),
    ("generic-40", "generic", "f32", "generic", 40, {}, [(90, 3), (6, 1), (11, 2), (96, 3)]),
    ("cluster-64", "cluster", "f32", "cluster", 64, {}, [(90, 2), (96, 3), (6, 1), (90, 3)]),
    ("cluster-128", "cluster", "f32", "cluster", 128, {}, [(96, 3), (6, 1), (90, 2), (6, 2)]),
    ("cluster-256", "cluster", "f32", "cluster", 256, {}, [(6, 1), (90, 2), (96, 3), (90, 1)]),
    ("wide-256-F256", "wide LSTM", "f32", "cluster", 256, {}, [(256, 3), (256, 1), (256, 2), (256, 3)]),
    ("wide-512-narrow", "wide LSTM", "f32", "auto", 512, {"FOV_NO_WIDE16": "1"}, [(90, 1), (96, 2), (6, 3), (90, 2)]),
    ("wide-512-zx", "wide LSTM", "f32", "auto", 512, {"FOV_NO_WIDE16": "1"}, [(256, 2), (100, 3), (256, 1), (256, 3)]),
    ("wide16-128", "wide16 LSTM", "f32", "auto", 128, {}, [(90, 3), (6, 2), (96, 1), (128, 2)]),
    ("wide16-256", "wide16 LSTM", "f32", "auto", 256, {}, [(256, 1), (90, 3), (6, 2), (96, 1)]),
    ("wide16-512", "wide16 LSTM", "f32", "auto", 512, {}, [(96, 2), (512, 1), (90, 3), (6, 2)]),
    # the three x stagings of lstm_layer_bf16.hip, each under its own trace name: F <= 96 narrow; wider with F % 4 == 0 and an aligned
    # x by 16-byte pieces; wider otherwise by elements
    ("bf16-vector-x", "bf16 LSTM layer (vector x)", "bf16", "auto", 256, {}, [(256, 2), (256, 3), (256, 1), (256, 3)]),
    ("bf16-narrow-x", "bf16 LSTM layer (narrow x)", "bf16", "auto", 256, {}, [(90, 1), (6, 2), (96, 3), (90, 2)]),
    ("bf16-scalar-x", "bf16 LSTM layer (scalar x)", "bf16", "auto", 256, {}, [(250, 2), (130, 1), (202, 3), (250, 2)]),
]

# (name, launched, dtype, H, knobs, [(F, T) for B = 1, 17, 30, 16]): the rows of BACKWARD_FORMS in tests/test_gpu_value_regimes.py
# (same knobs; asserted equal there), each with the trace name of its recurrence.  F = 256 on lstm_bwd8: dx in the kernel.
BACKWARD_FORMS = [
    ("bwd_cluster-64", "bwd cluster", "f32", 64, {}, [(6, 1), (90, 2), (96, 3), (90, 2)]),
    ("bwd_cluster-128", "bwd cluster", "f32", 128, {"FOV_NO_BWD16_NARROW": "1"}, [(90, 2), (96, 3), (6, 1), (6, 3)]),
    ("bwd_cluster-256", "bwd cluster", "f32", 256, {"FOV_NO_BWD16_NARROW": "1", "FOV_BWD_GROUPS4": "1"}, [(96, 3), (6, 1), (90, 2), (256, 2)]),
    ("bwd8-256", "8-group BPTT", "f32", 256, {"FOV_NO_BWD16_NARROW": "1"}, [(256, 1), (256, 2), (256, 3), (90, 2)]),
    ("bwd16-128", "16-unit BPTT", "f32", 128, {}, [(90, 3), (6, 2), (96, 1), (90, 2)]),
    ("bwd16-256", "16-unit BPTT", "f32", 256, {}, [(256, 2), (90, 3), (6, 1), (96, 2)]),
    ("bwd16-512", "16-unit BPTT", "f32", 512, {}, [(96, 1), (256, 2), (90, 3), (6, 2)]),
    ("bwd16-512-groups32", "16-unit BPTT", "f32", 512, {"FOV_BWD16_GROUPS": "32"}, [(6, 2), (90, 1), (96, 3), (90, 3)]),
    ("stepped-256", "lstm_bwd_pointwise", "f32", 256, {"FOV_BWD_STEPPED": "1"}, [(90, 3), (6, 2), (256, 1), (96, 2)]),
    ("bwd8-256-bf16", "8-group BPTT", "bf16", 256, {}, [(256, 2), (90, 1), (256, 3), (6, 2)]),
]
# what one backward case runs, in this order, on one tape.  state: h0 / c0 given; ups: s = dhs, h = dhT, c = dcT; adjacent: dK | dR
# | db in one flat buffer (the fused product where the form and the row count take it); base: accumulate onto a non-zero base
BACKWARD_VARIANTS = [
    dict(name="overwrite", state=True, ups="shc", adjacent=False, base=False),
    dict(name="accumulate-adjacent", state=False, ups="s", adjacent=True, base=True),
    dict(name="final-state-only", state=True, ups="hc", adjacent=False, base=False),
    # without the few-row kernels (which take dK, dR AND db of every fp32 case at these row counts) db is what the BPTT kernel
    # summed itself: per-tile partials over its rows, padded ones included unless masked, then a column sum
    dict(name="db-from-the-kernel", state=True, ups="s", adjacent=False, base=True, env={"FOV_NO_WGRAD_GROUP": "1"}),
]

# few-row weight gradients (fov_lstm_seq_wgrad): (name, trace line, H, F, B, T, h0 given)
WGRAD_CASES = [
    ("rows-64", "wgrad_rows", 64, 6, 17, 3, True),
    ("rows-256", "wgrad_rows", 256, 90, 30, 1, False),
    ("rows-256-F256", "wgrad_rows", 256, 256, 1, 3, True),
    ("rows-512", "wgrad_rows", 512, 96, 17, 2, False),
    # wgrad_rows takes up to 640 rows at H <= 512 and comes first: wgrad_group is reached from 641 to 1024 rows at H = 512
    ("group-512", "wgrad_group", 512, 90, 30, 23, True),
    ("group-512-wide-x", "wgrad_group", 512, 512, 17, 39, False),
]
# (name, H, F1, T1, F2, T2, B): fov_lstm_seq_wgrad_pair, T1 != T2, the decoder's h0 is the encoder's final h
WGRAD_PAIR_CASES = [("pair-64", 64, 90, 3, 6, 2, 17), ("pair-256", 256, 90, 2, 6, 3, 30), ("pair-128", 128, 96, 1, 6, 3, 1)]

# Dense heads: (name, trace name of the kernel, N rows, In, Out, activation).  launch_dense has four kernels, each under its own
# trace name: Out > 8, N <= 256, 128 <= In <= 2048 -> dense_fewrows_kernel (four rows per workgroup); Out <= 8 and N >= 64 ->
# dense_small_kernel (16 rows per workgroup; 16-byte x staging for In % 4 == 0 and an aligned x); else dense_kernel (a wave per row)
DENSE_FEW, DENSE_16V, DENSE_16S, DENSE_WAVE = "dense (few rows)", "dense (16 rows, vector x)", "dense (16 rows, scalar x)", "dense (wave per row)"
DENSE_CASES = [("dense-17x256x6", DENSE_WAVE, 17, 256, 6, "tanh"), ("dense-30x90x6", DENSE_WAVE, 30, 90, 6, "tanh"),
               ("dense-1x256x6", DENSE_WAVE, 1, 256, 6, "linear"), ("dense-85x256x6", DENSE_16V, 85, 256, 6, "tanh"),
               ("dense-70x90x6", DENSE_16S, 70, 90, 6, "tanh"), ("dense-17x400x32", DENSE_FEW, 17, 400, 32, "linear"),
               ("dense-30x130x12", DENSE_FEW, 30, 130, 12, "tanh"), ("dense-aligned", DENSE_16V, 64, 256, 6, "tanh")]
# (name, trace name, N, In, Out, add row stride): the strided `add` read of every kernel
DENSE_ADD_CASES = [("dense-add-6x6", DENSE_WAVE, 17, 6, 6, 11), ("dense-add-1row", DENSE_WAVE, 1, 6, 6, 6), ("dense-add-30", DENSE_WAVE, 30, 6, 6, 40),
                   ("dense-add-85x256", DENSE_16V, 85, 256, 6, 9), ("dense-add-70x90", DENSE_16S, 70, 90, 6, 6), ("dense-add-17x400x32", DENSE_FEW, 17, 400, 32, 37)]
MIX_HEAD_CASES = [("mix-head-17", 17, 256, 6), ("mix-head-1", 1, 256, 6), ("mix-head-30", 30, 64, 3), ("mix-head-16", 16, 256, 6)]


# fused encoder + free-running decoder: (name, launched, dtype, impl, H, [(F_enc, T_in, T_out) for B = 1, 17, 30, 16]); F_dec = 6
DECODE_FORMS = [
    ("decode-generic-32", "generic", "f32", "generic", 32, [(90, 1, 3), (6, 2, 1), (96, 3, 2), (90, 2, 2)]),
    ("decode-cluster-64", "fused cluster", "f32", "cluster", 64, [(90, 2, 1), (96, 3, 2), (6, 1, 3), (90, 3, 3)]),
    ("decode-cluster-128", "fused cluster", "f32", "cluster", 128, [(96, 3, 2), (6, 1, 3), (90, 2, 1), (6, 2, 2)]),
    ("decode-cluster-256", "fused cluster", "f32", "cluster", 256, [(6, 1, 3), (90, 2, 1), (96, 3, 2), (90, 1, 1)]),
    ("decode-wide16-128", "seq2seq decode (wide16)", "f32", "auto", 128, [(90, 3, 1), (6, 1, 2), (96, 2, 3), (90, 2, 2)]),
    ("decode-wide16-256", "seq2seq decode (wide16)", "f32", "auto", 256, [(96, 2, 3), (90, 3, 1), (6, 1, 2), (90, 3, 3)]),
    ("decode-bf16-vector-x", "bf16 seq2seq decode (vector x)", "bf16", "auto", 256, [(256, 1, 2), (256, 2, 3), (256, 3, 1), (256, 2, 2)]),
    ("decode-bf16-narrow-x", "bf16 seq2seq decode (narrow x)", "bf16", "auto", 256, [(90, 2, 3), (6, 3, 1), (96, 1, 2), (90, 2, 2)]),
    ("decode-bf16-scalar-x", "bf16 seq2seq decode (scalar x)", "bf16", "auto", 256, [(250, 2, 1), (130, 1, 2), (202, 3, 3), (250, 1, 1)]),
]
# the decoder half alone from a given state (fov_seq2seq_decoder_fwd): (name, launched, impl, H, [T_out for B = 1, 17, 30, 16])
DECODER_FORMS = [("decoder-generic-40", "generic", "generic", 40, [3, 1, 2, 2]), ("decoder-cluster-64", "cluster", "cluster", 64, [1, 2, 3, 2]),
                 ("decoder-cluster-256", "cluster", "cluster", 256, [2, 3, 1, 3]), ("decoder-wide16-256", "seq2seq decode (wide16)", "auto", 256, [3, 1, 2, 1])]
# the teacher-forced graph (fov_seq2seq_tf_fwd: two layer calls and the Dense head): (name, layer launches, impl, H, B, F_enc, T_in, T_out)
TF_CASES = [("tf-generic-32", ["generic"], "generic", 32, 17, 90, 2, 3), ("tf-cluster-128", ["cluster"], "cluster", 128, 30, 96, 3, 1),
            ("tf-auto-256", ["wide16 LSTM"], "auto", 256, 1, 6, 1, 2), ("tf-cluster-64", ["cluster"], "cluster", 64, 17, 90, 3, 2)]
F_DEC = 6


def decode_cases():
    return [("%s-B%d" % (f[0], B), f, B) + f[5][i] for f in DECODE_FORMS for i, B in enumerate(BATCHES)]


def decoder_cases():
    return [("%s-B%d" % (f[0], B), f, B, f[4][i]) for f in DECODER_FORMS for i, B in enumerate(BATCHES)]


def decode_inputs(name, B, T_in, T_dec, F_enc, H, rows=None):
    """Weights of the target-only seq2seq model and, per row, the encoder input (T_in, F_enc), the first decoder input, T_dec
    teacher-forced decoder inputs and an initial state."""
    rows = B if rows is None else rows
    w = O.init_seq2seq(seed_of(name) % (1 << 31), F_enc=F_enc, F_dec=F_DEC, H=H, bias_noise=0.1)
    per_row = []
    for r in range(rows):
        g = np.random.default_rng([seed_of(name), r + 1])
        per_row.append(dict(enc=g.uniform(-1, 1, (T_in, F_enc)), dec0=g.uniform(-1, 1, (1, F_DEC)), dec_in=g.uniform(-1, 1, (T_dec, F_DEC)),
                            h0=0.3 * g.standard_normal(H), c0=0.3 * g.standard_normal(H)))
    out = {k: np.stack([p[k] for p in per_row]).astype(np.float32) for k in per_row[0]}
    out["w"] = w
    return out


def decoder_reference(p, B, T_out, act):
    """The decoder half alone from (h0, c0): T_out steps of LSTM + Dense(tanh) fed back -> out, hT, cT (fp64)."""
    w = {k: f64(v) for k, v in p["w"].items()}
    y, h, c = f64(p["dec0"][:B, 0]), f64(p["h0"][:B]), f64(p["c0"][:B])
    out = []
    for _ in range(T_out):
        h, c = O.lstm_step(y, h, c, w["dec_K"], w["dec_R"], w["dec_b"], act)
        y = O.dense(h, w["dense_W"], w["dense_b"])
        out.append(y)
    return {"out": np.stack(out, 1), "hT": h, "cT": c}


# a layer from a precomputed input projection zx = x K (fov_lstm_seq_fwd_zx): (name, launched, impl, H, [T for B = 1, 17, 30, 16])
ZX_FORMS = [("zx-generic-40", "generic", "generic", 40, [1, 2, 3, 2]), ("zx-cluster-128", "cluster", "cluster", 128, [2, 3, 1, 3]),
            ("zx-cluster-256", "cluster", "auto", 256, [3, 1, 2, 1]), ("zx-wide-512", "wide LSTM", "auto", 512, [1, 3, 2, 2])]
# two stacked layers in one launch: (name, launched, dtype, H, [(F, T) for B = 1, 17, 30, 16]); T >= 2 (the launches require it)
STACK2_FORMS = [("stack2-512", "two-layer width-512", "f32", 512, [(90, 2), (6, 3), (96, 2), (90, 3)]),
                ("stack2-bf16", "bf16 two-layer", "bf16", 256, [(6, 3), (96, 2), (90, 3), (90, 2)])]


def zx_cases():
    return [("%s-B%d" % (f[0], B), f, B, f[4][i]) for f in ZX_FORMS for i, B in enumerate(BATCHES)]


def stack2_cases():
    return [("%s-B%d" % (f[0], B), f, B) + f[4][i] for f in STACK2_FORMS for i, B in enumerate(BATCHES)]


def zx_reference(zx, R, b, h0, c0, act):
    """fp64 layer from the projection as given -> hs, hT, cT, reserve."""
    zx, R, b = f64(zx), f64(R), f64(b)
    B, T, _ = zx.shape
    H = R.shape[0]
    h = np.zeros((B, H)) if h0 is None else f64(h0)
    c = np.zeros((B, H)) if c0 is None else f64(c0)
    s = O.hard_sigmoid if act == "hard_sigmoid" else O.sigmoid
    hs, res = np.empty((B, T, H)), np.empty((B, T, 5, H))
    for t in range(T):
        z = zx[:, t] + b + h @ R
        i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
        c = f * c + i * g
        h = o * np.tanh(c)
        hs[:, t] = h
        res[:, t] = np.stack([i, f, g, o, c], 1)
    return hs, h, c, res


def stack2_inputs(name, B, T, F, H, rows=None):
    """Layer 1 (F -> H) as layer_inputs; layer 2 (H -> H) with its own weights, state and upstream gradients."""
    a = layer_inputs(name, B, T, F, H, rows)
    b = layer_inputs(name + " upper", B, T, H, H, rows)
    return a, b


def stack2_reference(a, b, B, act, state, bf16=False):
    """-> [(hs, hT, cT, res)] * 2 on the first B rows."""
    st = lambda p: (p["h0"][:B], p["c0"][:B]) if state else None
    return O.regime_stack2_forward([(a["K"], a["R"], a["b"]), (b["K"], b["R"], b["b"])], a["x"][:B], [st(a), st(b)], act, np.float64, bf16)


# the fused others-mixing decoder (H = 256, O = 6: mix_decoder_supported): (name, dtype, [T for B = 1, 17, 30, 16])
MIX_FORMS = [("mix-decoder", "f32", [1, 3, 2, 2]), ("mix-decoder-bf16", "bf16", [3, 2, 1, 3])]
MIX_H, MIX_O = 256, 6
# the two-layer heads of the TF model: (B, H, M, O), accumulate
TF_HEAD_CASES = [((17, 400, 32, 3), False), ((1, 40, 32, 3), True), ((30, 400, 32, 3), True)]
# the fused Dense chains: (kind, B, H, mixtures, masks, accumulate)
MLP_HEAD_CASES = [("gmm", 1, 40, 3, False, False), ("gmm", 17, 400, 20, True, True), ("gmm", 30, 40, 3, True, False),
                  ("raw", 1, 400, 0, False, True), ("raw", 17, 40, 0, False, False), ("raw", 30, 400, 0, False, True)]
# Dense + mean squared error in one launch: (rows, H, O, activation)
DENSE_MSE_CASES = [(17, 256, 6, "tanh"), (257, 128, 6, "linear")]


def mix_cases():
    return [("%s-B%d" % (f[0], B), f, B, f[2][i]) for f in MIX_FORMS for i, B in enumerate(BATCHES)]


def mix_inputs(name, B, T, rows=None):
    """Weights of the unrolled others-mixing decoder and, per row: first input, the four initial states, the others' projection
    (T, O) and the loss gradient (T, O), of order 1 in the last live row."""
    rows = B if rows is None else rows
    H, O_ = MIX_H, MIX_O
    rng = np.random.default_rng(seed_of(name))
    w = {}
    for l, F in (("dec1", O_), ("dec2", H)):
        K, R, b = O.init_lstm(rng, F, H, np.float32)
        w[l + "_K"], w[l + "_R"], w[l + "_b"] = K, R, (b + 0.1 * rng.standard_normal(b.shape)).astype(np.float32)
    w["dense_W"] = (rng.standard_normal((H, O_)) / np.sqrt(H)).astype(np.float32)
    w["dense_b"] = (0.1 * rng.standard_normal(O_)).astype(np.float32)
    Wp = (rng.standard_normal((O_, O_)) / np.sqrt(O_)).astype(np.float32)
    per_row = []
    for r in range(rows):
        g = np.random.default_rng([seed_of(name), r + 1])
        per_row.append(dict(dec0=g.uniform(-1, 1, O_), h1=0.3 * g.standard_normal(H), c1=0.3 * g.standard_normal(H), h2=0.3 * g.standard_normal(H),
                            c2=0.3 * g.standard_normal(H), oth=g.uniform(-1, 1, (T, O_)), G=(1.0 if r == B - 1 else 0.2) * g.standard_normal((T, O_))))
    out = {k: np.stack([p[k] for p in per_row]).astype(np.float32) for k in per_row[0]}
    out.update(w=w, Wp=Wp)
    return out


def mix_forward_reference(p, B, T, act, bf16=False):
    c_ = lambda a: f64(a[:B])
    return O.mix_decoder_train_forward(c_(p["dec0"]), c_(p["h1"]), c_(p["c1"]), c_(p["h2"]), c_(p["c2"]), c_(p["oth"]),
                                       {k: f64(v) for k, v in p["w"].items()}, f64(p["Wp"]), T, act=act, round_fwd=bf16)


def mix_backward_reference(p, B, tape, dloss, act, bf16=False):
    """BPTT on the given tapes (M, P, res1, res2, C1, C2 after each step) -> the eight outputs of mix_decoder_bwd."""
    t = {k: f64(v) for k, v in tape.items()}
    C1f = np.concatenate([f64(p["c1"][:B])[None], t["C1"]])
    C2f = np.concatenate([f64(p["c2"][:B])[None], t["C2"]])
    return O.mix_decoder_backward(t["M"], t["P"], f64(dloss), t["res1"], t["res2"], C1f, C2f, {k: f64(v) for k, v in p["w"].items()},
                                  f64(p["Wp"]), act=act, round_rec=bf16, round_dx=bf16)


def tf_head_inputs(name, B, H, M, O_, rows=None):
    rows = B if rows is None else rows
    rng = np.random.default_rng(seed_of(name))
    w = {}
    for n in ("mu", "var"):
        w[n + "_W1"] = (rng.standard_normal((H, M)) / np.sqrt(H)).astype(np.float32)
        w[n + "_b1"] = (0.1 * rng.standard_normal(M)).astype(np.float32)
        w[n + "_W2"] = (rng.standard_normal((M, O_)) / np.sqrt(M)).astype(np.float32)
        w[n + "_b2"] = (0.1 * rng.standard_normal(O_)).astype(np.float32)
    hs, dm, dv = [], [], []
    for r in range(rows):
        g = np.random.default_rng([seed_of(name), r + 1])
        s = 1.0 if r == B - 1 else 0.2
        hs.append(g.uniform(-1, 1, H)), dm.append(s * g.standard_normal(O_)), dv.append(s * g.standard_normal(O_))
    return w, np.stack(hs).astype(np.float32), np.stack(dm).astype(np.float32), np.stack(dv).astype(np.float32)


TF_NAMES = ("mu_W1", "mu_b1", "mu_W2", "mu_b2", "var_W1", "var_b1", "var_W2", "var_b2")


def tf_head_backward_reference(h, w, a1, mu, a3, var, dmu, dvar):
    """The eight gradients and dh from d loss / d mu, d loss / d var on the given tape (the relu masks are the tape's)."""
    h, a1, mu, a3, var, dmu, dvar = (f64(a) for a in (h, a1, mu, a3, var, dmu, dvar))
    w = {k: f64(v) for k, v in w.items()}
    out, dh = {}, 0.0
    for n, a, dpre in (("mu", a1, dmu * (1 - mu * mu)), ("var", a3, dvar * var)):
        da = (dpre @ w[n + "_W2"].T) * (a > 0)
        out.update({n + "_W2": a.T @ dpre, n + "_b2": dpre.sum(0), n + "_W1": h.T @ da, n + "_b1": da.sum(0)})
        dh = dh + da @ w[n + "_W1"].T
    out["dh"] = dh
    return out


def mlp_head_inputs(kind, B, H, n_mix, with_masks, rows=None):
    """-> (head weights keyed like the oracle's, layers [(W, b, activation)], h, masks or None, dlast)."""
    rows = B if rows is None else rows
    name = "mlp %s B%d H%d" % (kind, B, H)
    rng = np.random.default_rng(seed_of(name))
    dims = [H, 64, 128, 256, 10 * n_mix] if kind == "gmm" else [H, 128, 256, 90]
    head, layers = {}, []
    for l in range(len(dims) - 1):
        W = (rng.standard_normal((dims[l], dims[l + 1])) / np.sqrt(dims[l])).astype(np.float32)
        b = (0.1 * rng.standard_normal(dims[l + 1])).astype(np.float32)
        if kind == "gmm":
            head["fc%d_W" % (l + 1)], head["fc%d_b" % (l + 1)] = W, b
            layers.append((W, b, "relu" if l < 3 else None))
        else:
            taps = np.zeros((5,) + W.shape, np.float32)
            taps[2] = W
            head["conv%d_W" % (l + 1)], head["conv%d_b" % (l + 1)] = taps, b
            layers.append((W, b, "relu" if l < 2 else "tanh"))
    hs, dl, m1, m2 = [], [], [], []
    for r in range(rows):
        g = np.random.default_rng([seed_of(name), r + 1])
        hs.append(g.uniform(-1, 1, H)), dl.append((1.0 if r == B - 1 else 0.2) * g.standard_normal(dims[-1]))
        m1.append((g.random(dims[1]) < 0.8) / 0.8), m2.append((g.random(dims[2]) < 0.8) / 0.8)
    masks = [np.stack(m1).astype(np.float32), np.stack(m2).astype(np.float32)] if with_masks else None
    return head, layers, np.stack(hs).astype(np.float32), masks, np.stack(dl).astype(np.float32)


def mlp_head_forward_reference(kind, h, head, masks, n_mix):
    """The last layer's output from the oracle's heads (tf_gmm3d_head / tf_raw_head) -> (out, hidden activations or None)."""
    head = {k: f64(v) for k, v in head.items()}
    if kind == "gmm":
        (pi, us, sg, rh), hidden = O.tf_gmm3d_head(f64(h), head, masks=None if masks is None else [f64(m) for m in masks], n_mix=n_mix)
        return np.concatenate([pi, us, sg, rh], 1), hidden
    return O.tf_raw_head(f64(h), head)[0][:, 0], None


def mlp_head_backward_reference(x, layers, acts, masks, dlast):
    """gW, gb of every layer and dx from dlast = d loss / d pre-activation of the last layer, on the given activations (every
    hidden layer is a relu, behind which the mask multiplies)."""
    d, gW, gb = f64(dlast), [None] * len(layers), [None] * len(layers)
    for l in reversed(range(len(layers))):
        a_prev = f64(x) if l == 0 else f64(acts[l - 1])
        gW[l], gb[l] = a_prev.T @ d, d.sum(0)
        d = d @ f64(layers[l][0]).T
        if l > 0:
            m = 1.0 if masks is None or l - 1 >= len(masks) or masks[l - 1] is None else f64(masks[l - 1])
            d = d * m * (f64(acts[l - 1]) > 0)
    return gW, gb, d


def dense_mse_reference(hs, W, b, target, activation, weight):
    hs, W, b, target = f64(hs), f64(W), f64(b), f64(target)
    y = hs @ W + b
    y = np.tanh(y) if activation == "tanh" else y
    dpre = weight * 2 * (y - target) / y.size * ((1 - y * y) if activation == "tanh" else 1.0)
    return {"y": y, "loss": np.array([weight * np.mean((y - target) ** 2)]), "dX": dpre @ W.T, "dW": hs.T @ dpre, "db": dpre.sum(0)}


# the heads' bounds as tests/test_gpu_lstm_py_heads.py states them inline: outputs 1e-3 |ref| + 2e-5, gradients 2e-4 of the tensor's
# max |ref| + 1e-6
HEAD_OUT_RTOL, HEAD_OUT_ATOL, HEAD_GRAD, HEAD_GRAD_FLOOR = 1e-3, 2e-5, 2e-4, 1e-6
MIX_HEAD_WGRAD_CASES = [(17, 3, 256, 6, 198), (1, 1, 256, 6, 6), (30, 2, 64, 3, 12)]         # (B, T, H, O, width of the others' row)


def head_grad_bounds(got, ref):
    """Worst error in units of the heads' gradient bound (<= 1 passes)."""
    got, ref = f64(got), f64(ref)
    return float(np.abs(got - ref).max() / (HEAD_GRAD * np.abs(ref).max() + HEAD_GRAD_FLOOR))


def mlp_hidden_activations(h, layers, masks):
    """The hidden layers' outputs (relu, then the mask) of either fused head, fp64."""
    a, out = f64(h), []
    for l, (W, b, _) in enumerate(layers[:-1]):
        a = np.maximum(a @ f64(W) + f64(b), 0)
        if masks is not None and l < len(masks) and masks[l] is not None:
            a = a * f64(masks[l])
        out.append(a)
    return out


def dense_mse_inputs(N, H, O_):
    name = "dense-mse-%d" % N
    p = dense_inputs(name, N, H, O_)
    target = np.random.default_rng(seed_of(name + " target")).uniform(-1, 1, (N, O_)).astype(np.float32)
    target[N - 1] += 3.0          # the last live row carries a large share of the gradient
    return p, target


def mix_head_wgrad_inputs(B, T, H, O_, n_oth):
    rng = np.random.default_rng(seed_of("mix-head-wgrad B%d T%d" % (B, T)))
    q = dict(h2=rng.uniform(-1, 1, (T, B, H)), p=rng.uniform(-1, 1, (T, B, O_)), oth=rng.uniform(-1, 1, (B, T, n_oth)),
             dp=0.2 * rng.standard_normal((T, B, O_)), dm=0.2 * rng.standard_normal((T, B, O_)))
    q["dp"][:, B - 1] *= 5.0
    q["dm"][:, B - 1] *= 5.0
    return {k: v.astype(np.float32) for k, v in q.items()}


def mix_head_wgrad_reference(q):
    """[dense_W ; dense_b ; mix_W (others' rows, then the prediction's) ; mix_b] over the T * B rows, fp64."""
    T, B, H = q["h2"].shape
    n, O_ = T * B, q["p"].shape[-1]
    one = np.ones((n, 1))
    a1 = np.concatenate([f64(q["h2"]).reshape(n, H), one], 1)
    a2 = np.concatenate([f64(q["oth"]).transpose(1, 0, 2).reshape(n, -1), f64(q["p"]).reshape(n, O_), one], 1)
    return np.concatenate([a1.T @ f64(q["dp"]).reshape(n, O_), a2.T @ f64(q["dm"]).reshape(n, O_)], 0)


def mix_head_wgrad_rows(H, n_oth, O_):
    ncol = H + 1 + n_oth + O_ + 1
    return {"dense_W": slice(0, H), "dense_b": slice(H, H + 1), "mix_W": slice(H + 1, ncol - 1), "mix_b": slice(ncol - 1, ncol)}


def layer_cases():
    """(id, form row, B, F, T) for every layer-forward case."""
    return [("%s-B%d" % (f[0], B), f, B, f[6][i][0], f[6][i][1]) for f in LAYER_FORMS for i, B in enumerate(BATCHES)]


def backward_cases():
    return [("%s-B%d" % (f[0], B), f, B, f[5][i][0], f[5][i][1]) for f in BACKWARD_FORMS for i, B in enumerate(BATCHES)]


def layer_inputs(name, B, T, F, H, rows=None):
    """Inputs of a layer case, every one a function of (name, row): `rows` (default B) may exceed B - the extra rows are the
    unrelated sequences the row-independence run fills the last tile with, the first B stay the same bits.  The upstream
    gradients are 0.2 N(0, 1); those of the last live row B - 1 are of order 1."""
    rows = B if rows is None else rows
    rng = np.random.default_rng(seed_of(name))
    K, R, b = O.init_lstm(rng, F, H, np.float32)
    b = (b + 0.1 * rng.standard_normal(b.shape)).astype(np.float32)
    per_row = []
    for r in range(rows):
        g = np.random.default_rng([seed_of(name), r + 1])
        s = 1.0 if r == B - 1 else 0.2
        per_row.append(dict(x=g.uniform(-1, 1, (T, F)), h0=0.3 * g.standard_normal(H), c0=0.3 * g.standard_normal(H),
                            dhs=s * g.standard_normal((T, H)), dhT=s * g.standard_normal(H), dcT=s * g.standard_normal(H)))
    out = {k: np.stack([p[k] for p in per_row]).astype(np.float32) for k in per_row[0]}
    out.update(K=K, R=R, b=b)
    return out


def f64(a):
    return None if a is None else np.asarray(a, np.float64)


def layer_reference(inp, act, state, bf16=False):
    """fp64 forward of a layer case (bf16: both products of every step on bf16-rounded operands) -> hs, hT, cT, reserve."""
    return O.lstm_layer_train(f64(inp["x"]), f64(inp["K"]), f64(inp["R"]), f64(inp["b"]), f64(inp["h0"]) if state else None,
                              f64(inp["c0"]) if state else None, act=act, round_fwd=bf16)


def backward_reference(inp, hs, res, variant, act, bf16=False):
    """fp64 BPTT on the given tape for one of BACKWARD_VARIANTS (without the accumulate base)."""
    st, ups = variant["state"], variant["ups"]
    return O.lstm_layer_backward(f64(inp["x"]), f64(inp["K"]), f64(inp["R"]), f64(inp["h0"]) if st else None, f64(inp["c0"]) if st else None,
                                 f64(hs), f64(res), f64(inp["dhs"]) if "s" in ups else None, f64(inp["dhT"]) if "h" in ups else None,
                                 f64(inp["dcT"]) if "c" in ups else None, act=act, round_rec=bf16, round_dx=bf16, round_wgrad=bf16)


def act_of(name):
    """Both recurrent activations over the table, a function of the case name."""
    return "hard_sigmoid" if seed_of(name) % 2 else "sigmoid"


def accumulate_base(name, shape):
    return (0.05 * np.random.default_rng(seed_of(name + " base")).standard_normal(shape)).astype(np.float32)


def dense_inputs(name, N, In, Out, rows=None):
    rows = N if rows is None else rows
    rng = np.random.default_rng(seed_of(name))
    W = (rng.standard_normal((In, Out)) / np.sqrt(In)).astype(np.float32)
    b = (0.1 * rng.standard_normal(Out)).astype(np.float32)
    xs, ds = [], []
    for r in range(rows):
        g = np.random.default_rng([seed_of(name), r + 1])
        xs.append(g.uniform(-1, 1, In))
        ds.append((1.0 if r == N - 1 else 0.2) * g.standard_normal(Out))
    return dict(W=W, b=b, x=np.stack(xs).astype(np.float32), dpre=np.stack(ds).astype(np.float32))


def dense_backward_reference(x, W, dpre):
    x, W, dpre = f64(x), f64(W), f64(dpre)
    return {"dW": x.T @ dpre, "db": dpre.sum(0), "dx": dpre @ W.T}


# ---------------------------------------------------------------------------------------------------------------------
# the bound of the gradient checks, and how far a value is from it
# ---------------------------------------------------------------------------------------------------------------------
def check_grads(got, ref, tag):
    """check_grads of tests/test_gpu_train.py (|err| <= 1e-3 |ref| + 2e-4 max|ref| per element, 1e-4 max|ref| + 1e-9 on the
    worst) over the keys of `ref` instead of a model's weight names.  got: tensors."""
    keys, TR._W_ORDER = TR._W_ORDER, tuple(ref)
    try:
        TR.check_grads(got, ref, tag)
    finally:
        TR._W_ORDER = keys


def grad_bounds(got, ref):
    """Worst error of `got` in units of check_grads' bound on the worst element (<= 1 passes).  For printing and for the
    margin of the wrong-on-purpose references; the assertion itself is check_grads."""
    got, ref = f64(got), f64(ref)
    return float(np.abs(got - ref).max() / (1e-4 * np.abs(ref).max() + 1e-9))


def pad_with_last_row(a, B):
    """Rows B .. the end of the 16-row tile as copies of row B - 1: what a clamped row index reads."""
    a = np.asarray(a)
    return np.concatenate([a, np.repeat(a[B - 1:B], round_up(B) - B, axis=0)], axis=0)


# ---------------------------------------------------------------------------------------------------------------------
# the harness catches what it is for
# ---------------------------------------------------------------------------------------------------------------------
def _fake_kernel(out, x, rows, mistake=None):
    """out (rows, n) = 2 x; the mistakes of a kernel at a ragged tile edge, through the storage underneath the views."""
    flat_out, o0 = out._base if out._base is not None else out, out.storage_offset()
    n = out.shape[1]
    src = x
    if mistake == "read one row past":
        flat_x = x._base
        src = flat_x[x.storage_offset() + n:x.storage_offset() + n + rows * n].view(rows, n)
    out.copy_(2 * src)
    if mistake == "write before":
        flat_out[o0 - 1] = 1.0
    if mistake == "write behind":
        flat_out[o0 + rows * n] = 1.0
    if mistake == "leave one":
        out[rows - 1, n - 1] = float("nan")


@pytest.mark.parametrize("mistake,caught", [(None, None), ("write before", "in front of"), ("write behind", "behind"),
                                            ("leave one", "NaN"), ("read one row past", "NaN")])
@pytest.mark.parametrize("off", [0, 1])
def test_the_harness_catches_each_mistake(mistake, caught, off):
    rows, n = 17, 24
    x = np.random.default_rng(1).standard_normal((rows, n)).astype(np.float32)
    xv, out = guarded(x, off), OutView((rows, n), off=off)
    _fake_kernel(out.v, xv, rows, mistake)
    if caught is None:
        assert same_bits(out.result(), 2 * x)
    else:
        with pytest.raises(AssertionError, match=caught):
            out.result()


def test_outview_int32_and_accumulate():
    out = OutView((5, 3), dtype=torch.int32)
    with pytest.raises(AssertionError, match="not written"):
        out.result()
    out.v.copy_(torch.arange(15, dtype=torch.int32).view(5, 3))
    assert (out.result().reshape(-1) == np.arange(15)).all()
    out.buf[out.hi] = 7
    with pytest.raises(AssertionError, match="behind"):
        out.result()
    base = np.arange(12, dtype=np.float32).reshape(3, 4)
    acc = OutView((3, 4), base=base)
    assert acc.untouched()
    acc.v.add_(1.0)
    assert not acc.untouched() and same_bits(acc.result(), base + 1)
    acc.reset()
    assert acc.untouched()


def test_margins_cover_a_padded_tile():
    """16 rows of the operand and 1024 floats at least on both sides; the view is where it says."""
    for shape in [(1, 3, 6), (17, 3, 5, 512), (30, 256), (4096,), (1, 1)]:
        m = margin_floats(shape)
        assert m >= 1024 and m >= 16 * int(np.prod(shape[1:])) and m % 4 == 0
        for off in (0, 1):
            v = guarded(np.zeros(shape, np.float32), off)
            base = v._base
            assert v.storage_offset() >= m and base.numel() - v.storage_offset() - v.numel() >= m
            assert bool(torch.isnan(base[:v.storage_offset()]).all()) and bool(torch.isnan(base[v.storage_offset() + v.numel():]).all())
            o = OutView(shape, off=off)
            assert o.lo >= m and o.buf.numel() - o.hi >= m


# ---------------------------------------------------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------------------------------------------------
def test_backward_forms_are_those_of_the_value_regime_table():
    import test_gpu_value_regimes as VR
    assert [(f[0], f[3], f[4], f[2]) for f in BACKWARD_FORMS] == [tuple(r) for r in VR.BACKWARD_FORMS]


def test_every_value_of_B_T_F_appears_for_every_family():
    for table, family in ((layer_cases(), lambda f: f[1]), (backward_cases(), lambda f: f[1])):
        seen = {}
        for _, f, B, F, T in table:
            s = seen.setdefault(family(f), dict(B=set(), T=set()))
            s["B"].add(B), s["T"].add(T)
        for fam, s in seen.items():
            assert s["B"] == set(BATCHES) and s["T"] == {1, 2, 3}, (fam, s)
    assert {F for _, _, _, F, _ in layer_cases()} >= {6, 90, 96, 256} and {F for _, _, _, F, _ in backward_cases()} >= {6, 90, 96, 256}


@pytest.mark.parametrize("cid,form,B,F,T", layer_cases(), ids=[c[0] for c in layer_cases()])
def test_layer_case_reference_is_finite_and_ragged(cid, form, B, F, T):
    assert B == 16 or B % TILE != 0
    inp = layer_inputs(cid, B, T, F, form[4])
    for state in (False, True):
        for a in layer_reference(inp, act_of(cid), state, form[2] == "bf16"):
            assert np.isfinite(a).all()
    more = layer_inputs(cid, B, T, F, form[4], rows=round_up(B))
    assert all(same_bits(more[k][:B], inp[k]) for k in ("x", "h0", "c0", "dhs", "dhT", "dcT")) and same_bits(more["K"], inp["K"])


@pytest.mark.parametrize("cid,form,B,F,T", backward_cases(), ids=[c[0] for c in backward_cases()])
def test_backward_case_reference_is_finite_and_unmasked_padding_misses_the_bound(cid, form, B, F, T):
    """The fp64 gradients of every variant are finite; and db, dK, dR summed over the padded tile too (rows B .. as copies of
    row B - 1) miss check_grads by MARGIN."""
    assert B == 16 or B % TILE != 0
    H, bf, act = form[3], form[2] == "bf16", act_of(cid)
    inp = layer_inputs(cid, B, T, F, H)
    assert 0.5 < np.abs(inp["dhs"][B - 1]).mean() < 2.0
    for v in BACKWARD_VARIANTS:
        hs, _, _, res = layer_reference(inp, act, v["state"], bf)
        ref = backward_reference(inp, hs, res, v, act, bf)
        assert all(np.isfinite(a).all() for a in ref.values())
        if B % TILE == 0:
            continue
        padded = {k: (pad_with_last_row(a, B) if k not in ("K", "R", "b") else a) for k, a in inp.items()}
        wrong = backward_reference(padded, pad_with_last_row(hs, B), pad_with_last_row(res, B), v, act, bf)
        for k in ("db", "dK", "dR"):
            if k == "dR" and T == 1 and not v["state"]:
                continue            # one step from a zero state: dR is zero whatever the rows
            r = grad_bounds(wrong[k], ref[k])
            assert r >= MARGIN, (cid, v["name"], k, r)
            with pytest.raises(AssertionError):
                check_grads({k: torch.from_numpy(wrong[k])}, {k: ref[k]}, cid)
        np.testing.assert_allclose(wrong["dz"][:B], ref["dz"], rtol=1e-12, atol=1e-14)      # the live rows' data path is the same: only the sums differ


@pytest.mark.parametrize("name,kernel,N,In,Out,activation", DENSE_CASES)
def test_dense_case_reference_and_unmasked_padding(name, kernel, N, In, Out, activation):
    p = dense_inputs(name, N, In, Out)
    ref = dense_backward_reference(p["x"], p["W"], p["dpre"])
    assert all(np.isfinite(a).all() for a in ref.values()) and np.isfinite(O.dense(f64(p["x"]), f64(p["W"]), f64(p["b"]), activation)).all()
    if name == "dense-aligned":
        assert N % TILE == 0
        return
    assert N % TILE != 0
    wrong = dense_backward_reference(pad_with_last_row(p["x"], N), p["W"], pad_with_last_row(p["dpre"], N))
    for k in ("dW", "db"):
        assert grad_bounds(wrong[k], ref[k]) >= MARGIN, (name, k)
        with pytest.raises(AssertionError):
            check_grads({k: torch.from_numpy(wrong[k])}, {k: ref[k]}, name)


def test_wgrad_and_head_tables_are_ragged():
    for c in WGRAD_CASES:
        assert (c[4] * c[5]) % TILE != 0, c
    for c in WGRAD_PAIR_CASES:
        assert (c[6] * c[3]) % TILE != 0 and (c[6] * c[5]) % TILE != 0 and c[3] != c[5], c
    assert all(c[2] % TILE != 0 for c in DENSE_ADD_CASES) and sum(c[5] > c[4] for c in DENSE_ADD_CASES) >= 4
    assert sum(c[1] % TILE != 0 for c in MIX_HEAD_CASES) == 3


@pytest.mark.parametrize("cid,form,B,F_enc,T_in,T_out", decode_cases(), ids=[c[0] for c in decode_cases()])
def test_decode_case_reference_is_finite_and_ragged(cid, form, B, F_enc, T_in, T_out):
    assert B == 16 or B % TILE != 0
    p = decode_inputs(cid, B, T_in, T_out, F_enc, form[4])
    r = O.regime_decode(p["enc"], p["dec0"], p["w"], T_out, act_of(cid), form[2] == "bf16")
    assert all(np.isfinite(r[k]).all() for k in ("out", "hT", "cT"))


def test_decoder_and_teacher_forced_references_are_finite():
    for cid, form, B, T_out in decoder_cases():
        assert B == 16 or B % TILE != 0
        r = decoder_reference(decode_inputs(cid, B, 1, 1, 6, form[3]), B, T_out, act_of(cid))
        assert all(np.isfinite(a).all() for a in r.values())
    for name, _, _, H, B, F_enc, T_in, T_out in TF_CASES:
        assert B % TILE != 0
        p = decode_inputs(name, B, T_in, T_out, F_enc, H)
        assert np.isfinite(O.seq2seq_teacher_forced(f64(p["enc"]), f64(p["dec_in"]), {k: f64(v) for k, v in p["w"].items()}, act_of(name))).all()
    assert {T for *_, T in decoder_cases()} == {1, 2, 3}


def test_zx_and_stack2_references_are_finite():
    for cid, form, B, T in zx_cases():
        assert B == 16 or B % TILE != 0
        p = layer_inputs(cid, B, T, 90, form[3])
        assert all(np.isfinite(a).all() for a in zx_reference(f64(p["x"]) @ f64(p["K"]), p["R"], p["b"], p["h0"], p["c0"], act_of(cid)))
    for cid, form, B, F, T in stack2_cases():
        assert (B == 16 or B % TILE != 0) and T >= 2
        a, b = stack2_inputs(cid, B, T, F, form[3])
        for layer in stack2_reference(a, b, B, act_of(cid), form[2] == "f32", form[2] == "bf16"):
            assert all(np.isfinite(t).all() for t in layer)


@pytest.mark.parametrize("cid,form,B,T", mix_cases(), ids=[c[0] for c in mix_cases()])
def test_mix_decoder_case_reference_is_finite(cid, form, B, T):
    assert B == 16 or B % TILE != 0
    bf, act = form[1] == "bf16", act_of(cid)
    p = mix_inputs(cid, B, T)
    tape = mix_forward_reference(p, B, T, act, bf)
    assert all(np.isfinite(v).all() for v in tape.values())
    dloss = np.transpose(f64(p["G"]), (1, 0, 2)) * (1 - tape["M"] ** 2)
    assert all(np.isfinite(v).all() for v in mix_backward_reference(p, B, tape, dloss, act, bf).values())


def test_head_references_are_finite_and_padding_misses_the_bound():
    """Every weight and bias gradient of every layer of the TF, mixture and raw heads, of the Dense + MSE head and of the mixing
    head's weight-gradient kernel, summed over the padded tile too, against the bound its GPU test asserts."""
    pad_of = lambda B: (lambda a: pad_with_last_row(a, B))
    for (B, H, M, O_), _ in TF_HEAD_CASES:
        assert B % TILE != 0
        w, h, dmu, dvar = tf_head_inputs("tf head B%d" % B, B, H, M, O_)
        w64 = {k: f64(v) for k, v in w.items()}
        mu, var = O.tf_mean_var_head(f64(h), w64)
        a1, a3 = np.maximum(f64(h) @ w64["mu_W1"] + w64["mu_b1"], 0), np.maximum(f64(h) @ w64["var_W1"] + w64["var_b1"], 0)
        ref = tf_head_backward_reference(h, w, a1, mu, a3, var, dmu, dvar)
        assert all(np.isfinite(v).all() for v in ref.values())
        pad = pad_of(B)
        wrong = tf_head_backward_reference(pad(h), w, pad(a1), pad(mu), pad(a3), pad(var), pad(dmu), pad(dvar))
        for k in TF_NAMES:
            assert head_grad_bounds(wrong[k], ref[k]) >= MARGIN, (B, k, head_grad_bounds(wrong[k], ref[k]))
    for kind, B, H, n_mix, with_masks, _ in MLP_HEAD_CASES:
        assert B % TILE != 0
        head, layers, h, masks, dlast = mlp_head_inputs(kind, B, H, n_mix, with_masks)
        out, hidden = mlp_head_forward_reference(kind, h, head, masks, n_mix)
        acts = mlp_hidden_activations(h, layers, masks)
        assert np.isfinite(out).all() and (hidden is None or all(np.allclose(a, b) for a, b in zip(hidden, acts)))
        gW, gb, dx = mlp_head_backward_reference(h, layers, acts + [out], masks, dlast)
        pad = pad_of(B)
        wW, wb, _ = mlp_head_backward_reference(pad(h), layers, [pad(a) for a in acts] + [pad(out)], None if masks is None else [pad(m) for m in masks],
                                                pad(dlast))
        assert np.isfinite(dx).all()
        for l in range(len(layers)):
            assert head_grad_bounds(wW[l], gW[l]) >= MARGIN and head_grad_bounds(wb[l], gb[l]) >= MARGIN, (kind, B, l)
    for N, H, O_, activation in DENSE_MSE_CASES:
        assert N % TILE != 0
        p, target = dense_mse_inputs(N, H, O_)
        ref = dense_mse_reference(p["x"], p["W"], p["b"], target, activation, 0.5)
        assert all(np.isfinite(v).all() for v in ref.values())
        # the padded rows as copies of the last one, under the live rows' 1 / n
        extra = round_up(N) - N
        y = ref["y"][N - 1]
        dpre = 0.5 * 2 * (y - f64(target[N - 1])) / ref["y"].size * ((1 - y * y) if activation == "tanh" else 1.0)
        assert grad_bounds(ref["dW"] + extra * np.outer(f64(p["x"][N - 1]), dpre), ref["dW"]) >= MARGIN
        assert grad_bounds(ref["db"] + extra * dpre, ref["db"]) >= MARGIN
    for B, T, H, O_, n_oth in MIX_HEAD_WGRAD_CASES:
        assert (B * T) % TILE != 0
        q = mix_head_wgrad_inputs(B, T, H, O_, n_oth)
        ref = mix_head_wgrad_reference(q)
        padt = lambda a: np.concatenate([a, np.repeat(a[:, B - 1:B], round_up(B) - B, axis=1)], axis=1)      # time-major tapes
        wrong = mix_head_wgrad_reference(dict(h2=padt(q["h2"]), p=padt(q["p"]), dp=padt(q["dp"]), dm=padt(q["dm"]), oth=pad_of(B)(q["oth"])))
        assert np.isfinite(ref).all()
        for rows in mix_head_wgrad_rows(H, n_oth, O_).values():
            assert grad_bounds(wrong[rows], ref[rows]) >= MARGIN
