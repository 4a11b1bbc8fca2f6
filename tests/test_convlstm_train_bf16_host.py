"""bf16 training of the ConvLSTM head without a GPU: the `train_dtype` surface of ConvLSTMSeq2Seq, and the yardsticks
tests/test_gpu_conv_wgrad_bf16.py and tests/test_gpu_convlstm_train_bf16.py measure with, checked where it is cheap.

Operator level.  wgrad_bf16_ref restates the contract of fov_conv2d_wgrad_bf16 in NumPy (operands through O.round_bf16, sums
in the arrays' dtype).  For every operator case of the GPU file the restatement runs on fp64 and on fp32 arrays - the same
rounded operands under two accumulations; e_ref is their largest difference in units of 1e-5 * max|ref|, and 8 * e_ref <= 10
must hold.  The GPU bound is max(1, 8 * e_ref) of those units: measured from the reference's own fp32
error (sums over up to about 10^4 pixels), not from the kernel.

Trainer level.  BF16Conv is the conv analogue of oracle/bf16_autograd.py's BF16MatMul: a torch.autograd.Function around
conv2d whose forward, data and weight products each see bf16-rounded operands.  It is wired into a copy of
tests/test_gpu_convlstm.py::_torch_convlstm_graph's head; the graph's forward is pinned to
test_convlstm_bf16_host.head_bf16_forward.  The bounds are the ones tests/test_gpu_bf16_backward.py (TRAINER, against the
rounded-operand autograd) and tests/test_gpu_bf16.py (FULL_PRECISION, against the full-precision graph; LOSS_REL) hold bf16
trainers' gradients to, each relative to the tensor's scale.  Here the rounded-operand autograd on fp32 tensors must stay
within HALF of TRAINER of itself on fp64 tensors, and within HALF of FULL_PRECISION of the full-precision fp64 graph, for
every model case of the GPU file: the bounds leave the kernels at least as much room as the reference's own noise takes."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_convlstm_bf16_host as HB  # noqa: E402

TRAINER = 5e-3           # tests/test_gpu_bf16_backward.py: vs the rounded-operand autograd, of each tensor's scale
FULL_PRECISION = 3e-2    # tests/test_gpu_bf16.py: vs the full-precision fp64 graph, of each tensor's scale
LOSS_REL = 2e-3          # tests/test_gpu_bf16.py: loss vs the full-precision graph, relative
LOOSE = HB.LOOSE

# operator cases of the GPU file: (name, B, H, W, C, N, kh, kw, extra channels of the map x is a slice of)
OP_CASES = [("plain form, odd pixel count", 3, 9, 6, 10, 24, 5, 5, 0),
            ("channel padding 56 -> 64, partial N tile, W = 18", 2, 36, 18, 56, 72, 5, 5, 0),
            ("channel slice of a wider map, split slices", 4, 36, 18, 64, 128, 5, 5, 24),
            ("N = 30", 2, 36, 18, 128, 30, 5, 5, 0),
            ("Conv1D 1x5", 3, 1, 30, 48, 32, 1, 5, 0),
            ("k = 3", 2, 7, 10, 20, 36, 3, 3, 4),
            ("1x1 map, k = 1", 1, 1, 1, 12, 8, 1, 1, 0)]

# model cases of the GPU file: the shapes of test_convlstm_bf16_host.SMALL_CASES, one with dropout, one with
# categorical_crossentropy: (name, head, B, T_in, T_out, H, W, C, latent_dim, head_filters, weight seed, dropout_rate, loss, act).
# The weight seeds and the recurrent activation of the conv2d cases are CHOSEN so that the reference's own noise fits
# (test_gradient_yardstick): at 2 x 2 x 54 pixels a handful of relu masks of the head's hidden layers flip under bf16
# rounding, each flip moves a gradient term by its whole size, and with most seeds that alone puts the rounded-operand
# gradients 3e-2 .. 1.5e-1 of scale away from the full-precision ones (40 seeds tried per case: about one in fourteen fits).
_C2D, _C1D = HB.SMALL_CASES
TRAIN_CASES = [_C2D[:10] + (1, 0.0, "mse", "sigmoid"),
               _C1D + (0.0, "mse", "hard_sigmoid"),
               ("conv2d 9x6 dropout", "conv2d", 2, 2, 2, 9, 6, 10, 8, (24, 40), 9, 0.25, "mse", "sigmoid"),
               ("conv2d 9x6 crossentropy", "conv2d", 2, 2, 2, 9, 6, 10, 8, (24, 40), 11, 0.0, "categorical_crossentropy", "sigmoid")]


# ---------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------
def _weights():
    return O.init_convlstm_seq2seq(3, C=10, latent_dim=8, head="conv2d", head_filters=(24, 40))


def test_train_dtype_table_raises_before_any_device_work():
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    w = _weights()
    assert ConvLSTMSeq2Seq(w).train_dtype is None
    assert ConvLSTMSeq2Seq(w, train_dtype="f32").train_dtype == "f32"
    m = ConvLSTMSeq2Seq(w, dtype="bf16", train_dtype="bf16")
    assert (m.dtype, m.train_dtype) == ("bf16", "bf16")
    wc = O.init_convlstm_seq2seq(3, C=3, latent_dim=16, head="conv1d", head_filters=(32, 48))
    assert ConvLSTMSeq2Seq(wc, head="conv1d", dtype="bf16", train_dtype="bf16").train_dtype == "bf16"
    with pytest.raises(ValueError, match="dtype"):
        ConvLSTMSeq2Seq(w, dtype="f32", train_dtype="bf16")
    with pytest.raises(ValueError, match="dtype"):
        ConvLSTMSeq2Seq(w, train_dtype="bf16")
    with pytest.raises(ValueError, match="dtype"):
        ConvLSTMSeq2Seq(w, dtype="bf16", train_dtype="f32")
    for bad in ("fp16", "bfloat16", "float32", 16):
        with pytest.raises(ValueError, match="train_dtype"):
            ConvLSTMSeq2Seq(w, dtype="bf16", train_dtype=bad)
    wd = O.init_convlstm_seq2seq(3, C=6, latent_dim=8, head="dense", map_hw=(1, 1))
    with pytest.raises(ValueError, match="dense"):
        ConvLSTMSeq2Seq(wd, head="dense", train_dtype="bf16")
    with pytest.raises(ValueError, match="dense"):
        ConvLSTMSeq2Seq(wd, head="dense", dtype="bf16", train_dtype="bf16")


def test_default_and_bf16_alone_still_refuse_to_train_and_so_does_a_bf16_cell():
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    w = _weights()
    m = ConvLSTMSeq2Seq(w, dtype="bf16")
    m.compile(optimizer="RMSprop", loss="mean_squared_error")
    with pytest.raises(NotImplementedError, match=r"f32.*get_weights\(\)"):
        m._make_trainer("rmsprop")
    for td in (None, "bf16"):
        kw = dict(dtype="bf16", train_dtype="bf16") if td else {}
        mc = ConvLSTMSeq2Seq(w, cell_dtype="bf16", **kw)
        mc.compile(optimizer="RMSprop", loss="mean_squared_error")
        with pytest.raises(NotImplementedError, match="cell_dtype"):
            mc._make_trainer("rmsprop")


def test_trainer_head_dtype_is_validated_before_any_device_work():
    from longterm360fov_amd.training import ConvLSTMTrainer
    wd = O.init_convlstm_seq2seq(3, C=6, latent_dim=8, head="dense", map_hw=(1, 1))
    with pytest.raises(ValueError, match="dense"):
        ConvLSTMTrainer(wd, head="dense", head_dtype="bf16", device="cpu")
    with pytest.raises(ValueError, match="head_dtype"):
        ConvLSTMTrainer(_weights(), head_dtype="fp16", device="cpu")


# ---------------------------------------------------------------------------------------
# operator level: the reference and its own error
# ---------------------------------------------------------------------------------------
def wgrad_bf16_ref(x, dy, kh, kw):
    """dw[i][j][c][n] = sum over the pixels of bf16(x[p + tap(i,j)][c]) * bf16(dy[p][n]): x (B,H,W,C), dy (B,H,W,N), 'same'
    zero padding, sums in the arrays' dtype."""
    B, H, W, C = x.shape
    N = dy.shape[-1]
    ph, pw = (kh - 1) // 2, (kw - 1) // 2
    xp = np.zeros((B, H + kh - 1, W + kw - 1, C), x.dtype)
    xp[:, ph:ph + H, pw:pw + W] = O.round_bf16(x)
    d = O.round_bf16(dy).reshape(B * H * W, N)
    dw = np.empty((kh, kw, C, N), x.dtype)
    for i in range(kh):
        for j in range(kw):
            dw[i, j] = np.ascontiguousarray(xp[:, i:i + H, j:j + W]).reshape(B * H * W, C).T @ d
    return dw


def op_inputs(case):
    """(x (B,H,W,C) fp32, dy (B,H,W,N) fp32) of an operator case."""
    _, B, H, W, C, N, kh, kw, _ = case
    rng = np.random.default_rng(B * 1000 + C + N + kh)
    return rng.standard_normal((B, H, W, C)).astype(np.float32), rng.standard_normal((B, H, W, N)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def op_reference(idx):
    """-> (fp64 reference, e_ref in units of 1e-5 * max|ref|) of OP_CASES[idx], computed once."""
    case = OP_CASES[idx]
    x, dy = op_inputs(case)
    kh, kw = case[6], case[7]
    r64 = wgrad_bf16_ref(x.astype(np.float64), dy.astype(np.float64), kh, kw)
    r32 = wgrad_bf16_ref(x, dy, kh, kw)
    assert r64.dtype == np.float64 and r32.dtype == np.float32
    e_ref = float(np.abs(r32 - r64).max() / (1e-5 * np.abs(r64).max()))
    r64.setflags(write=False)
    return r64, e_ref


def op_bound_units(idx):
    return max(1.0, 8.0 * op_reference(idx)[1])


@pytest.mark.parametrize("idx", range(len(OP_CASES)), ids=[c[0] for c in OP_CASES])
def test_operator_yardstick(idx):
    ref, e_ref = op_reference(idx)
    print("%s: e_ref %.3f units of 1e-5 max|ref| (max|ref| %.3e), GPU bound %.2f units" % (OP_CASES[idx][0], e_ref, np.abs(ref).max(),
                                                                                          op_bound_units(idx)))
    assert 8 * e_ref <= 10


def test_reference_is_the_weight_gradient_of_the_forward_restatement():
    """wgrad_bf16_ref on operands that bf16 holds exactly = the autograd weight gradient of the fp64 convolution."""
    rng = np.random.default_rng(0)
    x = O.round_bf16(rng.standard_normal((2, 5, 4, 3))).astype(np.float64)
    dy = O.round_bf16(rng.standard_normal((2, 5, 4, 6))).astype(np.float64)
    w = torch.zeros(3, 5, 3, 6, dtype=torch.float64, requires_grad=True)
    (_tconv(torch.from_numpy(x), w) * torch.from_numpy(dy)).sum().backward()
    assert np.abs(wgrad_bf16_ref(x, dy, 3, 5) - w.grad.numpy()).max() <= 1e-12


# ---------------------------------------------------------------------------------------
# trainer level: the rounded-operand autograd
# ---------------------------------------------------------------------------------------
def _tconv(x, w):
    """conv2d_same on NHWC / (kh,kw,C,N) operands with torch."""
    import torch.nn.functional as TF
    kh, kw = w.shape[:2]
    return TF.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), padding=(kh // 2, kw // 2)).permute(0, 2, 3, 1)


def rb(t):
    """bf16 rounding of a tensor (through fp32, as the kernels round the fp32 values they hold), in the tensor's dtype."""
    return torch.from_numpy(O.round_bf16(t.detach().numpy()))


class BF16Conv(torch.autograd.Function):
    """y = conv2d_same(x, w); each of the three products - forward, data gradient, weight gradient - rounds both operands."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return _tconv(rb(x), rb(w))

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gr = rb(g)
        with torch.enable_grad():
            xr, wr = rb(x).requires_grad_(True), rb(w).requires_grad_(True)
            dx, = torch.autograd.grad(_tconv(xr, rb(w)), xr, gr)       # bf16(dy) * bf16(w^T)
            dw, = torch.autograd.grad(_tconv(rb(x), wr), wr, gr)       # bf16(x) * bf16(dy)
        return dx, dw


def train_graph(enc, dec0, tgt, w, head, act="hard_sigmoid", masks=None, xent=False, rounded=True, dtype=torch.float64):
    """tests/test_gpu_convlstm.py::_torch_convlstm_graph with the head's convolutions through BF16Conv (rounded) or plain
    (full precision), on tensors of `dtype` -> (loss, {gradients}, prediction (B,T_out,H,W,Co))."""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    t = {k: torch.tensor(v.astype(npdt), requires_grad=True) for k, v in w.items()}
    s = torch.sigmoid if act == "sigmoid" else (lambda z: torch.clamp(0.2 * z + 0.5, 0, 1))
    hconv = BF16Conv.apply if rounded else _tconv

    def cell(x, h, c, K, R, b, m4=None):
        F = R.shape[2]
        if m4 is None:
            zx = _tconv(x, K)
        else:
            zx = torch.cat([_tconv(x * m4[g], K[..., g * F:(g + 1) * F]) for g in range(4)], -1)
        z = zx + b + _tconv(h, R)
        i, f, g, o = s(z[..., :F]), s(z[..., F:2 * F]), torch.tanh(z[..., 2 * F:3 * F]), s(z[..., 3 * F:])
        c = f * c + i * g
        return o * torch.tanh(c), c

    e, d0, tg = (torch.tensor(a.astype(npdt)) for a in (enc, dec0, tgt))
    B, T_in, H, W, _ = e.shape
    seq = [e[:, tt] for tt in range(T_in)]
    states = []
    for l in range(3):
        F = w["enc%d_R" % l].shape[2]
        h = torch.zeros(B, H, W, F, dtype=dtype)
        c = torch.zeros(B, H, W, F, dtype=dtype)
        nxt = []
        m4 = None if masks is None else torch.tensor(masks["enc%d" % l].astype(npdt))
        for tt in range(T_in):
            h, c = cell(seq[tt], h, c, t["enc%d_K" % l], t["enc%d_R" % l], t["enc%d_b" % l], m4)
            nxt.append(h)
        seq = nxt
        states.append([h, c])
    inp = d0[:, 0]
    outs = []
    for tt in range(tg.shape[1]):
        cur, feats = inp, []
        for l in range(3):
            m4 = None if masks is None else torch.tensor(masks["dec%d" % l][tt].astype(npdt))
            h, c = cell(cur, states[l][0], states[l][1], t["dec%d_K" % l], t["dec%d_R" % l], t["dec%d_b" % l], m4)
            states[l] = [h, c]
            feats.append(h)
            cur = h
        y = torch.cat(feats, -1)
        y = torch.relu(hconv(y, t["head0_W"]) + t["head0_b"])
        y = torch.relu(hconv(y, t["head1_W"]) + t["head1_b"])
        y = hconv(y, t["head2_W"]) + t["head2_b"]
        y = torch.softmax(torch.relu(y) if head == "conv2d" else y, -1)
        outs.append(y)
        inp = y
    P = torch.stack(outs, 1)
    loss = torch.mean((P - tg) ** 2)
    if xent:          # Keras-2.2 categorical_crossentropy, TF backend (convlstm_heatmap.py:192)
        q = torch.clamp(P / P.sum(-1, keepdim=True), 1e-7, 1 - 1e-7)
        loss = torch.mean(-(tg * torch.log(q)).sum(-1))
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in t.items()}, P.detach().numpy()


def train_inputs(case):
    """(weights, enc, dec0, target, masks or None) of a model case; the inputs are test_convlstm_bf16_host.small_inputs."""
    _, head, B, T_in, T_out, H, W, C, L, hf, seed, rate, _, _ = case
    w = O.init_convlstm_seq2seq(seed, C=C, latent_dim=L, head=head, head_filters=hf)
    enc, dec0 = HB.small_inputs(head, B, T_in, H, W, C)
    rng = np.random.default_rng(11)
    if head == "conv2d":     # one-hot target maps: one active cell per frame channel
        tgt = np.zeros((B, T_out, H, W, C), np.float32)
        idx = rng.integers(0, H * W, (B, T_out, C))
        bi, ti, ci = np.meshgrid(np.arange(B), np.arange(T_out), np.arange(C), indexing="ij")
        tgt[bi, ti, idx // W, idx % W, ci] = 1
    else:
        tgt = O.synthetic_xyz(rng, B, T_out, 30).reshape(B, T_out, 1, 30, 3).astype(np.float32)
    masks = None
    if rate > 0:             # the shapes of ConvLSTMTrainer.sample_masks
        F = [w["enc%d_R" % l].shape[2] for l in range(3)]
        cin = [C] + F[:2]
        keep = 1.0 - rate
        masks = {}
        for l in range(3):
            masks["enc%d" % l] = ((rng.random((4, B, H, W, cin[l])) < keep) / keep).astype(np.float32)
            masks["dec%d" % l] = ((rng.random((T_out, 4, B, H, W, cin[l])) < keep) / keep).astype(np.float32)
    return w, enc, dec0, tgt, masks


@functools.lru_cache(maxsize=None)
def train_references(idx):
    """-> ((loss, grads, P) of the rounded-operand autograd in fp64, the same of the full-precision fp64 graph), once per case."""
    case = TRAIN_CASES[idx]
    w, enc, dec0, tgt, masks = train_inputs(case)
    kw = dict(head=case[1], act=case[13], masks=masks, xent=case[12] == "categorical_crossentropy")
    return train_graph(enc, dec0, tgt, w, rounded=True, **kw), train_graph(enc, dec0, tgt, w, rounded=False, **kw)


def of_scale(got, ref):
    """max |got - ref| / max |ref|"""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (np.abs(ref).max() + 1e-30))


@pytest.mark.parametrize("idx", [0, 1], ids=[c[0] for c in TRAIN_CASES[:2]])
def test_graph_forward_is_the_bf16_head_restatement(idx):
    case = TRAIN_CASES[idx]
    w, enc, dec0, _, _ = train_inputs(case)
    P = train_references(idx)[0][2]
    ref = HB.head_bf16_forward(enc.astype(np.float64), dec0.astype(np.float64), HB.f64(w), case[4], case[1], case[13])
    assert np.abs(P - ref).max() <= 1e-10


@pytest.mark.parametrize("idx", range(len(TRAIN_CASES)), ids=[c[0] for c in TRAIN_CASES])
def test_gradient_yardstick(idx):
    case = TRAIN_CASES[idx]
    w, enc, dec0, tgt, masks = train_inputs(case)
    (l64, g64, _), (lf, gf, _) = train_references(idx)
    l32, g32, _ = train_graph(enc, dec0, tgt, w, head=case[1], act=case[13], masks=masks,
                              xent=case[12] == "categorical_crossentropy", rounded=True, dtype=torch.float32)
    worst_t = max((of_scale(g32[k], g64[k]), k) for k in g64)
    worst_f = max((of_scale(g64[k], gf[k]), k) for k in g64)
    print("%s: fp32 vs fp64 tensors %.2e of scale (%s) = %.2f of TRAINER; rounded vs full precision %.2e (%s) = %.2f of "
          "FULL_PRECISION; loss %.6e / %.6e / %.6e" % (case[0], worst_t[0], worst_t[1], worst_t[0] / TRAINER, worst_f[0], worst_f[1],
                                                      worst_f[0] / FULL_PRECISION, l32, l64, lf))
    assert worst_t[0] <= 0.5 * TRAINER
    assert worst_f[0] <= 0.5 * FULL_PRECISION
    assert abs(l32 - l64) <= 0.5 * LOSS_REL * abs(l64) and abs(l64 - lf) <= 0.5 * LOSS_REL * abs(lf)
    assert all(np.abs(g64[k]).max() > 0 for k in g64)
