"""torch.autograd restatement of the bf16-operand graphs, fp64 on the CPU (test infrastructure only, like all of oracle/).

The independent check of the closed-form bf16 backward restatements in fov_oracle.py (lstm_layer_backward and
mix_decoder_backward with their rounding switches) and the reference of the bf16 trainers' gradients: autograd derives the
backward graph, and one custom Function decides which of a product's three matrix products see bf16-rounded operands
(round-to-nearest-even of the fp32 value, fov_oracle.round_bf16):
    forward   y  = a w
    data      da = g w^T
    weight    dw = a^T g
"""
import numpy as np
import torch

from oracle import fov_oracle as O


def rb(t):
    """bf16 rounding of an fp64 tensor (through fp32, as the kernels round the fp32 values they hold)."""
    return torch.from_numpy(O.round_bf16(t.detach().cpu().numpy()))


class BF16MatMul(torch.autograd.Function):
    """a (N,K) @ w (K,M); flags = (fwd, data, weight): which of the three products round both operands."""

    @staticmethod
    def forward(ctx, a, w, flags):
        ctx.save_for_backward(a, w)
        ctx.flags = flags
        return (rb(a) @ rb(w)) if flags[0] else a @ w

    @staticmethod
    def backward(ctx, g):
        a, w = ctx.saved_tensors
        _, data, weight = ctx.flags
        da = (rb(g) @ rb(w).T) if data else g @ w.T
        dw = (rb(a).T @ rb(g)) if weight else a.T @ g
        return da, dw, None


def mm(a, w, fwd=False, data=False, weight=False):
    return BF16MatMul.apply(a, w, (fwd, data, weight))


def rec_act(act):
    return torch.sigmoid if act == "sigmoid" else (lambda z: torch.clamp(0.2 * z + 0.5, 0, 1))


def lstm_step(x, h, c, K, R, b, act, fwd=False, rec=False, dx=False, wgrad=False, keep=None):
    """One Keras LSTMCell step; x K takes the data-gradient flag, h R the recurrence flag.  keep: list that collects the
    step's gate pre-activation z (grad retained) and its activated (i, f, g, o, c')."""
    H = R.shape[0]
    z = mm(x, K, fwd, dx, wgrad) + b + mm(h, R, fwd, rec, wgrad)
    s = rec_act(act)
    i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
    c = f * c + i * g
    if keep is not None:
        z.retain_grad()
        keep.append((z, torch.stack([i, f, g, o, c], 1)))
    return o * torch.tanh(c), c


def leaf(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
