"""fused_encoder_bwd of OthersMixingTrainer (tile_decoder) and OthersContextTrainer: at width 32 / 64 the two encoder layers' BPTT
is ONE ops.lstm_stack2_bwd call (fov_lstm_stack2_bwd's one-workgroup-per-tile form) instead of two ops.lstm_seq_bwd calls.

The tiny cases of tests/test_gpu_mix_tile.py (model_case) and tests/test_gpu_selffed2_fused.py (_model_case): B 17, T_in 3, T_out 4,
with their fp64 torch.autograd references.  Bounds, those files': loss 1e-5 relative + 1e-9; prediction 2e-5 (and 1e-3 |ref| + 1e-5
per element for the others-context models); every gradient 1e-4 max|ref| + 1e-9; four Adam steps with the attribute on and off:
loss 1e-6 relative + 1e-9, every gradient 2e-5 max|ref| + 1e-9 (test_gpu_mix_tile.py's fused against step-wise)."""
import numpy as np
import pytest
import torch

import test_gpu_mix_tile as MT
import test_gpu_selffed2_fused as SF

pytestmark = pytest.mark.gpu

T_IN = 3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _spy(monkeypatch):
    """Counts ops.lstm_stack2_bwd calls and the ops.lstm_seq_bwd calls over the encoder's T_IN steps (by the shape of their input;
    the decoder's walk, where it remains, calls ops.lstm_seq_bwd with one step and the context's Bi-LSTMs with T_out = 4)."""
    from longterm360fov_amd import ops
    seen = {"stack2": 0, "enc_seq_bwd": 0, "other_seq_bwd": 0}
    stack2, seq = ops.lstm_stack2_bwd, ops.lstm_seq_bwd

    def stack2_spy(x, *a, **k):
        seen["stack2"] += 1
        assert x.shape[1] == T_IN
        return stack2(x, *a, **k)

    def seq_spy(x, *a, **k):
        seen["enc_seq_bwd" if x.shape[1] == T_IN else "other_seq_bwd"] += 1
        return seq(x, *a, **k)
    monkeypatch.setattr(ops, "lstm_stack2_bwd", stack2_spy)
    monkeypatch.setattr(ops, "lstm_seq_bwd", seq_spy)
    return seen


def _agree_over_four_steps(on, off, args, keys, loss0):
    for step in range(4):
        l1, l2 = float(on.train_step(*args).item()), float(off.train_step(*args).item())
        assert abs(l1 - l2) <= 1e-6 * abs(l2) + 1e-9, (step, l1, l2)
        for k in keys:
            d = (on.g[k] - off.g[k]).abs().max().item()
            assert d <= 2e-5 * off.g[k].abs().max().item() + 1e-9, (step, k, d)
    assert l1 < loss0


@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("act", ["sigmoid", "hard_sigmoid"])
def test_mixing_trainer_on_the_tile_path(monkeypatch, H, act):
    from longterm360fov_amd.training import OthersMixingTrainer, _MIX_ORDER
    mc = MT.model_case(H, act)
    args = [dev(mc[k]) for k in ("enc", "oth", "dec0", "tgt")]
    on = OthersMixingTrainer(mc["w"], act=act, tile_decoder=True)
    on.fused_encoder_bwd = True
    with monkeypatch.context() as mp:
        seen = _spy(mp)
        loss, y = on.forward_backward(*args)
        torch.cuda.synchronize()
        on.ws.check(); on.bwd_scratch.check()
        # H = 64 walks the decoder backward: 2 one-step calls per decoder step, none over the encoder
        assert seen == {"stack2": 1, "enc_seq_bwd": 0, "other_seq_bwd": 0 if H == 32 else 8}, seen
    loss0 = float(loss.item())
    assert abs(loss0 - mc["loss"]) <= 1e-5 * mc["loss"] + 1e-9
    np.testing.assert_allclose(y.cpu().numpy(), mc["y"], atol=2e-5)
    for k in _MIX_ORDER:
        MT.near("fused encoder BPTT, mixing H%d %s grad %s" % (H, act, k), on.g[k], mc["grads"][k], 1e-4)
    off = OthersMixingTrainer(mc["w"], act=act, tile_decoder=True)
    off.fused_encoder_bwd = False
    with monkeypatch.context() as mp:
        seen = _spy(mp)
        off.forward_backward(*args)
        assert seen["stack2"] == 0 and seen["enc_seq_bwd"] == 2, seen       # the parent's two calls
    _agree_over_four_steps(on, off, args, _MIX_ORDER, loss0)


def test_mixing_trainer_off_the_tile_path_keeps_its_two_calls(monkeypatch):
    """Without tile_decoder the attribute changes nothing: the step-wise trainer at width 32 makes the two encoder calls."""
    from longterm360fov_amd.training import OthersMixingTrainer
    mc = MT.model_case(32, "sigmoid")
    tr = OthersMixingTrainer(mc["w"], act="sigmoid")
    tr.fused_encoder_bwd = True
    seen = _spy(monkeypatch)
    tr.forward_backward(*[dev(mc[k]) for k in ("enc", "oth", "dec0", "tgt")])
    assert seen["stack2"] == 0 and seen["enc_seq_bwd"] == 2, seen


@pytest.mark.parametrize("mode,act", [("target_user_only", "sigmoid"), ("others_mlp", "hard_sigmoid"), ("others_lstm", "sigmoid")])
def test_others_context_trainer(monkeypatch, mode, act):
    from longterm360fov_amd.training import OthersContextTrainer
    H = 32
    mc = SF._model_case(mode, H, act)
    args = [dev(mc[k]) for k in ("enc", "oth", "dec0", "tgt")]
    on = OthersContextTrainer(mc["w"], mode, act=act)
    on.fused_encoder_bwd = True
    with monkeypatch.context() as mp:
        seen = _spy(mp)
        loss, y = on.forward_backward(*args)
        torch.cuda.synchronize()
        on.ws.check(); on.bwd_scratch.check()
        # others_lstm: the context's four directional layers (T_out steps each) keep their calls
        assert seen == {"stack2": 1, "enc_seq_bwd": 0, "other_seq_bwd": 4 if mode == "others_lstm" else 0}, seen
    loss0 = float(loss.item())
    assert abs(loss0 - mc["loss"]) <= 1e-5 * mc["loss"] + 1e-9
    SF._held("fused encoder BPTT, %s prediction" % mode, y.cpu().numpy(), mc["y"])
    for k in mc["order"]:
        SF._grad_held("fused encoder BPTT, %s grad %s" % (mode, k), on.g[k].detach().cpu().numpy(), mc["grads"][k])
    off = OthersContextTrainer(mc["w"], mode, act=act)
    off.fused_encoder_bwd = False
    with monkeypatch.context() as mp:
        seen = _spy(mp)
        off.forward_backward(*args)
        assert seen["stack2"] == 0 and seen["enc_seq_bwd"] == 2, seen
    _agree_over_four_steps(on, off, args, mc["order"], loss0)


def test_tf_lstm_trainer_padded_to_64_keeps_its_per_layer_calls(monkeypatch):
    """A two-layer lstm.py model of width 40 runs padded to 64 (the first case of test_gpu_train.py's
    test_tf_stacked_lstm_training_graph): the library would take that width now, the trainer's two-layer launch stays at 512."""
    from longterm360fov_amd import ops
    from longterm360fov_amd.training import TFLSTMTrainer
    H, B, T, F, fps = 40, 9, 4, 90, 30
    rng = np.random.default_rng(H + B)
    cells = []
    for l in range(2):
        Fin = F if l == 0 else H
        cells.append(((rng.standard_normal((Fin + H, 4 * H)) / np.sqrt(Fin + H)).astype(np.float32),
                      (0.1 * rng.standard_normal(4 * H)).astype(np.float32)))
    head = {}
    for br in ("mu", "var"):
        head[br + "_W1"] = (rng.standard_normal((H, 32)) / np.sqrt(H)).astype(np.float32)
        head[br + "_b1"] = (0.1 * rng.standard_normal(32)).astype(np.float32)
        head[br + "_W2"] = (rng.standard_normal((32, 3)) / np.sqrt(32)).astype(np.float32)
        head[br + "_b2"] = (0.1 * rng.standard_normal(3)).astype(np.float32)
    x = rng.uniform(-1, 1, (B, T, F)).astype(np.float32)
    y = rng.uniform(-1, 1, (B, 1, 3 * fps)).astype(np.float32)
    init = (0.2 * rng.standard_normal((2, 2, B, H))).astype(np.float32)
    tr = TFLSTMTrainer(cells, head, lr=1e-3, clip_value=1.0, fps=fps, running_length=10)
    assert tr.Hp == 64 and ops.lstm_stack2_bwd_supported(B, T, F, tr.Hp)
    seen = _spy(monkeypatch)
    tr.forward_backward(dev(x), dev(y), dev(init))
    torch.cuda.synchronize()
    assert seen["stack2"] == 0 and seen["enc_seq_bwd"] + seen["other_seq_bwd"] == 2, seen
