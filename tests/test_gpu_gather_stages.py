"""Seams of the gather of h_t in the cluster LSTM kernel.  The kernel completes the whole gather in the
tail of a step; a form that consumes it one partner slice at a time across the step boundary was measured and is not
shipped, and these tests were written for it.  They stay because they sit on the places where any gather that outlives its
step can go wrong: phases with no partner-slice run at all, with first and last steps only, with exactly one and exactly
three steady-state steps; a group that walks a second tile; the training forward, which writes `reserve` / `hs` from the same
step; and the hidden sizes with a single partner (H = 128) or no exchange (H = 64).

Bounds and helpers are test_gpu_fused_straightline.py's: the fused call, its repeat, the two-launch form, the write-through
exchange and the call after it are the same arithmetic in the same order - bit-equal; against the fp64 oracle the suite's
2e-5.  The training case uses test_gpu_train.py's bounds.  No test provokes a give-up: those paths are checked by reading."""
import numpy as np
import pytest
import torch

from oracle import fov_oracle as O
from test_gpu_fused_straightline import dev, device_weights, inputs, run_all_forms
from test_gpu_train import batch, check_grads, f64

pytestmark = pytest.mark.gpu


# T_in: 1 = the only step is first and last (no gather is consumed); 2 = one gather, consumed by a last step; 3 = first +
# two last steps; 4 = one steady-state step; 6 = three.  T_out: 1, 2 = none; 3 = one; 5 = three steady-state steps.
# B 16 = one tile (a padded grid of eight groups), B 40 = a ragged third tile
@pytest.mark.parametrize("B,act", [(16, "sigmoid"), (16, "hard_sigmoid"), (40, "sigmoid")])
@pytest.mark.parametrize("T_out", [1, 2, 3, 5])
@pytest.mark.parametrize("T_in", [1, 2, 3, 4, 6])
def test_phase_lengths_around_the_gather(B, act, T_in, T_out):
    run_all_forms(B, T_in, T_out, 256, act)


def test_second_tile_of_a_group_starts_clean():
    """B 1040 = 65 tiles on 64 groups: group 0 walks a second tile, so the call takes the tile loop (two launches).  Nothing
    of a tile's last gather may reach the next tile: the first 1024 sequences equal the B 1024 call's
    (one tile per group, the fused kernel), bit for bit."""
    from longterm360fov_amd import ops
    B, T_in, T_out, H = 1040, 3, 2, 256
    big = run_all_forms(B, T_in, T_out, H, "sigmoid")
    enc, dec0 = inputs(B, T_in, 90, 6)
    ws = ops.Workspace()
    head = ops.seq2seq_decode(dev(enc[:1024]), dev(dec0[:1024]), device_weights(H, 90, 6), T_out, impl="cluster", workspace=ws)
    ws.check()
    assert torch.equal(head, big[:1024])


def test_training_forward_writes_reserve_from_the_same_step():
    """Seq2SeqTrainer at H 256, B 32, T 4 -> 3: the layer launches that write the BPTT reserve and the hidden sequence run the
    same step.  Two consecutive identical steps from the same weights are bit-equal; loss, predictions and gradients
    are within test_gpu_train.py's bounds of the fp64 oracle."""
    from longterm360fov_amd.training import Seq2SeqTrainer
    H, B, T_in, T_out = 256, 32, 4, 3
    w = O.init_seq2seq(7300 + H, H=H, bias_noise=0.1)
    enc, dec_in, tgt = batch(7301, B, T_in, T_out)
    loss_ref, g_ref, y_ref = O.seq2seq_loss_and_grads(enc.astype(np.float64), dec_in.astype(np.float64), tgt.astype(np.float64), f64(w), "sigmoid")
    tr = Seq2SeqTrainer(w, impl="cluster")
    loss1, y1 = tr.forward_backward(dev(enc), dev(dec_in), dev(tgt))
    tr.ws.check()
    l1, y1, g1 = float(loss1.item()), y1.clone(), {k: v.clone() for k, v in tr.g.items()}
    loss2, y2 = tr.forward_backward(dev(enc), dev(dec_in), dev(tgt))
    tr.ws.check()
    assert float(loss2.item()) == l1
    assert torch.equal(y2, y1)
    for k in g1:
        assert torch.equal(tr.g[k], g1[k]), k
    assert abs(l1 - loss_ref) <= 1e-5 * max(loss_ref, 1e-6) + 1e-9
    np.testing.assert_allclose(y1.cpu().numpy(), y_ref, atol=2e-5)
    check_grads(g1, g_ref, "gather seams H256")


@pytest.mark.parametrize("H", [128, 64])
def test_hidden_sizes_with_one_partner_and_none(H):
    """H 128 has one partner (two gather loads per lane), H 64 has no exchange."""
    run_all_forms(40, 4, 3, H, "sigmoid")
