"""The packed fused seq2seq kernel's encoder prologue requests K, bias, x_0 / x_1 and the poison word FIRST and the R pack
last, behind everything step 0 consumes in front of its own-slice run (lstm_cluster.hip, KF): at H = 256 twelve k-blocks
between the MFMAs of x_0 . K and the other four between those of x_1 . K in step 0 (one lot each at any input width but the
90-odd one), so that the pack lands while step 0 computes.  The registers and the LDS hold the same values as in the kernel
without packs when they are read, so every output of the call on a workspace with packs must be the same bits as under
FOV_NO_WEIGHT_PACK=1 (torch.equal) - at the step counts where the encoder never reads R (T_in = 1: the pack must still have landed before the decoder phase loads its own R into the
same registers), reads it first in step 0's own-slice run and in its last step (T_in = 2), and runs the steady-state copy;
at input widths that take the general copy of the input projection (F_enc = 17) and that mask no column (F_enc = 96); on
the same-XCD and on the write-through exchange.  impl='cluster' throughout: impl='auto' takes the wide16 kernel at these
batches, which reads no pack."""
import contextlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F_DEC = 6
STEPS = [(1, 1), (2, 1), (3, 4), (9, 7)]


@contextlib.contextmanager
def env(**kv):
    before = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def weights(seed, H, F_enc, scale=0.15):
    g = np.random.default_rng(seed)
    mk = lambda *shape: torch.from_numpy((scale * g.standard_normal(shape)).astype(np.float32)).cuda()
    return {"enc_K": mk(F_enc, 4 * H), "enc_R": mk(H, 4 * H), "enc_b": mk(4 * H), "dec_K": mk(F_DEC, 4 * H), "dec_R": mk(H, 4 * H),
            "dec_b": mk(4 * H), "dense_W": mk(H, F_DEC), "dense_b": mk(F_DEC)}


def inputs(seed, B, T_in, F_enc):
    g = np.random.default_rng(seed)
    mk = lambda *shape: torch.from_numpy(g.uniform(-1, 1, shape).astype(np.float32)).cuda()
    return mk(B, T_in, F_enc), mk(B, 1, F_DEC)


def decode(ops, ws, enc, dec0, w, T_out, act):
    """-> (out, hT, cT) of one call on `ws`, the workspace checked clean."""
    B, H = enc.shape[0], w["enc_R"].shape[0]
    hT, cT = torch.empty((B, H), device="cuda"), torch.empty((B, H), device="cuda")
    out = ops.seq2seq_decode(enc, dec0, w, T_out, act=act, impl="cluster", workspace=ws, hT=hT, cT=cT)
    ws.check()
    return out, hT, cT


def unpacked(ops, enc, dec0, w, T_out, act):
    with env(FOV_NO_WEIGHT_PACK="1"):
        ws = ops.Workspace()
        r = decode(ops, ws, enc, dec0, w, T_out, act)
        assert ws._rpacks == {}
    return r


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def packed_now(ws):
    return all(k in ws._rpacks and ws._rpacks[k][3] is not None for k in ("enc_R", "dec_R"))


def packed_equals_unpacked(ops, H, B, F_enc, act, seed):
    """Per step pair: the calls before the packs exist, the call that makes them and the calls that reuse them."""
    w = weights(seed, H, F_enc)
    ws = ops.Workspace()
    calls = 0
    for T_in, T_out in STEPS:
        enc, dec0 = inputs(seed + 100 * B + T_in, B, T_in, F_enc)
        ref = unpacked(ops, enc, dec0, w, T_out, act)
        for _ in range(ops._PACK_AFTER + 3 if calls == 0 else 2):
            got = decode(ops, ws, enc, dec0, w, T_out, act)
            calls += 1
            assert packed_now(ws) == (calls > ops._PACK_AFTER), calls
            assert same(got, ref), (T_in, T_out, calls)


@pytest.mark.parametrize("B", [16, 40, 48])
@pytest.mark.parametrize("act", ["sigmoid", "hard_sigmoid"])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_packed_call_equals_unpacked_call(H, act, B):
    from longterm360fov_amd import ops
    packed_equals_unpacked(ops, H, B, 90, act, 2000 + H)


@pytest.mark.parametrize("F_enc", [17, 96], ids=["two-k-blocks-general-copy", "no-masked-column"])
def test_packed_call_at_other_input_widths(F_enc):
    from longterm360fov_amd import ops
    packed_equals_unpacked(ops, 256, 40, F_enc, "sigmoid", 3000 + F_enc)


def test_packed_call_on_the_general_exchange():
    """FOV_FORCE_SAFE_EXCHANGE=1: every step runs the general copy of the step, on write-through granules."""
    from longterm360fov_amd import ops
    H, B, (T_in, T_out) = 256, 40, (9, 7)
    w = weights(7, H, 90)
    enc, dec0 = inputs(8, B, T_in, 90)
    with env(FOV_FORCE_SAFE_EXCHANGE="1"):
        ref = unpacked(ops, enc, dec0, w, T_out, "sigmoid")
        ws = ops.Workspace()
        for i in range(ops._PACK_AFTER + 3):
            assert same(decode(ops, ws, enc, dec0, w, T_out, "sigmoid"), ref), i
        assert packed_now(ws) and ws.exchange_mode() == 2
    ops._sync_env()


def test_the_packed_entry_reads_the_k_it_is_given():
    """fov_seq2seq_decode_fwd_packed called directly with ANOTHER input kernel and bias of the encoder: the result is that of the
    unpacked call with those, and differs from the call with the first set - K and bias come from the caller's tensors, as they
    lie, in the reordered prologue too."""
    from longterm360fov_amd import _lib, ops
    H, B, T_in, T_out = 256, 48, 3, 4
    w, w2 = weights(21, H, 90), weights(22, H, 90)
    enc, dec0 = inputs(23, B, T_in, 90)
    mixed = dict(w, enc_K=w2["enc_K"], enc_b=w2["enc_b"])
    ref, ref_own = unpacked(ops, enc, dec0, mixed, T_out, "sigmoid"), unpacked(ops, enc, dec0, w, T_out, "sigmoid")
    assert not torch.equal(ref[0], ref_own[0])
    L = _lib.lib()
    packs = [torch.empty(H * 4 * H, device="cuda") for _ in range(2)]
    for p, k in zip(packs, ("enc_R", "dec_R")):
        ops.check(L.fov_lstm_pack_r(w[k].data_ptr(), H, p.data_ptr(), ops._stream()))
    ws = ops.Workspace()
    buf = ws.get(L.fov_seq2seq_decode_workspace_bytes(B, T_in, T_out, 90, F_DEC, H, ops.IMPL_CLUSTER), enc.device)
    out, hT, cT = torch.empty((B, T_out, F_DEC), device="cuda"), torch.empty((B, H), device="cuda"), torch.empty((B, H), device="cuda")
    ops.check(L.fov_seq2seq_decode_fwd_packed(enc.data_ptr(), dec0.data_ptr(), *[mixed[k].data_ptr() for k in ops._W_ORDER], out.data_ptr(),
                                              hT.data_ptr(), cT.data_ptr(), packs[0].data_ptr(), packs[1].data_ptr(), B, T_in, T_out, 90,
                                              F_DEC, H, ops.ACT_SIGMOID, ops.IMPL_CLUSTER, buf.data_ptr(), buf.numel(), ops._stream()))
    ws.check()
    assert same((out, hT, cT), ref)


def test_k_as_a_view_at_a_four_byte_offset_inside_nan():
    """enc_K inside a larger buffer with NaN in front of and behind it, 4 bytes off a 16-byte boundary: the K-first prologue
    reads rows [0, F) of it and nothing else (rows [F, 96) come from past the descriptor as zeros)."""
    from longterm360fov_amd import ops
    H, B, T_in, T_out, F_enc = 256, 40, 3, 4, 90
    w = weights(61, H, F_enc)
    big = torch.full((F_enc * 4 * H + 64 + 1,), float("nan"), device="cuda")
    v = big[33:33 + F_enc * 4 * H].view(F_enc, 4 * H)
    v.copy_(w["enc_K"])
    assert v.data_ptr() % 16 == 4
    enc, dec0 = inputs(62, B, T_in, F_enc)
    ref = unpacked(ops, enc, dec0, w, T_out, "sigmoid")
    w["enc_K"] = v
    ws = ops.Workspace()
    for i in range(ops._PACK_AFTER + 2):
        got = decode(ops, ws, enc, dec0, w, T_out, "sigmoid")
        assert same(got, ref) and bool(torch.isfinite(got[0]).all()), i
    assert packed_now(ws)
