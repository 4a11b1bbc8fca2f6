"""The fused seq2seq call with its recurrent kernels loaded from fragment-ordered packs (fov_lstm_pack_r,
fov_seq2seq_decode_fwd_packed; ops.seq2seq_decode keeps the packs with the Workspace it is given) against the same call
under FOV_NO_WEIGHT_PACK=1: the registers hold the same values either way, so every output must be the same bits
(torch.equal).  impl='cluster' throughout: at these batches impl='auto' takes the wide16 kernel, which reads no pack."""
import contextlib
import os

import numpy as np
import pytest
import torch

from test_weight_pack_host import pack_r

pytestmark = pytest.mark.gpu

F_ENC, F_DEC = 90, 6
# first-and-last-step-only paths, the steady-state copy, and the T_out = 1 decoder, where the R stream is the whole phase
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


def weights(seed, H, scale=0.15):
    g = np.random.default_rng(seed)
    mk = lambda *shape: torch.from_numpy((scale * g.standard_normal(shape)).astype(np.float32)).cuda()
    return {"enc_K": mk(F_ENC, 4 * H), "enc_R": mk(H, 4 * H), "enc_b": mk(4 * H), "dec_K": mk(F_DEC, 4 * H), "dec_R": mk(H, 4 * H),
            "dec_b": mk(4 * H), "dense_W": mk(H, F_DEC), "dense_b": mk(F_DEC)}


def inputs(seed, B, T_in):
    g = np.random.default_rng(seed)
    mk = lambda *shape: torch.from_numpy(g.uniform(-1, 1, shape).astype(np.float32)).cuda()
    return mk(B, T_in, F_ENC), mk(B, 1, F_DEC)


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
    return all(ws._rpacks[k][3] is not None for k in ("enc_R", "dec_R"))


@pytest.mark.parametrize("H", [64, 128, 256])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "view-at-4-bytes"])
def test_pack_kernel_equals_the_numpy_pack_bytewise(H, offset):
    from longterm360fov_amd import _lib, ops
    g = np.random.default_rng(H + offset)
    R = g.standard_normal((H, 4 * H)).astype(np.float32)
    buf = torch.zeros(H * 4 * H + offset, device="cuda")
    d_R = buf[offset:].view(H, 4 * H)
    d_R.copy_(torch.from_numpy(R))
    out = torch.full((H * 4 * H,), float("nan"), device="cuda")
    ops.check(_lib.lib().fov_lstm_pack_r(d_R.data_ptr(), H, out.data_ptr(), ops._stream()))
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == pack_r(R).tobytes()


def test_pack_entry_refuses_other_widths_and_unaligned_output():
    from longterm360fov_amd import _lib, ops
    L = _lib.lib()
    R, out = torch.zeros(32 * 128 + 4, device="cuda"), torch.zeros(64 * 256 + 4, device="cuda")
    assert L.fov_lstm_pack_r(R.data_ptr(), 32, out.data_ptr(), ops._stream()) == _lib.ERR_UNSUPPORTED
    assert L.fov_lstm_pack_r(R.data_ptr(), 64, out.data_ptr() + 4, ops._stream()) == _lib.ERR_INVALID


@pytest.mark.parametrize("B", [16, 40, 48])
@pytest.mark.parametrize("act", ["sigmoid", "hard_sigmoid"])
@pytest.mark.parametrize("H", [64, 128, 256])
def test_packed_call_equals_unpacked_call(H, act, B):
    """Per step pair: calls on one workspace until the packs exist (the first ops._PACK_AFTER run unpacked), the call that
    makes them and the call that reuses them - each equal to the unpacked call.  The packs persist across the step pairs."""
    from longterm360fov_amd import ops
    w = weights(1000 + H, H)
    ws = ops.Workspace()
    calls = 0
    for T_in, T_out in STEPS:
        enc, dec0 = inputs(B * 100 + T_in, B, T_in)
        ref = unpacked(ops, enc, dec0, w, T_out, act)
        for _ in range(ops._PACK_AFTER + 2 if calls == 0 else 2):
            got = decode(ops, ws, enc, dec0, w, T_out, act)
            calls += 1
            assert packed_now(ws) == (calls > ops._PACK_AFTER), calls
            assert same(got, ref), (T_in, T_out, calls)
    pk = [ws._rpacks[k][3] for k in ("enc_R", "dec_R")]
    assert [p.cpu().numpy().tobytes() for p in pk] == [pack_r(w[k].cpu().numpy()).tobytes() for k in ("enc_R", "dec_R")]


def test_packed_call_on_the_general_exchange():
    """FOV_FORCE_SAFE_EXCHANGE=1: every step runs the general copy of the step."""
    from longterm360fov_amd import ops
    H, B, (T_in, T_out) = 256, 40, (9, 7)
    w = weights(7, H)
    enc, dec0 = inputs(8, B, T_in)
    with env(FOV_FORCE_SAFE_EXCHANGE="1"):
        ref = unpacked(ops, enc, dec0, w, T_out, "sigmoid")
        ws = ops.Workspace()
        for i in range(ops._PACK_AFTER + 2):
            assert same(decode(ops, ws, enc, dec0, w, T_out, "sigmoid"), ref), i
        assert packed_now(ws) and ws.exchange_mode() == 2
    ops._sync_env()


def test_the_fused_kernel_reads_the_packs_it_is_given():
    """Packs of OTHER recurrent kernels handed to fov_seq2seq_decode_fwd_packed: the result is that of the unpacked call with
    those kernels - the packed kernel loads R from the packs and from nowhere else."""
    from longterm360fov_amd import _lib, ops
    H, B, T_in, T_out = 256, 48, 3, 4
    w, w2 = weights(21, H), weights(22, H)
    enc, dec0 = inputs(23, B, T_in)
    mixed = dict(w, enc_R=w2["enc_R"], dec_R=w2["dec_R"])
    ref, ref_own = unpacked(ops, enc, dec0, mixed, T_out, "sigmoid"), unpacked(ops, enc, dec0, w, T_out, "sigmoid")
    assert not torch.equal(ref[0], ref_own[0])
    L = _lib.lib()
    packs = [torch.empty(H * 4 * H, device="cuda") for _ in range(2)]
    for p, k in zip(packs, ("enc_R", "dec_R")):
        ops.check(L.fov_lstm_pack_r(w2[k].data_ptr(), H, p.data_ptr(), ops._stream()))
    ws = ops.Workspace()
    buf = ws.get(L.fov_seq2seq_decode_workspace_bytes(B, T_in, T_out, F_ENC, F_DEC, H, ops.IMPL_CLUSTER), enc.device)
    out, hT, cT = torch.empty((B, T_out, F_DEC), device="cuda"), torch.empty((B, H), device="cuda"), torch.empty((B, H), device="cuda")
    ops.check(L.fov_seq2seq_decode_fwd_packed(enc.data_ptr(), dec0.data_ptr(), *[w[k].data_ptr() for k in ops._W_ORDER], out.data_ptr(),
                                              hT.data_ptr(), cT.data_ptr(), packs[0].data_ptr(), packs[1].data_ptr(), B, T_in, T_out, F_ENC,
                                              F_DEC, H, ops.ACT_SIGMOID, ops.IMPL_CLUSTER, buf.data_ptr(), buf.numel(), ops._stream()))
    ws.check()
    assert same((out, hT, cT), ref)


def test_an_in_place_weight_update_makes_new_packs():
    from longterm360fov_amd import ops
    H, B, T_in, T_out = 128, 40, 3, 4
    w = weights(31, H)
    enc, dec0 = inputs(32, B, T_in)
    ws = ops.Workspace()
    for _ in range(ops._PACK_AFTER + 1):
        old = decode(ops, ws, enc, dec0, w, T_out, "sigmoid")
    assert packed_now(ws)
    old_packs = [ws._rpacks[k][3] for k in ("enc_R", "dec_R")]
    w["enc_R"].add_(0.01)
    w["dec_R"].add_(-0.02)
    ref = unpacked(ops, enc, dec0, w, T_out, "sigmoid")
    assert not torch.equal(ref[0], old[0])
    for i in range(ops._PACK_AFTER + 2):          # unpacked again, then packs of the new values
        assert same(decode(ops, ws, enc, dec0, w, T_out, "sigmoid"), ref), i
    assert packed_now(ws)
    new_packs = [ws._rpacks[k][3] for k in ("enc_R", "dec_R")]
    assert all(not torch.equal(a, b) for a, b in zip(old_packs, new_packs))


def test_an_optimizer_step_on_the_flat_buffer_is_seen():
    """The package's optimizers write through raw pointers: they advance the version counter that all views of the flat
    buffer share, so a pack of a view of it is not used after the step."""
    from longterm360fov_amd import ops
    flat, grads, acc = torch.zeros(1024, device="cuda"), torch.ones(1024, device="cuda"), torch.zeros(1024, device="cuda")
    view = flat[256:768].view(8, 64)
    before = view._version
    ops.rmsprop_step(flat, grads, acc)
    assert view._version != before


def test_r_as_a_view_at_a_four_byte_offset():
    from longterm360fov_amd import ops
    H, B, T_in, T_out = 256, 16, 2, 1
    w = weights(41, H)
    for k in ("enc_R", "dec_R"):
        big = torch.zeros(H * 4 * H + 1, device="cuda")
        v = big[1:].view(H, 4 * H)
        v.copy_(w[k])
        assert v.data_ptr() % 16 == 4
        w[k] = v
    enc, dec0 = inputs(42, B, T_in)
    ref = unpacked(ops, enc, dec0, w, T_out, "hard_sigmoid")
    ws = ops.Workspace()
    for i in range(ops._PACK_AFTER + 2):
        assert same(decode(ops, ws, enc, dec0, w, T_out, "hard_sigmoid"), ref), i
    assert packed_now(ws) and all(ws._rpacks[k][3].data_ptr() % 16 == 0 for k in ("enc_R", "dec_R"))


def test_no_pack_without_a_workspace_of_the_callers():
    from longterm360fov_amd import ops
    H, B, T_in, T_out = 64, 16, 2, 1
    w = weights(51, H)
    enc, dec0 = inputs(52, B, T_in)
    for _ in range(ops._PACK_AFTER + 2):
        ops.seq2seq_decode(enc, dec0, w, T_out, impl="cluster")
    dws = ops.default_workspace(enc.device)
    dws.check()
    assert dws._rpacks == {}
