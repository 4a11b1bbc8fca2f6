"""The bf16 BACKWARD kernels against a restatement that rounds exactly the products they round (BASELINE.json configs[4]).

test_gpu_bf16.py / test_gpu_s2s_bf16.py hold the bf16 gradients to the full-precision graph only, at 2e-2 .. 3e-2 of scale.
Here every backward form is compared with the fp64 restatement of ITS OWN rounding contract (include/fov360.h):
  * per kernel (lstm_seq_bwd, mix_decoder_bwd, dense_bwd): both sides get the GPU's own fp32 forward tape, so what is
    left is the backward alone; bound PER_KERNEL = 1e-3 of each tensor's max |ref| (measured maxima are printed);
  * the tapes the backward reads (lstm_seq_train / mix_decoder train tapes, bf16): TIGHT = 1e-3 absolute against the
    bf16-operand forward;
  * the bf16 trainers' forward_backward gradients against torch.autograd in fp64 with a product that rounds exactly the
    products the trainer's calls round (oracle/bf16_autograd.py); bound TRAINER = 5e-3 of each tensor's scale.
The reference's switches say which products round: round_rec (dz R^T), round_dx (dz K^T), round_wgrad (x^T dz, h^T dz);
db is always the sum of the unrounded dz.
"""
import os

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

pytestmark = pytest.mark.gpu

PER_KERNEL = 1e-3
# The state gradients after the last step (dh0 of a layer, dh1_0 / dh2_0 of the decoder) are one rounded product rb(dz_0) R^T
# each.  A dz element within an fp32 ulp of a bf16 rounding boundary rounds either way, moving its term by one bf16 ulp: the
# restatement fed the same tape perturbed by ONE fp32 ulp (relative 6e-8) moves its own dh1_0 / dh2_0 by 1.1e-3 / 1.0e-3 of
# scale at B 512, T 30 (kernel vs restatement measured: 1.2e-3).  That is the contract's noise floor, not the kernel's error:
# the bound of these tensors is twice it.
STATE = 2e-3
TIGHT = 1e-3
TRAINER = 5e-3
H = 256


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def d64(a):
    if a is None:
        return None
    return a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)


def rb(a):
    return O.round_bf16(np.asarray(a, dtype=np.float64))


def near(tag, got, ref, bound):
    """max |got - ref| <= bound * max |ref|; prints the measured error."""
    a, r = d64(got), d64(ref)
    scale = np.abs(r).max()
    err = np.abs(a - r).max()
    print("%-48s max|ref| %.3e  err %.3e (%.1e of scale)" % (tag, scale, err, err / (scale + 1e-30)))
    assert np.isfinite(a).all(), tag
    assert err <= bound * scale + 1e-9, (tag, err, scale)
    return err / (scale + 1e-30)


def offset_view(a, off):
    """a copy of `a` as a view that starts `off` floats into a flat device buffer."""
    flat = torch.zeros(off + a.size + 4, dtype=torch.float32, device="cuda")
    v = flat[off:off + a.size].view(*a.shape)
    v.copy_(dev(a))
    return v


# ---------------------------------------------------------------------------------------------------------------------
# lstm_seq_bwd(dtype="bf16"): the eight-workgroup N-split BPTT kernel, its dx forms and the weight-gradient products
# ---------------------------------------------------------------------------------------------------------------------
# state: h0/c0 given; ups: which upstream gradients (s = dhs, h = dhT, c = dcT); form: "" | "acc" (accumulate onto a non-zero
# base) | "nodx" (FOV_NO_DX_FUSION=1) | "adj" (dK | dR | db adjacent in one flat buffer: the fused products) | "koffN" (K a view
# N floats into a flat buffer: 4, 8, 12 bytes)
LAYER_CASES = [
    (1, 1, 256, "sigmoid", False, "s", ""),
    (15, 2, 6, "hard_sigmoid", True, "shc", ""),
    (16, 30, 90, "sigmoid", True, "s", "adj"),
    (17, 2, 96, "hard_sigmoid", False, "hc", ""),
    (16 * 32 + 9, 30, 256, "sigmoid", True, "shc", "adj"),
    (1024, 1, 6, "sigmoid", False, "sh", ""),
    (1024, 2, 200, "hard_sigmoid", True, "shc", ""),
    (48, 5, 250, "sigmoid", True, "c", ""),
    (37, 4, 90, "sigmoid", True, "shc", "acc"),
    (100, 5, 256, "hard_sigmoid", True, "shc", "nodx"),
    (64, 3, 256, "sigmoid", True, "shc", "koff1"),
    (40, 3, 90, "sigmoid", False, "sh", "koff2"),
    (33, 2, 256, "hard_sigmoid", True, "s", "koff3"),
]


@pytest.mark.parametrize("B,T,F,act,state,ups,form", LAYER_CASES)
def test_layer_bptt_bf16_matches_its_rounding_contract(B, T, F, act, state, ups, form):
    """Every output of lstm_seq_bwd(dtype='bf16') - dz, dx, dK, dR, db, dh0, dc0 - against lstm_layer_backward rounding the
    products of the form that runs: the recurrence always; dx when K is 16-byte aligned (in the kernel at F = 256, else the
    bf16 NT product), fp32 when it is not; x^T dz except the fp32 skinny product (F <= 8, >= 1024 rows); h_{t-1}^T dz.
    Bound 1e-3 of each tensor's max |ref| (dh0: STATE = 2e-3); measured at most 6.3e-4 (dx, B 521, T 30) and 8.7e-4 on dh0.
    The error against the other dx form is printed and must be larger."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(B * 7 + T * 3 + F)
    K, R, b = O.init_lstm(rng, F, H, np.float32)
    b = (b + 0.1 * rng.standard_normal(b.shape)).astype(np.float32)
    x = rng.uniform(-1, 1, (B, T, F)).astype(np.float32)
    h0 = (0.3 * rng.standard_normal((B, H))).astype(np.float32) if state else None
    c0 = (0.3 * rng.standard_normal((B, H))).astype(np.float32) if state else None
    dhs = (0.1 * rng.standard_normal((B, T, H))).astype(np.float32) if "s" in ups else None
    dhT = (0.1 * rng.standard_normal((B, H))).astype(np.float32) if "h" in ups else None
    dcT = (0.1 * rng.standard_normal((B, H))).astype(np.float32) if "c" in ups else None
    od = lambda a: None if a is None else dev(a)
    Kd = offset_view(K, int(form[4:])) if form.startswith("koff") else dev(K)
    xd, Rd, h0d, c0d = dev(x), dev(R), od(h0), od(c0)
    hs, _, _, res = ops.lstm_seq_train(xd, dev(K), Rd, dev(b), h0d, c0d, act=act)      # the fp32 tape, for both sides
    grads = {}
    if form == "adj":
        flat = torch.zeros((F + H + 1) * 4 * H, dtype=torch.float32, device="cuda")
        grads = dict(dK=flat[:F * 4 * H].view(F, 4 * H), dR=flat[F * 4 * H:(F + H) * 4 * H].view(H, 4 * H), db=flat[(F + H) * 4 * H:])
    base = {}
    if form == "acc":
        base = {k: (rng.standard_normal(s) * 0.01).astype(np.float32) for k, s in (("dK", (F, 4 * H)), ("dR", (H, 4 * H)), ("db", (4 * H,)))}
        grads = {k: dev(v) for k, v in base.items()}
    sc = ops.Scratch()
    if form == "nodx":
        os.environ["FOV_NO_DX_FUSION"] = "1"
    try:
        got = ops.lstm_seq_bwd(xd, Kd, Rd, hs, res, h0=h0d, c0=c0d, dhs=od(dhs), dhT=od(dhT), dcT=od(dcT), need_dx=True,
                               need_state_grads=True, act=act, accumulate=(form == "acc"), scratch=sc, dtype="bf16", **grads)
    finally:
        if form == "nodx":
            del os.environ["FOV_NO_DX_FUSION"]
    sc.check()
    dx_bf16 = Kd.data_ptr() % 16 == 0
    args = (d64(x), d64(K), d64(R), d64(h0), d64(c0), d64(hs), d64(res), d64(dhs), d64(dhT), d64(dcT))
    ref = O.lstm_layer_backward(*args, act=act, round_rec=True, round_dx=dx_bf16, round_wgrad=True)
    if F <= 8 and B * T >= 1024:     # the skinny fp32 product takes dK
        ref["dK"] = d64(x).reshape(B * T, F).T @ ref["dz"].reshape(B * T, 4 * H)
    for k, v in base.items():
        ref[k] = ref[k] + v
    tag = "bf16 BPTT B=%d T=%d F=%d %s %s" % (B, T, F, ups, form)
    for k in ("dz", "dx", "dK", "dR", "db", "dh0", "dc0"):
        near("%s %s" % (tag, k), got[k], ref[k], STATE if k == "dh0" else PER_KERNEL)
    dz = ref["dz"].reshape(B * T, 4 * H)
    other = (dz @ d64(K).T) if dx_bf16 else (rb(dz) @ rb(K).T)
    e_other = np.abs(d64(got["dx"]).reshape(B * T, F) - other).max()
    e_own = np.abs(d64(got["dx"]) - ref["dx"]).max()
    print("%s dx (%s) vs the other form: %.3e (own %.3e)" % (tag, "bf16" if dx_bf16 else "fp32", e_other, e_own))
    assert e_own < e_other


def test_layer_bptt_bf16_rejects_an_unaligned_recurrent_kernel():
    """The bf16 BPTT kernel reads R as 16-byte lines: R at a 4-, 8- or 12-byte offset is an error, not a wrong result
    (a trainer's R views lie at multiples of 4 KiB of its flat buffer)."""
    from longterm360fov_amd import ops
    from longterm360fov_amd._lib import FovError
    rng = np.random.default_rng(3)
    B, T, F = 20, 2, 90
    K, R, b = O.init_lstm(rng, F, H, np.float32)
    xd = dev(rng.uniform(-1, 1, (B, T, F)))
    hs, _, _, res = ops.lstm_seq_train(xd, dev(K), dev(R), dev(b))
    for off in (1, 2, 3):
        with pytest.raises(FovError):
            ops.lstm_seq_bwd(xd, dev(K), offset_view(R, off), hs, res, dhs=hs, scratch=ops.Scratch(), dtype="bf16")
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,T,F,act,state", [(37, 5, 90, "sigmoid", True), (16 * 32 + 9, 3, 256, "hard_sigmoid", False),
                                             (1, 30, 6, "sigmoid", True)])
def test_bf16_layer_training_tape_matches_bf16_operand_forward(B, T, F, act, state):
    """All five reserve planes (i, f, g, o, c of every step) and hs of lstm_seq_train(dtype='bf16') against
    lstm_layer_train(round_fwd=True): bound TIGHT = 1e-3 absolute; measured at most 1.2e-4."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(B + T + F)
    K, R, b = O.init_lstm(rng, F, H, np.float32)
    b = (b + 0.1 * rng.standard_normal(b.shape)).astype(np.float32)
    x = rng.uniform(-1, 1, (B, T, F)).astype(np.float32)
    h0 = (0.3 * rng.standard_normal((B, H))).astype(np.float32) if state else None
    c0 = (0.3 * rng.standard_normal((B, H))).astype(np.float32) if state else None
    od = lambda a: None if a is None else dev(a)
    ws = ops.Workspace()
    hs, hT, cT, res = ops.lstm_seq_train(dev(x), dev(K), dev(R), dev(b), od(h0), od(c0), act=act, workspace=ws, dtype="bf16")
    ws.check()
    rhs, rh, rc, rres = O.lstm_layer_train(d64(x), d64(K), d64(R), d64(b), d64(h0), d64(c0), act=act, round_fwd=True)
    tag = "bf16 tape B=%d T=%d F=%d" % (B, T, F)
    for q, name in enumerate("ifgoc"):
        e = np.abs(d64(res)[:, :, q] - rres[:, :, q]).max()
        print("%s %s err %.3e" % (tag, name, e))
        assert e <= TIGHT, (name, e)
    assert np.abs(d64(hs) - rhs).max() <= TIGHT and np.abs(d64(cT) - rc).max() <= TIGHT


# ---------------------------------------------------------------------------------------------------------------------
# mix_decoder_bwd: the fused decoder BPTT (head, both layers, feedback) on the tapes of mix_decoder(train=...)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("B,T,O_,act", [(1, 1, 3, "sigmoid"), (16, 2, 6, "hard_sigmoid"), (37, 10, 8, "sigmoid"),
                                        (512, 30, 6, "sigmoid"), (530, 2, 6, "hard_sigmoid"), (37, 30, 3, "hard_sigmoid")])
def test_mix_decoder_backward_matches_its_rounding_contract(dtype, B, T, O_, act):
    """mix_decoder(train=...) then mix_decoder_bwd: every tape (M, P, H1, C1, H2, C2, res1, res2) against
    mix_decoder_train_forward (bf16: bf16-operand products, TIGHT = 1e-3 absolute; fp32: 1e-4), then DZ1, DZ2, dpre_m,
    dpre_p and the four state gradients against mix_decoder_backward on the kernel's own tapes - bf16: the recurrences
    dz R^T and the data products dz2 K2^T, dz1 K1^T (the feedback) rounded, bound 1e-3 of each tensor's scale; fp32:
    nothing rounded, bound 1e-4.  Measured: bf16 tapes at most 8.1e-4 (M, B 512, T 30); bf16 gradients at most 3.9e-4 of
    scale (DZ1), the state gradients dh1_0 / dh2_0 1.2e-3 (bound STATE, see there); fp32 gradients 3.8e-7 of scale."""
    from longterm360fov_amd import ops
    bf = dtype == "bf16"
    rng = np.random.default_rng(B * 5 + T + O_)
    w = O.init_others_mixing(B + T, F_dec=O_, H=H, num_user=4, bias_noise=0.1)
    mix_Wp = (0.5 * rng.standard_normal((O_, O_))).astype(np.float32)
    st = [(0.4 * rng.standard_normal((B, H))).astype(np.float32) for _ in range(4)]
    dec0 = rng.uniform(-1, 1, (B, O_)).astype(np.float32)
    oth = (0.3 * rng.standard_normal((B, T, O_))).astype(np.float32)
    dw = {k: dev(v) for k, v in w.items()}
    e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    C1, C2 = e(T + 1, B, H), e(T + 1, B, H)        # row 0 = the initial state, row t+1 = after step t
    C1[0].copy_(dev(st[1])); C2[0].copy_(dev(st[3]))
    tape = {"P": e(T, B, O_), "H1": e(T, B, H), "C1": C1[1:], "H2": e(T, B, H), "C2": C2[1:], "res1": e(T, B, 5, H), "res2": e(T, B, 5, H)}
    ws = ops.Workspace()
    M = ops.mix_decoder(dev(dec0), dev(st[0]), C1[0], dev(st[2]), C2[0], dev(oth), dw, dev(mix_Wp), T, act=act, workspace=ws,
                        train=tape, dtype=dtype)
    ws.check()
    w64 = {k: d64(v) for k, v in w.items()}
    rf = O.mix_decoder_train_forward(d64(dec0), *[d64(s) for s in st], d64(oth), w64, d64(mix_Wp), T, act=act, round_fwd=bf)
    tag = "%s decoder B=%d T=%d O=%d" % (dtype, B, T, O_)
    tb = TIGHT if bf else 1e-4
    tape["M"] = M
    for k in ("M", "P", "H1", "C1", "H2", "C2", "res1", "res2"):
        err = np.abs(d64(tape[k]) - rf[k]).max()
        print("%s tape %-4s err %.3e" % (tag, k, err))
        assert err <= tb, (k, err)
    G = (0.2 * rng.standard_normal((T, B, O_))).astype(np.float32)
    dloss = dev(G) * (1 - M * M)
    out = {k: e(T, B, 4 * H) for k in ("DZ1", "DZ2")}
    out.update({k: e(T, B, O_) for k in ("dpre_m", "dpre_p")})
    out.update({k: e(B, H) for k in ("dh1_0", "dc1_0", "dh2_0", "dc2_0")})
    wsb = ops.Workspace()
    ops.mix_decoder_bwd(M, tape["P"], dloss, tape["res1"], tape["res2"], C1, C2, dw, dev(mix_Wp), out, act=act, workspace=wsb,
                        dtype=dtype)
    wsb.check()
    ref = O.mix_decoder_backward(d64(M), d64(tape["P"]), d64(dloss), d64(tape["res1"]), d64(tape["res2"]), d64(C1), d64(C2), w64,
                                 d64(mix_Wp), act=act, round_rec=bf, round_dx=bf)
    for k in ("DZ1", "DZ2", "dpre_m", "dpre_p", "dh1_0", "dc1_0", "dh2_0", "dc2_0"):
        near("%s %s" % (tag, k), out[k], ref[k], (STATE if k in ("dh1_0", "dh2_0") else PER_KERNEL) if bf else 1e-4)


# ---------------------------------------------------------------------------------------------------------------------
# dense_bwd(dtype="bf16"): which rounding each form applies
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Out", [6, 63, 64, 1024])
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("accumulate", [False, True])
def test_dense_backward_bf16_forms(Out, aligned, accumulate):
    """dW = x^T dpre takes bf16 operands only when Out >= 64, Out % 4 == 0 and dpre is 16-byte aligned (the bf16 TN product);
    otherwise it is the fp32 product (skinny for Out <= 8 at >= 1024 rows).  dx = dpre W^T and db are fp32 in every form.
    Each result within 1e-5 of scale of its own form's fp64 reference (measured at most 3.3e-7) and more than ten times farther
    from the other form's (measured 2e-3 .. 3e-3)."""
    from longterm360fov_amd import ops
    N, In = 1500, 90
    rng = np.random.default_rng(Out + 2 * aligned + accumulate)
    x = rng.standard_normal((N, In)).astype(np.float32)
    W = (0.1 * rng.standard_normal((In, Out))).astype(np.float32)
    d = (0.1 * rng.standard_normal((N, Out))).astype(np.float32)
    dd = dev(d) if aligned else offset_view(d, 1)
    assert (dd.data_ptr() % 16 == 0) == aligned
    base = (rng.standard_normal((In, Out)) if accumulate else np.zeros((In, Out))).astype(np.float32)
    bbase = (rng.standard_normal(Out) if accumulate else np.zeros(Out)).astype(np.float32)
    dW, db = dev(base), dev(bbase)
    dx, _, _ = ops.dense_bwd(dev(x), dev(W), dd, dW=dW, db=db, accumulate=accumulate, dtype="bf16")
    bf = Out >= 64 and Out % 4 == 0 and aligned
    r_bf, r_32 = rb(x).T @ rb(d), d64(x).T @ d64(d)
    own, other = (r_bf, r_32) if bf else (r_32, r_bf)
    a = d64(dW) - base
    tag = "dense_bwd bf16 Out=%d %s acc=%d dW (%s)" % (Out, "aligned" if aligned else "unaligned", accumulate, "bf16" if bf else "fp32")
    e_own = near(tag, a, own, 1e-5)
    e_other = np.abs(a - other).max() / np.abs(other).max()
    print("%s vs the other form %.1e of scale" % (tag, e_other))
    assert e_other > 10 * e_own
    near("dense_bwd bf16 Out=%d dx (fp32)" % Out, dx, d64(d) @ d64(W).T, 1e-5)
    near("dense_bwd bf16 Out=%d db (fp32)" % Out, d64(db) - bbase, d64(d).sum(0), 1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# the bf16 trainers: forward_backward against autograd with exactly the trainer's rounded products
# ---------------------------------------------------------------------------------------------------------------------
def _check_trainer_grads(tag, got, ref, order):
    worst = 0.0
    for k in order:
        worst = max(worst, near("%s %s" % (tag, k), got[k], ref[k], TRAINER))
    print("%s: worst gradient error %.2e of its scale" % (tag, worst))


def test_seq2seq_bf16_trainer_gradients_match_its_rounded_products():
    """Seq2SeqTrainer(dtype='bf16') at B 40, T 6 -> 5: forward products of both layers and of the Dense head rounded; the
    BPTT recurrences and every x^T dz / h_{t-1}^T dz rounded (no dx is formed); the head's backward fp32.  Bound 5e-3 of
    each gradient's scale; measured at most 1.4e-4."""
    from longterm360fov_amd.training import Seq2SeqTrainer
    from oracle import bf16_autograd as A
    from test_gpu_train import _W_ORDER, batch
    B, T_in, T_out, act = 40, 6, 5, "sigmoid"
    w = O.init_seq2seq(60, H=H, bias_noise=0.1)
    enc, dec_in, tgt = batch(61, B, T_in, T_out)
    tr = Seq2SeqTrainer(w, act=act, dtype="bf16")
    loss, _ = tr.forward_backward(dev(enc), dev(dec_in), dev(tgt))
    tr.ws.check()
    t = {k: A.leaf(v) for k, v in w.items()}
    z0 = torch.zeros(B, H, dtype=torch.float64)
    h, c = z0, z0
    x = torch.tensor(enc.astype(np.float64))
    for s in range(T_in):
        h, c = A.lstm_step(x[:, s], h, c, t["enc_K"], t["enc_R"], t["enc_b"], act, fwd=True, rec=True, wgrad=True)
    xd, hs = torch.tensor(dec_in.astype(np.float64)), []
    for s in range(T_out):
        h, c = A.lstm_step(xd[:, s], h, c, t["dec_K"], t["dec_R"], t["dec_b"], act, fwd=True, rec=True, wgrad=True)
        hs.append(h)
    hs = torch.stack(hs, 1).reshape(B * T_out, H)
    y = torch.tanh(A.mm(hs, t["dense_W"], fwd=True) + t["dense_b"])
    l = torch.mean((y - torch.tensor(tgt.astype(np.float64)).reshape(B * T_out, -1)) ** 2)
    l.backward()
    assert abs(float(loss.item()) - l.item()) <= 1e-3 * l.item()
    _check_trainer_grads("bf16 seq2seq trainer B=%d %d->%d" % (B, T_in, T_out), tr.g, {k: v.grad for k, v in t.items()}, _W_ORDER)


@pytest.mark.parametrize("B,U,T_in,T_out,act", [(37, 5, 2, 4, "hard_sigmoid"), (48, 34, 30, 30, "sigmoid")])
def test_mixing_bf16_trainer_gradients_match_its_rounded_products(B, U, T_in, T_out, act):
    """OthersMixingTrainer(dtype='bf16'): forward products of the four layers and of the Dense head rounded, the mixing layer
    fp32; backward: every recurrence rounded, the data products dz K^T of the decoder layers (dh1_t, the feedback dx_t) and
    of encoder layer 2 (its dx, the dhs of layer 1) rounded; weight products x^T dz, h^T dz rounded for enc1, enc2, dec2 and
    dec1_R, fp32 for dec1_K (dense_bwd) and the head (mix_head_wgrad).  Bound 5e-3 of each gradient's scale; measured at most
    2.7e-4."""
    from longterm360fov_amd.training import OthersMixingTrainer, _MIX_ORDER
    from oracle import bf16_autograd as A
    w = O.init_others_mixing(170, H=H, num_user=U, bias_noise=0.1)
    enc, dec0, tgt, oth = O.synthetic_batch(171 + B, B, T_in, T_out, num_others=U - 1)
    tr = OthersMixingTrainer(w, act=act, dtype="bf16")
    loss, _ = tr.forward_backward(dev(enc), dev(oth), dev(dec0), dev(tgt))
    tr.check()
    t = {k: A.leaf(v) for k, v in w.items()}
    z0 = torch.zeros(B, H, dtype=torch.float64)
    h1 = c1 = h2 = c2 = z0
    e = torch.tensor(enc.astype(np.float64))
    for s in range(T_in):
        h1, c1 = A.lstm_step(e[:, s], h1, c1, t["enc1_K"], t["enc1_R"], t["enc1_b"], act, fwd=True, rec=True, wgrad=True)
        h2, c2 = A.lstm_step(h1, h2, c2, t["enc2_K"], t["enc2_R"], t["enc2_b"], act, fwd=True, rec=True, dx=True, wgrad=True)
    o_ = torch.tensor(oth.astype(np.float64))
    x, outs = torch.tensor(dec0[:, 0].astype(np.float64)), []
    for s in range(T_out):
        H1 = A.mm(x, t["dec1_K"], True, True, False) + t["dec1_b"] + A.mm(h1, t["dec1_R"], True, True, True)
        h1, c1 = _gates(H1, c1, act)
        H2 = A.mm(h1, t["dec2_K"], True, True, True) + t["dec2_b"] + A.mm(h2, t["dec2_R"], True, True, True)
        h2, c2 = _gates(H2, c2, act)
        p = torch.tanh(A.mm(h2, t["dense_W"], fwd=True) + t["dense_b"])
        cat = torch.cat([o_[:, s], p[:, None, :]], dim=1)
        x = torch.tanh(cat.reshape(B, -1) @ t["mix_W"] + t["mix_b"])
        outs.append(x)
    l = torch.mean((torch.stack(outs, 1) - torch.tensor(tgt.astype(np.float64))) ** 2)
    l.backward()
    assert abs(float(loss.item()) - l.item()) <= 1e-3 * l.item()
    _check_trainer_grads("bf16 mixing trainer B=%d %d->%d" % (B, T_in, T_out), tr.g, {k: v.grad for k, v in t.items()}, _MIX_ORDER)


def _gates(z, c, act):
    s = torch.sigmoid if act == "sigmoid" else (lambda v: torch.clamp(0.2 * v + 0.5, 0, 1))
    i, f, g, o = s(z[:, :H]), s(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), s(z[:, 3 * H:])
    c = f * c + i * g
    return o * torch.tanh(c), c
