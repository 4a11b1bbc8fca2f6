"""The small kernels that close every training step - the loss kernels, the three optimizers, the activation / softmax helpers
and the sampled re-feed - each alone, through longterm360fov_amd.ops, at the sizes where their loops, block partials, 16-byte
accesses and clip masks change path.

Every comparison is against fp64 arithmetic on the fp32-rounded inputs AND hyper-parameters (oracle/fov_oracle.py, "Loss /
optimizer / pointwise references"; each reference is checked against torch.autograd in tests/test_oracle.py).  Bounds are per
element:  |err| <= c * 2^-24 * w,  w = the sum of the |terms| that make up that element (the oracle returns it), c = the depth
of the kernel's summation (trips of its strided loop + levels of its tree) + the roundings of one term + a margin of 4; the
count is written where each c is set.  Scalar losses: 1e-5 relative; softmax: 1e-6 (forward) / 1e-5 (backward) of max|ref|.
Every call is made twice and must give the same bits; outputs that are views of a larger buffer have canaries on both sides.
Each test prints its worst figure before it asserts."""
import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

pytestmark = pytest.mark.gpu

U = O.U24
CANARY = 1234.5
PAD = 4          # floats of canary on each side of a view: the view itself stays 16-byte aligned

# Worst errors of the two fast intrinsics and of tanh_f against fp64, MEASURED on the MI355X over the inputs of the tests below
# ("Loss, optimizer and pointwise kernels"); the bound in force is 4 x the measured figure where that is
# tighter than the derived one.  exp / log: as a fraction of the derived per-element bound; tanh: absolute.
EXP_MEASURED = 0.383      # so the derived (1.5 |x| + 4) 2^-23 is the bound in force
LOG_MEASURED = 0.405      # so the derived (3 |log v| + 1) 2^-23 is the bound in force
TANH_MEASURED = 2.07e-7   # 4 x = 8.3e-7: the derived 6.2e-7 is the bound in force
TANH_DERIVED = 5.2 * 2.0 ** -23


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def guarded(n, off=PAD, fill=None):
    """A view of n floats inside a buffer of canaries -> (buffer, view).  off = 1: a 4-byte-aligned view."""
    base = torch.full((n + 2 * PAD,), CANARY, dtype=torch.float32, device="cuda")
    view = base[off:off + n]
    if fill is not None:
        view.copy_(dev(fill).reshape(-1))
    return base, view


def canaries_intact(base, view):
    off = (view.data_ptr() - base.data_ptr()) // 4
    ref = torch.full_like(base, CANARY)
    return same_bits(base[:off], ref[:off]) and same_bits(base[off + view.numel():], ref[off + view.numel():])


def worst(got, ref, w):
    """max over the elements of |got - ref| / (2^-24 * w): the c that the result needs."""
    got, ref, w = (np.asarray(a, np.float64) for a in (got, ref, w))
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    return float((err / (U * w + 2.0 ** -149)).max()) if err.size else 0.0


def within(got, ref, w, c, tag):
    r = worst(got, ref, w)
    print("%-46s worst error %8.3f x 2^-24 x terms, bound %g" % (tag, r, c))
    assert r <= c, (tag, r, c)


def loss_close(got, ref, tag):
    got = float(got.item())
    print("%-46s loss %.9g ref %.9g rel %.2e" % (tag, got, ref, abs(got - ref) / max(abs(ref), 1e-300)))
    assert abs(got - ref) <= 1e-5 * abs(ref) + 1e-30, (tag, got, ref)


# --------------------------------------------------------------------------------------
# 1. Gaussian NLL
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("i", range(len(O.NLL_EDGE_SHAPES)))
def test_gauss_nll_blocks_trips_and_clip_mask(i, scale):
    """gauss_nll_kernel: one block per sequence, a 256-strided loop over per = 3 * T_y * fps elements, an 8-level tree, the
    last block adds the B block partials 256-strided.  c: a lane adds trips = ceil(per / 256) terms, the tree 8 more; one dmu
    term -2 (y - mu) / (var + eps) has 3 roundings (difference, var + eps, quotient), one dvar term 1 / v - d^2 / v^2 has 7
    (v, 1 / v, d, d^2, v^2, quotient, difference), the final * scale / B two more: c_dmu = trips + 8 + 5 + 4, c_dvar = trips +
    8 + 9 + 4.  All three populations are present (l < -10, l > 10, interior; none within 1e-3 of a bound, so fp32 and fp64
    mask the same elements); the reference WITHOUT the clip's mask misses the same bound, so the case tests the mask."""
    from longterm360fov_amd import ops
    B, Ty, fps = O.NLL_EDGE_SHAPES[i]
    mu, var, y, again = O.nll_edge_inputs(100 + i, B, Ty, fps)
    lo, hi, mid, dist = O.nll_populations(mu, var, y, fps)
    n = y.size
    assert dist >= 1e-3
    if n >= 90:
        assert lo >= 0.05 and hi >= 0.05 and mid >= 0.5 and again < 0.01 * n
    (loss_r, dmu_r, dvar_r), (wm, wv), _ = O.gauss_nll(mu, var, y, fps, scale)
    d = [dev(a) for a in (mu, var, y)]
    loss, dmu, dvar = ops.gauss_nll_grad(d[0], d[1], d[2], fps, scale)
    loss2, dmu2, dvar2 = ops.gauss_nll_grad(d[0], d[1], d[2], fps, scale)
    assert same_bits(loss, loss2) and same_bits(dmu, dmu2) and same_bits(dvar, dvar2)
    trips = -(-3 * Ty * fps // 256)
    tag = "nll %s scale %g" % ((B, Ty, fps), scale)
    loss_close(loss, loss_r, tag)
    within(host(dmu), dmu_r, wm, trips + 8 + 5 + 4, tag + " dmu")
    within(host(dvar), dvar_r, wv, trips + 8 + 9 + 4, tag + " dvar")
    if n >= 90:
        (_, dmu_n, dvar_n), _, _ = O.gauss_nll(mu, var, y, fps, scale, clip_mask=False)
        assert worst(host(dmu), dmu_n, wm) > trips + 8 + 5 + 4 and worst(host(dvar), dvar_n, wv) > trips + 8 + 9 + 4


def test_gauss_nll_empty_batch_is_a_zero_loss():
    from longterm360fov_amd import ops
    e = lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")
    loss, dmu, dvar = ops.gauss_nll_grad(e(0, 3), e(0, 3), e(0, 1, 90), 30, 1.0)
    assert float(loss.item()) == 0.0 and dmu.shape == (0, 3) and dvar.shape == (0, 3)


def test_fast_log_through_the_nll_loss():
    """__logf has no kernel of its own: one sequence, one frame, y = mu and var = (v, 1, 1) make the loss log(v) + 0 + 0.
    Derived bound: v_log_f32 is good to 1 ulp of log2 v, the product with ln 2 and its rounding add one more, the loss
    scale a last one - (3 |log v| + 1) * 2^-23.  The measured worst case is printed as a fraction of that."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(41)
    vs = np.concatenate([10.0 ** rng.uniform(-4, 4, 40), 1 + np.array([1e-3, -1e-3, 2.0 ** -20, -2.0 ** -20, 0.0]), [0.5, 2.0, 1e-4, 1e4]])
    vs = vs.astype(np.float32)
    mu = dev(np.zeros((1, 3)))
    y = dev(np.zeros((1, 1, 3)))
    frac = 0.0
    for v in vs:
        loss, _, _ = ops.gauss_nll_grad(mu, dev(np.array([[v, 1.0, 1.0]])), y, 1, 1.0)
        ref = np.log(np.float64(v) + O.r32(1e-20))
        frac = max(frac, abs(float(loss.item()) - ref) / ((3 * abs(ref) + 1) * 2.0 ** -23))
    k = 1.0 if LOG_MEASURED is None else min(4 * LOG_MEASURED, 1.0)
    print("__logf through the NLL loss: worst error %.4f of the derived (3 |log v| + 1) * 2^-23, bound in force %.4f" % (frac, k))
    assert frac <= k


# --------------------------------------------------------------------------------------
# 2. MSE behind Dense
# --------------------------------------------------------------------------------------
C_MSE = 6 + 4     # y - t, weight / n, 2 d * scale, y^2, 1 - y^2, the product: six roundings of the one term; no sum


def _mse_check(y, tgt, act, weight, time_major, tag, own_loss):
    from longterm360fov_amd import ops
    (loss_r, dpre_r), w = O.mse_dense(y, tgt, act, weight, time_major=time_major)
    base, view = guarded(y.size)
    dpre = view.view(y.shape)
    dy, dt = dev(y), dev(tgt)
    loss = torch.full((1,), CANARY, dtype=torch.float32, device="cuda") if own_loss else None
    _, l1 = ops.mse_dense_grad(dy, dt, act, dpre=dpre, loss=loss, weight=weight, time_major=time_major)
    first, l1 = dpre.clone(), l1.clone()
    _, l2 = ops.mse_dense_grad(dy, dt, act, dpre=dpre, loss=loss, weight=weight, time_major=time_major)
    assert same_bits(first, dpre) and same_bits(l1, l2) and canaries_intact(base, view)
    loss_close(l2, loss_r, tag)
    within(host(dpre), dpre_r, w, C_MSE, tag + " dpre")
    return host(dpre), w


@pytest.mark.parametrize("weight", [1.0, 0.37])
@pytest.mark.parametrize("act", ["tanh", "linear"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537 + 3])
def test_mse_dense_grad_block_edges(n, act, weight):
    """One element per thread, the last block ragged; 65 540 elements are 257 blocks, so the last block's sum of the block
    partials takes a second trip.  With the caller's loss tensor and with loss=None (the wrapper's own)."""
    rng = np.random.default_rng(300 + n)
    y = np.tanh(rng.standard_normal(n)).astype(np.float32) if act == "tanh" else rng.standard_normal(n).astype(np.float32)
    tgt = rng.uniform(-1, 1, n).astype(np.float32)
    for own in (True, False):
        _mse_check(y, tgt, act, weight, False, "mse n %d %s w %g %s" % (n, act, weight, "loss" if own else "loss=None"), own)


@pytest.mark.parametrize("act", ["tanh", "linear"])
@pytest.mark.parametrize("T,B,Od", [(3, 5, 6), (10, 32, 6), (7, 37, 3), (2, 130, 1)])
def test_mse_dense_grad_time_major_index_map(T, B, Od, act):
    """y / dpre (T,B,O) against a target (B,T,O): element (t*B + b)*O + o reads target (b*T + t)*O + o.  The reference with the
    target left un-transposed misses the bound."""
    rng = np.random.default_rng(310 + T)
    y = np.tanh(rng.standard_normal((T, B, Od))).astype(np.float32)
    tgt = rng.uniform(-1, 1, (B, T, Od)).astype(np.float32)
    got, w = _mse_check(y, tgt, act, 0.37, True, "mse time-major %s %s" % ((T, B, Od), act), True)
    (_, wrong), _ = O.mse_dense(y, tgt, act, 0.37, time_major=True, transpose_target=False)
    assert worst(got, wrong, w) > C_MSE


# --------------------------------------------------------------------------------------
# 3. Categorical cross-entropy on probabilities
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(O.CCE_EDGE_SHAPES)))
def test_categorical_crossentropy_clips_and_renormalisation(i):
    """cce_grad_kernel: a thread per row, two sequential passes over the C channels.  c: S is C - 1 additions, 1 / S and q one
    each: q carries C + 1 roundings, g = -t / q' one more; a term g q of the row's dot 2 C + 4, the sequential dot C - 1 on top:
    3 C + 3; g - dot one, the factor (1 / S) / n_pix and the product C + 2:  c = 4 C + 6, + 4.  Rows are unnormalised; 1e-9 under
    the target class (lower clip) and exactly one-hot rows (q = 1, upper clip 1 - 2^-23) have a zero gradient; no other q lies
    within 2 ulp of a bound."""
    from longterm360fov_amd import ops
    n_pix, C = O.CCE_EDGE_SHAPES[i]
    p, t, onehot = O.cce_edge_inputs(200 + i, n_pix, C)
    assert not O.cce_near_clip_rows(p, onehot).any()
    (loss_r, dp_r), w, _ = O.categorical_crossentropy(p, t)
    base, view = guarded(p.size)
    dp = view.view(n_pix, C)
    dp_, dt_ = dev(p), dev(t)
    _, l1 = ops.categorical_crossentropy_grad(dp_, dt_, dp=dp)
    first = dp.clone()
    _, l2 = ops.categorical_crossentropy_grad(dp_, dt_, dp=dp)
    assert same_bits(first, dp) and same_bits(l1, l2) and canaries_intact(base, view)
    tag = "cce %s" % ((n_pix, C),)
    loss_close(l2, loss_r, tag)
    within(host(dp), dp_r, w, 4 * C + 6 + 4, tag + " dp")
    assert (host(dp)[onehot] == 0).all()
    if C > 1 and n_pix >= 255:
        r = np.arange(n_pix)
        assert (host(dp)[(r % 5 == 1) & ~onehot & (r % 7 != 3)] == 0).all()


# --------------------------------------------------------------------------------------
# 4. Unit-norm regulariser
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pix", [1, 256, 257, 70000])
@pytest.mark.parametrize("C", [3, 4, 6, 33])
def test_xyz_sum1_adds_into_three_channels_only(C, n_pix):
    """xyz_sum1_kernel: a thread per row of C channels; r = x^2 + y^2 + z^2 - 1 (three squares, three additions: at most 4
    roundings of the weight x^2 + y^2 + z^2 + 1), 2 r / n_pix, * u_k, the addition into dp: c = 7 + 4.  dp holds noise before
    the call; channels >= 3 keep their bits."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(400 + C)
    p = rng.standard_normal((n_pix, C)).astype(np.float32)
    dp0 = rng.standard_normal((n_pix, C)).astype(np.float32)
    (reg_r, dp_r), w = O.xyz_sum1(p, dp0)
    base, view = guarded(p.size, fill=dp0)
    dp = view.view(n_pix, C)
    reg = ops.xyz_sum1_grad(dev(p), dp)
    first = dp.clone()
    view.copy_(dev(dp0).reshape(-1))
    reg2 = ops.xyz_sum1_grad(dev(p), dp)
    assert same_bits(first, dp) and same_bits(reg, reg2) and canaries_intact(base, view)
    tag = "xyz_sum1 n_pix %d C %d" % (n_pix, C)
    loss_close(reg, reg_r, tag)
    within(host(dp), dp_r, w, 7 + 4, tag + " dp")
    assert same_bits(dp[:, 3:], dev(dp0)[:, 3:])


# --------------------------------------------------------------------------------------
# 5. Optimizers
# --------------------------------------------------------------------------------------
def _grads(rng, n):
    g = rng.standard_normal(n)
    g[0::7] = 0.0
    g[1::7] = 1e-8 * np.sign(g[1::7])
    g[2::7] = 1e3 * np.sign(g[2::7])
    return g.astype(np.float32)


def _poisoned_guard():
    guard = torch.zeros(256, dtype=torch.uint8, device="cuda")
    guard[:4] = torch.tensor([1, 0, 0, 0], dtype=torch.uint8, device="cuda")     # what a give-up leaves behind
    return guard


# m: b1 m, 1 - b1, * g, the sum: 4 roundings; v: one more product: 5; + 4 each
C_ADAM_M, C_ADAM_V = 4 + 4, 5 + 4


def _adam_p_bound(w):
    """p - lr_t m / (sqrt(v) + eps) from the kernel's own fp32 m and v: the 4 roundings of m reach the update as 4 * upd_m; v's 5
    are halved by the root, root, sum, product and quotient add 4: 6.5 * |update|; the difference one of |p| + |update|, + 4."""
    return (4 * w["upd_m"] + 6.5 * w["upd"] + 5 * w["p"]) / w["p"]


@pytest.mark.parametrize("variant", ["aligned", "all", "p", "g", "m", "v"])
@pytest.mark.parametrize("n", [1, 3, 1023, 1024, 1025, 1026, 1027, 4099])
def test_adam_vector_kernel_tails_and_alignment(n, variant):
    """adam_kernel4 (16-byte accesses, n >= 1024 and all four buffers 16-byte aligned) with its scalar tail n % 4 != 0, and
    adam_kernel for 4-byte-aligned views: all four, or only one of them.  Steps 1, 2 and 1000 (the bias correction is formed in
    double on the host), each checked as ONE step from the GPU's own state; exact zeros, 1e-8 and 1e3 among the gradients;
    canaries on both sides of every view; `applied` rises by one per call.  At n = 4099 the reference on the exact fp64 betas
    misses the bound of v."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(500 + n)
    names = ("p", "g", "m", "v")
    init = {"p": rng.standard_normal(n), "g": np.zeros(n), "m": 0.1 * rng.standard_normal(n), "v": 0.01 * rng.random(n)}
    buf = {k: guarded(n, off=1 if variant in ("all", k) else PAD, fill=init[k]) for k in names}
    assert all((buf[k][1].data_ptr() % 16 == 0) != (variant in ("all", k)) for k in names)
    applied = torch.zeros(1, dtype=torch.int64, device="cuda")
    calls = 0
    for step in (1, 2, 1000):
        buf["g"][1].copy_(dev(_grads(rng, n)))
        state = {k: buf[k][1].clone() for k in names}
        ops.adam_step(*[buf[k][1] for k in names], step, applied=applied)
        got = {k: buf[k][1].clone() for k in names}
        for k in names:
            buf[k][1].copy_(state[k])
        ops.adam_step(*[buf[k][1] for k in names], step, applied=applied)
        calls += 2
        assert int(applied.item()) == calls
        for k in names:
            assert same_bits(got[k], buf[k][1]) and canaries_intact(*buf[k]), k
        assert same_bits(got["g"], state["g"])
        s = {k: host(state[k]) for k in names}
        (pr, mr, vr), w = O.adam_step_f32args(s["p"], s["g"], s["m"], s["v"], step)
        tag = "adam n %d %s step %d" % (n, variant, step)
        within(host(got["m"]), mr, w["m"], C_ADAM_M, tag + " m")
        within(host(got["v"]), vr, w["v"], C_ADAM_V, tag + " v")
        within(host(got["p"]), pr, w["p"], float(_adam_p_bound(w).max()), tag + " p")
        assert (np.abs(host(got["p"]) - pr) <= U * (4 * w["upd_m"] + 6.5 * w["upd"] + 5 * w["p"])).all()
        if n == 4099:
            (_, _, vx), _ = O.adam_step_f32args(s["p"], s["g"], s["m"], s["v"], step, exact_betas=True)
            assert worst(host(got["v"]), vx, w["v"]) > C_ADAM_V


@pytest.mark.parametrize("variant", ["aligned", "all"])
def test_adam_poisoned_guard_skips_the_vector_kernel_too(variant):
    """n = 1027: the vector kernel with a scalar tail (or the scalar kernel on unaligned views).  A set guard word: all four
    buffers and `applied` keep their bits; with the word clear the same call updates."""
    from longterm360fov_amd import ops
    n = 1027
    rng = np.random.default_rng(55)
    names = ("p", "g", "m", "v")
    buf = {k: guarded(n, off=1 if variant == "all" else PAD, fill=rng.standard_normal(n) ** 2) for k in names}
    before = {k: buf[k][0].clone() for k in names}
    applied = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    guard = _poisoned_guard()
    for _ in range(2):
        ops.adam_step(*[buf[k][1] for k in names], 1, guards=[guard], applied=applied)
    assert int(applied.item()) == 7
    for k in names:
        assert same_bits(before[k], buf[k][0]), k
    guard.zero_()
    ops.adam_step(*[buf[k][1] for k in names], 1, guards=[guard], applied=applied)
    assert int(applied.item()) == 8 and not same_bits(before["p"], buf["p"][0]) and all(canaries_intact(*buf[k]) for k in names)


# a: rho a, 1 - rho, * g, * g, the sum: 5 roundings, + 4.  p - lr g / (sqrt(a) + eps): a's 5 halved by the root, then root, sum (the
# TF form: sum, root), lr g and the quotient: 6.5 * |update|; the difference one of |p| + |update|, + 4
C_RMS_A = 5 + 4


def _rms_p_ok(got, ref, w, tag):
    bound = (6.5 * w["upd"] + 5 * w["p"]) / w["p"]
    within(got, ref, w["p"], float(bound.max()), tag)
    assert (np.abs(got - ref) <= U * (6.5 * w["upd"] + 5 * w["p"]) + 2.0 ** -149).all(), tag


@pytest.mark.parametrize("kind", ["keras", "tf_clip1", "tf_clip0"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_rmsprop_kernels_block_edges_clip_and_guard(n, kind):
    """rmsprop_kernel and rmsprop_tf_kernel (ms starts at ONE, eps inside the root; clip 1.0 with gradients below, exactly at
    and above +-clip, and clip 0 = no clipping), two consecutive steps each checked alone from the GPU's own state; then a
    poisoned guard word: nothing moves."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(600 + n)
    names = ("p", "g", "a")
    edge = np.array([-3.0, 1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0)), 0.5, 0.0,
                     -np.nextafter(np.float32(1), np.float32(2)), 1.5], np.float32)
    buf = {"p": guarded(n, fill=rng.standard_normal(n)), "g": guarded(n),
           "a": guarded(n, fill=np.ones(n) if kind != "keras" else 0.01 * rng.random(n))}
    applied = torch.zeros(1, dtype=torch.int64, device="cuda")
    if kind == "keras":
        run = lambda **kw: ops.rmsprop_step(buf["p"][1], buf["g"][1], buf["a"][1], lr=1e-3, rho=0.9, eps=1e-7, **kw)
        ref = lambda s: O.rmsprop_step_f32args(s["p"], s["g"], s["a"], 1e-3, 0.9, 1e-7)
    else:
        clip = 1.0 if kind == "tf_clip1" else 0.0
        run = lambda **kw: ops.rmsprop_tf_step(buf["p"][1], buf["g"][1], buf["a"][1], lr=0.1, decay=0.9, eps=1e-10, clip_value=clip, **kw)
        ref = lambda s: O.rmsprop_tf_step(s["p"], s["g"], s["a"], 0.1, 0.9, 1e-10, clip)
    for step in range(2):
        g = _grads(rng, n) if kind == "keras" else (0.7 * rng.standard_normal(n)).astype(np.float32)
        if kind != "keras":
            k = min(n, edge.size)
            g[:k] = np.roll(edge, -step)[:k]
        buf["g"][1].copy_(dev(g))
        state = {k: buf[k][1].clone() for k in names}
        run(applied=applied)
        got = {k: buf[k][1].clone() for k in names}
        for k in names:
            buf[k][1].copy_(state[k])
        run(applied=applied)
        assert int(applied.item()) == 2 * step + 2
        for k in names:
            assert same_bits(got[k], buf[k][1]) and canaries_intact(*buf[k]), k
        s = {k: host(state[k]) for k in names}
        (pr, ar), w = ref(s)
        tag = "rmsprop %s n %d step %d" % (kind, n, step)
        within(host(got["a"]), ar, w["a"], C_RMS_A, tag + " a")
        _rms_p_ok(host(got["p"]), pr, w, tag + " p")
    before = {k: buf[k][0].clone() for k in names}
    run(guards=[_poisoned_guard()], applied=applied)
    assert int(applied.item()) == 4 and all(same_bits(before[k], buf[k][0]) for k in names)


# --------------------------------------------------------------------------------------
# 6. Pointwise
# --------------------------------------------------------------------------------------
_SIZES = [1, 255, 256, 257, 70001]


def _act_inputs(act, n, rng):
    if act == "exp":
        x, sp = rng.uniform(-80, 80, n), [80.0, -80.0, 0.0, 1e-4, 79.99]
    elif act == "tanh":
        x, sp = 3 * rng.standard_normal(n), [20.0, -20.0, 1e-4, -1e-4, 0.0, 0.5, -9.0]
    else:
        x, sp = 3 * rng.standard_normal(n), [0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 2.5]
    x = x.astype(np.float32)
    k = min(n, len(sp))
    x[:k] = np.array(sp, np.float32)[:k]
    return x


@pytest.mark.parametrize("act", ["tanh", "relu", "exp", None])
@pytest.mark.parametrize("n", _SIZES)
def test_act_fwd_every_code_in_and_out_of_place(n, act):
    """act_fwd_kernel.  relu and linear are exact (0.0, -0.0 and denormals included).  tanh_f = 1 - 2 rcp(1 + exp(2x)) has an
    ABSOLUTE error: exp(2x) is good to (3 |x| + 4) 2^-23 relative and reaches the result through 2 e / (1 + e)^2 (at most 2.2 x
    2^-23 together, near x = 0.5), the reciprocal's 1 ulp twice, the sum and the difference half an ulp each: 5.2 x 2^-23 =
    6.2e-7.  __expf: relative (1.5 |x| + 4) 2^-23 from the rounding of x log2(e).  Where measured (module constants), the bound in
    force is 4 x the measured worst case, if that is tighter."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(700 + n)
    x = _act_inputs(act, n, rng)
    base, out = guarded(n)
    dx = dev(x)
    ops.act_fwd(dx, act, out=out)
    first = out.clone()
    ops.act_fwd(dx, act, out=out)
    inplace = dx.clone()
    ops.act_fwd(inplace, act, out=inplace)
    assert same_bits(first, out) and same_bits(first, inplace) and canaries_intact(base, out) and same_bits(dx, dev(x))
    got, x64 = host(out), x.astype(np.float64)
    tag = "act_fwd %s n %d" % (act, n)
    if act == "tanh":
        err = float(np.abs(got - np.tanh(x64)).max())
        bound = TANH_DERIVED if TANH_MEASURED is None else min(4 * TANH_MEASURED, TANH_DERIVED)
        print("%-46s worst absolute error %.3e, bound %.3e" % (tag, err, bound))
        assert err <= bound and (np.abs(got) <= 1).all()
    elif act == "exp":
        ref = np.exp(x64)
        frac = float((np.abs(got - ref) / (ref * (1.5 * np.abs(x64) + 4) * 2.0 ** -23)).max())
        k = 1.0 if EXP_MEASURED is None else min(4 * EXP_MEASURED, 1.0)
        print("%-46s worst error %.4f of the derived (1.5 |x| + 4) 2^-23 relative, bound %.4f" % (tag, frac, k))
        assert np.isfinite(got).all() and frac <= k
    else:
        ref = np.maximum(x64, 0) if act == "relu" else x64
        assert (got == ref).all(), tag


@pytest.mark.parametrize("mode", ["no_base", "base_is_out", "dy_is_out"])
@pytest.mark.parametrize("act", ["tanh", "relu", "exp", None])
@pytest.mark.parametrize("n", _SIZES)
def test_act_bwd_every_code_and_aliasing(n, act, mode):
    """out = base + dy * act'(y): y^2, 1 - y^2, the product and the sum are 4 roundings of |base| + |dy| (1 + y^2) (tanh; fewer for
    the others): c = 4 + 4.  relu's y > 0 at 0.0, -0.0 and denormals; out aliasing base, out aliasing dy."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(720 + n)
    x = _act_inputs(act, n, rng)
    x64 = x.astype(np.float64)
    y = {"tanh": np.tanh(x64), "relu": np.where(x64 > 0, x64, x64 * 0), "exp": np.exp(x64), None: x64}[act].astype(np.float32)
    if act == "tanh" and n > 2:
        y[-1], y[-2] = 1.0, -1.0
    dy = rng.standard_normal(n).astype(np.float32)
    bs = rng.standard_normal(n).astype(np.float32)
    y64, dy64 = y.astype(np.float64), dy.astype(np.float64)
    da = {"tanh": 1 - y64 * y64, "relu": (y64 > 0).astype(np.float64), "exp": y64, None: np.ones(n)}[act]
    wa = {"tanh": 1 + y64 * y64, "relu": np.ones(n), "exp": np.abs(y64), None: np.ones(n)}[act]
    b64 = np.zeros(n) if mode == "no_base" else bs.astype(np.float64)
    ref, w = b64 + dy64 * da, np.abs(b64) + np.abs(dy64) * wa

    def once():
        base, out = guarded(n)
        if mode == "no_base":
            ops.act_bwd(dev(dy), dev(y), None, act, out=out)
        elif mode == "base_is_out":
            out.copy_(dev(bs))
            ops.act_bwd(dev(dy), dev(y), out, act, out=out)
        else:
            out.copy_(dev(dy))
            ops.act_bwd(out, dev(y), dev(bs), act, out=out)
        assert canaries_intact(base, out)
        return out

    a, b = once(), once()
    assert same_bits(a, b)
    within(host(a), ref, w, 4 + 4, "act_bwd %s %s n %d" % (act, mode, n))


@pytest.mark.parametrize("n", _SIZES)
def test_scale_in_place(n):
    """x *= s: one correctly rounded product, half an ulp (c = 1), on a view between canaries."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(740 + n)
    x = _act_inputs("relu", n, rng)
    outs = []
    for _ in range(2):
        base, view = guarded(n, fill=x)
        assert ops.scale_(view, 0.37) is view and canaries_intact(base, view)
        outs.append(view)
    assert same_bits(*outs)
    ref = x.astype(np.float64) * O.r32(0.37)
    within(host(outs[0]), ref, np.abs(ref), 1, "scale_ n %d" % n)


# --------------------------------------------------------------------------------------
# 7. Softmax over the last axis
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plus80", "minus80", "spread100"])
@pytest.mark.parametrize("rows,n", [(1, 1), (255, 30), (257, 30), (300, 3), (5, 64), (2, 1000)])
def test_softmax_forward_and_backward_shifted_and_wide_logits(rows, n, kind):
    """A thread per row.  Logits around +80 and -80 (the row maximum is subtracted first) and with a spread of 100 (a tail that
    underflows to an exact 0 is fine): forward within 1e-6 of max|ref|, rows sum to 1 within 1e-6; backward against torch.autograd
    in fp64 within 1e-5 of max|ref|."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(800 + rows + n)
    x = rng.standard_normal((rows, n))
    x = {"plus80": x + 80, "minus80": x - 80, "spread100": rng.uniform(-50, 50, (rows, n))}[kind].astype(np.float32)
    tx = torch.tensor(x.astype(np.float64), requires_grad=True)
    ty = torch.softmax(tx, -1)
    dp = rng.standard_normal((rows, n)).astype(np.float32)
    ty.backward(torch.tensor(dp.astype(np.float64)))
    ref, dref = ty.detach().numpy(), tx.grad.numpy()
    base, view = guarded(rows * n)
    out = view.view(rows, n)
    ops.softmax_lastdim(dev(x), out=out)
    first = out.clone()
    ops.softmax_lastdim(dev(x), out=out)
    assert same_bits(first, out) and canaries_intact(base, view)
    got = host(out)
    tag = "softmax %s %s" % ((rows, n), kind)
    print("%-46s forward err %.3e of max %.3e, row sums off by %.3e" % (tag, np.abs(got - ref).max(), ref.max(), np.abs(got.sum(-1) - 1).max()))
    assert np.isfinite(got).all() and np.abs(got - ref).max() <= 1e-6 * ref.max()
    assert np.abs(got.sum(-1) - 1).max() <= 1e-6
    bbase, bview = guarded(rows * n)
    dy = bview.view(rows, n)
    p32 = dev(ref)
    ops.softmax_lastdim_bwd(dev(dp), p32, out=dy)
    first = dy.clone()
    ops.softmax_lastdim_bwd(dev(dp), p32, out=dy)
    assert same_bits(first, dy) and canaries_intact(bbase, bview)
    print("%-46s backward err %.3e of max %.3e" % (tag, np.abs(host(dy) - dref).max(), np.abs(dref).max()))
    assert np.abs(host(dy) - dref).max() <= 1e-5 * np.abs(dref).max() + 1e-300


# --------------------------------------------------------------------------------------
# 8. Sampled re-feed
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("std", ["sqrt", "var"])
@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("fps", [1, 21, 22, 30, 43])
def test_sample_refeed_lane_loop_layouts_and_window_slot(fps, B, planar, std):
    """One wave per sequence, a 64-strided loop over 3 fps = 3, 63, 66, 90, 129 elements.  Forward x = mu + sd * noise into slot t
    of a (B, T, 3 fps) window: root, product, sum: c = 3 + 4; the rest of the window keeps its bits.  Backward from the same
    slot: a lane adds trips = ceil(3 fps / 64) terms, the wave's tree 6 levels, dx * noise, the root, the quotient and the
    accumulation 4 roundings: c = trips + 6 + 4 + 4; var = 1e-6 under the sqrt convention is there (sd' = 500)."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(900 + fps + B)
    n, T, t = 3 * fps, 3, 1
    mu = rng.uniform(-1, 1, (B, 3)).astype(np.float32)
    var = rng.uniform(0.01, 1, (B, 3)).astype(np.float32)
    var[0, 0] = 1e-6
    noise = rng.standard_normal((B, n)).astype(np.float32)
    xr, wx = O.sample_refeed(mu, var, noise, std, planar)
    win0 = rng.standard_normal((B, T, n)).astype(np.float32)
    wins = []
    for _ in range(2):
        win = dev(win0)
        ops.sample_refeed(dev(mu), dev(var), dev(noise), out=win[:, t, :], std=std, planar=planar)
        wins.append(win)
    assert same_bits(*wins)
    win = wins[0]
    assert same_bits(win[:, 0], dev(win0)[:, 0]) and same_bits(win[:, 2], dev(win0)[:, 2])
    tag = "refeed fps %d B %d %s %s" % (fps, B, "planar" if planar else "interleaved", std)
    within(host(win[:, t]), xr, wx, 3 + 4, tag + " x")
    dwin = dev(rng.standard_normal((B, T, n)).astype(np.float32))
    keep = dwin.clone()
    g0 = rng.standard_normal((2, B, 3)).astype(np.float32)
    trips = -(-n // 64)
    for acc in (True, False):
        outs = []
        for _ in range(2):
            dmu, dvar = dev(g0[0]), dev(g0[1])
            ops.sample_refeed_bwd(dwin[:, t, :], dev(var), dev(noise), dmu, dvar, std=std, planar=planar, accumulate=acc)
            outs.append((dmu, dvar))
        assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]) and same_bits(dwin, keep)
        (gm, gv), (wm, wv) = O.sample_refeed_bwd(host(dwin[:, t]), var, noise, std, planar, g0[0] if acc else None, g0[1] if acc else None)
        within(host(outs[0][0]), gm, wm, trips + 6 + 4 + 4, tag + " dmu acc %d" % acc)
        within(host(outs[0][1]), gv, wv, trips + 6 + 4 + 4, tag + " dvar acc %d" % acc)


# --------------------------------------------------------------------------------------
# 9. One ticket word, three kernels
# --------------------------------------------------------------------------------------
def test_loss_ticket_shared_by_three_kernels_back_to_back():
    """mse_dense_grad_kernel, gauss_nll_kernel and dense_mse_head_kernel take the same ticket word of their stream and must leave
    it at zero: four rounds of five calls with grids of 361, 5, 5, 300 and 1 blocks back to back on one stream, every result
    bit-equal to the same call made alone (computed once, each followed by a synchronize)."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(99)
    f = lambda *s: dev(rng.uniform(-1, 1, s))
    Od = 6
    big_y, big_t = f(15402, Od), f(15402, Od)                 # 92 412 elements: 361 blocks, with the fused db
    one_y, one_t = f(40, Od), f(40, Od)                       # one block
    nll = {}
    for B in (5, 300):
        mu, var, y, _ = O.nll_edge_inputs(7 + B, B, 3, 30)
        nll[B] = (dev(mu), dev(var), dev(y))
    H, N = 128, 320
    hs, W, b, tgt = f(N, H), dev(rng.standard_normal((H, Od)) / np.sqrt(H)), f(Od), f(N, Od)

    def calls():
        db = torch.empty(Od, dtype=torch.float32, device="cuda")
        dpre, loss = ops.mse_dense_grad(big_y, big_t, "tanh", db=db)
        yield (dpre, loss.clone(), db)
        yield tuple(t.clone() for t in ops.gauss_nll_grad(*nll[5], 30, 1.0))
        dW, dbh = torch.empty(H, Od, dtype=torch.float32, device="cuda"), torch.empty(Od, dtype=torch.float32, device="cuda")
        yy, dx, loss = ops.dense_mse_head(hs, W, b, tgt, "tanh", dW=dW, db=dbh)
        yield (yy, dx, loss.clone(), dW, dbh)
        yield tuple(t.clone() for t in ops.gauss_nll_grad(*nll[300], 30, 0.37))
        dpre, loss = ops.mse_dense_grad(one_y, one_t, "linear")
        yield (dpre, loss.clone())

    alone = []
    for out in calls():
        torch.cuda.synchronize()
        alone.append(out)
    assert (-(-big_y.numel() // 256), -(-one_y.numel() // 256)) == (361, 1)
    rounds = [list(calls()) for _ in range(4)]
    torch.cuda.synchronize()
    for r, outs in enumerate(rounds):
        for k, (a, o) in enumerate(zip(alone, outs)):
            for j, (ta, to) in enumerate(zip(a, o)):
                assert same_bits(ta, to), (r, k, j)
    # and against fp64: the losses are what they should be (a ticket that is not re-zeroed leaves the loss unwritten or early)
    (lr, _), _ = O.mse_dense(host(big_y), host(big_t), "tanh")
    loss_close(alone[0][1], lr, "ticket: mse 361 blocks")
    (lr, _, _), _, _ = O.gauss_nll(*[host(a) for a in nll[300]], 30, 0.37)
    loss_close(alone[3][0], lr, "ticket: nll B 300")
