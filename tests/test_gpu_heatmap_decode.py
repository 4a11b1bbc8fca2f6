"""The heat-map decode on the device: ops.heatmap_argmax (fov_heatmap_argmax), ops.heatmap_index_xyz
(fov_heatmap_index_xyz) and ConvLSTMSeq2Seq's predict_index_device / predict_index / predict_trajectories(output=...) /
evaluate_trajectories.

Every arg-max comparison is exact, against np.argmax on the same float32 data (and against the position the test put the
maximum at); values are compared as bits with the element np.argmax points at.  Every operator call is made twice and has
to give the same bits; index outputs are views between canaries.  The one tolerance is one float32 ulp for the bin centres
(the device's fp64 sin / cos may differ from libm's in the last place) and test_gpu_parity's 2e-5 for the hit rate.

Shapes follow the kernel: a workgroup of ops.HEATMAP_ARGMAX_THREADS threads takes G = ops.heatmap_argmax_pass_pixels(C,
vector) pixels per pass, pixel p belongs to thread group p % G in pass p // G, so n_pix and the maxima sit at 1, 2, G - 1,
G, G + 1, 2G, 2G + 1 and at the model's 648 (+1)."""
import numpy as np
import pytest

from longterm360fov_amd import utility
from oracle import fov_oracle as O

pytestmark = pytest.mark.gpu

CANARY = -7777
CHANNELS = (1, 2, 3, 29, 30, 31, 32, 33, 64)


def _torch():
    import torch
    return torch


def _ops():
    from longterm360fov_amd import ops
    return ops


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def strides_for(C):
    """Pixel strides of the issue: C, C rounded up to 4, and 30 inside 32."""
    return sorted({C, C + (-C) % 4} | ({32} if C == 30 else set()))


def is_vector(C, ps, ms=0):
    return C % 2 == 0 and ps % 2 == 0 and ms % 2 == 0


def pass_pixels(C, ps, ms=0):
    return _ops().heatmap_argmax_pass_pixels(C, is_vector(C, ps, ms))


def pix_counts(G):
    return sorted({1, 2, G - 1, G, G + 1, 2 * G, 2 * G + 1, 648, 649})


def boundary_pixels(G, n_pix):
    """Pixel 0, the last pixel and both sides of every pass boundary the map has (the first three and the last)."""
    edges = [k * G for k in (1, 2, 3, (n_pix - 1) // G) if k >= 1]
    return sorted({p for p in [0, n_pix - 1] + [e - 1 for e in edges] + edges if 0 <= p < n_pix})


def pad_maps(a, ps, slack=0, fill=np.inf):
    """(n_maps, n_pix, C) host data -> (H = n_pix, W = 1) device maps with pixel stride ps and `slack` extra pixels between
    maps; the padding holds +inf, so a kernel that read it would answer wrongly."""
    torch = _torch()
    n_maps, n_pix, C = a.shape
    buf = np.full((n_maps, n_pix + slack, ps), fill, np.float32)
    buf[:, :n_pix, :C] = a
    t = torch.from_numpy(buf).cuda()
    return t[:, :n_pix, :C].unsqueeze(2)


def run_argmax(maps, values=True):
    """ops.heatmap_argmax twice into a canaried (n_maps + 2, C + 3) int32 buffer -> (index, value) as NumPy."""
    torch, ops = _torch(), _ops()
    n_maps, C = maps.shape[0], maps.shape[-1]
    got = []
    for _ in range(2):
        buf = torch.full((n_maps + 2, C + 3), CANARY, dtype=torch.int32, device="cuda")
        out = buf[1:-1, :C]
        res = ops.heatmap_argmax(maps, values=values, out=out)
        idx, val = res if values else (res, None)
        assert idx.data_ptr() == out.data_ptr()
        h = buf.cpu().numpy()
        assert (h[0] == CANARY).all() and (h[-1] == CANARY).all() and (h[:, C:] == CANARY).all(), "canary overwritten"
        got.append((h[1:-1, :C].copy(), None if val is None else val.cpu().numpy()))
    np.testing.assert_array_equal(got[0][0], got[1][0])
    if values:
        assert got[0][1].shape == (n_maps, C)
        np.testing.assert_array_equal(bits(got[0][1]), bits(got[1][1]))
    return got[0]


def check_against_numpy(a, idx, val):
    """Exactly np.argmax over the pixels, and the value is the element it points at, bit for bit."""
    ref = np.argmax(a, axis=1)
    np.testing.assert_array_equal(idx, ref)
    if val is not None:
        np.testing.assert_array_equal(bits(val), bits(np.take_along_axis(a, ref[:, None, :], axis=1)[:, 0]))
        np.testing.assert_array_equal(val, np.max(a, axis=1))     # by value: NaN == NaN, -0.0 == +0.0


@pytest.mark.parametrize("C", CHANNELS)
def test_argmax_shapes_and_strides(C):
    """Every n_pix of the pass / whole-map edges x every pixel stride x 1 and 3 maps (257 maps at two passes plus one), a map
    stride larger than the map, random data: equals np.argmax."""
    rng = np.random.default_rng(100 + C)
    for ps in strides_for(C):
        G = pass_pixels(C, ps)
        for n_pix in pix_counts(G):
            for n_maps in (1, 3) + ((257,) if n_pix == 2 * G + 1 else ()):
                a = rng.standard_normal((n_maps, n_pix, C)).astype(np.float32)
                slack = 2 if n_maps == 3 else 0
                maps = pad_maps(a, ps, slack=slack)
                assert maps.stride(1) == ps or n_pix == 1
                idx, val = run_argmax(maps)
                check_against_numpy(a, idx, val)


@pytest.mark.parametrize("C,ps", [(30, 30), (30, 32), (31, 31), (64, 64), (3, 4), (2, 2), (1, 1)])
def test_argmax_placement_at_every_boundary(C, ps):
    """The maximum at pixel 0, at the last pixel and on both sides of every pass boundary, a different placement for every
    channel of one map (and rotated from map to map)."""
    G = pass_pixels(C, ps)
    rng = np.random.default_rng(7)
    for n_pix in (2 * G + 1, 3 * G, 648):
        spots = boundary_pixels(G, n_pix)
        n_maps = len(spots)
        a = rng.uniform(0, 1, (n_maps, n_pix, C)).astype(np.float32)
        want = np.empty((n_maps, C), np.int64)
        for m in range(n_maps):
            for c in range(C):
                want[m, c] = spots[(m + c) % len(spots)]
                a[m, want[m, c], c] = 2.0
        idx, val = run_argmax(pad_maps(a, ps))
        np.testing.assert_array_equal(idx, want)
        check_against_numpy(a, idx, val)
        assert (val == 2.0).all()


@pytest.mark.parametrize("C,ps", [(30, 30), (30, 32), (31, 31), (64, 64), (3, 3)])
def test_argmax_ties_take_the_lower_pixel(C, ps):
    G = pass_pixels(C, ps)
    n_pix = 3 * G + 1
    # constant maps -> pixel 0 everywhere
    for const in (0.0, -3.5):
        a = np.full((2, n_pix, C), const, np.float32)
        idx, val = run_argmax(pad_maps(a, ps))
        assert (idx == 0).all() and (val == const).all()
    # the same maximal value at p < q owned by different thread groups (p % G) and different passes (p // G) -> p
    spots = boundary_pixels(G, n_pix)
    pairs = [(p, q) for p in spots for q in spots if p < q and p % G != q % G and p // G != q // G]
    assert any(p % G > q % G for p, q in pairs) and any(p % G < q % G for p, q in pairs)
    n_maps = -(-len(pairs) // C)
    rng = np.random.default_rng(8)
    a = rng.uniform(0, 1, (n_maps, n_pix, C)).astype(np.float32)
    want = np.empty((n_maps, C), np.int64)
    for m in range(n_maps):
        for c in range(C):
            p, q = pairs[(m * C + c) % len(pairs)]
            a[m, p, c] = a[m, q, c] = 2.0
            want[m, c] = p
    idx, val = run_argmax(pad_maps(a, ps))
    np.testing.assert_array_equal(idx, want)
    check_against_numpy(a, idx, val)
    # random maps quantised to four levels: nearly every maximum is taken more than once
    q4 = rng.integers(0, 4, (5, 648, C)).astype(np.float32)
    tied = ((q4 == q4.max(axis=1, keepdims=True)).sum(axis=1) > 1).mean()
    assert tied >= 0.9, tied
    idx, val = run_argmax(pad_maps(q4, ps))
    check_against_numpy(q4, idx, val)


@pytest.mark.parametrize("C,ps", [(30, 30), (30, 32), (31, 31), (2, 2), (1, 1)])
def test_argmax_signed_zeros_infinities_and_nans(C, ps):
    G = pass_pixels(C, ps)
    nan = np.float32(np.nan)
    for n_pix in (2 * G, 2 * G + 1):
        spots = boundary_pixels(G, n_pix)
        pairs = [(p, q) for p in spots for q in spots if p < q]
        rng = np.random.default_rng(9)
        cases, want = [], []

        def case(base, put, expect):
            a = base.copy()
            w = np.empty(C, np.int64)
            for c in range(C):
                p, q = pairs[(3 * c + len(cases)) % len(pairs)]
                put(a[:, c], p, q)
                w[c] = expect(p, q)
            cases.append(a)
            want.append(w)

        low = np.full((n_pix, C), -1.0, np.float32)
        mid = rng.uniform(1, 2, (n_pix, C)).astype(np.float32)

        def zeros_neg_first(col, p, q): col[p], col[q] = -0.0, 0.0
        def zeros_pos_first(col, p, q): col[p], col[q] = 0.0, -0.0
        def inf_twice(col, p, q): col[p] = col[q] = np.inf
        def one_nan(col, p, q): col[q] = nan
        def two_nans(col, p, q): col[p] = col[q] = nan
        def nan_last(col, p, q): col[n_pix - 1] = nan
        def nan_after_inf(col, p, q): col[p], col[q] = np.inf, nan

        case(low, zeros_neg_first, lambda p, q: p)
        case(low, zeros_pos_first, lambda p, q: p)
        case(np.full((n_pix, C), -np.inf, np.float32), lambda col, p, q: None, lambda p, q: 0)
        case(mid, inf_twice, lambda p, q: p)
        case(mid, one_nan, lambda p, q: q)                 # a NaN among larger finite values is the maximum
        case(mid, two_nans, lambda p, q: p)
        case(mid, nan_last, lambda p, q: n_pix - 1)        # the last pixel of the last pass
        case(mid, nan_after_inf, lambda p, q: q)           # a later NaN beats an earlier +inf
        a = np.stack(cases)
        idx, val = run_argmax(pad_maps(a, ps))
        np.testing.assert_array_equal(idx, np.stack(want))
        check_against_numpy(a, idx, val)
        assert np.signbit(val[0]).all() and not np.signbit(val[1]).any()     # the FIRST zero's bits


def test_argmax_view_offset_by_one_float_takes_the_scalar_form():
    """The same data at an 8-byte aligned base (8-byte loads) and one float further (scalar form): identical results."""
    torch, ops = _torch(), _ops()
    rng = np.random.default_rng(10)
    n_maps, H, W, C = 3, 36, 18, 30
    a = rng.integers(0, 6, (n_maps, H * W, C)).astype(np.float32)        # with ties
    flat = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(a.reshape(-1)).cuda()
    shifted = flat[1:].view(n_maps, H, W, C)
    assert shifted.data_ptr() % 8 == 4
    aligned = torch.from_numpy(a).cuda().view(n_maps, H, W, C)
    assert aligned.data_ptr() % 8 == 0
    i0, v0 = run_argmax(aligned)
    i1, v1 = run_argmax(shifted)
    np.testing.assert_array_equal(i0, i1)
    np.testing.assert_array_equal(bits(v0), bits(v1))
    check_against_numpy(a, i0, v0)
    # an odd map stride does the same
    buf = torch.full((n_maps, H * W * 30 + 1), float("inf"), dtype=torch.float32, device="cuda")
    buf[:, :H * W * 30] = torch.from_numpy(a.reshape(n_maps, -1)).cuda()
    odd = buf[:, :H * W * 30].view(n_maps, H, W, C)
    assert odd.stride(0) % 2 == 1
    i2, v2 = run_argmax(odd)
    np.testing.assert_array_equal(i0, i2)


def test_argmax_more_maps_than_workgroups():
    """65 536 workgroups at the most: map 65 536 and later ones are a second round of the same workgroups."""
    rng = np.random.default_rng(11)
    a = rng.integers(0, 3, (65536 + 5, 3, 2)).astype(np.float32)
    idx, val = run_argmax(pad_maps(a, 2))
    check_against_numpy(a, idx, val)


def test_argmax_outputs_strided_empty_and_collapsed():
    torch, ops = _torch(), _ops()
    rng = np.random.default_rng(12)
    N, T, H, W, C = 4, 3, 36, 18, 30
    a = rng.standard_normal((N, T, H, W, C)).astype(np.float32)
    ref = utility.heatmap_argmax(a)
    dev = torch.from_numpy(a).cuda()
    # all (N, T) maps in one call: the leading dims collapse
    whole = ops.heatmap_argmax(dev)
    assert whole.dtype == torch.int32 and tuple(whole.shape) == (N, T, C)
    np.testing.assert_array_equal(whole.cpu().numpy(), ref)
    # step t's maps (map stride T * H * W * C) into slot t of an (N, T, C) tensor: the other slots stay
    for t in range(T):
        out = torch.full((N, T, C), CANARY, dtype=torch.int32, device="cuda")
        idx, val = ops.heatmap_argmax(dev[:, t], values=True, out=out[:, t])
        h = out.cpu().numpy()
        np.testing.assert_array_equal(h[:, t], ref[:, t])
        assert (np.delete(h, t, axis=1) == CANARY).all()
        assert tuple(val.shape) == (N, C)
        np.testing.assert_array_equal(bits(val.cpu().numpy()), bits(a[:, t].reshape(N, -1, C).max(axis=1)))
    # a channel slice: pixel stride 30, 10 channels from an even and from an odd offset (vector / scalar form)
    for lo in (4, 5):
        np.testing.assert_array_equal(ops.heatmap_argmax(dev[..., lo:lo + 10]).cpu().numpy(), ref[..., lo:lo + 10])
    # no maps
    idx, val = ops.heatmap_argmax(dev[:0], values=True)
    assert tuple(idx.shape) == (0, T, C) and idx.dtype == torch.int32
    assert tuple(val.shape) == (0, T, C) and val.dtype == torch.float32
    # leading dims that do not collapse, and shapes outside the kernel's domain, raise instead of copying
    with pytest.raises(ValueError):
        ops.heatmap_argmax(torch.from_numpy(a).cuda().transpose(0, 1))
    with pytest.raises(ValueError):
        ops.heatmap_argmax(dev.permute(0, 1, 2, 4, 3))
    with pytest.raises(ops.FovError):
        ops.heatmap_argmax(torch.zeros((1, 2, 2, 65), dtype=torch.float32, device="cuda"))
    with pytest.raises(ops.FovError):
        ops.heatmap_argmax(torch.zeros((1, (1 << 20) + 1, 1, 1), dtype=torch.float32, device="cuda"))
    np.testing.assert_array_equal(ops.heatmap_argmax(dev).cpu().numpy(), ref)      # and a later valid call works


def test_argmax_value_output_between_canaries():
    """The C entry point with a value buffer of its own row stride: nothing outside the (n_maps, C) window is written."""
    torch = _torch()
    from longterm360fov_amd import _lib
    rng = np.random.default_rng(13)
    n_maps, n_pix, C, stride = 5, 70, 30, 33
    a = rng.standard_normal((n_maps, n_pix, C)).astype(np.float32)
    maps = torch.from_numpy(a).cuda()
    index = torch.full((n_maps + 2, stride), CANARY, dtype=torch.int32, device="cuda")
    value = torch.full((n_maps + 2, stride), float(CANARY), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().fov_heatmap_argmax(maps.data_ptr(), n_pix * C, C, index[1].data_ptr(), value[1].data_ptr(), stride,
                                             n_maps, n_pix, C, torch.cuda.current_stream().cuda_stream))
    hi, hv = index.cpu().numpy(), value.cpu().numpy()
    check_against_numpy(a, hi[1:-1, :C], hv[1:-1, :C])
    for h in (hi, hv):
        assert (h[0] == CANARY).all() and (h[-1] == CANARY).all() and (h[:, C:] == CANARY).all()


def test_index_xyz_all_pixels():
    torch, ops = _torch(), _ops()
    pix = np.arange(660).reshape(1, 22, 30) % 648            # all 648 pixels in the (N, T, 30) layout
    index = torch.from_numpy(pix.astype(np.int32)).cuda()
    xyz = ops.heatmap_index_xyz(index)
    again = ops.heatmap_index_xyz(index)
    assert xyz.dtype == torch.float32 and tuple(xyz.shape) == (1, 22, 30, 3)
    got = xyz.cpu().numpy()
    np.testing.assert_array_equal(bits(got), bits(again.cpu().numpy()))
    ref = utility.bin_centre_xyz(pix).astype(np.float32)
    assert (np.abs(got - ref) <= np.spacing(np.abs(ref))).all(), np.abs(got - ref).max()
    ti, pi = ops.theta_phi_index(xyz)                        # exact round trip through the binning kernel
    np.testing.assert_array_equal(ti.cpu().numpy(), pix // 18)
    np.testing.assert_array_equal(pi.cpu().numpy(), pix % 18)
    for bad in (-1, 648):
        broken = index.clone()
        broken[0, 3, 7] = bad
        with pytest.raises(ValueError):
            ops.heatmap_index_xyz(broken)
        np.testing.assert_array_equal(bits(ops.heatmap_index_xyz(index).cpu().numpy()), bits(got))   # a later valid call
    assert tuple(ops.heatmap_index_xyz(index[:0]).shape) == (0, 22, 30, 3)


# ---- the model ----
B, T_IN, T_OUT = 3, 2, 2


def unit_xyz(seed, *lead):
    v = np.random.default_rng(seed).standard_normal(lead + (30, 3))
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def reference_line(decoded, fps):
    """mycode/convlstm_seq2seq.py:537-542."""
    return np.argmax(decoded.reshape(decoded.shape[0], decoded.shape[1], -1, fps), axis=-2)


@pytest.mark.parametrize("kw", [{}, {"dtype": "bf16"}, {"dtype": "bf16", "cell_dtype": "bf16"}],
                         ids=["f32", "bf16-head", "bf16-head-cells"])
def test_model_decodes_on_the_device(kw):
    torch, ops = _torch(), _ops()
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    w = O.init_convlstm_seq2seq(21, C=30, latent_dim=8, k=3, head="conv2d", head_filters=(16, 16))
    m = ConvLSTMSeq2Seq(w, head="conv2d", **kw)
    enc_xyz, tgt_xyz = unit_xyz(31, B, T_IN), unit_xyz(32, B, T_OUT)
    dec_xyz = enc_xyz[:, -1:]
    e32 = ops.one_hot_maps(torch.from_numpy(enc_xyz).cuda(), channels=32)
    d32 = ops.one_hot_maps(torch.from_numpy(dec_xyz).cuda(), channels=32)
    before = m.predict_device(e32, d32, T_OUT).cpu().numpy()
    index = m.predict_index_device(e32, d32, T_OUT)
    assert index.dtype == torch.int32 and tuple(index.shape) == (B, T_OUT, 30)
    index2, value = m.predict_index_device(e32, d32, T_OUT, values=True)
    np.testing.assert_array_equal(index.cpu().numpy(), index2.cpu().numpy())
    maps_dev = m.predict_device(e32, d32, T_OUT)
    maps = maps_dev.cpu().numpy()
    np.testing.assert_array_equal(bits(maps), bits(before))          # the shared step runner changed nothing
    np.testing.assert_array_equal(index.cpu().numpy(), ops.heatmap_argmax(maps_dev).cpu().numpy())
    np.testing.assert_array_equal(index.cpu().numpy(), reference_line(maps, 30))
    np.testing.assert_array_equal(bits(value.cpu().numpy()), bits(maps.reshape(B, T_OUT, -1, 30).max(axis=-2)))
    # host maps in, NumPy out: the reference's line on predict(x)
    ti, pi = utility.theta_phi_index_for_onehot(enc_xyz)
    host_maps = utility.create_one_hot(ti, pi).transpose(0, 1, 3, 4, 2).astype(np.float32)
    x = [host_maps, host_maps[:, -1:]]
    whole = m.predict_index(x, predict_step=T_OUT)
    assert whole.dtype == np.int64 and whole.shape == (B, T_OUT, 30)
    np.testing.assert_array_equal(whole, reference_line(m.predict(x, predict_step=T_OUT), 30))
    chunked = m.predict_index(x, batch_size=2, predict_step=T_OUT)
    assert chunked.dtype == np.int64
    np.testing.assert_array_equal(chunked, whole)
    empty = m.predict_index([host_maps[:0], host_maps[:0, -1:]], predict_step=T_OUT)
    assert empty.shape == (0, T_OUT, 30) and empty.dtype == np.int64
    # frame centres in
    tmaps = m.predict_trajectories(enc_xyz, dec_xyz, predict_step=T_OUT)
    np.testing.assert_array_equal(bits(tmaps), bits(maps))
    tindex = m.predict_trajectories(enc_xyz, dec_xyz, predict_step=T_OUT, output="index", batch_size=2)
    assert tindex.dtype == np.int64
    np.testing.assert_array_equal(tindex, reference_line(tmaps, 30))
    txyz = m.predict_trajectories(enc_xyz, dec_xyz, predict_step=T_OUT, output="xyz")
    assert txyz.dtype == np.float32 and txyz.shape == (B, T_OUT, 30, 3)
    centres = utility.bin_centre_xyz(tindex).astype(np.float32)
    assert (np.abs(txyz - centres) <= np.spacing(np.abs(centres))).all()
    with pytest.raises(ValueError):
        m.predict_trajectories(enc_xyz, dec_xyz, predict_step=T_OUT, output="bogus")
    # evaluation: the same two quantities in NumPy from the maps
    gi, gp = utility.theta_phi_index_for_onehot(tgt_xyz)
    accuracy = float((tindex == (gi * 18 + gp).astype(np.int64)).sum()) / tindex.size
    rate = O.fov_hit_rate(txyz.astype(np.float64), tgt_xyz.astype(np.float64)).mean(axis=-1)
    for bs in (None, 2):
        ev = m.evaluate_trajectories(enc_xyz, dec_xyz, tgt_xyz, batch_size=bs, predict_step=T_OUT)
        assert ev["index_accuracy"] == accuracy
        assert ev["hit_rate"].shape == (B, T_OUT) and ev["hit_rate"].dtype == np.float32
        assert np.abs(ev["hit_rate"] - rate).max() < 2e-5, np.abs(ev["hit_rate"] - rate).max()
    # a target that IS the prediction scores 1 on both
    ev = m.evaluate_trajectories(enc_xyz, dec_xyz, txyz, predict_step=T_OUT)
    assert ev["index_accuracy"] == 1.0 and np.abs(ev["hit_rate"] - 1.0).max() < 2e-5


def test_conv1d_head_decodes_and_dense_head_raises():
    from longterm360fov_amd.models import ConvLSTMSeq2Seq
    w = O.init_convlstm_seq2seq(9, C=3, latent_dim=8, head="conv1d", head_filters=(16, 24))
    m = ConvLSTMSeq2Seq(w, head="conv1d")
    x = unit_xyz(41, B, T_IN).reshape(B, T_IN, 1, 30, 3)
    inputs = [x, x[:, -1:]]
    index = m.predict_index(inputs, predict_step=T_OUT)
    assert index.shape == (B, T_OUT, 3) and index.dtype == np.int64
    np.testing.assert_array_equal(index, reference_line(m.predict(inputs, predict_step=T_OUT), 3))
    d = ConvLSTMSeq2Seq(O.init_convlstm_seq2seq(77, C=6, latent_dim=8, k=3, head="dense", map_hw=(1, 1)), head="dense")
    e = np.zeros((B, T_IN, 1, 1, 6), np.float32)
    with pytest.raises(ValueError):
        d.predict_index([e, e[:, -1:]], predict_step=T_OUT)
    assert d.predict([e, e[:, -1:]], predict_step=T_OUT).shape == (B, T_OUT, 6)
