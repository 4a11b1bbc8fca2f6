"""The 3-D mixture-density head at its chunk, tie and value edges: the references, the case tables of tests/test_gpu_gmm_head.py and
the proof, without a GPU, that the cases are sharp.

gmm3d_reference   costfunc.mixture_3d_gaussian_loss and its gradient at the head's pre-activations in NumPy fp64, written out: the
                  covariance with the eigenvalue repair, its inverse by cofactors, the densities, the ten sums per component (d/dmu 3,
                  d/dSigma' 6, d/dpi 1) and the chain to the pre-activations.  Its parameters are the fp32 values the kernel receives,
                  promoted: what is left between it and the kernel is the kernel's own arithmetic and its fp32 stores.
gmm3d_autograd    the same quantities on torch.autograd fp64 with the parameters as leaves (eigvalsh, inv, logdet).
spread(case)      the worst |difference| of the two on dpre: the reference's own error, which the GPU bound carries with a margin of 16.
sample_reference  the sampler: a SEQUENTIAL fp32 running sum of pi, the first m with cum[m] > u clamped to n - 1, mu_m + L_m z in fp64.

mistake=          references that are WRONG ON PURPOSE, each one plausible slip of a kernel: the gradient sums restarted at every
                  chunk, the entries kept in LDS restarted, the loss over the first 256 rows only, y rows 3 P apart, the repair's
                  gradient lost, no floor in the weight, the softmax backward without its dot; for the sampler >= for >, a double
                  running sum, no clamp.  Each must miss the bound of the GPU test by MARGIN on the cases named and be the same
                  bits as the truth on its control - or the case's inputs are too tame.

Shapes: the smallest at which each seam of gmm3d_loss_grad_kernel exists (tc = min(6144 / (10 n), P) frames per chunk of the sums;
entries 10 m + c >= 256 live in LDS between chunks; the last workgroup adds the rows' parts 256 at a time).  Value regimes: frames
at the 1e-20 floor and at S == 0, sigmas of e^-7, correlations of 1 - 2^-k, dead and denormal-small weights, rows whose parts
cancel.  Every regime's conditions are asserted here on the reference."""
import functools

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O
from test_guarded_views_host import MARGIN, f64, same_bits, seed_of

FLOOR = 1e-20
LOG_2PI = float(np.log(2 * np.pi))
LDS_ENTRY = 256                     # entry e = 10 m + c of the ten sums: thread e's register below, LDS from here on
ROW_TRIP = 256                      # rows the last workgroup adds per trip
MISTAKES = ("chunk restart", "spilled entries", "first 256 rows", "row stride", "no repair gradient", "no floor in the weight",
            "softmax without the dot")
SAMPLER_MISTAKES = ("ties go left", "fp64 cumsum", "no clamp")


def chunk_frames(n, P):
    """Frames per chunk of the gradient sums, as fov_gmm3d_loss_grad sets it."""
    return min(6144 // (10 * n), P)


def split_params(params, n):
    """(B, 10 n) [pi n | mu 3 n | sigma 3 n | rho 3 n], component m at 3 m .. 3 m + 2 of its block -> pi (B, n) and three (B, n, 3)."""
    B = params.shape[0]
    return params[:, :n], params[:, n:4 * n].reshape(B, n, 3), params[:, 4 * n:7 * n].reshape(B, n, 3), params[:, 7 * n:].reshape(B, n, 3)


def join_params(pi, mu, sig, rho):
    B = pi.shape[0]
    return np.concatenate([pi, mu.reshape(B, -1), sig.reshape(B, -1), rho.reshape(B, -1)], 1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the loss and its gradient
# ---------------------------------------------------------------------------------------------------------------------
def gmm3d_reference(pi, mu, sig, rho, pts, scale, weight_by_pi, ldy_rows=None, mistake=None):
    """pi (B, n), mu / sig / rho (B, n, 3) (rho: 12, 13, 23), pts (B, P, 3); ldy_rows: the (B, ldy) buffer the kernel is given, from
    which the frames are then taken (row b at b * ldy; `row stride`: at b * 3 P).  -> dict: part (B,), loss, dpre (B, 10 n), S (B, P),
    eig2 (B, n, 2) the two smallest eigenvalues of every covariance before the repair, repaired (B, n), terms (B, P) the largest |term|
    a frame adds to any of the ten sums."""
    assert mistake is None or mistake in MISTAKES
    pi, mu, sig, rho, scale = f64(pi), f64(mu), f64(sig), f64(rho), float(scale)
    B, n = pi.shape
    P = pts.shape[1]
    if ldy_rows is not None:
        rows = f64(ldy_rows)
        flat, stride = rows.reshape(-1), (3 * P if mistake == "row stride" else rows.shape[1])
        pts = np.stack([flat[b * stride:b * stride + 3 * P] for b in range(B)]).reshape(B, P, 3)
    pts = f64(pts)
    s1, s2, s3 = sig[..., 0], sig[..., 1], sig[..., 2]
    r12, r13, r23 = rho[..., 0], rho[..., 1], rho[..., 2]
    a00, a01, a02, a11, a12, a22 = s1 * s1, r12 * s1 * s2, r13 * s1 * s3, s2 * s2, r23 * s2 * s3, s3 * s3
    lam, V = np.linalg.eigh(np.stack([np.stack([a00, a01, a02], -1), np.stack([a01, a11, a12], -1), np.stack([a02, a12, a22], -1)], -2))
    repaired = lam[..., 0] < 0
    shift = np.where(repaired, -10.0 * lam[..., 0], 0.0)          # cost.py:335-348: Sigma' = Sigma - 10 lambda_min I
    v = V[..., :, 0]
    a00, a11, a22 = a00 + shift, a11 + shift, a22 + shift
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    det = a00 * c00 + a01 * c01 + a02 * c02
    Pm = [c00 / det, c01 / det, c02 / det, (a00 * a22 - a02 * a02) / det, (a01 * a02 - a00 * a12) / det, (a00 * a11 - a01 * a01) / det]
    Pm = [p[:, :, None] for p in Pm]                              # 00 01 02 11 12 22
    lognorm = -0.5 * (3.0 * LOG_2PI + np.log(det))
    d = pts[:, None, :, :] - mu[:, :, None, :]                    # (B, n, P, 3)
    d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
    b0 = Pm[0] * d0 + Pm[1] * d1 + Pm[2] * d2
    b1 = Pm[1] * d0 + Pm[3] * d1 + Pm[4] * d2
    b2 = Pm[2] * d0 + Pm[4] * d1 + Pm[5] * d2
    p = np.exp(lognorm[:, :, None] - 0.5 * (d0 * b0 + d1 * b1 + d2 * b2))
    w = pi[:, :, None] if weight_by_pi else np.ones((B, n, 1))
    S = (w * p).sum(1)
    part = -np.log(S + FLOOR).sum(1)
    loss = scale * (part[:ROW_TRIP] if mistake == "first 256 rows" else part).sum()
    wt = -scale / (S + FLOOR)
    if mistake == "no floor in the weight":
        wt = np.where(S > 0, -scale / np.where(S > 0, S, 1.0), wt)
    wp = wt[:, None, :] * w * p
    h = 0.5 * wp
    terms = np.stack([wp * b0, wp * b1, wp * b2, h * (b0 * b0 - Pm[0]), h * (b0 * b1 - Pm[1]), h * (b0 * b2 - Pm[2]), h * (b1 * b1 - Pm[3]),
                      h * (b1 * b2 - Pm[4]), h * (b2 * b2 - Pm[5]), wt[:, None, :] * p], -1)             # (B, n, P, 10)
    tc = chunk_frames(n, P)
    last = ((P - 1) // tc) * tc                                   # first frame of the last chunk
    acc = terms[:, :, (last if mistake == "chunk restart" else 0):].sum(2)
    if mistake == "spilled entries":
        spilled = (10 * np.arange(n)[:, None] + np.arange(10)[None, :]) >= LDS_ENTRY
        acc = np.where(spilled[None], terms[:, :, last:].sum(2), acc)
    G = [acc[..., 3 + k] for k in range(6)]
    if mistake != "no repair gradient":                           # d lambda_min / d Sigma = v v^T
        k = np.where(repaired, -10.0 * (G[0] + G[3] + G[5]), 0.0)
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        G = [G[i] + k * v[..., a] * v[..., b] for i, (a, b) in enumerate(pairs)]
    ds1 = 2.0 * (s1 * G[0] + r12 * s2 * G[1] + r13 * s3 * G[2])
    ds2 = 2.0 * (s2 * G[3] + r12 * s1 * G[1] + r23 * s3 * G[4])
    ds3 = 2.0 * (s3 * G[5] + r13 * s1 * G[2] + r23 * s2 * G[4])
    dsig = np.stack([ds1 * s1, ds2 * s2, ds3 * s3], -1)
    drho = np.stack([2.0 * G[1] * s1 * s2 * (1.0 - r12 * r12), 2.0 * G[2] * s1 * s3 * (1.0 - r13 * r13), 2.0 * G[4] * s2 * s3 * (1.0 - r23 * r23)], -1)
    dpi = np.zeros((B, n))
    if weight_by_pi:
        dot = 0.0 if mistake == "softmax without the dot" else (pi * acc[..., 9]).sum(1, keepdims=True)
        dpi = pi * (acc[..., 9] - dot)
    dpre = np.concatenate([dpi, acc[..., :3].reshape(B, -1), dsig.reshape(B, -1), drho.reshape(B, -1)], 1)
    return dict(part=part, loss=loss, dpre=dpre, S=S, eig2=lam[..., :2], repaired=repaired, terms=np.abs(terms).max((1, 3)))


def gmm3d_autograd(pi, mu, sig, rho, pts, scale, weight_by_pi):
    """The same on torch.autograd fp64, the parameters as leaves; the chain to the pre-activations (d sigma * sigma, d rho (1 - rho^2),
    pi (d pi - sum pi d pi), d mu) is applied to the leaves' gradients."""
    t = lambda a: torch.tensor(f64(a), dtype=torch.float64, requires_grad=True)
    tpi, tmu, tsig, trho = t(pi), t(mu), t(sig), t(rho)
    y = torch.tensor(f64(pts), dtype=torch.float64)
    s1, s2, s3 = tsig.unbind(-1)
    r12, r13, r23 = trho.unbind(-1)
    S = torch.stack([torch.stack([s1 * s1, r12 * s1 * s2, r13 * s1 * s3], -1), torch.stack([r12 * s1 * s2, s2 * s2, r23 * s2 * s3], -1),
                     torch.stack([r13 * s1 * s3, r23 * s2 * s3, s3 * s3], -1)], -2)
    lam = torch.linalg.eigvalsh(S)[..., 0]
    S2 = S + torch.where(lam < 0, -10.0 * lam, torch.zeros_like(lam))[..., None, None] * torch.eye(3, dtype=torch.float64)
    Pm, logdet = torch.linalg.inv(S2), torch.logdet(S2)
    d = y[:, None, :, :] - tmu[:, :, None, :]
    q = torch.einsum("bnpi,bnij,bnpj->bnp", d, Pm, d)
    p = torch.exp(-0.5 * q - 0.5 * (3.0 * LOG_2PI + logdet)[:, :, None])
    if weight_by_pi:
        p = p * tpi[:, :, None]
    St = p.sum(1)
    part = -torch.log(St + FLOOR).sum(1)
    loss = float(scale) * part.sum()
    loss.backward()
    B, n = pi.shape
    dpi = np.zeros((B, n))
    if weight_by_pi:
        g, pv = tpi.grad.numpy(), f64(pi)
        dpi = pv * (g - (pv * g).sum(1, keepdims=True))
    dsig, drho = tsig.grad.numpy() * f64(sig), trho.grad.numpy() * (1.0 - f64(rho) ** 2)
    dpre = np.concatenate([dpi, tmu.grad.numpy().reshape(B, -1), dsig.reshape(B, -1), drho.reshape(B, -1)], 1)
    return dict(part=part.detach().numpy(), loss=float(loss.detach()), dpre=dpre, S=St.detach().numpy())


def dpre_bound(ref, spread):
    """Per element: one fp32 store with a factor two; the measured disagreement of the two fp64 references with a margin of 16 (the
    device's fp64 exp, log, sqrt and division are not correctly rounded); 1e-12 of the largest element."""
    ref = f64(ref)
    return 2.0 ** -23 * np.abs(ref) + 16.0 * spread + 1e-12 * np.abs(ref).max()


def loss_bound(part, loss, scale):
    """part[b] is stored as fp32, then summed in double and stored as fp32."""
    return 2.0 ** -23 * abs(float(scale)) * float(np.abs(part).sum()) + 2.0 ** -23 * abs(float(loss))


def over_bound(got, ref, spread):
    return float((np.abs(f64(got) - f64(ref)) / dpre_bound(ref, spread)).max())


# ---------------------------------------------------------------------------------------------------------------------
# cases.  A case: name, n, P, B, weight_by_pi, ldy, scale (an fp32 value), params (B, 10 n) fp32, y (B, ldy) fp32
# ---------------------------------------------------------------------------------------------------------------------
# (n_mix, n_pts, B): the seam
SHAPES = [(20, 29, 3), (20, 30, 3), (20, 31, 3), (20, 61, 3),       # tc clamps to P / one full chunk / a second chunk of one frame / three chunks
          (25, 25, 2),                                             # 250 entries: the last register entry, nothing in LDS; chunks 24 + 1
          (26, 24, 2), (26, 47, 2),                                # entries 256 .. 259 in LDS; chunks 23 + 1 and 23 + 23 + 1
          (32, 20, 3),                                             # tc 19, 64 entries in LDS, more than one row
          (1, 1, 2), (1, 256, 2),                                  # one component, one frame; n P = 256: exactly one trip of the density loop
          (3, 86, 2),                                              # n P = 258: a second trip with two entries
          (2, 3, 1), (2, 3, 256), (2, 3, 257), (2, 3, 300)]        # the last workgroup's row sum: one trip, a full trip, a second trip
REGIMES = ("floor", "needle", "saturated", "dead weights", "mixed rows")
# a regime without a repaired covariance (the control of `no repair gradient`) and one whose frames all sit off the floor
NOTHING_REPAIRED, OFF_THE_FLOOR = "floor-pi0", "needle-pi0"


def shape_cases():
    return ["n%d-P%d-B%d-pi%d-ld%d" % (n, P, B, w, pad) for n, P, B in SHAPES for w in (0, 1) for pad in (0, 1)]


def regime_cases():
    return ["%s-pi%d" % (r, w) for r in REGIMES for w in (0, 1)]


def all_cases():
    return shape_cases() + regime_cases()


def _softmax32(logits):
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def _finish(name, pi, mu, sig, rho, pts, w, pad, scale=None):
    B, P = pts.shape[:2]
    y = np.concatenate([pts.reshape(B, -1), np.random.default_rng(seed_of(name + " pad")).uniform(-1, 1, (B, pad))], 1).astype(np.float32)
    scale = float(np.float32(1.0 / (B * P) if scale is None else scale))
    return dict(name=name, n=pi.shape[1], P=P, B=B, weight_by_pi=bool(w), ldy=3 * P + pad, scale=scale, params=join_params(pi, mu, sig, rho), y=y)


def _moderate(rng, B, n):
    """Moderate values: pi a softmax of 0.6 N, means in the unit box, log sigma near -1, rho = tanh(0.6 N); component (b + m) % 5 == 0
    has correlations of +-tanh(2) with a negative product of signs: indefinite, so repaired."""
    pi = _softmax32(0.6 * rng.standard_normal((B, n)))
    mu, sig = rng.uniform(-1, 1, (B, n, 3)), np.exp(-1.0 + 0.3 * rng.standard_normal((B, n, 3)))
    rho = np.tanh(0.6 * rng.standard_normal((B, n, 3)))
    bad = (np.arange(B)[:, None] + np.arange(n)[None, :]) % 5 == 0
    signs = np.array([[1.0, 1.0, -1.0], [1.0, -1.0, 1.0], [-1.0, 1.0, 1.0], [-1.0, -1.0, -1.0]])[rng.integers(0, 4, (B, n))]
    rho = np.where(bad[..., None], np.tanh(2.0) * signs, rho)
    return pi, mu, sig, rho


def _shape_case(name, n, P, B, w, pad):
    rng = np.random.default_rng(seed_of("gmm shape n%d P%d B%d" % (n, P, B)))
    pi, mu, sig, rho = _moderate(rng, B, n)
    return _finish(name, pi, mu, sig, rho, rng.uniform(-1, 1, (B, P, 3)), w, pad)


def _unit(rng, shape):
    g = rng.standard_normal(shape + (3,))
    return g / np.linalg.norm(g, axis=-1, keepdims=True)


def _floor_rows(rng, B, n, P, dist):
    """Isotropic sigma of about 0.1, means 3 apart on x; frame (b, t) lies dist[b, t] sigmas from the mean of component (b + t) % n:
    in a random direction, or (40 sigmas and more) straight off the line of means."""
    sig = np.repeat((0.1 * (1.0 + 0.03 * (np.arange(n) - (n - 1) / 2.0)))[None, :, None], 3, 2).astype(np.float32).astype(np.float64)
    sig = np.repeat(sig, B, 0)
    mu = np.zeros((B, n, 3))
    mu[:, :, 0] = 3.0 * np.arange(n)
    mu = (mu + 0.05 * rng.uniform(-1, 1, (B, n, 3))).astype(np.float32).astype(np.float64)
    m = (np.arange(B)[:, None] + np.arange(P)[None, :]) % n
    u = np.where((dist >= 40.0)[..., None], np.array([0.0, 1.0, 0.0]), _unit(rng, (B, P)))
    rows = np.arange(B)[:, None]
    pts = mu[rows, m] + (dist * sig[rows, m, 0])[..., None] * u
    return _softmax32(0.6 * rng.standard_normal((B, n))), mu, sig, np.zeros((B, n, 3)), pts, m


def _needle_rows(rng, B, n, P, near):
    """log sigma in [-7, -5] (component 0: -7 on every axis), small correlations.  The first near[b] frames of row b lie within two
    sigmas of a mean - all of row 0's on the same side of component 0, so that its d/dmu adds up; the rest at 0.45 and more from
    every mean (60 sigmas at least: a density of exactly zero)."""
    logs = rng.uniform(-7.0, -5.0, (B, n, 3))
    logs[:, 0] = -7.0
    sig, rho = np.exp(logs).astype(np.float32).astype(np.float64), 0.3 * np.tanh(rng.standard_normal((B, n, 3)))
    while True:
        mu = rng.uniform(-1, 1, (B, n, 3)).astype(np.float32).astype(np.float64)
        if min(np.linalg.norm(mu[b, i] - mu[b, j]) for b in range(B) for i in range(n) for j in range(i)) > 0.3 if n > 1 else True:
            break
    pts = np.empty((B, P, 3))
    for b in range(B):
        for t in range(P):
            if t < near[b]:
                m = 0 if b == 0 else int(rng.integers(0, n))
                off = np.array([rng.uniform(1.5, 2.0), 0.0, 0.0]) if b == 0 else _unit(rng, ()) * rng.uniform(0.3, 1.9)
                pts[b, t] = mu[b, m] + sig[b, m] * off
            else:
                while True:
                    c = rng.uniform(-1, 1, 3)
                    if np.linalg.norm(mu[b] - c, axis=-1).min() >= 0.45:
                        break
                pts[b, t] = c
    return _softmax32(0.6 * rng.standard_normal((B, n))), mu, sig, rho, pts


SATURATED_SEED = 3


def _saturated_params(seed, B=4, n=6):
    """|rho| = 1 - 2^-k, k in 6 .. 10, random signs; log sigma uniform in [-4, -1], distinct per axis."""
    rng = np.random.default_rng([seed_of("gmm saturated"), seed])
    rho = (1.0 - 2.0 ** -rng.integers(6, 11, (B, n, 3))) * rng.choice([-1.0, 1.0], (B, n, 3))
    sig = np.exp(rng.uniform(-4.0, -1.0, (B, n, 3))).astype(np.float32).astype(np.float64)
    return rng, _softmax32(0.6 * rng.standard_normal((B, n))), rng.uniform(-1, 1, (B, n, 3)), sig, rho


def _regime_case(name, regime, w):
    rng = np.random.default_rng(seed_of("gmm regime " + regime))
    if regime == "floor":
        B, n, P = 6, 3, 9
        dist = np.concatenate([[45.0, 60.0, 90.0], [1.0, 2.0, 3.0], np.linspace(8.5, 11.5, B * P - 6)])
        pi, mu, sig, rho, pts, _ = _floor_rows(rng, B, n, P, rng.permutation(dist).reshape(B, P))
    elif regime == "needle":
        B, n, P = 6, 4, 9
        pi, mu, sig, rho, pts = _needle_rows(rng, B, n, P, [9, 5, 2, 1, 1, 0])
    elif regime == "saturated":
        B, n, P = 4, 6, 9
        rng, pi, mu, sig, rho = _saturated_params(SATURATED_SEED, B, n)
        L = np.linalg.cholesky(O.gmm3d_covariance(sig, rho))
        m = np.arange(P) % n
        pts = mu[:, m] + 1.2 * np.einsum("bpij,bpj->bpi", L[:, m], np.clip(rng.standard_normal((B, P, 3)), -2, 2))
    elif regime == "dead weights":
        B, n, P = 4, 6, 9
        pi, mu, sig, rho = _moderate(rng, B, n)
        pi = pi.copy()
        pi[0] = [0.0, 1e-30, 0.97, 0.01, 0.02, 0.0]
        pi[1] = [0.3, 0.0, 0.0, 0.7, 0.0, 1e-30]
        pi[2] = [1.0 - 2.0 ** -20, 1e-30, 0.0, 2.0 ** -20, 0.0, 0.0]
        pts = rng.uniform(-1, 1, (B, P, 3))
    elif regime == "mixed rows":
        return _mixed_rows(name, rng, w)
    return _finish(name, pi, mu, sig, rho, pts, w, 0)


def _mixed_rows(name, rng, w):
    """Five rows of `needle` (every frame near a mean: parts of about -140), two of `floor` (about +370 and, with four frames near
    a mean, +190) and one more row of `floor` whose nine frames sit at the one distance from component 0 at which the eight parts
    add up to nothing: the loss is the small remainder of large parts."""
    n, P = 3, 9
    pn = _needle_rows(rng, 5, n, P, [9] * 5)
    dist = np.stack([rng.permutation(np.linspace(8.5, 11.5, P)), rng.permutation(np.concatenate([[1.0, 2.0, 2.5, 3.0], np.linspace(8.5, 11.5, P - 4)])),
                     np.zeros(P)])
    pf = _floor_rows(rng, 3, n, P, dist)
    pi, mu, sig, rho, pts = (np.concatenate([a, b], 0) for a, b in zip(pn, pf[:5]))
    pts = pts.astype(np.float32)
    rest = gmm3d_reference(pi, mu, sig, rho, pts, 1.0, bool(w))["part"][:7].sum()
    # the tuner row: nine frames d sigmas from the mean of component 0, each adding -log w_0 - lognorm_0 + d^2 / 2
    s0, w0 = sig[7, 0, 0], (float(pi[7, 0]) if w else 1.0)
    d2 = 2.0 * (-rest / P + np.log(w0) - 1.5 * LOG_2PI - 3.0 * np.log(s0))
    assert 0.0 < d2 < 81.0, (rest, d2)
    pts[7] = mu[7, 0] + np.sqrt(d2) * s0 * _unit(rng, (P,))
    return _finish(name, pi, mu, sig, rho, pts, w, 0, scale=1.0 / 64)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in shape_cases():
        n, P, B, w, pad = (int(f.lstrip("nPBpild")) for f in name.split("-"))
        return _shape_case(name, n, P, B, w, pad)
    regime, w = name.rsplit("-pi", 1)
    return _regime_case(name, regime, int(w))


def case_operands(c):
    """-> pi, mu, sig, rho of the case's fp32 parameters and the frames (B, P, 3) its y rows start with."""
    return split_params(c["params"], c["n"]) + (c["y"][:, :3 * c["P"]].reshape(c["B"], c["P"], 3),)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (gmm3d_reference of the case, spread(case)): computed once, shared by every test, never written to."""
    c = case(name)
    pi, mu, sig, rho, pts = case_operands(c)
    ref = gmm3d_reference(pi, mu, sig, rho, pts, c["scale"], c["weight_by_pi"], ldy_rows=c["y"])
    auto = gmm3d_autograd(pi, mu, sig, rho, pts, c["scale"], c["weight_by_pi"])
    for k in ("part", "loss", "S"):
        # the loss is a sum of parts of either sign: 1e-9 of what is added, not of what is left
        np.testing.assert_allclose(auto[k], ref[k], rtol=1e-9, atol=1e-9 * c["scale"] * np.abs(ref["part"]).sum() if k == "loss" else 1e-300,
                                   err_msg="%s %s" % (name, k))
    spread = float(np.abs(auto["dpre"] - ref["dpre"]).max())
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref, spread


def wrong(name, mistake):
    c = case(name)
    pi, mu, sig, rho, pts = case_operands(c)
    return gmm3d_reference(pi, mu, sig, rho, pts, c["scale"], c["weight_by_pi"], ldy_rows=c["y"], mistake=mistake)


# ---------------------------------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------------------------------
def sample_reference(params_f32, u, z, mistake=None):
    """params (B, 10 n) fp32, u (B, P) fp32, z (B, P, 3) fp32 -> (component (B, P), draw (B, P, 3) fp64).  The running sum is the
    kernel's: fp32, one addition after the other."""
    assert mistake is None or mistake in SAMPLER_MISTAKES
    params_f32, u = np.asarray(params_f32, np.float32), np.asarray(u, np.float32)
    n = params_f32.shape[1] // 10
    pi, mu, sig, rho = split_params(params_f32, n)
    B, P = u.shape
    cum = np.cumsum(pi.astype(np.float64), 1) if mistake == "fp64 cumsum" else np.cumsum(pi, 1, dtype=np.float32)
    L = np.linalg.cholesky(O.gmm3d_covariance(f64(sig), f64(rho)))
    comp, out = np.empty((B, P), np.int64), np.empty((B, P, 3))
    for b in range(B):
        for f in range(P):
            hit = (cum[b] >= u[b, f]) if mistake == "ties go left" else (cum[b] > u[b, f])
            m = int(np.argmax(hit)) if hit.any() else n
            m = (0 if mistake == "no clamp" else n - 1) if m >= n else m
            comp[b, f] = m
            out[b, f] = f64(mu[b, m]) + L[b, m] @ f64(z[b, f])
    return comp, out


def sample_bound(ref):
    return 2.0 ** -22 * np.abs(ref) + 1e-7


def near_a_tie(params_f32, u, tol=1e-6):
    """(B, P): u within tol of a cumulative weight."""
    n = params_f32.shape[1] // 10
    cum = np.cumsum(f64(params_f32[:, :n]), 1)
    return (np.abs(cum[:, None, :] - f64(u)[:, :, None]) <= tol).any(-1)


SAMPLER_TIES = [1, 2, 20, 32]                 # n_mix of the tie cases, B = 3
SAMPLER_LONG = [257, 300]                     # n_pts past one trip of the frame loop (n_mix 20, B 2)
MEAN_STEP = 8.0                               # mu_m = 8 m on x: the component is read back from the draw


def _sampler_params(rng, B, n, zero_rows=True):
    logits = 1.5 * rng.standard_normal((B, n))
    pi = np.exp(logits)
    if zero_rows and n >= 3:                  # exact zeros at the first, a middle and the last component (row 0), at the first (row 1)
        pi[0, [0, n // 2, n - 1]] = 0.0
        pi[1, 0] = 0.0
    elif zero_rows and n == 2:
        pi[0, 0], pi[1, 1] = 0.0, 0.0
    pi = (pi / pi.sum(1, keepdims=True)).astype(np.float32)
    mu = 0.3 * rng.uniform(-1, 1, (B, n, 3))
    mu[:, :, 0] = MEAN_STEP * np.arange(n)
    sig = rng.uniform(0.01, 0.05, (B, n, 3))
    rho = np.tanh(0.6 * rng.standard_normal((B, n, 3)))
    rho[:, ::3] = np.tanh(2.0) * np.array([1.0, 1.0, -1.0])        # every third component repaired
    return join_params(pi, mu, sig, rho)


def _tie_values(pi_row):
    """0; around and at several cumulative weights; cum[n - 1]; 1 - 2^-24, 1, 2; a few values away from every tie."""
    n = pi_row.size
    cum = np.cumsum(pi_row, dtype=np.float32)
    u = [np.float32(0.0)]
    for m in sorted({0, 1, n // 2 - 1, n // 2, n - 2, n - 1} & set(range(n))):
        u += [np.nextafter(cum[m], np.float32(-np.inf)), cum[m], np.nextafter(cum[m], np.float32(np.inf))]
    u += [cum[n - 1], np.float32(1.0 - 2.0 ** -24), np.float32(1.0), np.float32(2.0)]
    mids = [0.5 * (lo + hi) for lo, hi in zip(np.concatenate([[0.0], f64(cum[:-1])]), f64(cum)) if hi - lo > 1e-3][:4]
    return np.array(u + mids, np.float32)


@functools.lru_cache(maxsize=None)
def sampler_case(name):
    """-> dict(params (B, 10 n), u (B, P), z (B, P, 3)), all fp32.  Names: ties-n<N>, long-P<P>, saturated, window."""
    rng = np.random.default_rng(seed_of("gmm sampler " + name))
    kind, _, arg = name.partition("-")
    if kind == "ties":
        n, B = int(arg[1:]), 3
        params = _sampler_params(rng, B, n)
        rows = [_tie_values(params[b, :n]) for b in range(B)]
        P = min(r.size for r in rows)
        u = np.stack([r[:P] for r in rows])
    elif kind in ("long", "window"):
        n, B, P = 20, 2, (int(arg[1:]) if kind == "long" else 9)
        params = _sampler_params(rng, B, n)
        u = rng.random((B, P)).astype(np.float32)
        cum = np.cumsum(params[:, :n], 1, dtype=np.float32)
        u[:, ::7] = cum[:, rng.integers(0, n, u[:, ::7].shape[1])]
        u[:, P - 1] = 1.0
    else:
        assert name == "saturated"
        _, pi, mu, sig, rho = _saturated_params(SATURATED_SEED)
        B, n, P = pi.shape[0], pi.shape[1], 12
        mu[:, :, 0] = MEAN_STEP * np.arange(n)
        params = join_params(pi, mu, sig, rho)
        u = rng.random((B, P)).astype(np.float32)
    z = np.clip(rng.standard_normal((B, P, 3)), -1.5, 1.5).astype(np.float32)
    return dict(params=params, u=u, z=z)


def sampler_cases():
    return ["ties-n%d" % n for n in SAMPLER_TIES] + ["long-P%d" % P for P in SAMPLER_LONG] + ["saturated", "window"]


# ---------------------------------------------------------------------------------------------------------------------
# the split at the end of mlp_head_fwd_kernel: the last layer's bias blocks carry the spans
# ---------------------------------------------------------------------------------------------------------------------
SPLIT_H, SPLIT_B, SPLIT_N = 40, 5, 20


def split_head_inputs(dead_layer=False):
    """Head weights (fc1 .. fc4, the oracle's keys, fp32) and h (B, H).  fc4_b: logits over +-40, log sigma over -12 .. 6, the rho
    pre-activations with +-15 and +-1e-4 among values of order 1; fc4_W small, so every row stays within 1 of its bias.
    dead_layer: fc3_b = -1e3, every unit of the third layer off in every row."""
    n, H, B = SPLIT_N, SPLIT_H, SPLIT_B
    rng = np.random.default_rng(seed_of("gmm split head"))
    dims = [H, 64, 128, 256, 10 * n]
    head = {}
    for l in range(4):
        head["fc%d_W" % (l + 1)] = (rng.standard_normal((dims[l], dims[l + 1])) / np.sqrt(dims[l])).astype(np.float32)
        head["fc%d_b" % (l + 1)] = (0.1 * rng.standard_normal(dims[l + 1])).astype(np.float32)
    head["fc4_W"] *= np.float32(0.02)
    b4 = head["fc4_b"]
    b4[:n] = rng.permutation(np.linspace(-40.0, 40.0, n))
    b4[n:4 * n] = rng.uniform(-2, 2, 3 * n)
    b4[4 * n:7 * n] = rng.permutation(np.linspace(-12.0, 6.0, 3 * n))
    b4[7 * n:] = rng.standard_normal(3 * n)
    b4[7 * n:7 * n + 4] = [15.0, -15.0, 1e-4, -1e-4]
    head["fc4_W"][:, 7 * n:7 * n + 4] = 0.0                 # these four pre-activations are the bias itself in every row
    if dead_layer:
        head["fc3_b"][:] = -1e3
    return head, rng.uniform(-1, 1, (B, H)).astype(np.float32)


def split_reference(head, h):
    """O.tf_gmm3d_head in fp64 -> (pi, mu, sigma, rho), the last layer's pre-activation (B, 10 n)."""
    h64 = {k: f64(v) for k, v in head.items()}
    (pi, us, sg, rh), (_, _, a3) = O.tf_gmm3d_head(f64(h), h64, n_mix=SPLIT_N)
    return (pi, us, sg, rh), a3 @ h64["fc4_W"] + h64["fc4_b"]


# ---------------------------------------------------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------------------------------------------------
SPREADS = {}


@pytest.mark.parametrize("name", all_cases())
def test_the_two_fp64_references_agree(name):
    """part, loss and S to 1e-9; dpre within spread(case), which with its margin of 16 stays inside the project's 2e-4 max|ref|:
    the GPU bound is never looser than the heads' existing one."""
    ref, spread = reference(name)
    c = case(name)
    top = np.abs(ref["dpre"]).max()
    SPREADS[name] = spread
    print("%-28s spread %.3e   max|dpre| %.3e   ratio %.3e" % (name, spread, top, spread / top))
    assert all(np.isfinite(ref[k]).all() for k in ("part", "dpre", "S")) and np.isfinite(ref["loss"])
    assert dpre_bound(ref["dpre"], spread).max() <= 2e-4 * top
    if not c["weight_by_pi"]:
        assert (ref["dpre"][:, :c["n"]] == 0).all()
    direct = gmm3d_reference(*case_operands(c), c["scale"], c["weight_by_pi"])
    assert same_bits(direct["dpre"], ref["dpre"]) and same_bits(direct["part"], ref["part"])        # the frames taken from the y rows are the frames


def test_the_reference_is_the_oracles_loss():
    for name in ("n20-P31-B3-pi0-ld1", "n3-P86-B2-pi1-ld0", "saturated-pi1", "floor-pi0"):
        c = case(name)
        pi, mu, sig, rho, pts = (f64(a) for a in case_operands(c))
        got = O.mixture_3d_gaussian_loss(pts, (pi, mu.reshape(c["B"], -1), sig.reshape(c["B"], -1), rho.reshape(c["B"], -1)), 1, 1,
                                         process_in_seconds=False, weight_by_pi=c["weight_by_pi"])
        np.testing.assert_allclose(reference(name)[0]["loss"], c["scale"] * got, rtol=1e-9)


def test_shape_cases_sit_on_their_seams():
    by = {}
    for n, P, B in SHAPES:
        tc = chunk_frames(n, P)
        by[(n, P, B)] = (tc, -(-P // tc), P - (P - 1) // tc * tc)            # frames per chunk, chunks, frames of the last chunk
    assert by[(20, 29, 3)] == (29, 1, 29) and by[(20, 30, 3)] == (30, 1, 30) and by[(20, 31, 3)] == (30, 2, 1) and by[(20, 61, 3)] == (30, 3, 1)
    assert by[(25, 25, 2)] == (24, 2, 1) and 10 * 25 <= LDS_ENTRY
    assert by[(26, 24, 2)] == (23, 2, 1) and by[(26, 47, 2)] == (23, 3, 1) and 10 * 26 - LDS_ENTRY == 4
    assert by[(32, 20, 3)] == (19, 2, 1) and 10 * 32 - LDS_ENTRY == 64
    assert 1 * 256 == 256 and 3 * 86 == 258
    assert sorted(B for n, P, B in SHAPES if (n, P) == (2, 3)) == [1, ROW_TRIP, ROW_TRIP + 1, 300]
    for name in shape_cases():
        c, (ref, _) = case(name), reference(name)
        assert c["ldy"] in (3 * c["P"], 3 * c["P"] + 1) and c["params"].dtype == np.float32 and c["y"].shape == (c["B"], c["ldy"])
        if c["B"] * c["n"] >= 2:
            assert 0 < ref["repaired"].sum() < ref["repaired"].size, name


def test_floor_regime():
    """A quarter of the frames within a factor of 100 of the floor, one at S == 0 exactly - no term in any sum, a loss term of
    -log 1e-20 - and one well above it."""
    for w in (0, 1):
        ref, _ = reference("floor-pi%d" % w)
        S = ref["S"]
        at_floor = (S > 1e-22) & (S < 1e-18)
        print("floor-pi%d: %d of %d frames at the floor, %d at zero, %d above 1e-10" % (w, at_floor.sum(), S.size, (S == 0).sum(), (S > 1e-10).sum()))
        assert at_floor.sum() * 4 >= S.size and (S == 0).sum() >= 1 and (S > 1e-10).sum() >= 1
        assert (ref["terms"][S == 0] == 0).all() and not ref["repaired"].any()
        b = int(np.argmax((S == 0).any(1)))
        rest = -np.log(S[b][S[b] > 0] + FLOOR).sum()
        np.testing.assert_allclose(ref["part"][b] - rest, (S[b] == 0).sum() * -np.log(FLOOR), rtol=1e-12)


def test_needle_regime():
    for w in (0, 1):
        c, (ref, _) = case("needle-pi%d" % w), reference("needle-pi%d" % w)
        sig = split_params(c["params"], c["n"])[2]
        assert -7.01 <= np.log(sig).min() and np.log(sig).max() <= -4.99
        near = ref["S"] > 1.0
        print("needle-pi%d: parts %s, %d near frames of %d, max|dpre| / scale %.3e" % (w, np.round(ref["part"], 1), near.sum(), near.size, np.abs(ref["dpre"]).max() / c["scale"]))
        assert near.sum() * 3 == near.size and (ref["S"][~near] == 0).all()
        assert ref["part"].min() < 0 and np.abs(ref["dpre"]).max() >= 1e4 * c["scale"]


def test_saturated_regime():
    for w in (0, 1):
        c, (ref, _) = case("saturated-pi%d" % w), reference("saturated-pi%d" % w)
        _, _, sig, rho = split_params(f64(c["params"]), c["n"])
        k = -np.log2(1.0 - np.abs(rho))
        assert (k == np.round(k)).all() and k.min() >= 6 and k.max() <= 10
        trace = (sig ** 2).sum(-1)
        rep, lam = ref["repaired"], ref["eig2"]
        print("saturated-pi%d: %d of %d repaired, min |lambda_0| / trace %.2e, min gap / trace %.2e" % (
            w, rep.sum(), rep.size, (np.abs(lam[..., 0]) / trace).min(), ((lam[..., 1] - lam[..., 0]) / trace).min()))
        assert rep.sum() * 2 >= rep.size and (~rep).sum() >= 2
        assert (np.abs(lam[..., 0]) / trace).min() >= 1e-6 and ((lam[..., 1] - lam[..., 0]) / trace).min() >= 1e-4
        assert np.abs(ref["dpre"]).max() > 0


def test_dead_weights_regime():
    c = case("dead weights-pi1")
    pi = c["params"][:, :c["n"]]
    assert (pi == 0).sum() >= 6 and (pi == np.float32(1e-30)).sum() == 3 and pi.max() > 0.999 and np.float32(1e-30) > 0
    assert same_bits(c["params"], case("dead weights-pi0")["params"])
    ref, _ = reference("dead weights-pi1")
    assert (ref["dpre"][:, :c["n"]][pi == 0] == 0).all() and np.abs(ref["dpre"][:, :c["n"]]).max() > 0


def test_mixed_rows_regime():
    for w in (0, 1):
        ref, _ = reference("mixed rows-pi%d" % w)
        part = ref["part"]
        print("mixed rows-pi%d: parts %s: sum |part| / |sum part| %.3e" % (w, np.round(part, 2), np.abs(part).sum() / abs(part.sum())))
        assert np.abs(part).sum() >= 100 * abs(part.sum()) and part.min() < -50 and part.max() > 50


def _misses(name, mistake):
    """Worst error of the wrong-on-purpose reference in units of the GPU test's bounds: (dpre, loss)."""
    c, (ref, spread), bad = case(name), reference(name), wrong(name, mistake)
    return over_bound(bad["dpre"], ref["dpre"], spread), abs(bad["loss"] - ref["loss"]) / loss_bound(ref["part"], ref["loss"], c["scale"])


def _same(name, mistake):
    ref, bad = reference(name)[0], wrong(name, mistake)
    return same_bits(bad["dpre"], ref["dpre"]) and same_bits(bad["part"], ref["part"]) and bad["loss"] == ref["loss"]


def test_every_mistake_misses_its_cases_and_is_the_truth_on_its_control():
    chunked = lambda c: c["P"] > chunk_frames(c["n"], c["P"])
    for name in all_cases():
        c = case(name)
        if chunked(c):
            assert _misses(name, "chunk restart")[0] >= MARGIN, name
        else:
            assert _same(name, "chunk restart"), name
        if c["n"] in (26, 32):
            assert chunked(c) and _misses(name, "spilled entries")[0] >= MARGIN, name
        else:
            assert c["n"] <= 25 and _same(name, "spilled entries"), name
        if c["B"] > ROW_TRIP:
            assert _misses(name, "first 256 rows")[1] >= MARGIN, name
        else:
            assert _same(name, "first 256 rows"), name
        if c["ldy"] > 3 * c["P"] and c["B"] > 1:
            assert _misses(name, "row stride")[0] >= MARGIN, name
        elif c["ldy"] == 3 * c["P"]:
            assert _same(name, "row stride"), name
        if c["weight_by_pi"]:
            assert _misses(name, "softmax without the dot")[0] >= MARGIN, name
        else:
            assert _same(name, "softmax without the dot"), name
    assert {c["B"] for c in map(case, all_cases()) if c["B"] > ROW_TRIP} == {257, 300}
    for w in (0, 1):
        assert _misses("saturated-pi%d" % w, "no repair gradient")[0] >= MARGIN
        assert _misses("floor-pi%d" % w, "no floor in the weight")[0] >= MARGIN
    assert not reference(NOTHING_REPAIRED)[0]["repaired"].any() and _same(NOTHING_REPAIRED, "no repair gradient")
    S = reference(OFF_THE_FLOOR)[0]["S"]
    assert ((S == 0) | (S > 1.0)).all() and (S > 1.0).any() and _same(OFF_THE_FLOOR, "no floor in the weight")


# the sampler --------------------------------------------------------------------------------------------------------
def test_the_running_sum_is_sequential_fp32():
    for name in sampler_cases():
        p = sampler_case(name)["params"]
        n = p.shape[1] // 10
        for b in range(p.shape[0]):
            c, loop = np.float32(0.0), []
            for m in range(n):
                c = np.float32(c + p[b, m])
                loop.append(c)
            assert same_bits(np.cumsum(p[b, :n], dtype=np.float32), np.array(loop, np.float32))


@pytest.mark.parametrize("name", sampler_cases())
def test_sampler_reference_against_the_oracle_and_its_cases(name):
    s = sampler_case(name)
    params, u, z = s["params"], s["u"], s["z"]
    B, P = u.shape
    n = params.shape[1] // 10
    comp, out = sample_reference(params, u, z)
    pi, mu, sig, rho = (f64(a) for a in split_params(params, n))
    ora = O.sample_mixture_3d((pi, mu.reshape(B, -1), sig.reshape(B, -1), rho.reshape(B, -1)), f64(u), f64(z)).reshape(B, P, 3)
    away = ~near_a_tie(params, u)
    np.testing.assert_allclose(out[away], ora[away], rtol=1e-12, atol=1e-12)
    assert away.any() and np.abs(out[..., 0] - MEAN_STEP * comp).max() < 3.5          # the component can be read back from the draw
    assert np.isfinite(out).all()
    if name.startswith("ties"):
        assert not away.all() and (u == 0).any() and (u == 1).any() and (u == 2).any() and (u == np.float32(1 - 2.0 ** -24)).any()
        cum = np.cumsum(params[:, :n], 1, dtype=np.float32)
        assert all((u[b] == cum[b, m]).any() for b in range(B) for m in (0, n - 1))
        if n >= 3:
            assert (params[0, [0, n // 2, n - 1]] == 0).all() and params[1, 0] == 0 and (params[2, :n] > 0).all()
    if name.startswith("long"):
        assert P > 256
    if name == "saturated":
        lam = np.linalg.eigvalsh(_raw_cov(sig, rho))[..., 0]
        assert (lam < 0).sum() * 2 >= lam.size


def _raw_cov(sig, rho):
    s = sig[..., :, None] * sig[..., None, :]
    R = np.ones(rho.shape[:-1] + (3, 3))
    for k, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
        R[..., i, j] = R[..., j, i] = rho[..., k]
    return s * R


def test_sampler_mistakes():
    """`ties go left` and `no clamp` choose another component on the tie cases (n >= 2), `fp64 cumsum` at n = 32; all three are
    the truth, bit for bit, on the frames away from every tie."""
    for name in sampler_cases():
        s = sampler_case(name)
        params, u, z = s["params"], s["u"], s["z"]
        n = params.shape[1] // 10
        comp, out = sample_reference(params, u, z)
        away = ~near_a_tie(params, u) & (u < 0.999)
        cum = np.cumsum(params[:, :n], 1, dtype=np.float32)
        for mistake in SAMPLER_MISTAKES:
            bad_comp, bad = sample_reference(params, u, z, mistake)
            assert (bad_comp[away] == comp[away]).all() and same_bits(bad[away], out[away]), (name, mistake)
            differs = bad_comp != comp
            assert ((np.abs(bad - out) / sample_bound(out)).max(-1)[differs] >= MARGIN).all()
            if name.startswith("ties") and n >= 2:
                if mistake == "ties go left":
                    assert differs.any() and (u[differs][:, None] == cum[np.nonzero(differs)[0]]).any(-1).all(), name
                if mistake == "no clamp":
                    past = u >= cum[:, -1:]
                    assert past.any() and (differs == past).all(), name
                if mistake == "fp64 cumsum" and n == 32:
                    assert differs.any(), name


# the head's split ---------------------------------------------------------------------------------------------------
def test_split_head_inputs_span_what_they_say():
    head, h = split_head_inputs()
    (pi, us, sg, rh), pre = split_reference(head, h)
    n = SPLIT_N
    assert np.abs(pre - f64(head["fc4_b"])).max() < 1.0
    assert pre[:, :n].max() > 39 and pre[:, :n].min() < -39 and pi.min() >= 1e-36 and pi.min() < 1e-30
    assert np.log(sg).min() < -11 and np.log(sg).max() > 5
    r = pre[:, 7 * n:7 * n + 4]
    assert (r[:, 0] > 14).all() and (r[:, 1] < -14).all() and (np.abs(r[:, 2:]) < 1.0).all()
    dead, _ = split_head_inputs(dead_layer=True)
    (dpi, dus, dsg, drh), dpre = split_reference(dead, h)
    assert (dpre == f64(dead["fc4_b"])).all()             # the third layer is off: every row is the split of fc4_b


def test_zz_spread_per_case():
    """Prints spread(case) of every case this run has computed (the table of DESIGN.md, Tests)."""
    for name in sorted(SPREADS):
        print("%-28s %.3e" % (name, SPREADS[name]))
