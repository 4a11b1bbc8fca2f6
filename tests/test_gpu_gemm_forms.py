"""Every form of the fp32 GEMM (gemm_f32_kernel: five tile variants x four staging modes per operand, two-level k, periodic
shift, second A operand, bias row, epilogue accumulate, split-K with and without the XCD remap, both splitk_reduce forms),
of skinny_tn and of the bf16 TN GEMMs, through the public entry points ops.matmul, ops.dense_bwd, ops.wgrad_fused and
ops.lstm_seq_wgrad, at the tile, K and slice edges.

The form a case reaches is ASSERTED from the FOV_DBG_TRACE line of its product (a heuristic that moves makes the case fail
instead of silently testing something else).  Operands are views into buffers whose margins are NaN (a read outside an
operand gives a wrong value, not a fault); outputs are views into buffers whose margins hold a sentinel that must survive
bit for bit, pre-filled with NaN where the call overwrites.  Two data passes per case:
  exact: small integers in [-4, 4] - every product and partial sum is an integer below 2^24, so the fp64 product is the
         exact fp32 AND bf16 answer whatever the summation order (overwrite, accumulate on an integer base, the bias row, and
         a second call with other data through the same Scratch: stale partials of a slice not fully rewritten show up);
  real:  standard normal operands against the fp64 product (bf16: of the bf16-rounded operands), bound
         1e-5 * max|ref| + 1e-6 as in test_matmul_and_zx_layer / test_bf16_weight_gradient_product, run twice: bit-identical."""
import contextlib
import os
import re
import zlib

import numpy as np
import pytest
import torch

from oracle import fov_oracle as O

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
rb = lambda a: O.round_bf16(np.asarray(a, np.float32)).astype(np.float64)
f64 = lambda a: np.asarray(a, np.float64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


@contextlib.contextmanager
def knobs(**kv):
    """Set FOV_* knobs for the calls inside (the library re-reads its environment at the next scratch fetch)."""
    for k in kv:
        assert k not in os.environ, k
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k in kv:
            del os.environ[k]


def _margin(a):
    row = a.shape[-1] if a.ndim > 1 else 1
    return (max(1024, 2 * row) + 3) // 4 * 4


def guarded(a, off=0):
    """A contiguous device view of `a` inside a NaN buffer: margin >= two operand rows and >= 1024 floats on both sides,
    starting on a 16-byte boundary (off = 0) or one float later (off = 1)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    m = _margin(a)
    buf = torch.full((2 * m + a.size + 8,), float("nan"), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[m + off:m + off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return v


class OutView:
    """An output view inside a sentinel buffer; `base` None: pre-filled with NaN (the call must write every element)."""

    def __init__(self, shape, base=None, off=0, row=None):
        n = int(np.prod(shape))
        self.m = m = (max(1024, 2 * (row or shape[-1])) + 3) // 4 * 4
        self.buf = torch.full((2 * m + n + 8,), SENTINEL, dtype=torch.float32, device="cuda")
        self.lo, self.hi = m + off, m + off + n
        self.flat = self.buf[self.lo:self.hi]
        if base is None:
            self.flat.fill_(float("nan"))
        else:
            self.flat.copy_(torch.from_numpy(np.ascontiguousarray(base, dtype=np.float32).reshape(-1)))
        self.v = self.flat.view(shape)
        assert self.v.data_ptr() % 16 == 4 * off

    def part(self, start, shape):
        n = int(np.prod(shape))
        return self.flat[start:start + n].view(shape)

    def result(self):
        torch.cuda.synchronize()
        bits = self.buf.view(torch.int32)
        want = torch.tensor([SENTINEL], dtype=torch.float32).view(torch.int32).item()
        assert bool((bits[:self.lo] == want).all()) and bool((bits[self.hi:] == want).all()), "a write outside the output"
        return self.v.cpu().numpy().astype(np.float64)


def poison(*shape):
    """The caching allocator hands the block of a freed tensor to the next one of its size: an output that ops allocates
    itself (torch.empty) starts from NaN."""
    t = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    del t


F32_LINE = re.compile(r"\[fov trace\] gemm_f32 next: M=(\d+) N=(\d+) KO=(\d+) KI=(\d+) variant=(\d+) amode=(\d+) bmode=(\d+) split=(\d+) "
                      r"a2=(\d+) periods=(\d+)/(\d+) bias=(\d+) add_c=(\d+)")
BF16_LINE = re.compile(r"\[fov trace\] gemm_bf16_tn next: M=(\d+) N=(\d+) RO=(\d+) RI=(\d+) form=(\w+) avec=(\d+) split=(\d+) rows_per_split=(\d+) "
                       r"remap=(\d+) a2=(\d+) shifts=(\d+)/(\d+) bias=(\d+) add_c=(\d+)")
SKINNY_LINE = re.compile(r"\[fov trace\] skinny_tn next: ns=(\d+) nw=(\d+) rows=(\d+) vec=(\d+) chunks=(\d+)")


def f32_forms(err, M, N, KO, KI):
    """The gemm_f32 trace lines of the product (M, N, KO, KI) as dicts."""
    out = []
    for m in F32_LINE.finditer(err):
        v = [int(x) for x in m.groups()]
        if v[:4] == [M, N, KO, KI]:
            out.append(dict(variant=v[4], amode=v[5], bmode=v[6], split=v[7], a2=v[8], periods=(v[9], v[10]), bias=v[11], add_c=v[12]))
    return out


def bf16_forms(err, M, N, RO, RI):
    out = []
    for m in BF16_LINE.finditer(err):
        g = m.groups()
        if [int(g[0]), int(g[1]), int(g[2]), int(g[3])] == [M, N, RO, RI]:
            out.append(dict(form=g[4], avec=int(g[5]), split=int(g[6]), rows_per_split=int(g[7]), remap=int(g[8]), a2=int(g[9]),
                            shifts=(int(g[10]), int(g[11])), bias=int(g[12]), add_c=int(g[13])))
    return out


def expect_form(forms, want, what):
    """Exactly one trace line, and every field the table names equal to it; split may be 'split' (> 1) or 'single' (== 1)."""
    assert len(forms) == 1, (what, forms)
    got = forms[0]
    for k, v in want.items():
        if v is None:
            continue
        if k == "split" and v == "split":
            assert got["split"] > 1, (what, got)
        elif k == "split" and v == "single":
            assert got["split"] == 1, (what, got)
        else:
            assert got[k] == v, (what, k, got, want)
    print("gemm forms trace %s: %s" % (what, " ".join("%s=%s" % kv for kv in sorted(got.items()))))
    return got


def traced(capfd, fn):
    """fn() with FOV_DBG_TRACE=1 -> (its result, the trace)."""
    capfd.readouterr()
    with knobs(FOV_DBG_TRACE="1"):
        r = fn()
        torch.cuda.synchronize()
    return r, capfd.readouterr().err


def close(got, ref, what, scale=None):
    """The real-valued bound of the suite's GEMM tests: 1e-5 of the reference's largest element + 1e-6."""
    s = np.abs(ref).max() if scale is None else scale
    err = np.abs(got - ref).max() if ref.size else 0.0
    print("gemm forms %s: worst error %.3e, max|ref| %.3e, bound %.3e" % (what, err, s, 1e-5 * s + 1e-6))
    assert np.isfinite(got).all() and err <= 1e-5 * s + 1e-6, (what, err, s)


def run_case(capfd, launch, reference, make, check_trace, accumulate, what, env=None):
    """launch(data, bases or None, scratch) -> dict of fp64 arrays; reference(data) -> dict of fp64 arrays; make(rng, exact) -> data,
    bases (dict name -> integer / real base for the outputs that accumulate).  The two passes of the module docstring."""
    from longterm360fov_amd import ops
    rng = np.random.default_rng(zlib.crc32(what.encode()))
    with knobs(**(env or {})):
        scratch = ops.Scratch()
        for rep in range(2):   # exact pass, twice with different data through the same scratch
            data, bases = make(rng, True)
            if rep == 0:
                got, err = traced(capfd, lambda: launch(data, bases if accumulate else None, scratch))
                check_trace(err)
            else:
                got = launch(data, bases if accumulate else None, scratch)
            ref = reference(data)
            for k in ref:
                want = ref[k] + (bases[k] if accumulate and k in bases else 0.0)
                np.testing.assert_array_equal(got[k], want, err_msg="%s: %s, exact pass %d" % (what, k, rep))
        data, bases = make(rng, False)
        got = launch(data, bases if accumulate else None, scratch)
        again = launch(data, bases if accumulate else None, scratch)
        ref = reference(data)
        for k in ref:
            np.testing.assert_array_equal(got[k].astype(np.float32).view(np.uint32), again[k].astype(np.float32).view(np.uint32),
                                          err_msg="%s: %s differs between two runs" % (what, k))
            want = ref[k] + (bases[k] if accumulate and k in bases else 0.0)
            close(got[k], want, "%s %s" % (what, k), scale=np.abs(ref[k]).max() if ref[k].size else 0.0)


def draw(rng, exact, *shape):
    return (rng.integers(-4, 5, shape) if exact else rng.standard_normal(shape)).astype(np.float32)


def ids(cases):
    return ["-".join(str(x).replace(" ", "") for x in c) for c in cases]


# ---------------------------------------------------------------------------------------------------------------------
# ops.matmul(M, K, N): A k-fast, B k-slow
# ---------------------------------------------------------------------------------------------------------------------
X = None   # a field the table does not name
MATMUL = [
    # M, K, N, variant, amode, bmode, split, variant knob, split knob, A off, B off
    (1, 1, 1, 0, X, X, X, 0, 0, 0, 0),
    (31, 15, 255, 0, 2, 1, X, 0, 0, 0, 0),
    (32, 16, 256, 0, 3, 0, X, 0, 0, 0, 0),           # exact tile, exact k-tile
    (33, 17, 257, 1, 2, 1, X, 0, 0, 0, 0),
    (96, 20, 256, 1, 3, 0, X, 0, 0, 0, 0),           # K % 16 != 0 with 16-byte k loads
    (63, 100, 65, 1, 3, 1, X, 0, 0, 0, 0),
    (97, 64, 260, 3, 3, 0, X, 0, 0, 0, 0),
    (64, 512, 64, 1, X, X, 8, 0, 0, 0, 0),           # remap
    (65, 513, 129, 1, 2, 1, 7, 0, 0, 0, 0),          # last slice short
    (40, 1000, 36, 1, X, X, 13, 0, 0, 0, 0),         # remap with 3 idle slice slots
    (129, 2052, 130, 4, 3, 1, 26, 0, 0, 0, 0),
    (128, 4096, 128, 4, X, X, 64, 0, 0, 0, 0),
    (130, 8200, 132, 2, X, X, 57, 0, 0, 0, 0),
    (96, 512, 1024, 3, X, X, X, 0, 0, 0, 0),         # reached through the `variant == 1` rule
]
for _s in ((97, 64, 260), (96, 512, 1024), (129, 2052, 130), (128, 4096, 128)):      # the variant-3 and variant-4 rows with the tile shape forced
    for _v in (2, 3, 4):
        MATMUL.append(_s + (_v, 3, X, "split" if _s[1] > 64 else "single", _v, 0, 0, 0))
MATMUL += [(65, 513, 129, 1, 2, 1, 1, 0, 1, 0, 0), (65, 513, 129, 1, 2, 1, 9, 0, 9, 0, 0)]   # one slice; nine, the last one k-tile, remap
for _s, _v in (((32, 16, 256), 0), ((97, 64, 260), 3)):             # A and / or B one float off alignment
    MATMUL += [_s + (_v, 2, 0, X, 0, 0, 1, 0), _s + (_v, 3, 1, X, 0, 0, 0, 1), _s + (_v, 2, 1, X, 0, 0, 1, 1)]


@pytest.mark.parametrize("M,K,N,variant,amode,bmode,split,vknob,sknob,aoff,boff", MATMUL, ids=ids(MATMUL))
def test_matmul_forms(capfd, M, K, N, variant, amode, bmode, split, vknob, sknob, aoff, boff):
    from longterm360fov_amd import ops
    env = {}
    if vknob:
        env["FOV_GEMM_VARIANT"] = vknob
    if sknob:
        env["FOV_GEMM_SPLIT"] = sknob

    def make(rng, exact):
        return (draw(rng, exact, M, K), draw(rng, exact, K, N)), {}

    def launch(data, bases, scratch):
        a, b = guarded(data[0], aoff), guarded(data[1], boff)
        poison(M, N)
        c = ops.matmul(a, b, scratch=scratch)
        return {"c": c.cpu().numpy().astype(np.float64)}

    def check_trace(err):
        expect_form(f32_forms(err, M, N, 1, K), dict(variant=variant, amode=amode, bmode=bmode, split=split, a2=0, periods=(0, 0), bias=0, add_c=0),
                    "matmul")

    run_case(capfd, launch, lambda d: {"c": f64(d[0]) @ f64(d[1])}, make, check_trace, False, "matmul %dx%dx%d v%d s%d a%d b%d" % (M, K, N, vknob, sknob, aoff, boff), env)


# ---------------------------------------------------------------------------------------------------------------------
# ops.dense_bwd: dW = x^T dpre (both operands k-slow), db, dx = dpre W^T (both operands k-fast)
# ---------------------------------------------------------------------------------------------------------------------
def dense_case(capfd, N, In, Out, accumulate, check_trace, what, env=None, offs=None, need_dx=True, dtype="f32", bf16_ref=False):
    from longterm360fov_amd import ops
    offs = offs or {}

    def make(rng, exact):
        return ((draw(rng, exact, N, In), draw(rng, exact, In, Out), draw(rng, exact, N, Out)),
                {"dW": draw(rng, exact, In, Out).astype(np.float64), "db": draw(rng, exact, Out).astype(np.float64)})

    def launch(data, bases, scratch):
        x, W, d = guarded(data[0], offs.get("x", 0)), guarded(data[1], offs.get("W", 0)), guarded(data[2], offs.get("d", 0))
        dW = OutView((In, Out), bases and bases["dW"], offs.get("dW", 0))
        db = OutView((Out,), bases and bases["db"])
        if need_dx:
            poison(N, In)
        dx, _, _ = ops.dense_bwd(x, W, d, dW=dW.v, db=db.v, need_dx=need_dx, accumulate=bases is not None, scratch=scratch, dtype=dtype)
        r = {"dW": dW.result(), "db": db.result()}
        if need_dx:
            r["dx"] = dx.cpu().numpy().astype(np.float64)
        return r

    def reference(data):
        x, W, d = data
        r = {"dW": (rb(x).T @ rb(d)) if bf16_ref else f64(x).T @ f64(d), "db": f64(d).sum(0)}
        if need_dx:
            r["dx"] = f64(d) @ f64(W).T
        return r

    run_case(capfd, launch, reference, make, check_trace, accumulate, what, env)


DENSE_DW = [
    # N, In, Out, variant, amode, bmode, split
    (17, 36, 20, 1, 0, 0, "single"),
    (100, 33, 70, 1, 1, 1, "single"),
    (40, 7, 64, 0, 1, 0, "single"),
    (50, 36, 21, 1, 0, 1, "single"),
    (1000, 90, 64, 1, 1, 0, 13),
    (1000, 33, 65, X, X, X, "split"),       # (In * Out) % 4 != 0: the scalar splitk_reduce
    (333, 100, 36, 3, X, X, 7),
    (600, 132, 260, 3, X, X, 8),            # remap
]


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("N,In,Out,variant,amode,bmode,split", DENSE_DW, ids=ids(DENSE_DW))
def test_dense_bwd_weight_gradient_forms(capfd, N, In, Out, variant, amode, bmode, split, accumulate):
    def check_trace(err):
        got = expect_form(f32_forms(err, In, Out, 1, N), dict(variant=variant, amode=amode, bmode=bmode, split=split, a2=0, periods=(0, 0), bias=0), "dW")
        assert got["add_c"] == (1 if accumulate and got["split"] == 1 else 0), got    # add_c only where nothing is split
        assert "[fov trace] launched: skinny_tn" not in err
    dense_case(capfd, N, In, Out, accumulate, check_trace, "dense_bwd dW %d,%d,%d acc%d" % (N, In, Out, accumulate))


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
def test_dense_bwd_split_weight_gradient_unaligned_output(capfd, accumulate):
    """A split product whose dW starts one float off a 16-byte boundary: the partials are reduced by the scalar splitk_reduce."""
    def check_trace(err):
        expect_form(f32_forms(err, 90, 64, 1, 1000), dict(variant=1, amode=1, bmode=0, split=13, add_c=0), "dW")
        assert "[fov trace] launched: splitk_reduce" in err
    dense_case(capfd, 1000, 90, 64, accumulate, check_trace, "dense_bwd dW 1000,90,64 unaligned dW acc%d" % accumulate, offs={"dW": 1}, need_dx=False)


DENSE_DX = [
    # N, In, Out, variant, amode, bmode, split, W off, dpre off
    (17, 36, 20, 0, 3, 3, "single", 0, 0),
    (300, 64, 24, 3, 3, 3, "single", 0, 0),
    (513, 40, 132, X, X, X, 3, 0, 0),
    (100, 33, 70, 3, 2, 2, "single", 0, 0),
    (130, 36, 17, X, 2, 2, "single", 0, 0),
    (300, 64, 24, 3, 3, 2, "single", 1, 0),
    (300, 64, 24, 3, 2, 3, "single", 0, 1),
]


@pytest.mark.parametrize("N,In,Out,variant,amode,bmode,split,woff,doff", DENSE_DX, ids=ids(DENSE_DX))
def test_dense_bwd_data_gradient_forms(capfd, N, In, Out, variant, amode, bmode, split, woff, doff):
    def check_trace(err):
        expect_form(f32_forms(err, N, In, 1, Out), dict(variant=variant, amode=amode, bmode=bmode, split=split, a2=0, periods=(0, 0), bias=0, add_c=0), "dx")
    dense_case(capfd, N, In, Out, False, check_trace, "dense_bwd dx %d,%d,%d W%d d%d" % (N, In, Out, woff, doff), offs={"W": woff, "d": doff})


# ---------------------------------------------------------------------------------------------------------------------
# skinny_tn through ops.dense_bwd: a narrow output (ns = Out, columns = In) or a narrow input (ns = In, columns = Out), >= 1024 rows
# ---------------------------------------------------------------------------------------------------------------------
SKINNY = ([(N, In, ns) for N in (1024, 1055, 4097) for ns in range(1, 9) for In in ((40, 512, 513) if ns in (1, 4, 5, 8) else (40,))] +
          [(N, ns, Out) for N in (1024, 1055, 4097) for ns in (1, 3, 6, 8) for Out in (64, 1024, 1028)])


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("N,In,Out", SKINNY, ids=ids(SKINNY))
def test_skinny_weight_gradient_forms(capfd, N, In, Out, accumulate):
    ns, nw = (Out, In) if Out <= 8 else (In, Out)

    def check_trace(err):
        assert "[fov trace] launched: skinny_tn" in err and not f32_forms(err, In, Out, 1, N), err
        m = SKINNY_LINE.findall(err)
        assert len(m) == 1 and [int(v) for v in m[0][:4]] == [ns, nw, N, 1 if nw >= 512 and nw % 4 == 0 else 0], m
    dense_case(capfd, N, In, Out, accumulate, check_trace, "skinny %d,%d,%d acc%d" % (N, In, Out, accumulate), need_dx=False)


SKINNY_NOT = [(1023, 40, 3), (1023, 512, 8), (1023, 513, 1), (1023, 6, 64), (1023, 1, 1028), (1023, 8, 1024)]


@pytest.mark.parametrize("N,In,Out", SKINNY_NOT, ids=ids(SKINNY_NOT))
def test_one_row_short_of_skinny_takes_the_mfma_gemm(capfd, N, In, Out):
    def check_trace(err):
        assert "skinny_tn" not in err
        expect_form(f32_forms(err, In, Out, 1, N), dict(split="split", a2=0, bias=0, add_c=0), "dW")
    dense_case(capfd, N, In, Out, False, check_trace, "not skinny %d,%d,%d" % (N, In, Out), need_dx=False)


# ---------------------------------------------------------------------------------------------------------------------
# ops.wgrad_fused(x1, x2, dz): second A operand and bias row
# ---------------------------------------------------------------------------------------------------------------------
def fused_case(capfd, N, In1, In2, Out, bias, accumulate, check_trace, what, env=None, dtype="f32"):
    from longterm360fov_amd import ops
    rows = In1 + In2 + (1 if bias else 0)
    r16 = rb if dtype == "bf16" else f64

    def make(rng, exact):
        return ((draw(rng, exact, N, In1), draw(rng, exact, N, In2) if In2 else None, draw(rng, exact, N, Out)),
                {"out": draw(rng, exact, rows, Out).astype(np.float64)})

    def launch(data, bases, scratch):
        x1, x2, d = guarded(data[0]), None if data[1] is None else guarded(data[1]), guarded(data[2])
        out = OutView((rows, Out), bases and bases["out"])
        ops.wgrad_fused(x1, x2, d, out.v, bias=bias, accumulate=bases is not None, scratch=scratch, dtype=dtype)
        return {"out": out.result()}

    def reference(data):
        x1, x2, d = data
        parts = [r16(x1).T @ r16(d)] + ([r16(x2).T @ r16(d)] if x2 is not None else []) + ([f64(d).sum(0)[None]] if bias else [])
        return {"out": np.concatenate(parts, 0)}

    run_case(capfd, launch, reference, make, check_trace, accumulate, what, env)


FUSED = [(40, 128, 4, 68, "single"), (33, 100, 0, 64, "single"), (520, 256, 20, 260, 7), (1000, 128, 36, 132, 13)]


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("N,In1,In2,Out,split", FUSED, ids=ids(FUSED))
def test_wgrad_fused_forms(capfd, N, In1, In2, Out, split, bias, accumulate):
    def check_trace(err):
        got = expect_form(f32_forms(err, In1 + In2, Out, 1, N), dict(amode=0, bmode=0, split=split, a2=1 if In2 else 0, periods=(0, 0), bias=1 if bias else 0),
                          "wgrad_fused")
        assert got["add_c"] == (1 if accumulate and got["split"] == 1 else 0), got
    fused_case(capfd, N, In1, In2, Out, bias, accumulate, check_trace, "wgrad_fused %d,%d,%d,%d bias%d acc%d" % (N, In1, In2, Out, bias, accumulate))


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
def test_wgrad_fused_falls_back_to_separate_products(capfd, accumulate):
    """In1 = 90 with a second operand is not fusable (the first operand must fill whole row tiles): the separate products."""
    def check_trace(err):
        for M in (90, 20):
            expect_form(f32_forms(err, M, 64, 1, 200), dict(a2=0, bias=0, periods=(0, 0)), "fallback")
        assert not f32_forms(err, 110, 64, 1, 200)
    fused_case(capfd, 200, 90, 20, 64, True, accumulate, check_trace, "wgrad_fused fallback acc%d" % accumulate)


# ---------------------------------------------------------------------------------------------------------------------
# ops.lstm_seq_wgrad: dK, dR, db as views of one flat buffer (fuse_kr: a2 + two periods; fuse_r: one period), and the
# two-level product KO = B, KI = T - 1 with FOV_NO_WGRAD_FUSION=1
# ---------------------------------------------------------------------------------------------------------------------
def lstm_case(capfd, B, T, F, H, with_h0, accumulate, check_trace, what, env=None, adjacent_k=True, dtype="f32"):
    from longterm360fov_amd import ops
    N4 = 4 * H
    r16 = rb if dtype == "bf16" else f64
    nk, nr = F * N4, H * N4

    def make(rng, exact):
        return ((draw(rng, exact, B, T, F), draw(rng, exact, B, T, H), draw(rng, exact, B, T, N4), draw(rng, exact, B, H) if with_h0 else None),
                {"dK": draw(rng, exact, F, N4).astype(np.float64), "dR": draw(rng, exact, H, N4).astype(np.float64),
                 "db": draw(rng, exact, N4).astype(np.float64)})

    def launch(data, bases, scratch):
        x, hs, dz = guarded(data[0]), guarded(data[1]), guarded(data[2])
        h0 = None if data[3] is None else guarded(data[3])
        cat = lambda *names: None if bases is None else np.concatenate([bases[n].reshape(-1) for n in names])
        if adjacent_k:
            flat = OutView((nk + nr + N4,), cat("dK", "dR", "db"), row=N4)
            dK, dR, db = flat.part(0, (F, N4)), flat.part(nk, (H, N4)), flat.part(nk + nr, (N4,))
            outs = [flat]
        else:
            kbuf = OutView((F, N4), bases and bases["dK"])
            flat = OutView((nr + N4,), cat("dR", "db"), row=N4)
            dK, dR, db = kbuf.v, flat.part(0, (H, N4)), flat.part(nr, (N4,))
            outs = [kbuf, flat]
        ops.lstm_seq_wgrad(x, hs, dz, dK=dK, dR=dR, db=db, h0=h0, accumulate=bases is not None, scratch=scratch, dtype=dtype)
        got = np.concatenate([o.result().reshape(-1) for o in outs])
        return {"dK": got[:nk].reshape(F, N4), "dR": got[nk:nk + nr].reshape(H, N4), "db": got[nk + nr:]}

    def reference(data):
        x, hs, dz, h0 = data
        x, hs, z, zb = r16(x), r16(hs), r16(dz), f64(dz)
        dK = np.einsum("btf,btn->fn", x, z)
        dR = np.einsum("bth,btn->hn", hs[:, :-1], z[:, 1:]) if T > 1 else np.zeros((H, N4))
        if h0 is not None:
            dR = dR + r16(h0).T @ z[:, 0]
        return {"dK": dK, "dR": dR, "db": zb.sum((0, 1))}

    e = {"FOV_NO_WGRAD_GROUP": "1"}
    e.update(env or {})
    run_case(capfd, launch, reference, make, check_trace, accumulate, what, e)


def h0_product(err, B, T, H, with_h0):
    forms = f32_forms(err, H, 4 * H, 1, B)
    if with_h0:
        expect_form(forms, dict(amode=0, bmode=0, a2=0, periods=(0, 0), bias=0), "h0^T dz_0")   # accumulates: add_c, or split and an accumulating reduce
    else:
        assert not forms


LSTM_KR = [(1, 2, 20, "single"), (1, 16, 20, "single"), (3, 5, 20, "single"), (2, 17, 36, "single"), (7, 3, 132, "single"), (35, 30, 20, 14)]


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("with_h0", [False, True], ids=["zero", "h0"])
@pytest.mark.parametrize("B,T,H,split", LSTM_KR, ids=ids(LSTM_KR))
def test_lstm_wgrad_one_product_for_all_three(capfd, B, T, H, split, with_h0, accumulate):
    """fuse_kr: [x | h_{t-1} | 1]^T dz, the second operand shifted with period T (below, at and above the 16-row k-tile)."""
    F = 128

    def check_trace(err):
        got = expect_form(f32_forms(err, F + H, 4 * H, 1, B * T), dict(amode=0, bmode=0, split=split, a2=1, periods=(0, T), bias=1), "fuse_kr")
        assert got["add_c"] == (1 if accumulate and got["split"] == 1 else 0), got
        h0_product(err, B, T, H, with_h0)
    lstm_case(capfd, B, T, F, H, with_h0, accumulate, check_trace, "lstm_seq_wgrad fuse_kr %d,%d,%d h0%d acc%d" % (B, T, H, with_h0, accumulate))


LSTM_R = [(1, 2, 100, "single"), (4, 4, 100, "single"), (3, 17, 100, "single"), (50, 15, 100, 10), (33, 16, 132, "split")]


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("with_h0", [False, True], ids=["zero", "h0"])
@pytest.mark.parametrize("B,T,H,split", LSTM_R, ids=ids(LSTM_R))
def test_lstm_wgrad_one_product_for_dR_and_db(capfd, B, T, H, split, with_h0, accumulate):
    """fuse_r (dK lies elsewhere): [h_{t-1} | 1]^T dz, the first operand shifted; dK on its own."""
    F = 12

    def check_trace(err):
        expect_form(f32_forms(err, H, 4 * H, 1, B * T), dict(amode=0, bmode=0, split=split, a2=0, periods=(T, 0), bias=1), "fuse_r")
        expect_form(f32_forms(err, F, 4 * H, 1, B * T), dict(variant=0, amode=0, bmode=0, a2=0, periods=(0, 0), bias=0), "dK")
        h0_product(err, B, T, H, with_h0)
    lstm_case(capfd, B, T, F, H, with_h0, accumulate, check_trace, "lstm_seq_wgrad fuse_r %d,%d,%d h0%d acc%d" % (B, T, H, with_h0, accumulate),
              adjacent_k=False)


LSTM_TWO_LEVEL = [(3, 2, 100, "single"), (3, 16, 100, "single"), (3, 17, 100, "single"), (3, 18, 100, "single"), (5, 30, 100, "split"),
                  (40, 3, 36, 10), (2, 33, 20, "single")]


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("with_h0", [False, True], ids=["zero", "h0"])
@pytest.mark.parametrize("B,T,H,split", LSTM_TWO_LEVEL, ids=ids(LSTM_TWO_LEVEL))
def test_lstm_wgrad_two_level_recurrent_product(capfd, B, T, H, split, with_h0, accumulate):
    """FOV_NO_WGRAD_FUSION=1: dR = sum_b sum_{t>=1} hs[b,t-1]^T dz[b,t] as the two-level product KO = B, KI = T - 1 (k-tiles that
    end with every ko row: KI below, at and above 16; slices that cut across ko rows)."""
    F = 12

    def check_trace(err):
        got = expect_form(f32_forms(err, H, 4 * H, B, T - 1), dict(amode=0, bmode=0, split=split, a2=0, periods=(0, 0), bias=0), "dR")
        assert got["add_c"] == (1 if accumulate and got["split"] == 1 else 0), got
        assert not f32_forms(err, H, 4 * H, 1, B * T)
        h0_product(err, B, T, H, with_h0)
    lstm_case(capfd, B, T, F, H, with_h0, accumulate, check_trace, "lstm_seq_wgrad two-level %d,%d,%d h0%d acc%d" % (B, T, H, with_h0, accumulate),
              env={"FOV_NO_WGRAD_FUSION": "1"})


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("with_h0", [False, True], ids=["zero", "h0"])
@pytest.mark.parametrize("fusion", [True, False], ids=["adjacent", "nofusion"])
def test_lstm_wgrad_single_step(capfd, fusion, with_h0, accumulate):
    """T = 1: nothing recurrent - dR = h0^T dz_0, or zero."""
    B, F, H = 5, 128, 20

    def check_trace(err):
        assert not f32_forms(err, H, 4 * H, B, 0) and not f32_forms(err, F + H, 4 * H, 1, B)
        h0_product(err, B, 1, H, with_h0)
    lstm_case(capfd, B, 1, F, H, with_h0, accumulate, check_trace, "lstm_seq_wgrad T=1 fusion%d h0%d acc%d" % (fusion, with_h0, accumulate),
              env=None if fusion else {"FOV_NO_WGRAD_FUSION": "1"})


# ---------------------------------------------------------------------------------------------------------------------
# bf16 operands: gemm_bf16_tn3_kernel (deep) / gemm_bf16_tn_kernel (FOV_GEMM_BF16_SHALLOW=1), <AVEC> each
# ---------------------------------------------------------------------------------------------------------------------
def bf16_split(rows, want):
    rps = ((rows + want - 1) // want + 31) // 32 * 32
    return (rows + rps - 1) // rps


BF16_DENSE = [
    # N, In, Out, split knob, no remap, x off
    (31, 127, 64, 0, 0, 0), (256, 128, 128, 0, 0, 0), (257, 129, 132, 0, 0, 0), (513, 36, 68, 0, 0, 0), (2304, 130, 124, 0, 0, 0),
    (5000, 128, 64, 0, 0, 0), (2304, 130, 124, 3, 0, 0), (2304, 130, 124, 9, 0, 0), (5000, 128, 64, 3, 0, 0), (5000, 128, 64, 9, 0, 0),
    (5000, 128, 64, 9, 1, 0), (256, 128, 128, 0, 0, 1), (5000, 128, 64, 9, 0, 1),
]


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("shallow", [False, True], ids=["deep", "shallow"])
@pytest.mark.parametrize("N,In,Out,sknob,noremap,xoff", BF16_DENSE, ids=ids(BF16_DENSE))
def test_bf16_dense_bwd_forms(capfd, N, In, Out, sknob, noremap, xoff, shallow, accumulate):
    env = {}
    if sknob:
        env["FOV_GEMM_BF16_SPLIT"] = sknob
    if noremap:
        env["FOV_GEMM_BF16_NOREMAP"] = 1
    if shallow:
        env["FOV_GEMM_BF16_SHALLOW"] = 1
    split = bf16_split(N, sknob) if sknob else (1 if N < 512 else 2 if N == 513 else "split")

    def check_trace(err):
        got = expect_form(bf16_forms(err, In, Out, 1, N), dict(form="shallow" if shallow else "deep", avec=1 if In % 4 == 0 and not xoff else 0, split=split,
                                                               a2=0, shifts=(0, 0), bias=0, add_c=1 if accumulate else 0), "bf16 dW")
        assert got["remap"] == (1 if got["split"] >= 8 and not noremap else 0), got
        assert got["rows_per_split"] % 32 == 0 and (got["split"] - 1) * got["rows_per_split"] < N <= got["split"] * got["rows_per_split"], got
        assert not f32_forms(err, In, Out, 1, N)
    dense_case(capfd, N, In, Out, accumulate, check_trace, "bf16 dense_bwd %d,%d,%d s%d r%d x%d sh%d acc%d" % (N, In, Out, sknob, noremap, xoff, shallow, accumulate),
               env=env, offs={"x": xoff}, need_dx=False, dtype="bf16", bf16_ref=True)


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("Out", [62, 60])
def test_bf16_dense_bwd_narrow_output_falls_back_to_fp32(capfd, Out, accumulate):
    def check_trace(err):
        assert not BF16_LINE.search(err)
        expect_form(f32_forms(err, 128, Out, 1, 300), dict(a2=0, bias=0), "fp32 dW")
    dense_case(capfd, 300, 128, Out, accumulate, check_trace, "bf16 dense_bwd fallback Out=%d acc%d" % (Out, accumulate), need_dx=False, dtype="bf16")


BF16_FUSED = [(40, 128, 4, 68), (1000, 128, 36, 132), (2304, 256, 20, 64)]


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shallow", [False, True], ids=["deep", "shallow"])
@pytest.mark.parametrize("N,In1,In2,Out", BF16_FUSED, ids=ids(BF16_FUSED))
def test_bf16_wgrad_fused_forms(capfd, N, In1, In2, Out, shallow, bias, accumulate):
    def check_trace(err):
        expect_form(bf16_forms(err, In1 + In2, Out, 1, N), dict(form="shallow" if shallow else "deep", avec=1, split="single" if N < 512 else "split", a2=1, shifts=(0, 0),
                                                                bias=1 if bias else 0, add_c=1 if accumulate else 0), "bf16 wgrad_fused")
        assert not F32_LINE.search(err)
    fused_case(capfd, N, In1, In2, Out, bias, accumulate, check_trace, "bf16 wgrad_fused %d,%d,%d,%d sh%d bias%d acc%d" % (N, In1, In2, Out, shallow, bias, accumulate),
               env={"FOV_GEMM_BF16_SHALLOW": 1} if shallow else None, dtype="bf16")


BF16_LSTM = [(1, 2), (3, 5), (2, 17), (9, 31), (8, 33)]


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("with_h0", [False, True], ids=["zero", "h0"])
@pytest.mark.parametrize("shallow", [False, True], ids=["deep", "shallow"])
@pytest.mark.parametrize("B,T", BF16_LSTM, ids=ids(BF16_LSTM))
def test_bf16_lstm_wgrad_one_product_for_all_three(capfd, B, T, shallow, with_h0, accumulate):
    """The shifted second operand, the bias row and the h0 product of both bf16 kernels (periods below and above the 32-row stage)."""
    F, H = 128, 256

    def check_trace(err):
        expect_form(bf16_forms(err, F + H, 4 * H, B, T), dict(form="shallow" if shallow else "deep", avec=1, split="single", a2=1, shifts=(0, 1), bias=1,
                                                                   add_c=1 if accumulate else 0), "bf16 fuse_kr")
        h0 = bf16_forms(err, H, 4 * H, 1, B)
        if with_h0:
            expect_form(h0, dict(a2=0, shifts=(0, 0), bias=0, add_c=1), "bf16 h0^T dz_0")
        else:
            assert not h0
        assert not F32_LINE.search(err)
    lstm_case(capfd, B, T, F, H, with_h0, accumulate, check_trace, "bf16 lstm_seq_wgrad fuse_kr %d,%d sh%d h0%d acc%d" % (B, T, shallow, with_h0, accumulate),
              env={"FOV_GEMM_BF16_SHALLOW": 1} if shallow else None, dtype="bf16")


BF16_TWO_LEVEL = [(B, RI) for B in (1, 9) for RI in (1, 2, 3, 31, 32, 33)]


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("B,RI", BF16_TWO_LEVEL, ids=ids(BF16_TWO_LEVEL))
def test_bf16_lstm_wgrad_two_level_recurrent_product(capfd, B, RI, accumulate):
    """FOV_NO_WGRAD_FUSION=1: the two-level rows (ro, ri) of the bf16 kernel, ri by the magic-number division by RI = T - 1."""
    F, H, T = 128, 256, RI + 1

    def check_trace(err):
        expect_form(bf16_forms(err, H, 4 * H, B, RI), dict(form="deep", avec=1, a2=0, shifts=(0, 0), bias=0, add_c=1 if accumulate else 0), "bf16 dR")
        expect_form(bf16_forms(err, F, 4 * H, 1, B * T), dict(form="deep", avec=1, a2=0, shifts=(0, 0), bias=0), "bf16 dK")
        assert not F32_LINE.search(err)
    lstm_case(capfd, B, T, F, H, B == 9, accumulate, check_trace, "bf16 lstm_seq_wgrad two-level %d,%d acc%d" % (B, RI, accumulate),
              env={"FOV_NO_WGRAD_FUSION": "1"}, dtype="bf16")
