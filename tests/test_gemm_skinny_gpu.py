"""``C.gemm_skinny`` (csrc/kernels/gemm_skinny.hip), the weight-streaming GEMM of the decode steps, on the GPU.

Shapes (M, N, K): M in {1, 3, 16, 17, 33, 64} (one row, a partial 16-row group, a full one, the first row of the
second group, of the third, the limit), N in {16, 48, 272} (one workgroup, three, seventeen), K in {32, 96, 1024,
1056}: one 32-k step (fewer steps than waves), three (uneven over the waves), 32 (divides evenly), 33 (a batch tail
and the odd last step). All operands are made once per module and sliced.

Bounds: ``helpers.gemm_bound`` / ``gelu_out_bound`` against the fp64 ``gemm_expected`` (derived, not tuned); the
exact-operand cases compare bits with ``C.gemm``."""
import itertools

import pytest
import torch

from ml_trainer_amd.ops._ext import require_native
from tests.helpers import (assert_guard_intact, assert_within, bf16_t_used, gelu64, gelu_out_bound, gemm_bound,
                           gemm_expected, gemm_t32, guarded, guarded_like)

pytestmark = pytest.mark.gpu

MS, NS, KS = (1, 3, 16, 17, 33, 64), (16, 48, 272), (32, 96, 1024, 1056)
SHAPES = list(itertools.product(MS, NS, KS))
MMAX, NMAX, KMAX = max(MS), max(NS), max(KS)
CASES = ("bias", "bias_res", "bias_f32", "gelu")
BF, F32 = torch.bfloat16, torch.float32


class _Data:
    def __init__(self, dev):
        g = torch.Generator().manual_seed(21)
        tri = lambda *s: (torch.randint(-1, 2, s, generator=g).float() / 4).to(BF).to(dev)
        rnd = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(BF).to(dev)
        # exact operands: entries in {-1, 0, 1} / 4 -> every partial sum is a multiple of 1/16 below 2^7: exact in fp32
        self.xe, self.we = tri(MMAX, KMAX), tri(NMAX, KMAX)
        self.xr, self.wr = rnd(MMAX, KMAX), rnd(NMAX, KMAX, k=0.05)
        self.bias = (torch.randn(NMAX, generator=g) * 2).to(dev)
        self.res = rnd(MMAX, NMAX, k=2.0)


@pytest.fixture(scope="module")
def data():
    return _Data(torch.device("cuda", 0))


def _run(fn, x, w, case, bias, res, M, N):
    """One launch of `fn(x, w, y, bias=, aux=, res=, mode=)` for `case`: (y, aux or None)."""
    dev = x.device
    y = torch.empty(M, N, dtype=F32 if case == "bias_f32" else BF, device=dev)
    aux = torch.empty(M, N, dtype=BF, device=dev) if case == "gelu" else None
    fn(x, w, y, bias=bias, aux=aux, res=res if case == "bias_res" else None, mode=1 if case == "gelu" else 0)
    return y, aux


def _skinny(C):
    return lambda x, w, y, **kw: C.gemm_skinny(x, w, y, **kw)


def _gemm(C):
    return lambda x, w, y, **kw: C.gemm(x, w, y, False, False, **kw)


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


@pytest.mark.parametrize("case", CASES)
def test_same_bits_as_gemm_on_exact_operands(data, case):
    """With exact partial sums every summation order reaches the same fp32 value, and the epilogue is the
    shared one: output (and the saved GELU pre-activation) are C.gemm's bit for bit at every shape."""
    C = require_native()
    for M, N, K in SHAPES:
        x, w = data.xe[:M, :K].contiguous(), data.we[:N, :K].contiguous()
        bias, res = data.bias[:N].contiguous(), data.res[:M, :N].contiguous()
        y, aux = _run(_skinny(C), x, w, case, bias, res, M, N)
        y0, aux0 = _run(_gemm(C), x, w, case, bias, res, M, N)
        assert torch.equal(_bits(y), _bits(y0)), (case, M, N, K)
        if aux is not None:
            assert torch.equal(_bits(aux), _bits(aux0)), (case, M, N, K)


@pytest.mark.parametrize("case", CASES)
def test_random_operands_within_derived_bound(data, case):
    C = require_native()
    used = 0.0
    for M, N, K in SHAPES:
        x, w = data.xr[:M, :K].contiguous(), data.wr[:N, :K].contiguous()
        bias, res = data.bias[:N].contiguous(), data.res[:M, :N].contiguous()
        y, aux = _run(_skinny(C), x, w, case, bias, res, M, N)
        A64, B64 = x.double(), w.double().t()
        terms = {"bias": bias.double()[None, :].expand(M, N)}
        if case == "bias_res":
            terms["res"] = res.double()
        exp = gemm_expected(A64, B64, terms)
        pre = aux if case == "gelu" else y
        assert_within(pre, exp, gemm_bound(A64, B64, K, terms, pre.dtype), f"{case} {(M, N, K)}")
        if pre.dtype == BF:
            used = max(used, bf16_t_used(pre, exp, gemm_t32(A64, B64, K, terms)))
        if case == "gelu":
            a64 = aux.double()
            assert_within(y, gelu64(a64), gelu_out_bound(a64), f"gelu out {(M, N, K)}")
    print(f"{case}: bf16_t_used {used:.4f} of the fp32 allowance over {len(SHAPES)} shapes")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", [(1, 16, 32), (3, 48, 96), (17, 272, 1056), (64, 48, 1024)])
def test_strided_views_and_guards(data, case, shape):
    """X, Y, aux and res as guarded views (ld = cols + 8, column offset 8): the buffer's rows after row M - 1 of X
    hold NaN, nothing outside the output views is written, and the output has the contiguous run's bits."""
    C = require_native()
    M, N, K = shape
    dev = data.xr.device
    x, w = data.xr[:M, :K].contiguous(), data.wr[:N, :K].contiguous()
    bias, res = data.bias[:N].contiguous(), data.res[:M, :N].contiguous()
    y0, aux0 = _run(_skinny(C), x, w, case, bias, res, M, N)
    xbuf, xv = guarded_like(x, ld=K + 8, col_off=8)
    assert bool(torch.isnan(xbuf[M + 1]).all())  # the row after X's last
    rbuf, rv = guarded_like(res, ld=N + 8, col_off=8)
    ybuf, yv = guarded(M, N, y0.dtype, dev, ld=N + 8, col_off=8)
    abuf, av = guarded(M, N, BF, dev, ld=N + 8, col_off=8)
    C.gemm_skinny(xv, w, yv, bias=bias, aux=av if case == "gelu" else None, res=rv if case == "bias_res" else None,
                  mode=1 if case == "gelu" else 0)
    assert torch.equal(_bits(yv.contiguous()), _bits(y0))
    assert_guard_intact(ybuf, yv)
    if case == "gelu":
        assert torch.equal(_bits(av.contiguous()), _bits(aux0))
        assert_guard_intact(abuf, av)
    else:
        assert_guard_intact(abuf, (0, 0, 0, 0))  # never handed over, never touched
    assert_guard_intact(xbuf, xv)
    assert_guard_intact(rbuf, rv)


@pytest.mark.parametrize("case", ("bias_res", "bias_f32", "gelu"))
def test_nan_row_stays_in_its_row(data, case):
    C = require_native()
    N, K = 272, 1056
    w, bias = data.wr[:N, :K].contiguous(), data.bias[:N].contiguous()
    for M, m in ((3, 1), (17, 16), (17, 3), (64, 47)):
        x, res = data.xr[:M, :K].contiguous(), data.res[:M, :N].contiguous()
        y0, aux0 = _run(_skinny(C), x, w, case, bias, res, M, N)
        xn = x.clone()
        xn[m] = float("nan")
        y, aux = _run(_skinny(C), xn, w, case, bias, res, M, N)
        keep = torch.arange(M, device=x.device) != m
        for got, clean in ((y, y0), (aux, aux0)):
            if got is None:
                continue
            assert bool(torch.isnan(got[m]).all()), (case, M, m)
            assert torch.equal(_bits(got[keep]), _bits(clean[keep])), (case, M, m)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("nk", [(272, 1056), (48, 96), (16, 32)])
def test_row_zero_does_not_depend_on_the_batch(data, case, nk):
    """The partition depends on (N, K) only: row 0 of the result is the same bits for M = 1, 5, 16, 17, 64."""
    C = require_native()
    N, K = nk
    w, bias = data.wr[:N, :K].contiguous(), data.bias[:N].contiguous()
    rows = []
    for M in (1, 5, 16, 17, 64):
        x, res = data.xr[:M, :K].contiguous(), data.res[:M, :N].contiguous()
        y, aux = _run(_skinny(C), x, w, case, bias, res, M, N)
        rows.append((M, _bits(y)[0].clone(), None if aux is None else _bits(aux)[0].clone()))
    for M, y, aux in rows[1:]:
        assert torch.equal(y, rows[0][1]), (case, nk, M)
        if aux is not None:
            assert torch.equal(aux, rows[0][2]), (case, nk, M)


def test_refusals(dev):
    C = require_native()
    assert C.gemm_skinny_max_rows() == 64
    z = lambda r, c, dt=BF: torch.zeros(r, c, dtype=dt, device=dev)
    good = dict(X=z(4, 64), W=z(32, 64), Y=z(4, 32))
    C.gemm_skinny(**good)  # the baseline the refusals vary
    torch.cuda.synchronize()
    sentinel = torch.full((65, 32), 7.0, dtype=BF, device=dev)
    bad = [
        dict(X=z(65, 64), W=z(32, 64), Y=sentinel),                          # M = 65
        dict(X=z(4, 64), W=z(24, 64), Y=z(4, 24)),                            # N = 24
        dict(X=z(4, 48), W=z(32, 48), Y=z(4, 32)),                            # K = 48
        dict(good, aux=z(4, 32), mode=2),                                     # dGELU
        dict(good, mode=3),                                                   # tanh
        dict(good, X=z(4, 64, torch.float16)),                                # a float16 operand
        dict(good, W=z(64, 32).t()),                                          # a k-strided operand
        dict(good, mode=1),                                                   # GELU without aux
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            C.gemm_skinny(**kw)
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())  # refused before any launch
