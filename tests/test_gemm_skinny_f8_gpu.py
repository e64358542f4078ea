"""``C.gemm_skinny_f8`` / ``C.gemm_skinny_glu_f8`` (csrc/kernels/gemm_skinny_f8.hip), the fp8-weight skinny GEMMs.

K in {32, 96, 1024, 1056, 2144}: the 32-k tail step only; one 64-k double step and the tail (fewer steps than waves);
16 double steps (an even split); the same plus the tail; 33 plus the tail (a second, partial batch of loads and the
odd last double step). The reference operand is always the dequantised weight of the torch quantiser, so
``helpers.gemm_bound`` / ``gelu_out_bound`` apply unchanged."""
import itertools

import pytest
import torch

from ml_trainer_amd.ops import decode as DC
from ml_trainer_amd.ops._ext import require_native
from tests.helpers import (assert_guard_intact, assert_within, gelu64, gelu_out_bound, gemm_bound, gemm_expected,
                           guarded)

pytestmark = pytest.mark.gpu

MS, NS, KS = (1, 3, 16, 17, 64), (16, 48, 272), (32, 96, 1024, 1056, 2144)
MMAX, NMAX, KMAX = max(MS), max(NS), max(KS)
CASES = ("bias", "bias_res", "bias_f32", "gelu")
BF, F32 = torch.bfloat16, torch.float32


class _Data:
    def __init__(self, dev):
        g = torch.Generator().manual_seed(23)
        tri = lambda *s: torch.randint(-1, 2, s, generator=g).float() / 4
        # exact operands: {-1, 0, 1} / 4, row n of W times 2^(n % 5 - 2) (neighbouring rows, other scales): every
        # partial sum is a multiple of 2^-6 below 2^10, exact in fp32 in any order
        self.xe = tri(MMAX, KMAX).to(BF).to(dev)
        self.we = tri(NMAX, KMAX) * torch.exp2((torch.arange(NMAX) % 5 - 2).float())[:, None]
        self.xr = torch.randn(MMAX, KMAX, generator=g).to(BF).to(dev)
        self.wr = torch.randn(NMAX, KMAX, generator=g) * 0.05
        self.bias = (torch.randn(NMAX, generator=g) * 2).to(dev)
        self.res = (torch.randn(MMAX, NMAX, generator=g) * 2).to(BF).to(dev)

    def weight(self, w, N, K):
        """(codes, scales, dequantised bf16) of ``w[:N, :K]`` on the device."""
        codes, scales = DC.weight_quantize_reference(w[:N, :K].contiguous())
        deq = DC.kv_dequantize_reference(codes, scales)
        assert torch.equal(deq.to(BF).float(), deq)  # a bf16 number
        return codes.to(self.bias.device), scales.to(self.bias.device), deq.to(BF).to(self.bias.device)


@pytest.fixture(scope="module")
def data():
    return _Data(torch.device("cuda", 0))


def _run(fn, x, case, bias, res, M, N):
    """One launch of ``fn(x, y, bias=, aux=, res=, mode=)`` into guarded outputs for ``case``: (y, aux or None)."""
    ybuf, y = guarded(M, N, F32 if case == "bias_f32" else BF, x.device, ld=N + 8, col_off=8)
    abuf, aux = guarded(M, N, BF, x.device, ld=N + 8, col_off=8)
    fn(x, y, bias=bias, aux=aux if case == "gelu" else None, res=res if case == "bias_res" else None,
       mode=1 if case == "gelu" else 0)
    assert_guard_intact(ybuf, y)
    assert_guard_intact(abuf, aux if case == "gelu" else (0, 0, 0, 0))
    return y.contiguous(), aux.contiguous() if case == "gelu" else None


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


@pytest.mark.parametrize("case", CASES)
def test_same_bits_as_gemm_skinny_on_exact_operands(data, case):
    """(a) Exact partial sums: output and pre-activation are ``C.gemm_skinny(x, dequant(W8).bf16)`` bit for bit."""
    C = require_native()
    for N, K in itertools.product(NS, KS):
        codes, scales, deq = data.weight(data.we, N, K)
        for M in MS:
            x, bias, res = data.xe[:M, :K].contiguous(), data.bias[:N].contiguous(), data.res[:M, :N].contiguous()
            y, aux = _run(lambda x, y, **kw: C.gemm_skinny_f8(x, codes, scales, y, **kw), x, case, bias, res, M, N)
            y0, aux0 = _run(lambda x, y, **kw: C.gemm_skinny(x, deq, y, **kw), x, case, bias, res, M, N)
            assert torch.equal(_bits(y), _bits(y0)), (case, M, N, K)
            if aux is not None:
                assert torch.equal(_bits(aux), _bits(aux0)), (case, M, N, K)


@pytest.mark.parametrize("case", CASES)
def test_random_operands_within_derived_bound_and_batch_invariant(data, case):
    """(b) fp64 ``gemm_expected`` on the dequantised weight within the bf16 kernel's derived bound; (c) rows 0 .. 2 of
    the M = 16 and M = 64 runs are the M = 3 run bit for bit."""
    C = require_native()
    for N, K in itertools.product(NS, KS):
        codes, scales, deq = data.weight(data.wr, N, K)
        B64, bias = deq.double().t(), data.bias[:N].contiguous()
        first = {}
        for M in MS:
            x, res = data.xr[:M, :K].contiguous(), data.res[:M, :N].contiguous()
            y, aux = _run(lambda x, y, **kw: C.gemm_skinny_f8(x, codes, scales, y, **kw), x, case, bias, res, M, N)
            A64 = x.double()
            terms = dict(bias=bias.double()[None, :].expand(M, N), **({"res": res.double()} if case == "bias_res" else {}))
            pre = aux if case == "gelu" else y
            assert_within(pre, gemm_expected(A64, B64, terms), gemm_bound(A64, B64, K, terms, pre.dtype),
                          f"{case} {(M, N, K)}")
            if case == "gelu":
                assert_within(y, gelu64(aux.double()), gelu_out_bound(aux.double()), f"gelu out {(M, N, K)}")
            if M in (3, 16, 64):
                first[M] = [_bits(t)[:3].clone() for t in (y, aux) if t is not None]
        for M in (16, 64):
            assert all(torch.equal(a, b) for a, b in zip(first[M], first[3])), (case, M, N, K)


def test_every_code_and_the_scale_index(dev):
    """(d) K = 256, N = 16: row n of W8 holds the 256 byte values rotated by n (NaN codes replaced by 0), mixed
    power-of-two scales, X the four 64-row slices of the identity: the fp32 output must be ``value(code) * d``
    exactly, subnormals and signs included. (g) One code, sixteen different scales: a wrong scale index shows."""
    C = require_native()
    n = torch.arange(16)
    codes = ((torch.arange(256)[None, :] + n[:, None]) % 256).to(torch.uint8)
    codes[(codes & 0x7F) == 0x7F] = 0
    scales = torch.exp2(((n * 7) % 16 - 8).float())
    want = DC.kv_dequantize_reference(codes, scales)  # [16, 256] fp32, exact
    eye = torch.eye(256, dtype=BF, device=dev)
    for j in range(4):
        y = torch.empty(64, 16, dtype=F32, device=dev)
        C.gemm_skinny_f8(eye[64 * j:64 * j + 64].contiguous(), codes.to(dev), scales.to(dev), y)
        assert torch.equal(y.cpu(), want[:, 64 * j:64 * j + 64].t()), j  # (values: the code of -0 sums to +0)
    same = torch.full((16, 64), 0x3C, dtype=torch.uint8)  # 0x3C = 1.5
    scales = torch.exp2((n - 8).float())
    y = torch.empty(1, 16, dtype=F32, device=dev)
    C.gemm_skinny_f8(torch.ones(1, 64, dtype=BF, device=dev), same.to(dev), scales.to(dev), y)
    assert torch.equal(y.cpu()[0], 96.0 * scales)


def test_glu_form_equals_gemm_then_swiglu(data):
    """(e) ``C.gemm_skinny_glu_f8`` is ``C.gemm_skinny_f8`` with N = 2F followed by ``C.swiglu_fwd``, bit for bit."""
    C, dev = require_native(), data.bias.device
    for Fh, K in itertools.product((16, 48), KS):
        codes, scales, _ = data.weight(data.wr, 2 * Fh, K)
        bias = data.bias[:2 * Fh].contiguous()
        for M in MS:
            x = data.xr[:M, :K].contiguous()
            h1 = torch.empty(M, 2 * Fh, dtype=BF, device=dev)
            C.gemm_skinny_f8(x, codes, scales, h1, bias=bias)
            want = torch.empty(M, Fh, dtype=BF, device=dev)
            C.swiglu_fwd(h1, want)
            buf, got = guarded(M, Fh, BF, dev, ld=Fh + 8, col_off=8)
            C.gemm_skinny_glu_f8(x, codes, scales, got, bias=bias)
            assert_guard_intact(buf, got)
            assert torch.equal(_bits(got.contiguous()), _bits(want)), (M, Fh, K)


def test_refusals(dev):
    C = require_native()
    z = lambda r, c, dt=BF: torch.zeros(r, c, dtype=dt, device=dev)
    one = lambda n: torch.ones(n, dtype=F32, device=dev)
    good = dict(X=z(4, 64), W8=z(32, 64, torch.uint8), wscale=one(32), Y=z(4, 32))
    C.gemm_skinny_f8(**good)  # the baseline the refusals vary
    sentinel = torch.full((65, 32), 7.0, dtype=BF, device=dev)
    # int8 codes, bf16 codes, a scale vector of the wrong length (short, long), K = 48, M = 65
    for kw in (dict(good, W8=z(32, 64, torch.int8)), dict(good, W8=z(32, 64)), dict(good, wscale=one(31)),
               dict(good, wscale=one(48)), dict(good, X=z(4, 48), W8=z(32, 48, torch.uint8)),
               dict(good, X=z(65, 64), Y=sentinel)):
        with pytest.raises(RuntimeError):
            C.gemm_skinny_f8(**kw)
    with pytest.raises(RuntimeError):
        C.gemm_skinny_glu_f8(z(4, 64), z(32, 64, torch.uint8), one(31), z(4, 16))
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())  # refused before any launch
