"""The summation order of ``C.gemm_skinny`` (csrc/kernels/gemm_skinny.hip) emulated in fp32 torch on the CPU, held
against ``helpers.gemm_bound``, and the routing function ``ops.decode.decode_linear_path``.

The emulation: 32-k step s belongs to wave (s >> 1) % 4; a wave adds its steps' 32-term products onto its own fp32
accumulator in increasing order; the four partials are summed in wave order; bias and residual follow; one rounding
to bf16. The bound has to hold for it at every shape of tests/test_gemm_skinny_gpu.py, and three defects a kernel
of this layout could have must leave it (a bound that a wrong result passes checks nothing)."""
import itertools

import pytest
import torch

from ml_trainer_amd.ops import decode as DC
from tests.helpers import gemm_bound, gemm_expected

MS, NS, KS = (1, 3, 16, 17, 33, 64), (16, 48, 272), (32, 96, 1024, 1056)
WAVES = 4


def _emulate(x, w, bias, res, drop_last_step=False, drop_wave=None, bias_shift=0):
    M, K = x.shape
    N = w.shape[0]
    xf, wf = x.float(), w.float()
    acc = [torch.zeros(M, N) for _ in range(WAVES)]
    nsteps = K // 32 - (1 if drop_last_step else 0)
    for s in range(nsteps):
        acc[(s >> 1) % WAVES] += xf[:, 32 * s:32 * s + 32] @ wf[:, 32 * s:32 * s + 32].t()
    total = torch.zeros(M, N)
    for i in range(WAVES):
        if i != drop_wave:
            total = total + acc[i]
    total = total + torch.roll(bias, -bias_shift)[None, :]
    if res is not None:
        total = total + res.float()
    return total.to(torch.bfloat16)


def _inputs(M, N, K, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(torch.bfloat16)
    bias = torch.randn(N, generator=g) * 2
    res = (torch.randn(M, N, generator=g) * 2).to(torch.bfloat16)
    return x, w, bias, res


def _outside(out, x, w, bias, res, K):
    terms = {"bias": bias.double()[None, :].expand(out.shape), "res": res.double()}
    A64, B64 = x.double(), w.double().t()
    err = (out.double() - gemm_expected(A64, B64, terms)).abs()
    return int((err > gemm_bound(A64, B64, K, terms, torch.bfloat16)).sum())


def test_kernel_order_stays_inside_gemm_bound():
    for M, N, K in itertools.product(MS, NS, KS):
        x, w, bias, res = _inputs(M, N, K)
        assert _outside(_emulate(x, w, bias, res), x, w, bias, res, K) == 0, (M, N, K)


@pytest.mark.parametrize("shape", [(17, 272, 1056), (3, 48, 96)])
@pytest.mark.parametrize("defect", [dict(drop_last_step=True), dict(drop_wave=1), dict(bias_shift=1)])
def test_defects_leave_the_bound(shape, defect):
    M, N, K = shape
    x, w, bias, res = _inputs(M, N, K)
    assert _outside(_emulate(x, w, bias, res, **defect), x, w, bias, res, K) > 0


def test_decode_linear_path(monkeypatch):
    monkeypatch.delenv("MLT_DECODE_GEMM", raising=False)
    top = DC.SKINNY_MAX_ROWS
    assert 16 <= top <= 64
    assert DC.decode_linear_path(1, 768, 768) == "skinny"
    assert DC.decode_linear_path(top, 30720, 768) == "skinny"
    assert DC.decode_linear_path(top + 1, 768, 768) == "gemm"      # the row limit
    assert DC.decode_linear_path(0, 768, 768) == "gemm"
    assert DC.decode_linear_path(8, 776, 768) == "gemm"            # N % 16
    assert DC.decode_linear_path(8, 768, 784) == "gemm"            # K % 32 (784 = 16 * 49)
    monkeypatch.setenv("MLT_DECODE_GEMM", "0")                     # read per call
    assert DC.decode_linear_path(1, 768, 768) == "gemm"
    monkeypatch.setenv("MLT_DECODE_GEMM", "1")
    assert DC.decode_linear_path(1, 768, 768) == "skinny"


def test_linear_small_on_the_cpu():
    x, w, bias, res = _inputs(5, 48, 96)
    y = DC.linear_small(x, w, bias, res=res)
    ref = torch.nn.functional.linear(x.float(), w.float(), bias) + res.float()
    assert torch.equal(y, ref)
    pre = torch.empty(5, 48, dtype=torch.bfloat16)
    a = DC.linear_small(x, w, bias, gelu_aux=pre)
    assert torch.equal(pre, torch.nn.functional.linear(x.float(), w.float(), bias).to(torch.bfloat16))
    assert torch.equal(a, torch.nn.functional.gelu(pre.float()))
