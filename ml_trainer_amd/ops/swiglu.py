"""SwiGLU: the activation of the gated feed-forward (``BertConfig.ffn = "swiglu"``).

``h1`` [rows, 2F] is FFN1's output: columns ``[0, F)`` the gate ``g``, ``[F, 2F)`` the up-projection ``u``.

    s  = 1 / (1 + exp(-g))
    a  = (g * s) * u
    du = da * (g * s)
    dg = (da * u) * (s * (1 + g * (1 - s)))

``swiglu_reference`` / ``swiglu_bwd_reference`` are that definition in plain torch, in any dtype: the CPU path and
the tests' definition. Given bf16 they widen to fp32 and round ``a``, ``dg`` and ``du`` to bf16 once, which are the
rounding points of the kernels (csrc/include/mlt_swiglu.h; the kernels' exp and reciprocal are the hardware's 1-ulp
forms, so they agree with these to a few fp32 ulps before that rounding, not bit for bit). ``exp(-g)`` may overflow
to ``+inf`` for very negative ``g``: ``s`` is then 0, ``a`` is +-0 and ``dg`` 0, with no branch.

``swiglu_fwd`` / ``swiglu_bwd`` launch the streaming kernels of csrc/kernels/swiglu.hip; ``swiglu`` is the
differentiable torch form the reference models call (its backward is ``swiglu_bwd_reference``).
"""
from __future__ import annotations

import torch

from ml_trainer_amd.ops._ext import require_native


def _widen(t):
    return t.float() if t.dtype == torch.bfloat16 else t


def swiglu_reference(h1):
    """a [..., F] from h1 [..., 2F], in the dtype of ``h1`` (bf16: computed in fp32, rounded once)."""
    F = h1.shape[-1] // 2
    w = _widen(h1)
    g, u = w[..., :F], w[..., F:]
    s = 1.0 / (1.0 + torch.exp(-g))
    return ((g * s) * u).to(h1.dtype)


def swiglu_bwd_reference(da, h1):
    """dh1 [..., 2F] = dg | du from da [..., F] and h1, in the dtype of ``h1``."""
    F = h1.shape[-1] // 2
    w, d = _widen(h1), _widen(da)
    g, u = w[..., :F], w[..., F:]
    s = 1.0 / (1.0 + torch.exp(-g))
    du = d * (g * s)
    dg = (d * u) * (s * (1.0 + g * (1.0 - s)))
    return torch.cat((dg, du), -1).to(h1.dtype)


class _Swiglu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h1):
        ctx.save_for_backward(h1)
        return swiglu_reference(h1)

    @staticmethod
    def backward(ctx, da):
        return swiglu_bwd_reference(da.to(ctx.saved_tensors[0].dtype), ctx.saved_tensors[0])


def swiglu(h1):
    """``swiglu_reference`` as an autograd node whose backward is ``swiglu_bwd_reference``: autograd through
    ``exp(-g) = inf`` would give ``inf * 0``, the written-out gradient gives 0."""
    return _Swiglu.apply(h1)


def swiglu_fwd(h1):
    """a [rows, F] bf16 from h1 [rows, 2F] bf16 (row stride a multiple of 8) on the GPU: ``C.swiglu_fwd``."""
    a = torch.empty(h1.shape[0], h1.shape[1] // 2, dtype=torch.bfloat16, device=h1.device)
    require_native().swiglu_fwd(h1, a)
    return a


def swiglu_bwd(da, h1, db1, accumulate: bool = False):
    """dh1 [rows, 2F] bf16 on the GPU (``C.swiglu_bwd``), and ``db1`` fp32 [2F] set to (``accumulate``: increased by)
    the column sums of the rounded dh1: FFN1's bias gradient, summed in one fixed order."""
    C = require_native()
    dh1 = torch.empty_like(h1, memory_format=torch.contiguous_format)
    part = torch.empty(C.swiglu_partial_blocks(h1.shape[0]) * h1.shape[1], dtype=torch.float32, device=h1.device)
    C.swiglu_bwd(da, h1, dh1, part, db1, accumulate)
    return dh1
