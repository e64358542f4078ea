"""Incremental decoding: the key/value cache and single-token attention over it.

One layer's cache is ``kv`` [2, B, H, Smax, 64]: ``kv[0]`` the keys, ``kv[1]`` the values, head-major, so the
key stream of one (b, h) is contiguous. ``pos`` (int32 [B], on the device) is the number of tokens sequence b
has cached = the row its next token takes. Rows ``j > pos[b]`` are stale memory and never enter the arithmetic.
``pos`` never leaves the device: a decode step reads nothing back, so it can be captured in a graph.

``attn_decode`` is the native kernel (csrc/kernels/attn_decode.hip: bf16 cache, the append of the new token
fused in); ``attn_decode_reference`` the same function in plain fp32 torch (the CPU path and the oracle of the
tests). ``fill_from_prefill`` copies a prompt's K / V out of the padded forward's QKV buffer with torch ops: once
per layer per prompt, not a hot path.

``linear_small`` is the linear layer of a decode step (M = B rows): ``decode_linear_path`` sends it to the
weight-streaming kernel ``C.gemm_skinny`` (csrc/kernels/gemm_skinny.hip) or to the planner's GEMM. With the skinny
kernel every kernel of a step works row by row, so a sequence's logits do not depend on the batch it is decoded in.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Optional

import torch
import torch.nn.functional as F

from ml_trainer_amd.ops._ext import require_native

HEAD_DIM = 64
ATTN_SCALE = 1.0 / 8.0  # 1/sqrt(head_dim = 64)
# rows up to which a decode step's linears take C.gemm_skinny (the kernel itself takes C.gemm_skinny_max_rows() =
# 64): the largest of 16 / 32 / 64 at which it beat C.gemm at EVERY bert-base decode shape by more than C.gemm's
# run-to-run spread. At 32 rows the vocabulary decoder ties (20.7 against 20.5 us), at 64 the decoder and FFN2
# lose: every workgroup re-reads X from L2 (profiles/generate/README.md has the table).
SKINNY_MAX_ROWS = 16


@dataclass
class KVCache:
    """``kv[l]`` [2, B, H, Smax, 64] per layer (bf16 on the GPU, fp32 on the CPU), ``pos`` int32 [B] on the
    same device, ``Smax`` the rows per sequence."""
    kv: List[torch.Tensor]
    pos: torch.Tensor
    Smax: int

    @classmethod
    def allocate(cls, layers: int, B: int, H: int, Smax: int, device, dtype=None) -> "KVCache":
        device = torch.device(device)
        if dtype is None:
            dtype = torch.bfloat16 if device.type == "cuda" else torch.float32
        if Smax < 1:
            raise ValueError(f"a cache needs Smax >= 1, got {Smax}")
        # zeros, not empty: stale rows are never used, but a cache that is inspected should not show garbage
        kv = [torch.zeros(2, B, H, Smax, HEAD_DIM, dtype=dtype, device=device) for _ in range(layers)]
        return cls(kv, torch.zeros(B, dtype=torch.int32, device=device), Smax)


@dataclass
class DecodeState:
    """What ``prefill`` hands to ``decode_step``: the cache (with ``pos``) and the hidden row [B, h] of every
    sequence's last token, from which the next token's logits come."""
    cache: KVCache
    hidden: torch.Tensor

    @property
    def pos(self) -> torch.Tensor:
        return self.cache.pos


def attn_decode(qkv_new, cache_layer, pos, H: int, scale: float = ATTN_SCALE):
    """out [B, H * 64] bf16 = attention of the B new tokens' queries over their cached keys and themselves;
    rows ``pos[b]`` of ``cache_layer`` become the new tokens' k / v (the native kernel). ``qkv_new``
    [B, 3 * H * 64] bf16 may be a row-strided view (row stride a multiple of 8)."""
    C = require_native()
    out = torch.empty(qkv_new.shape[0], H * HEAD_DIM, dtype=torch.bfloat16, device=qkv_new.device)
    C.attn_decode(qkv_new, cache_layer, pos, out, H, scale)
    return out


def attn_decode_reference(qkv_new, cache_layer, pos, H: int, scale: float = ATTN_SCALE):
    """``attn_decode`` in plain fp32 torch, on any device: appends into ``cache_layer`` (any float dtype) and
    returns out [B, H * 64] fp32. Stale rows are selected out (scores to -inf, values to 0), never multiplied
    by zero; nothing is read back from the device."""
    B = qkv_new.shape[0]
    Smax = cache_layer.shape[3]
    q, k, v = qkv_new.float().view(B, 3, H, HEAD_DIM).unbind(1)
    idx = pos.long()
    ar = torch.arange(B, device=qkv_new.device)
    cache_layer[0, ar, :, idx] = k.to(cache_layer.dtype)
    cache_layer[1, ar, :, idx] = v.to(cache_layer.dtype)
    j = torch.arange(Smax, device=qkv_new.device)
    cached = (j[None, :] < idx[:, None])[:, None, :]  # [B, 1, Smax]
    own = (j[None, :] == idx[:, None])[:, None, :]
    K = torch.where(own[..., None], k[:, :, None, :], cache_layer[0].float())  # the new token from qkv_new itself
    V = torch.where(own[..., None], v[:, :, None, :], cache_layer[1].float())
    valid = cached | own
    s = (K @ q[..., None])[..., 0] * scale  # [B, H, Smax]
    s = torch.where(valid, s, torch.full_like(s, float("-inf")))
    V = torch.where(valid[..., None], V, torch.zeros_like(V))
    p = torch.softmax(s, -1)
    return (p[:, :, None, :] @ V)[:, :, 0, :].reshape(B, H * HEAD_DIM)


def decode_linear_path(M: int, N: int, K: int) -> str:
    """Which kernel a decode step's linear ``[M, K] x [N, K]^T`` takes: ``"skinny"`` (the weight-streaming
    ``C.gemm_skinny``, whose summation order depends on (N, K) only, so a row's result does not depend on the
    batch) or ``"gemm"`` (the planner's tile kernels). A pure function of the shape and of ``MLT_DECODE_GEMM``
    (read per call; ``0`` forces ``"gemm"``: the launches of the model before the skinny kernel, the A/B switch)."""
    if os.environ.get("MLT_DECODE_GEMM", "1") == "0":
        return "gemm"
    if 1 <= M <= SKINNY_MAX_ROWS and N > 0 and K > 0 and N % 16 == 0 and K % 32 == 0:
        return "skinny"
    return "gemm"


def linear_small(x, w16, bias=None, gelu_aux=None, res=None, out=None):
    """``y = epilogue(x . w16^T)`` for the few rows of a decode step: x [M, K] bf16, w16 [N, K] bf16 (the layout
    of ``bf16_weight``), fp32 ``bias`` [N], ``gelu_aux`` [M, N] bf16 (GELU epilogue; receives the pre-activation),
    ``res`` [M, N] bf16 added last, ``out`` [M, N] bf16 or fp32 (default: a new bf16 tensor). The skinny kernel
    where ``decode_linear_path`` says so, otherwise the launches of ``transformer.linear_fwd``. On the CPU:
    ``F.linear`` and the same epilogue in fp32."""
    M, K = x.shape
    N = w16.shape[0]
    if not x.is_cuda:
        y = F.linear(x.float(), w16.float(), None if bias is None else bias.float())
        if gelu_aux is not None:
            gelu_aux.copy_(y)
            y = F.gelu(gelu_aux.float())
        if res is not None:
            y = y + res.float()
        return y if out is None else out.copy_(y)
    if decode_linear_path(M, N, K) == "skinny":
        if out is None:
            out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
        require_native().gemm_skinny(x, w16, out, bias=bias, aux=gelu_aux, res=res, mode=1 if gelu_aux is not None else 0)
        return out
    from ml_trainer_amd.ops import transformer as T
    if out is None:
        return T.linear_fwd(x, w16, bias, gelu_aux=gelu_aux, res=res)
    require_native().gemm(x, w16, out, False, False, bias=bias, aux=gelu_aux, res=res,
                          mode=1 if gelu_aux is not None else 0)
    return out


def fill_from_prefill(cache: KVCache, layer: int, qkv, lens: Optional[torch.Tensor], B: int, S: int) -> None:
    """Copy the K / V columns of a layer's padded ``qkv`` [B * S, 3 * H * 64] into rows 0 .. S - 1 of the
    head-major cache. Rows at and past ``lens[b]`` receive the pad positions' projections: they are stale by
    the definition of ``pos`` (the caller sets ``pos = lens``) and never read."""
    kv = cache.kv[layer]
    H = kv.shape[2]
    if S > cache.Smax:
        raise ValueError(f"a prompt of width {S} does not fit a cache of {cache.Smax} rows")
    x = qkv.view(B, S, 3, H, HEAD_DIM)
    kv[0, :, :, :S] = x[:, :, 1].permute(0, 2, 1, 3).to(kv.dtype)
    kv[1, :, :, :S] = x[:, :, 2].permute(0, 2, 1, 3).to(kv.dtype)


def sample_tokens(logits, temperature: float = 0.0, top_k: Optional[int] = None, generator=None):
    """Next tokens [B] (int64) from fp32 logits [B, V] with torch ops on the logits' device: the argmax at
    ``temperature == 0``, else one draw from softmax(logits / temperature) restricted to the ``top_k`` largest."""
    if temperature == 0:
        return logits.argmax(-1)
    z = logits.float() / temperature
    if top_k is not None and top_k < z.shape[-1]:
        kth = z.topk(top_k, dim=-1).values[:, -1:]
        z = torch.where(z < kth, torch.full_like(z, float("-inf")), z)
    return torch.multinomial(torch.softmax(z, -1), 1, generator=generator)[:, 0]
