"""Grouped-query attention (GQA): ``Hkv < H`` key/value heads, each shared by ``G = H / Hkv`` query heads; query
head ``h`` reads KV head ``h // G`` (contiguous groups).

Two layouts of a QKV (or dQKV) row, 64 dims per head:

* **compact** ``q (H heads) | k (Hkv heads) | v (Hkv heads)``: what the QKV projection of a GQA model writes and
  what its weight gradient and dgrad read;
* **wide** ``q | k | v`` with H heads each: what the flash attention kernels read and write.

``gqa_expand`` (compact -> wide: every k / v head repeated G times, a bitwise copy) and ``gqa_reduce`` (wide dQKV ->
compact: dk / dv summed over the group) are the native kernels of csrc/kernels/gqa.hip; ``gqa_expand_reference`` /
``gqa_reduce_reference`` the same functions in plain torch: the CPU path and the bitwise oracle of the tests. The
reduction is defined as the sequential fp32 sum ``((x_0 + x_1) + ... + x_{G-1})`` in ascending head order, rounded
once to the input's dtype.

The decode side needs neither: ``ops.decode.attn_decode`` reads compact rows and a ``[2, B, Hkv, Smax, 64]`` cache
directly (``C.attn_decode_gqa``).
"""
from __future__ import annotations

from typing import Optional

import torch

from ml_trainer_amd.ops._ext import require_native

HEAD_DIM = 64


def check_kv_heads(heads: int, kv_heads: Optional[int]) -> int:
    """``kv_heads`` (None: ``heads``) as an int, after ``1 <= kv_heads <= heads`` and ``heads % kv_heads == 0``."""
    if kv_heads is None:
        return heads
    if not 1 <= kv_heads <= heads or heads % kv_heads:
        raise ValueError(f"kv_heads must divide heads = {heads} (1 <= kv_heads <= heads), got {kv_heads}")
    return int(kv_heads)


def compact_width(H: int, Hkv: int) -> int:
    return (H + 2 * Hkv) * HEAD_DIM


def infer_kv_heads(qkv_features: int, H: int) -> Optional[int]:
    """The ``kv_heads`` of a QKV projection with ``qkv_features`` outputs: None for the wide ``3 * H * 64``."""
    if qkv_features == 3 * H * HEAD_DIM:
        return None
    Hkv, rem = divmod(qkv_features - H * HEAD_DIM, 2 * HEAD_DIM)
    if rem or Hkv < 1:
        raise ValueError(f"a QKV projection of {qkv_features} features is neither 3 * H * 64 nor (H + 2 Hkv) * 64 "
                         f"for H = {H}")
    return check_kv_heads(H, Hkv)


def gqa_expand_reference(compact, H: int, Hkv: int):
    """[rows, (H + 2 Hkv) * 64] -> [rows, 3 * H * 64]: q as it is, every k / v head repeated ``H // Hkv`` times."""
    rows, G = compact.shape[0], H // Hkv
    q, k, v = compact.split((H * HEAD_DIM, Hkv * HEAD_DIM, Hkv * HEAD_DIM), dim=1)
    rep = lambda t: t.reshape(rows, Hkv, 1, HEAD_DIM).expand(rows, Hkv, G, HEAD_DIM).reshape(rows, H * HEAD_DIM)
    return torch.cat((q, rep(k), rep(v)), dim=1)


def gqa_reduce_reference(wide, H: int, Hkv: int, reverse: bool = False):
    """[rows, 3 * H * 64] -> [rows, (H + 2 Hkv) * 64]: dq as it is, dk / dv the sequential fp32 sum over the group
    in ascending head order (``reverse``: descending, which the tests use to show that the order matters), rounded
    once to ``wide``'s dtype."""
    rows, G = wide.shape[0], H // Hkv
    q, k, v = wide.split(H * HEAD_DIM, dim=1)

    def red(t):
        x = t.float().reshape(rows, Hkv, G, HEAD_DIM)
        order = range(G - 1, -1, -1) if reverse else range(G)
        acc = None
        for j in order:
            acc = x[:, :, j] if acc is None else acc + x[:, :, j]
        return acc.reshape(rows, Hkv * HEAD_DIM).to(wide.dtype)

    return torch.cat((q, red(k), red(v)), dim=1)


def gqa_expand(compact, H: int, Hkv: int):
    """``gqa_expand_reference`` on the native kernel (bf16 device rows; ``compact`` may be row-strided)."""
    if not compact.is_cuda:
        return gqa_expand_reference(compact, H, Hkv)
    wide = torch.empty(compact.shape[0], 3 * H * HEAD_DIM, dtype=compact.dtype, device=compact.device)
    require_native().gqa_expand(compact, wide, H, Hkv)
    return wide


def gqa_reduce(wide, H: int, Hkv: int):
    """``gqa_reduce_reference`` on the native kernel."""
    if not wide.is_cuda:
        return gqa_reduce_reference(wide, H, Hkv)
    compact = torch.empty(wide.shape[0], compact_width(H, Hkv), dtype=wide.dtype, device=wide.device)
    require_native().gqa_reduce(wide, compact, H, Hkv)
    return compact
