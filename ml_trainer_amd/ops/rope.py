"""Rotary position embeddings (RoPE) in plain torch: the oracle of csrc/kernels/rope.hip and of the ROPE
instantiation of csrc/kernels/attn_decode.hip, and the CPU path of the models.

One definition, shared with the HIP kernels:

* **Table.** ``rope_table(P, base, device)`` is fp32 ``[P, 32, 2]``: for position ``p`` and pair ``i`` in 0..31 the
  angle is ``p * base ** (-2 i / 64)`` in float64; ``cos`` and ``sin`` are taken in float64 and each rounded once
  to fp32. Built on the host, copied to the device once and cached per ``(P, base, device)``. The kernels never
  evaluate a sine.
* **Pairs.** Within a head's 64 dims pair ``i`` is dims ``(2 i, 2 i + 1)`` (the interleaved form): a pair stays
  inside one 16-byte vector and inside one lane of ``attn_decode`` (lane ``c`` owns dims ``8 c .. 8 c + 7``).
* **Rotation.** A bf16 pair ``(a, b)`` widened to fp32, the table entry ``(c, s)`` of its position, ``sign = +1``
  forward and ``-1`` backward:

      a' = bf16_rn(a * c - b * (sign * s))        b' = bf16_rn(a * (sign * s) + b * c)

  Every product is rounded to fp32, then the sum or difference is rounded to fp32; nothing is contracted into an
  fma (the device uses ``__fmul_rn`` / ``__fadd_rn`` / ``__fsub_rn``). The fp32 tensor expression below performs
  exactly these roundings, so it is a bitwise oracle. The backward of the rotation is the rotation by the
  negative angle, applied to dq and dk.

Scores of rotated queries and keys depend on ``i - j`` only, there is no position table to train, and a key/value
cache stores already-rotated keys (a decode step rotates one new row per sequence).
"""
from __future__ import annotations

from typing import Optional

import torch

from ml_trainer_amd.ops._ext import require_native

HEAD_DIM = 64
PAIRS = HEAD_DIM // 2
DEFAULT_BASE = 10000.0

_TABLES = {}


def rope_angles(P: int, base: float = DEFAULT_BASE) -> torch.Tensor:
    """float64 ``[P, 32]``: the angle of position ``p`` and pair ``i``, ``p * base ** (-2 i / 64)``."""
    if P < 1:
        raise ValueError(f"a rope table needs P >= 1 positions, got {P}")
    if not base > 0:
        raise ValueError(f"rope base must be > 0, got {base}")
    i = torch.arange(PAIRS, dtype=torch.float64)
    inv = torch.tensor(float(base), dtype=torch.float64) ** (-2.0 * i / HEAD_DIM)
    return torch.arange(P, dtype=torch.float64)[:, None] * inv[None, :]


def rope_table64(P: int, base: float = DEFAULT_BASE) -> torch.Tensor:
    """float64 ``[P, 32, 2]`` (cos, sin) on the host: the table before its one rounding to fp32."""
    a = rope_angles(P, base)
    return torch.stack((torch.cos(a), torch.sin(a)), -1)


def rope_table(P: int, base: float = DEFAULT_BASE, device=None) -> torch.Tensor:
    """fp32 ``[P, 32, 2]`` on ``device``, cached per ``(P, base, device)`` (the same tensor on every call: its
    address is stable under a captured graph). Treat it as read-only."""
    device = torch.device("cpu" if device is None else device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(P), float(base), str(device))
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = rope_table64(P, base).to(torch.float32).to(device).contiguous()
    return t


def positions(rows: int, S: int, pos: Optional[torch.Tensor], P: int, device) -> torch.Tensor:
    """int64 [rows]: ``pos[row]`` clamped into ``[0, P)`` as the kernels clamp it, or ``row % S`` without ``pos``."""
    if pos is not None:
        return pos.to(device=device, dtype=torch.int64).clamp(0, P - 1)
    if not 0 < S <= P:
        raise ValueError(f"sequence length {S} does not fit a rope table of {P} positions")
    return torch.arange(rows, device=device) % S


def rotate(x: torch.Tensor, cs: torch.Tensor, sign: int = 1) -> torch.Tensor:
    """The rotation itself: ``x`` [..., 64] (any float dtype) against ``cs`` [..., 32, 2] (broadcastable), computed
    in the dtype of ``cs`` with separately rounded products, returned in that dtype (the caller rounds to bf16)."""
    xp = x.to(cs.dtype).reshape(*x.shape[:-1], PAIRS, 2)
    a, b = xp[..., 0], xp[..., 1]
    c, s = cs[..., 0], cs[..., 1] * float(sign)
    ya = a * c - b * s
    yb = a * s + b * c
    return torch.stack((ya, yb), -1).reshape(x.shape)


def rope_heads(x: torch.Tensor, table: torch.Tensor, pos: torch.Tensor, sign: int = 1) -> torch.Tensor:
    """``x`` [rows, H * 64] rotated head by head at positions ``pos`` (int64 [rows], in range), in ``x``'s dtype:
    bf16 in, bf16 out is the kernels' result bit for bit; fp32 in stays fp32 (``forward_reference``)."""
    rows = x.shape[0]
    cs = table.index_select(0, pos)[:, None]  # [rows, 1, 32, 2]
    return rotate(x.reshape(rows, -1, HEAD_DIM), cs, sign).to(x.dtype).reshape(x.shape)


def rope_qk_reference(qkv: torch.Tensor, table: torch.Tensor, H: int, S: int = 1,
                      pos: Optional[torch.Tensor] = None, sign: int = 1) -> torch.Tensor:
    """``rope_qk`` in plain torch, out of place, on any device: a copy of ``qkv`` [rows, 3 * H * 64] whose q and k
    columns are rotated and whose v columns are untouched."""
    rows, D = qkv.shape[0], H * HEAD_DIM
    if qkv.shape[1] != 3 * D:
        raise ValueError(f"qkv has {qkv.shape[1]} columns, expected 3 * H * 64 = {3 * D}")
    p = positions(rows, S, pos, table.shape[0], qkv.device)
    out = qkv.clone()
    out[:, :D] = rope_heads(qkv[:, :D], table, p, sign)
    out[:, D:2 * D] = rope_heads(qkv[:, D:2 * D], table, p, sign)
    return out


def rope_qk(qkv: torch.Tensor, table: torch.Tensor, H: int, S: int = 1, pos: Optional[torch.Tensor] = None,
            sign: int = 1) -> torch.Tensor:
    """Rotate the q and k columns of ``qkv`` [rows, 3 * H * 64] bf16 IN PLACE on the GPU (``C.rope_qk``; ``qkv`` may
    be a row-strided view with a row stride that is a multiple of 8) and return it. The position of a row is
    ``pos[row]`` (int32 [rows] on the device, clamped into the table) or ``row % S``. ``sign=-1``: the backward."""
    require_native().rope_qk(qkv, table, H, S, pos=pos, sign=sign)
    return qkv
