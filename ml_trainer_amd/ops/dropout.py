"""The dropout mask in plain torch: the oracle of csrc/include/mlt_philox.h.

One definition, shared with the HIP kernels (dropout.hip, the dropout variants of the LayerNorm
kernels in layernorm.hip): flat element ``e = row * D + col`` of a ``[rows, D]`` tensor at dropout
site ``site`` takes word ``e & 3`` of

    philox4x32-10(counter = (lo32(e >> 2), hi32(e >> 2), site, rank), key = (lo32(seed), hi32(seed)))

and is kept iff ``word >= thr`` with ``thr = min(int(p * 2**32), 0xFFFFFFFF)``; kept elements are
scaled by ``1 / (1 - p)`` (computed in double, rounded once to fp32). Sites: 0 = embedding output
(after its LayerNorm), ``1 + 2 l`` = attention sub-layer of layer ``l``, ``2 + 2 l`` = its FFN
sub-layer. ``rank`` is the data-parallel rank, so ranks draw different masks from one seed.

Attention-probability dropout (inside the flash attention kernels, attention.hip) has ``B*H*S*S``
elements per layer, recomputed by three kernels, so it spends one BYTE per element and one Philox
call per 4 x 4 tile of (query, key). With ``T = ceil(S / 4)`` and

    vec = ((b * H + h) * T + (q >> 2)) * T + (k >> 2)

element ``(b, h, q, k)`` takes byte ``k & 3`` (little-endian: ``>> 8 * (k & 3)``) of word ``q & 3`` of
the same ``philox4x32-10(counter = (lo32(vec), hi32(vec), site, rank), key = seed words)`` and is kept
iff ``byte >= thr8`` with ``thr8 = round(p * 256)``. The probability actually applied is ``p_eff =
thr8 / 256`` (``p = 0.1`` -> ``26 / 256 = 0.1015625``) and kept probabilities are scaled by
``1 / (1 - p_eff)`` (double, rounded once to fp32), so the expectation is exact for ``p_eff``. A ``p > 0``
that rounds to ``thr8 == 0`` is an error, not a silent no-op. ``S`` need not be a multiple of 4 (edge
tiles are partly used). Sites: ``attention_site(l) = 0x40000000 + l``, disjoint from the hidden sites.

Everything here is int64 tensor arithmetic that runs on CPU and GPU tensors alike: the CPU model
path trains with the same masks, and the GPU tests compare the kernels against it bit for bit.
"""
from __future__ import annotations

import torch

_M0, _M1 = 0xD2511F53, 0xCD9E8D57  # round multipliers
_W0, _W1 = 0x9E3779B9, 0xBB67AE85  # Weyl key increments
_MASK32 = 0xFFFFFFFF


def _mulhilo(m: int, b: torch.Tensor):
    """(hi32, lo32) of the 64-bit product m * b, for a 32-bit constant m and b in [0, 2^32) held
    in int64 (two 48-bit partial products: no int64 overflow)."""
    p0 = m * (b & 0xFFFF)
    p1 = m * (b >> 16)
    s = ((p1 & 0xFFFF) << 16) + (p0 & _MASK32)
    return (p1 >> 16) + (p0 >> 32) + (s >> 32), s & _MASK32


def philox4x32(counter: torch.Tensor, key: torch.Tensor) -> torch.Tensor:
    """Philox4x32-10. ``counter`` [..., 4] and ``key`` [..., 2] are int64 tensors of 32-bit words
    (key broadcasts against counter); returns the four output words, int64 [..., 4]."""
    c0, c1, c2, c3 = (counter[..., i] & _MASK32 for i in range(4))
    k0, k1 = key[..., 0] & _MASK32, key[..., 1] & _MASK32
    for _ in range(10):
        hi0, lo0 = _mulhilo(_M0, c0)
        hi1, lo1 = _mulhilo(_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + _W0) & _MASK32
        k1 = (k1 + _W1) & _MASK32
    return torch.stack((c0, c1, c2, c3), dim=-1)


def threshold(p: float) -> int:
    """Keep iff word >= threshold(p)."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability must satisfy 0 <= p < 1, got {p}")
    return min(int(p * 4294967296.0), 0xFFFFFFFF)


def scale(p: float) -> float:
    """1 / (1 - p) as the kernels apply it: computed in double, rounded once to fp32."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability must satisfy 0 <= p < 1, got {p}")
    return torch.tensor(1.0 / (1.0 - p), dtype=torch.float64).to(torch.float32).item()


def keep_mask(seed: int, site: int, rank: int, rows: int, D: int, p: float, device=None) -> torch.Tensor:
    """bool [rows, D]: True where the element survives dropout ``p`` at (seed, site, rank)."""
    thr = threshold(p)
    n = rows * D
    vec = torch.arange((n + 3) // 4, dtype=torch.int64, device=device)
    counter = torch.stack((vec & _MASK32, vec >> 32, torch.full_like(vec, site & _MASK32),
                           torch.full_like(vec, rank & _MASK32)), dim=-1)
    key = torch.tensor([seed & _MASK32, (seed >> 32) & _MASK32], dtype=torch.int64, device=device)
    words = philox4x32(counter, key).reshape(-1)[:n]
    return (words >= thr).view(rows, D)


ATTENTION_SITE0 = 0x40000000  # attention-probability sites: ATTENTION_SITE0 + layer


def attention_threshold(p: float) -> int:
    """thr8 = round(p * 256) (halves up): an attention probability is kept iff its byte >= thr8."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f"attention dropout probability must satisfy 0 <= p < 1, got {p}")
    thr8 = int(p * 256.0 + 0.5)
    if p > 0.0 and thr8 == 0:
        raise ValueError(f"attention dropout probability {p} rounds to 0/256: no element would be dropped "
                         "(the smallest effective p is 1/256)")
    if thr8 >= 256:
        raise ValueError(f"attention dropout probability {p} rounds to 256/256: every element dropped")
    return thr8


def attention_p(p: float) -> float:
    """p_eff = thr8 / 256: the probability the byte rule actually applies for a requested ``p``."""
    return attention_threshold(p) / 256.0


def attention_scale(p: float) -> float:
    """1 / (1 - p_eff) as the kernels apply it: computed in double, rounded once to fp32."""
    return torch.tensor(1.0 / (1.0 - attention_p(p)), dtype=torch.float64).to(torch.float32).item()


def attention_site(l: int) -> int:
    """Dropout site of layer ``l``'s attention probabilities."""
    return ATTENTION_SITE0 + l


def attention_keep_mask(seed: int, site: int, rank: int, B: int, H: int, S: int, p: float,
                        device=None) -> torch.Tensor:
    """bool [B, H, S, S]: True where attention probability (b, h, q, k) survives dropout ``p``."""
    thr8 = attention_threshold(p)
    T = (S + 3) // 4
    vec = torch.arange(B * H * T * T, dtype=torch.int64, device=device)
    counter = torch.stack((vec & _MASK32, vec >> 32, torch.full_like(vec, site & _MASK32),
                           torch.full_like(vec, rank & _MASK32)), dim=-1)
    key = torch.tensor([seed & _MASK32, (seed >> 32) & _MASK32], dtype=torch.int64, device=device)
    words = philox4x32(counter, key)  # [tiles, 4 queries]
    shifts = torch.arange(4, dtype=torch.int64, device=device) * 8
    byts = (words[..., None] >> shifts) & 0xFF  # [tiles, 4 queries, 4 keys]
    keep = (byts >= thr8).view(B, H, T, T, 4, 4).permute(0, 1, 2, 4, 3, 5).reshape(B, H, 4 * T, 4 * T)
    return keep[:, :, :S, :S]


def apply(x: torch.Tensor, p: float, seed: int, site: int, rank: int) -> torch.Tensor:
    """Reference dropout of a [rows, D] tensor in its own dtype: ``keep ? dtype(float(x) * scale) : 0``
    (for bf16 ``x`` the rounding the kernels apply to a stand-alone dropout output)."""
    keep = keep_mask(seed, site, rank, x.shape[0], x.shape[1], p, x.device)
    y = (x.float() * scale(p)).to(x.dtype)
    return torch.where(keep, y, torch.zeros_like(y))


def data_parallel_rank() -> int:
    """The ``rank`` word of the counter: the data-parallel rank, 0 when not distributed."""
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
