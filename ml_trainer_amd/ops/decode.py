"""Incremental decoding: the key/value cache and single-token attention over it.

One layer's cache is ``kv`` [2, B, H, Smax, 64]: ``kv[0]`` the keys, ``kv[1]`` the values, head-major, so the
key stream of one (b, h) is contiguous. ``pos`` (int32 [B], on the device) is the number of tokens sequence b
has cached = the row its next token takes. Rows ``j > pos[b]`` are stale memory and never enter the arithmetic.
``pos`` never leaves the device: a decode step reads nothing back, so it can be captured in a graph.

``attn_decode`` is the native kernel (csrc/kernels/attn_decode.hip: bf16 cache, the append of the new token
fused in); ``attn_decode_reference`` the same function in plain fp32 torch (the CPU path and the oracle of the
tests). ``fill_from_prefill`` copies a prompt's K / V out of the padded forward's QKV buffer with torch ops: once
per layer per prompt, not a hot path. Over a long cache (``decode_attn_path``) ``attn_decode`` launches
``C.attn_decode_split`` (csrc/kernels/attn_decode_split.hip): the cached keys of a head split over workgroups and a
merge launch, so that the whole machine fetches the cache of a small batch.

The fp8 cache (``KVCache.allocate(kv_cache="fp8")``): ``kv`` holds uint8 OCP e4m3 codes and ``scales`` one fp32
power-of-two scale per cached row. ``kv_quantize_reference`` / ``kv_dequantize_reference`` define the format;
``attn_decode`` then launches ``C.attn_decode_f8`` (csrc/kernels/attn_decode_f8.hip, single and split forms) and
``fill_from_prefill`` ``C.kv_fill_f8``; ``attn_decode_reference`` takes the same cache on the CPU.

``attn_append`` is the multi-token form (csrc/kernels/attn_append.hip): T = 1 .. 16 new tokens per sequence in one
launch, attending to the cache and causally to each other, their k / v appended at rows ``pos[b] .. pos[b] + T - 1``;
``pos`` is the caller's to advance, so accepting ``a <= T`` of them is ``pos += a`` and the rest is stale by
definition. It streams the cache once for the T tokens where T ``attn_decode`` launches stream it T times, on the
matrix cores; the bf16 cache only. ``attn_append_reference`` is its definition and CPU path;
``BertLMHeadModel.extend`` the model-level caller.

The paged cache (``PagePool`` / ``PagedKVCache``): the rows live in pages of ``PAGE_ROWS = 64`` rows drawn from one
pool, ``kv[l]`` [2, P, Hkv, 64, 64], and a sequence names its pages in a row of ``block_table`` (int32
[B, max_pages], on the device, written by the host; page 0 is the null page of every unowned entry). A sequence pays
for the rows it holds, grows past the reservation it started with and returns its pages when it is done.
``attn_decode(block_table=)`` launches ``C.attn_decode_paged`` (csrc/kernels/attn_decode_paged.hip: always split +
merge, the bits of ``C.attn_decode_split`` on the gathered cache), ``fill_from_prefill`` ``C.kv_fill_paged``;
``attn_decode_paged_reference`` is the definition and the CPU path. Paging is a layout, not a format: it is reached
through ``pool=`` / ``block_table=``, never through ``kv_cache=``.

``linear_small`` is the linear layer of a decode step (M = B rows): ``decode_linear_path`` sends it to the
weight-streaming kernel ``C.gemm_skinny`` (csrc/kernels/gemm_skinny.hip) or to the planner's GEMM. With the skinny
kernel every kernel of a step works row by row, so a sequence's logits do not depend on the batch it is decoded in.
``linear_small_glu`` is the gated FFN1 of a SwiGLU model's step: ``C.gemm_skinny_glu``, or the unfused pair.

fp8 layer weights (``DecodeState.weights = "fp8"``, set by ``prefill`` / ``generate(weights="fp8")``): weight-only
quantisation of the four layer linears of a decode step. ``weight_quantize_reference`` defines the format (e4m3
codes and one power-of-two scale per output row of the bf16-rounded weight), ``fp8_weight_rows`` caches it per
parameter, and ``linear_small(w8=)`` / ``linear_small_glu(w8=)`` launch ``C.gemm_skinny_f8`` /
``C.gemm_skinny_glu_f8`` (csrc/kernels/gemm_skinny_f8.hip), which stream half the bytes. The quantised layer is
exactly the bf16 layer on the dequantised weight. Prefill and the head keep the bf16 weights, and the fp32 masters
and bf16 copies remain: the option halves a step's weight traffic, it does not save memory.

``sample_step`` is the on-device sampler (csrc/kernels/sample.hip): greedy / temperature / top-k / top-p and the
token / EOS bookkeeping of ``generate`` in one launch per step, over a ``SamplerState``. Its result is defined in
integers (the definition is the header of csrc/include/mlt_sample.h and the docstring of
``sample_step_reference``, the same function in plain torch and the CPU path), so it is bitwise reproducible
and a row's tokens depend on ``(seed, seq_ids[b], draws[b])`` and its own logits only, never on the batch.
``sample_tokens`` is the older torch sampler (one ``multinomial`` stream for the whole batch); it is unchanged.
"""
from __future__ import annotations

import os
import struct
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
# cache rows from which a decode step's attention takes the split kernels (decode_attn_path): the smallest measured
# Smax (512, 2048, 8192, 32768; bert-base heads, Hkv 12 / 4 / 1) at which split + merge beat the single kernel at batch 1
# AND at batch 8 by more than the single kernel's run-to-run spread. At 512 they lose everywhere (7.8 against 6.2 us at
# batch 1: the second launch); at 2048 they win by 1.5 - 2.4 x, at 32768 by 2 - 10 x. At batch 64 with 12 KV heads the
# single kernel already fills the machine and the split form is 1 - 4 % slower (profiles/decode_split/README.md):
# the price of a routing that does not look at the batch; MLT_DECODE_SPLIT=0 is the switch.
DECODE_SPLIT_MIN_SMAX = 2048
# new tokens per sequence one attn_append launch takes (C.attn_append_max_tokens(): the 16 columns of the MFMA tile)
APPEND_MAX_TOKENS = 16
# rows of one page of a paged cache (C.attn_decode_paged_page_rows(): a compile-time constant of the kernels). A
# wave's 32-key run of the decode kernels lies inside one page, and a split of 256 keys is 4 pages.
PAGE_ROWS = 64


KV_CACHE_FORMATS = (None, "bf16", "fp8")


def check_kv_cache(kv_cache) -> bool:
    """True for the fp8 cache, False for ``None`` / ``"bf16"`` (the cache as it always was); anything else raises."""
    if kv_cache not in KV_CACHE_FORMATS:
        raise ValueError(f"kv_cache must be None, 'bf16' or 'fp8', got {kv_cache!r}")
    return kv_cache == "fp8"


@dataclass
class KVCache:
    """``kv[l]`` [2, B, H, Smax, 64] per layer (bf16 on the GPU, fp32 on the CPU), ``pos`` int32 [B] on the
    same device, ``Smax`` the rows per sequence. The fp8 cache (``allocate(kv_cache="fp8")``, any device): ``kv[l]``
    holds uint8 OCP e4m3 codes in the same layout and ``scales[l]`` fp32 [2, B, H, Smax] one power-of-two scale per
    cached row (``kv_quantize_reference`` is the format's definition); 68 bytes per row and tensor instead of 128."""
    kv: List[torch.Tensor]
    pos: torch.Tensor
    Smax: int
    scales: Optional[List[torch.Tensor]] = None

    @classmethod
    def allocate(cls, layers: int, B: int, H: int, Smax: int, device, dtype=None, kv_cache=None) -> "KVCache":
        device = torch.device(device)
        fp8 = check_kv_cache(kv_cache)
        if fp8 and dtype is not None:
            raise ValueError("an fp8 cache has uint8 codes and fp32 scales: dtype cannot be given with it")
        if dtype is None:
            dtype = torch.uint8 if fp8 else torch.bfloat16 if device.type == "cuda" else torch.float32
        if Smax < 1:
            raise ValueError(f"a cache needs Smax >= 1, got {Smax}")
        # zeros, not empty: stale rows are never used, but a cache that is inspected should not show garbage
        kv = [torch.zeros(2, B, H, Smax, HEAD_DIM, dtype=dtype, device=device) for _ in range(layers)]
        scales = [torch.ones(2, B, H, Smax, dtype=torch.float32, device=device) for _ in range(layers)] if fp8 else None
        return cls(kv, torch.zeros(B, dtype=torch.int32, device=device), Smax, scales)

    @property
    def kv_cache(self) -> str:
        return "bf16" if self.scales is None else "fp8"

    def scale(self, layer: int):
        return None if self.scales is None else self.scales[layer]


def kv_quantize_reference(x):
    """(codes uint8 [..., 64], scales fp32 [...]) of rows ``x`` [..., 64] (bf16, or fp32 on the CPU path): the
    definition of the fp8 cache format, which ``C.attn_decode_f8`` and ``C.kv_fill_f8`` equal byte for byte. Per row:
    ``amax = max |x_d|``; ``d = 2^e`` with ``e = max(E - 7, -126)``, ``E`` the unbiased fp32 exponent of ``amax``, and
    ``d = 1`` where ``amax`` is 0 or not finite (a NaN in the row makes it so); ``code_d = e4m3(x_d * 2^-e)``, round to
    nearest even, saturating at +-448, NaN -> the NaN code. The scaled ``amax`` lies in [128, 256): nothing
    saturates, and the product and ``value(code) * d`` are exact (one corner: an ``amax`` in fp32's last binade whose
    scaled value rounds up to 256 dequantises to ``256 * 2^120``, an infinity). The body is generic in the last
    dimension: ``weight_quantize_reference`` applies it to the [N, K] rows of a linear layer's weight."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    e = (((amax.view(torch.int32) >> 23) & 0xFF) - 134).clamp(min=-126)
    e = torch.where(torch.isfinite(amax) & (amax > 0), e, torch.zeros_like(e))
    scales = ((e + 127) << 23).view(torch.float32)
    inv = ((127 - e) << 23).view(torch.float32)
    codes = (xf * inv[..., None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes, scales


def kv_dequantize_reference(codes, scales):
    """fp32 [..., 64] ``= value(code) * scale`` of uint8 e4m3 ``codes`` [..., 64] and fp32 ``scales`` [...]: exact."""
    return codes.view(torch.float8_e4m3fn).float() * scales[..., None]


WEIGHT_FORMATS = (None, "bf16", "fp8")


def check_weights(weights) -> bool:
    """True for fp8 layer weights, False for ``None`` / ``"bf16"`` (the weights as they always were); anything else
    raises."""
    if weights not in WEIGHT_FORMATS:
        raise ValueError(f"weights must be None, 'bf16' or 'fp8', got {weights!r}")
    return weights == "fp8"


def weight_quantize_reference(w):
    """(codes uint8 [N, K], scales fp32 [N]) of a linear layer's weight ``w`` [N, K]: the definition of the fp8
    weight format of the decode steps. ``w`` is first rounded to bf16 (the weight the bf16 step multiplies by, and
    what makes every device produce the same codes), then every output row is quantised by the rules of
    ``kv_quantize_reference`` with K in place of 64: one power-of-two scale ``d = 2^max(E - 7, -126)`` per row,
    ``code = e4m3(w * 2^-e)``. ``value(code)`` has 3 mantissa bits, so it is a bf16 number, and ``d`` is a power of
    two, so a layer on these weights is EXACTLY the bf16 layer whose weight is
    ``kv_dequantize_reference(codes, scales)``: ``|dequant - bf16(w)| <= 2^-4 |bf16(w)| + 2^-10 d`` per entry
    (half a unit of 3 mantissa bits, or half the smallest subnormal ``2^-9`` of the scaled row)."""
    return kv_quantize_reference(w.to(torch.bfloat16))


def fp8_weight_rows(p: torch.Tensor):
    """``weight_quantize_reference`` of parameter ``p`` [N, K] on ``p``'s device, cached on the parameter and keyed
    as ``bf16_weight`` keys its copy (version counters and address): a captured graph sees stable tensors until
    the weight changes. Quantising runs on the CPU, from the bf16 copy, and the result is copied over (the float8
    casts are not relied on on the GPU build); once per weight version, not a hot path."""
    from ml_trainer_amd.ops.transformer import bf16_weight
    from ml_trainer_amd.utils.flat import FlatParams
    fp = FlatParams.owner(p)
    key = ((fp.generation, fp.data._version, p._version) if fp is not None else p._version, p.data_ptr())
    cache = getattr(p, "_mlt_f8_rows", None)
    if cache is not None and cache[0] == key:
        return cache[1]
    codes, scales = weight_quantize_reference(bf16_weight(p).detach().cpu())
    w8 = (codes.to(p.device).contiguous(), scales.to(p.device).contiguous())
    p._mlt_f8_rows = (key, w8)
    return w8


def w8_dequantized(w8, dtype):
    """The dequantised weight of a ``(codes, scales)`` pair on its device in ``dtype`` (exact in bf16 and fp32),
    kept beside the codes: what a decode linear multiplies by where it does not take the fp8 kernel."""
    codes, scales = w8
    cache = getattr(codes, "_mlt_deq", None)
    if cache is None or cache.dtype != dtype:
        cache = kv_dequantize_reference(codes.cpu(), scales.cpu()).to(dtype).to(codes.device)
        codes._mlt_deq = cache
    return cache


class PagePool:
    """The memory of a paged cache: ``kv[l]`` [2, P, Hkv, 64, 64] per layer (keys / values, page, KV head, row in
    page, dim; bf16 on the GPU, fp32 on the CPU, as ``KVCache`` chooses), shared by every ``PagedKVCache`` built on
    it. A page id names the same page in every layer. Page 0 is the null page: never handed out, and what every
    unowned block-table entry points at, so a stale or clamped position cannot land outside the pool or in another
    sequence's rows. The free list lives on the host: ``alloc`` / ``free`` touch no device memory."""

    def __init__(self, layers: int, pages: int, Hkv: int, device, dtype=None):
        device = torch.device(device)
        if layers < 1 or pages < 2 or Hkv < 1:
            raise ValueError(f"a page pool needs layers >= 1, pages >= 2 (page 0 is the null page) and Hkv >= 1, got "
                             f"{layers}, {pages}, {Hkv}")
        if dtype is None:
            dtype = torch.bfloat16 if device.type == "cuda" else torch.float32
        self.kv = [torch.zeros(2, pages, Hkv, PAGE_ROWS, HEAD_DIM, dtype=dtype, device=device) for _ in range(layers)]
        self.pages, self.Hkv = pages, Hkv
        self._free = list(range(pages - 1, 0, -1))  # a stack: alloc hands out 1, 2, ... first
        self._owned = [False] * pages

    @property
    def device(self) -> torch.device:
        return self.kv[0].device

    @property
    def num_free(self) -> int:
        return len(self._free)

    def alloc(self, n: int) -> List[int]:
        """``n`` page ids off the free list, or ``RuntimeError`` with the list unchanged."""
        if n > len(self._free):
            raise RuntimeError(f"page pool exhausted: {n} pages asked, {len(self._free)} of {self.pages - 1} free")
        ids = [self._free.pop() for _ in range(n)]
        for i in ids:
            self._owned[i] = True
        return ids

    def free(self, ids) -> None:
        for i in ids:
            if not 0 < i < self.pages or not self._owned[i]:
                raise ValueError(f"page {i} is not an allocated page of this pool")
            self._owned[i] = False
            self._free.append(i)


class PagedKVCache:
    """A cache of B sequences over a ``PagePool``: ``block_table`` int32 [B, max_pages] on the device (entry i = the
    page of rows ``64 i .. 64 i + 63``; 0 = the null page = not owned), ``pos`` int32 [B] as in ``KVCache``, ``Smax =
    max_pages * 64`` the rows the table can name. ``kv`` is the pool's, ``scales`` is None and ``kv_cache`` "bf16", so
    code that asks a ``KVCache`` those questions gets the same answers. ``pages[b]`` (host) are the ids sequence b
    owns, in row order. The host writes the table, so every entry lies in [0, P): the kernels rely on it."""

    def __init__(self, pool: PagePool, B: int, max_pages: int):
        if B < 1 or max_pages < 1:
            raise ValueError(f"a paged cache needs B >= 1 and max_pages >= 1, got {B}, {max_pages}")
        self.pool, self.max_pages = pool, int(max_pages)
        self.block_table = torch.zeros(B, self.max_pages, dtype=torch.int32, device=pool.device)
        self.pos = torch.zeros(B, dtype=torch.int32, device=pool.device)
        self.pages: List[List[int]] = [[] for _ in range(B)]
        self.scales = None

    @property
    def kv(self) -> List[torch.Tensor]:
        return self.pool.kv

    @property
    def Smax(self) -> int:
        return self.max_pages * PAGE_ROWS

    @property
    def kv_cache(self) -> str:
        return "bf16"

    def scale(self, layer: int):
        return None

    def reserve(self, rows: int) -> None:
        """Make every sequence own ``ceil(rows / 64)`` pages (never fewer than it has). Host-side: ``rows`` comes
        from a host bound such as ``DecodeState.width``, ``pos`` is not read back. New ids reach the device in one
        small host-to-device copy of the table, which is replaced by a wider one when ``rows > Smax``. An exhausted
        pool raises ``RuntimeError`` before the table or the free list changed."""
        need = -(-int(rows) // PAGE_ROWS)
        short = [max(0, need - len(p)) for p in self.pages]
        if not any(short):
            return
        ids = self.pool.alloc(sum(short))
        for p, k in zip(self.pages, short):
            p.extend(ids.pop() for _ in range(k))
        self.max_pages = max(self.max_pages, need)
        host = torch.tensor([p + [0] * (self.max_pages - len(p)) for p in self.pages], dtype=torch.int32)
        if self.block_table.shape[1] == self.max_pages:
            self.block_table.copy_(host)
        else:
            self.block_table = host.to(self.pool.device)

    def release(self) -> None:
        """Give every page back to the pool and zero the table (every entry the null page again)."""
        for p in self.pages:
            self.pool.free(p)
            p.clear()
        self.block_table.zero_()


@dataclass
class DecodeState:
    """What ``prefill`` hands to ``decode_step``: the cache (with ``pos``) and the hidden row [B, h] of every
    sequence's last token, from which the next token's logits come. ``width`` is a host-side upper bound of every
    ``pos[b]`` (the prompt's width plus the columns fed since), kept so that ``generate(past=)`` can check the room
    left in the cache without reading ``pos`` back; ``None``: not recorded. Over a ``PagedKVCache`` it is what
    ``decode_step`` reserves pages by, and ``release()`` returns the pages to the pool. ``weights``: ``None`` /
    ``"bf16"`` (the layer weights as they are) or ``"fp8"`` (``decode_step`` and ``extend`` take the four layer
    linears through ``fp8_weight_rows``; the head and everything in ``prefill`` stay bf16), checked by
    ``check_weights`` where a step reads it."""
    cache: KVCache
    hidden: torch.Tensor
    width: Optional[int] = None
    weights: Optional[str] = None

    @property
    def pos(self) -> torch.Tensor:
        return self.cache.pos

    def release(self) -> None:
        """Return a paged cache's pages to its pool; a contiguous cache owns its memory: nothing to do."""
        if isinstance(self.cache, PagedKVCache):
            self.cache.release()


def attn_decode(qkv_new, cache_layer, pos, H: int, scale: float = ATTN_SCALE, rope=None, kv_scale=None,
                block_table=None):
    """out [B, H * 64] bf16 = attention of the B new tokens' queries over their cached keys and themselves;
    rows ``pos[b]`` of ``cache_layer`` become the new tokens' k / v (the native kernel). ``qkv_new``
    [B, 3 * H * 64] bf16 may be a row-strided view (row stride a multiple of 8). ``rope`` (the fp32 table of
    ``ops.rope.rope_table``, at least Smax rows): the kernel's ROPE instantiation rotates q and the new k by
    ``pos[b]`` and rounds them to bf16 before the dot product and the append, so the cache holds the rotated keys
    the training path's QKV buffer holds. Without it the launch is the one before rotary positions existed.
    A cache of ``Hkv = cache_layer.shape[2] != H`` heads is grouped-query attention: ``qkv_new`` is then the compact
    [B, (H + 2 Hkv) * 64] row (ops/gqa.py) and the launch ``C.attn_decode_gqa``, which streams every cached row once
    for the ``H // Hkv`` query heads of its group and returns the bits ``C.attn_decode`` returns on the repeated
    cache. ``Hkv`` must divide ``H``.
    A cache of ``Smax`` rows with ``decode_attn_path(Smax) == "split"`` takes ``C.attn_decode_split`` instead, for both
    layouts: two launches, with a workspace allocated here beside ``out``.
    ``kv_scale`` (fp32 [2, B, Hkv, Smax]): ``cache_layer`` is an fp8 cache (uint8 e4m3 codes) and the launch
    ``C.attn_decode_f8`` (csrc/kernels/attn_decode_f8.hip), for every layout; the same ``decode_attn_path`` gives it the
    workspace of the split form. The new k / v are quantised first and enter their own step dequantised.
    ``block_table`` (int32 [B, max_pages] on the device): the paged cache. ``cache_layer`` is then a ``PagePool``
    layer [2, P, Hkv, 64, 64] and the launch ``C.attn_decode_paged`` (csrc/kernels/attn_decode_paged.hip), always
    split + merge over ``max_pages * 64`` rows (``decode_attn_path`` is not consulted), with the bits of
    ``C.attn_decode_split`` on the gathered cache. There is no fp8 page: ``kv_scale`` with it raises ``ValueError``."""
    if block_table is not None and kv_scale is not None:
        raise ValueError("attn_decode: a paged cache is bf16, kv_scale cannot be given with block_table")
    C = require_native()
    out = torch.empty(qkv_new.shape[0], H * HEAD_DIM, dtype=torch.bfloat16, device=qkv_new.device)
    if block_table is not None:
        ws = torch.empty(C.attn_decode_split_ws(qkv_new.shape[0], H, block_table.shape[1] * PAGE_ROWS),
                         dtype=torch.float32, device=qkv_new.device)
        C.attn_decode_paged(qkv_new, cache_layer, block_table, pos, out, ws, H, scale, rope=rope)
    elif kv_scale is not None:
        ws = None
        if decode_attn_path(cache_layer.shape[3]) == "split":
            ws = torch.empty(C.attn_decode_split_ws(qkv_new.shape[0], H, cache_layer.shape[3]), dtype=torch.float32,
                             device=qkv_new.device)
        C.attn_decode_f8(qkv_new, cache_layer, kv_scale, pos, out, H, scale, rope=rope, ws=ws)
    elif decode_attn_path(cache_layer.shape[3]) == "split":
        # the workspace beside out: a captured step places both in the graph's pool, two kernel nodes in one chain
        ws = torch.empty(C.attn_decode_split_ws(qkv_new.shape[0], H, cache_layer.shape[3]), dtype=torch.float32,
                         device=qkv_new.device)
        C.attn_decode_split(qkv_new, cache_layer, pos, out, ws, H, scale, rope=rope)
    elif cache_layer.shape[2] != H:
        C.attn_decode_gqa(qkv_new, cache_layer, pos, out, H, scale, rope=rope)
    elif rope is None:
        C.attn_decode(qkv_new, cache_layer, pos, out, H, scale)
    else:
        C.attn_decode(qkv_new, cache_layer, pos, out, H, scale, rope=rope)
    return out


def decode_attn_path(Smax: int) -> str:
    """Which kernels a decode step's attention takes over a cache of ``Smax`` rows: ``"single"`` (``C.attn_decode`` /
    ``C.attn_decode_gqa``: one workgroup walks all cached rows of its head) or ``"split"`` (``C.attn_decode_split``:
    the cached keys split over workgroups, ``C.attn_decode_split_keys()`` each, and a merge launch). A pure function
    of the cache geometry and of ``MLT_DECODE_SPLIT`` (read per call; ``0`` forces ``"single"``: the A/B baseline).
    It does not look at the batch, so a sequence takes the same kernels, and gets the same bits, alone and in a
    batch."""
    if os.environ.get("MLT_DECODE_SPLIT", "1") == "0":
        return "single"
    return "split" if Smax >= DECODE_SPLIT_MIN_SMAX else "single"


def attn_decode_reference(qkv_new, cache_layer, pos, H: int, scale: float = ATTN_SCALE, rope=None, kv_scale=None):
    """``attn_decode`` in plain fp32 torch, on any device: appends into ``cache_layer`` (any float dtype) and
    returns out [B, H * 64] fp32. Stale rows are selected out (scores to -inf, values to 0), never multiplied
    by zero; nothing is read back from the device. ``rope`` (the table): q and the new k are rotated by
    ``pos[b]`` (clamped into the cache, as the kernel clamps it) before use, in ``qkv_new``'s own dtype (bf16 in:
    rounded to bf16 as the kernel rounds them; fp32 in: fp32). A cache of ``Hkv != H`` heads (``Hkv`` divides ``H``):
    grouped-query attention on the compact ``qkv_new`` [B, (H + 2 Hkv) * 64]; the Hkv new k / v heads are appended and
    every query head reads KV head ``h // (H // Hkv)``. ``kv_scale`` (fp32 [2, B, Hkv, Smax]): the fp8 cache;
    ``cache_layer`` holds uint8 codes, the new k (after rotation) and v are quantised by ``kv_quantize_reference``,
    stored as codes + scale, and enter this step as the dequantised values: attention over the dequantised rows."""
    B = qkv_new.shape[0]
    Hkv, Smax = cache_layer.shape[2], cache_layer.shape[3]
    if Hkv != H:
        from ml_trainer_amd.ops.gqa import check_kv_heads, gqa_expand_reference
        check_kv_heads(H, Hkv)
        qkv_new = gqa_expand_reference(qkv_new, H, Hkv)
    if rope is not None:
        from ml_trainer_amd.ops.rope import rope_qk_reference
        qkv_new = rope_qk_reference(qkv_new, rope, H, pos=pos.clamp(0, Smax - 1))
    q, k, v = qkv_new.float().view(B, 3, H, HEAD_DIM).unbind(1)
    G = H // Hkv
    idx = pos.long()
    ar = torch.arange(B, device=qkv_new.device)
    if kv_scale is not None:
        (kq, kd), (vq, vd) = kv_quantize_reference(k[:, ::G]), kv_quantize_reference(v[:, ::G])
        cache_layer[0, ar, :, idx], cache_layer[1, ar, :, idx] = kq, vq
        kv_scale[0, ar, :, idx], kv_scale[1, ar, :, idx] = kd, vd
        k = kv_dequantize_reference(kq, kd).repeat_interleave(G, dim=1)  # what every later step will read
        v = kv_dequantize_reference(vq, vd).repeat_interleave(G, dim=1)
        Kc, Vc = kv_dequantize_reference(cache_layer, kv_scale).unbind(0)
    else:
        cache_layer[0, ar, :, idx] = k[:, ::G].to(cache_layer.dtype)
        cache_layer[1, ar, :, idx] = v[:, ::G].to(cache_layer.dtype)
        Kc, Vc = cache_layer[0].float(), cache_layer[1].float()
    j = torch.arange(Smax, device=qkv_new.device)
    cached = (j[None, :] < idx[:, None])[:, None, :]  # [B, 1, Smax]
    own = (j[None, :] == idx[:, None])[:, None, :]
    if G > 1:  # every query head sees its group's KV head
        Kc, Vc = Kc.repeat_interleave(G, dim=1), Vc.repeat_interleave(G, dim=1)
    K = torch.where(own[..., None], k[:, :, None, :], Kc)  # the new token from qkv_new itself
    V = torch.where(own[..., None], v[:, :, None, :], Vc)
    valid = cached | own
    s = (K @ q[..., None])[..., 0] * scale  # [B, H, Smax]
    s = torch.where(valid, s, torch.full_like(s, float("-inf")))
    V = torch.where(valid[..., None], V, torch.zeros_like(V))
    p = torch.softmax(s, -1)
    return (p[:, :, None, :] @ V)[:, :, 0, :].reshape(B, H * HEAD_DIM)


def gather_pages(pool_layer, block_table):
    """The contiguous cache [2, B, Hkv, max_pages * 64, 64] a block table names in ``pool_layer`` [2, P, Hkv, 64, 64]
    (a copy; unowned entries show the null page)."""
    B, mp = block_table.shape
    g = pool_layer[:, block_table.long()]  # [2, B, max_pages, Hkv, 64, 64]
    return g.permute(0, 1, 3, 2, 4, 5).reshape(2, B, pool_layer.shape[2], mp * PAGE_ROWS, HEAD_DIM)


def attn_decode_paged_reference(qkv_new, pool_layer, block_table, pos, H: int, scale: float = ATTN_SCALE, rope=None):
    """``attn_decode`` over a paged cache in plain torch, on any device (the CPU path and the definition): gather
    the pages into the contiguous cache (``gather_pages``), ``attn_decode_reference`` on it, and the one new row per
    (b, KV head) written back to row ``pos[b] % 64`` of page ``block_table[b, pos[b] // 64]``. Returns out
    [B, H * 64] fp32."""
    kv = gather_pages(pool_layer, block_table)
    out = attn_decode_reference(qkv_new, kv, pos, H, scale, rope)
    n = pos.long()
    ar = torch.arange(n.numel(), device=n.device)
    page = block_table.long()[ar, n // PAGE_ROWS]
    pool_layer[:, page, :, n % PAGE_ROWS] = kv[:, ar, :, n]  # both [B, 2, Hkv, 64]
    return out


def _append_tokens(qkv_new, B: int, Smax: int, kv_scale=None, fp8: bool = False, block_table=None) -> int:
    """T of an ``attn_append`` call, or the ``ValueError`` both the native op and its reference raise."""
    if block_table is not None:
        raise ValueError("attn_append takes a contiguous cache: the paged cache has no multi-token kernel")
    if kv_scale is not None or fp8:
        raise ValueError("attn_append takes a bf16 cache: the fp8 cache has no multi-token kernel")
    rows = qkv_new.shape[0]
    T = rows // B if B > 0 else 0
    if B < 1 or T * B != rows or not 1 <= T <= APPEND_MAX_TOKENS:
        raise ValueError(f"attn_append takes 1 .. {APPEND_MAX_TOKENS} new tokens per sequence, got {rows} rows for "
                         f"B = {B}")
    if T > Smax:
        raise ValueError(f"attn_append: {T} new tokens do not fit a cache of {Smax} rows")
    return T


def attn_append(qkv_new, cache_layer, pos, B: int, H: int, scale: float = ATTN_SCALE, rope=None, kv_scale=None,
                block_table=None):
    """out [B * T, H * 64] bf16 = attention of T = rows / B new tokens per sequence (row ``b * T + t`` of ``qkv_new``
    is token t of sequence b; 1 <= T <= 16) over the cached rows ``j < pos[b]`` and, causally, over each other; rows
    ``pos[b] .. pos[b] + T - 1`` of ``cache_layer`` become their k / v; ``pos`` is not changed. One launch of
    ``C.attn_append`` (csrc/kernels/attn_append.hip: MFMA scores and P . V, the cache streamed once for all T tokens
    and the query heads of a group), or over a cache with ``decode_attn_path(Smax) == "split"`` its split form and the
    decode merge launch, with the workspace and ``row_pos`` allocated here beside ``out``. ``qkv_new``, ``rope`` and a
    cache of ``Hkv != H`` heads as in ``attn_decode``; the token at row ``pos[b] + t`` is rotated by that position.
    The caller keeps ``pos[b] + T <= Smax`` (the kernel clamps). An fp8 cache (``kv_scale``) and a ``T`` out of range
    raise ``ValueError``, and so does ``block_table`` (a paged cache: it has no multi-token kernel). A non-finite
    value in a new token may reach the rows of earlier tokens of its sequence (the matrix cores multiply masked
    probabilities, 0 * NaN): finite inputs are the caller's duty."""
    Smax = cache_layer.shape[3]
    T = _append_tokens(qkv_new, B, Smax, kv_scale, cache_layer.dtype == torch.uint8, block_table)
    C = require_native()
    out = torch.empty(B * T, H * HEAD_DIM, dtype=torch.bfloat16, device=qkv_new.device)
    ws = row_pos = None
    if decode_attn_path(Smax) == "split":
        ws = torch.empty(C.attn_append_ws(B, T, H, Smax), dtype=torch.float32, device=qkv_new.device)
        row_pos = torch.empty(B * T, dtype=torch.int32, device=qkv_new.device)
    C.attn_append(qkv_new, cache_layer, pos, out, B, H, scale, rope=rope, ws=ws, row_pos=row_pos)
    return out


def attn_append_reference(qkv_new, cache_layer, pos, B: int, H: int, scale: float = ATTN_SCALE, rope=None,
                          kv_scale=None, block_table=None):
    """``attn_append`` in plain fp32 torch, on any device (the CPU path and the definition): appends into
    ``cache_layer`` (any float dtype) and returns out [B * T, H * 64] fp32. With ``n = clamp(pos[b], 0, Smax - T)``,
    token t of sequence b sees the cached rows ``j < n`` and the new tokens ``t' <= t``; stale rows and invisible
    tokens are selected out (scores to -inf, values to 0), never multiplied by zero, and the new k / v enter from
    ``qkv_new`` itself. ``rope`` and grouped-query caches as in ``attn_decode_reference``, token t at position
    ``n + t``. It equals T successive ``attn_decode_reference`` calls up to the summation order."""
    Hkv, Smax = cache_layer.shape[2], cache_layer.shape[3]
    T = _append_tokens(qkv_new, B, Smax, kv_scale, cache_layer.dtype == torch.uint8, block_table)
    dev = qkv_new.device
    if Hkv != H:
        from ml_trainer_amd.ops.gqa import check_kv_heads, gqa_expand_reference
        check_kv_heads(H, Hkv)
        qkv_new = gqa_expand_reference(qkv_new, H, Hkv)
    n = pos.long().clamp(0, Smax - T)
    rows = n[:, None] + torch.arange(T, device=dev)[None, :]  # [B, T]: the cache row = the position of every token
    if rope is not None:
        from ml_trainer_amd.ops.rope import rope_qk_reference
        qkv_new = rope_qk_reference(qkv_new, rope, H, pos=rows.reshape(-1))
    q, k, v = qkv_new.float().view(B, T, 3, H, HEAD_DIM).unbind(2)  # [B, T, H, 64]
    G = H // Hkv
    ar = torch.arange(B, device=dev)[:, None]
    cache_layer[0, ar, :, rows] = k[:, :, ::G].to(cache_layer.dtype)
    cache_layer[1, ar, :, rows] = v[:, :, ::G].to(cache_layer.dtype)
    Kc, Vc = cache_layer[0].float(), cache_layer[1].float()
    if G > 1:
        Kc, Vc = Kc.repeat_interleave(G, dim=1), Vc.repeat_interleave(G, dim=1)
    cached = (torch.arange(Smax, device=dev)[None, :] < n[:, None])[:, None, None, :]  # [B, 1, 1, Smax]
    t = torch.arange(T, device=dev)
    tri = (t[None, :] <= t[:, None])[None, None]  # [1, 1, T(query), T(key)]
    qh, kh, vh = (x.permute(0, 2, 1, 3) for x in (q, k, v))  # [B, H, T, 64]
    neg = torch.tensor(float("-inf"), device=dev)
    sc = torch.where(cached, (qh @ Kc.transpose(-1, -2)) * scale, neg)
    sn = torch.where(tri, (qh @ kh.transpose(-1, -2)) * scale, neg)
    p = torch.softmax(torch.cat((sc, sn), -1), -1)
    Vc = torch.where(cached.transpose(-1, -2), Vc, torch.zeros_like(Vc))
    o = p[..., :Smax] @ Vc + p[..., Smax:] @ vh
    return o.permute(0, 2, 1, 3).reshape(B * T, H * HEAD_DIM)


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


def linear_small(x, w16, bias=None, gelu_aux=None, res=None, out=None, w8=None):
    """``y = epilogue(x . w16^T)`` for the few rows of a decode step: x [M, K] bf16, w16 [N, K] bf16 (the layout
    of ``bf16_weight``), fp32 ``bias`` [N], ``gelu_aux`` [M, N] bf16 (GELU epilogue; receives the pre-activation),
    ``res`` [M, N] bf16 added last, ``out`` [M, N] bf16 or fp32 (default: a new bf16 tensor). The skinny kernel
    where ``decode_linear_path`` says so, otherwise the launches of ``transformer.linear_fwd``. On the CPU:
    ``F.linear`` and the same epilogue in fp32.
    ``w8`` (the ``(codes, scales)`` pair of ``fp8_weight_rows``; ``w16`` is then not read and may be ``None``): the
    layer on the dequantised weight. Where the path is ``"skinny"`` it is ``C.gemm_skinny_f8``
    (csrc/kernels/gemm_skinny_f8.hip), which streams the codes; elsewhere the dequantised bf16 weight goes through
    the path above, so it is the same function at every M; on the CPU ``F.linear`` on the dequantised fp32 weight."""
    M, K = x.shape
    if w8 is not None:
        if x.is_cuda and decode_linear_path(M, w8[0].shape[0], K) == "skinny":
            if out is None:
                out = torch.empty(M, w8[0].shape[0], dtype=torch.bfloat16, device=x.device)
            require_native().gemm_skinny_f8(x, w8[0], w8[1], out, bias=bias, aux=gelu_aux, res=res,
                                            mode=1 if gelu_aux is not None else 0)
            return out
        w16 = w8_dequantized(w8, torch.bfloat16 if x.is_cuda else torch.float32)
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


def linear_small_glu(x, w16, bias=None, w8=None):
    """The gated FFN1 of a SwiGLU decode step: ``swiglu(x . w16^T + bias)`` [M, F] for x [M, K] bf16 and w16 [2F, K]
    bf16 (gate rows, then up rows: ops/swiglu.py), fp32 ``bias`` [2F]. Where ``decode_linear_path(M, F, K)`` says
    ``"skinny"`` it is ONE launch, ``C.gemm_skinny_glu`` (two weight streams, the activation in the epilogue);
    otherwise, and with ``MLT_DECODE_GLU=0`` (read per call: the A/B baseline), ``linear_small`` into the [M, 2F]
    intermediate followed by ``swiglu_fwd``. The two agree bit for bit. On the CPU: ``F.linear`` and the torch
    definition. ``w8`` as in ``linear_small``: the one launch is then ``C.gemm_skinny_glu_f8``, and the unfused pair
    and the CPU path take the dequantised weight."""
    from ml_trainer_amd.ops import swiglu as SG
    M, K = x.shape
    Fh = (w16 if w8 is None else w8[0]).shape[0] // 2
    if not x.is_cuda:
        if w8 is not None:
            w16 = w8_dequantized(w8, torch.float32)
        return SG.swiglu_reference(F.linear(x.float(), w16.float(), None if bias is None else bias.float()))
    if os.environ.get("MLT_DECODE_GLU", "1") != "0" and decode_linear_path(M, Fh, K) == "skinny":
        out = torch.empty(M, Fh, dtype=torch.bfloat16, device=x.device)
        if w8 is not None:
            require_native().gemm_skinny_glu_f8(x, w8[0], w8[1], out, bias=bias)
        else:
            require_native().gemm_skinny_glu(x, w16, out, bias=bias)
        return out
    return SG.swiglu_fwd(linear_small(x, w16, bias, w8=w8))


def fill_from_prefill(cache: KVCache, layer: int, qkv, lens: Optional[torch.Tensor], B: int, S: int,
                      heads: Optional[int] = None) -> None:
    """Copy the K / V columns of a layer's padded ``qkv`` [B * S, 3 * H * 64] into rows 0 .. S - 1 of the
    head-major cache. Rows at and past ``lens[b]`` receive the pad positions' projections: they are stale by
    the definition of ``pos`` (the caller sets ``pos = lens``) and never read. ``heads`` (default: the cache's own
    head count): the H of ``qkv`` when the cache holds fewer heads (grouped-query attention: ``qkv`` is the wide
    buffer, whose k / v heads are equal within a group, and the cache takes every ``H // Hkv``-th of them).
    An fp8 cache is filled by ``C.kv_fill_f8`` on the GPU (one launch per layer, the quantiser of the decode step's
    append) and by ``kv_quantize_reference`` on the CPU. A ``PagedKVCache`` (which must own pages for S rows:
    ``reserve``) is filled by ``C.kv_fill_paged`` on the GPU, one launch per layer, and by torch indexing on the CPU:
    row s of sequence b goes to row ``s % 64`` of page ``block_table[b, s // 64]``."""
    kv = cache.kv[layer]
    H = kv.shape[2] if heads is None else heads
    G = H // kv.shape[2]
    if G * kv.shape[2] != H:
        raise ValueError(f"a cache of {kv.shape[2]} heads does not divide heads = {H}")
    if S > cache.Smax:
        raise ValueError(f"a prompt of width {S} does not fit a cache of {cache.Smax} rows")
    if isinstance(cache, PagedKVCache):
        if min(len(p) for p in cache.pages) * PAGE_ROWS < S:
            raise ValueError(f"a prompt of width {S} needs pages reserved for it (PagedKVCache.reserve)")
        if qkv.is_cuda:
            require_native().kv_fill_paged(qkv.view(B * S, 3 * H * HEAD_DIM), kv, cache.block_table, B, S, H)
        else:
            x = qkv.view(B, S, 3, H, HEAD_DIM)
            s = torch.arange(S, device=qkv.device)
            page = cache.block_table.long()[:, s // PAGE_ROWS]  # [B, S]
            kv[0][page, :, s % PAGE_ROWS] = x[:, :, 1, ::G].to(kv.dtype)  # both [B, S, Hkv, 64]
            kv[1][page, :, s % PAGE_ROWS] = x[:, :, 2, ::G].to(kv.dtype)
        return
    if cache.scales is not None:
        if qkv.is_cuda:
            require_native().kv_fill_f8(qkv.view(B * S, 3 * H * HEAD_DIM), kv, cache.scales[layer], B, S, H)
        else:
            x = qkv.view(B, S, 3, H, HEAD_DIM)[:, :, 1:, ::G].permute(2, 0, 3, 1, 4)  # [2, B, Hkv, S, 64]
            kv[:, :, :, :S], cache.scales[layer][:, :, :, :S] = kv_quantize_reference(x)
        return
    x = qkv.view(B, S, 3, H, HEAD_DIM)
    kv[0, :, :, :S] = x[:, :, 1, ::G].permute(0, 2, 1, 3).to(kv.dtype)
    kv[1, :, :, :S] = x[:, :, 2, ::G].permute(0, 2, 1, 3).to(kv.dtype)


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


# ----------------------------------------------------------------------------- the on-device sampler
SAMPLE_SITE = 0x53414D50  # word 2 of the sampler's Philox counter (kSampleSite in mlt_sample.h)
SAMPLE_ONE = 1 << 24      # the fixed-point weight of the row maximum
_LOG2E = 1.4426950408889634


def top_p_to_p16(top_p: Optional[float]) -> int:
    """``p16 = round(top_p * 65536)``: the probability the sampler applies is ``p16 / 65536`` (``None`` = off =
    65536). A ``top_p`` outside (0, 1], or one that rounds to 0 / 65536, is an error, not a silent greedy."""
    if top_p is None:
        return 65536
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p must satisfy 0 < top_p <= 1, got {top_p}")
    p16 = int(top_p * 65536.0 + 0.5)
    if p16 == 0:
        raise ValueError(f"top_p {top_p} rounds to 0 / 65536: no token would be kept (the smallest is 2 ** -16)")
    return min(p16, 65536)


@dataclass
class SamplerState:
    """What ``sample_step`` reads and writes, all on one device. ``params`` int32 [8] is the parameter block
    (``SampleParams`` in mlt_sample.h: inv_t_log2e as fp32 bits, top_k, p16, seed_lo, seed_hi, eos_id, fill_id, 0);
    per row: ``draws`` int32 (tokens drawn so far = the next output column), ``seq_ids`` int32 (the row's identity
    in the random stream), ``finished`` int32, ``n_kept`` int32 (size of the last candidate set), ``lengths`` int64,
    ``next_ids`` int64 (the last token: what the next decode step embeds) and ``tokens`` int64 [B, T]. ``host`` is
    the parameter block as Python values (what the torch reference reads: nothing comes back from the device)."""
    params: torch.Tensor
    draws: torch.Tensor
    seq_ids: torch.Tensor
    finished: torch.Tensor
    n_kept: torch.Tensor
    lengths: torch.Tensor
    next_ids: torch.Tensor
    tokens: torch.Tensor
    host: dict

    @classmethod
    def allocate(cls, B: int, T: int, device, seed: int = 0, temperature: float = 0.0, top_k: Optional[int] = None,
                 top_p: Optional[float] = None, eos_id: Optional[int] = None, fill_id: int = 0,
                 seq_ids=None) -> "SamplerState":
        device = torch.device(device)
        if B < 1 or T < 1:
            raise ValueError(f"a sampler needs B >= 1 and T >= 1, got B = {B}, T = {T}")
        i32 = dict(dtype=torch.int32, device=device)
        if seq_ids is None:
            ids = torch.arange(B, **i32)
        else:
            ids = torch.as_tensor(seq_ids, dtype=torch.int32).reshape(-1).to(device).contiguous()
            if ids.numel() != B:
                raise ValueError(f"seq_ids must have B = {B} entries, got {ids.numel()}")
        st = cls(torch.zeros(8, **i32), torch.zeros(B, **i32), ids, torch.zeros(B, **i32), torch.zeros(B, **i32),
                 torch.zeros(B, dtype=torch.int64, device=device), torch.zeros(B, dtype=torch.int64, device=device),
                 torch.zeros(B, T, dtype=torch.int64, device=device), {})
        st.set_params(seed, temperature, top_k, top_p, eos_id, fill_id)
        return st

    def set_params(self, seed: int = 0, temperature: float = 0.0, top_k: Optional[int] = None,
                   top_p: Optional[float] = None, eos_id: Optional[int] = None, fill_id: int = 0) -> None:
        """Rewrite the parameter block in place: one small host-to-device copy (call it outside a captured
        region; a captured ``sample_step`` then samples with the new settings)."""
        if temperature < 0:
            raise ValueError(f"temperature must be >= 0, got {temperature}")
        if top_k is not None and top_k < 1:
            raise ValueError(f"top_k must be >= 1, got {top_k}")
        p16 = top_p_to_p16(top_p)
        # log2(e) / temperature in double, rounded once to fp32; 0 = greedy
        s = 0.0 if temperature == 0 else torch.tensor(_LOG2E / temperature, dtype=torch.float64).float().item()
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.host = dict(inv_t_log2e=s, top_k=0 if top_k is None else int(top_k), p16=p16, seed=seed,
                         eos_id=-1 if eos_id is None else int(eos_id), fill_id=int(fill_id))
        words = struct.unpack("8i", struct.pack("<fiiIIiii", s, min(self.host["top_k"], 0x7FFFFFFF), p16,
                                                seed & 0xFFFFFFFF, seed >> 32, self.host["eos_id"],
                                                self.host["fill_id"], 0))
        self.params.copy_(torch.tensor(words, dtype=torch.int32))

    def reset(self) -> None:
        """Start a new generation in the same buffers: no tokens drawn, nothing finished."""
        for t in (self.draws, self.finished, self.n_kept, self.lengths, self.next_ids, self.tokens):
            t.zero_()


def _sample_logits_operand(logits, V: int):
    """``logits`` as the kernel takes them: fp32, unit column stride, 16-byte aligned rows a multiple of 4 apart.
    The [B, V] view of ``ops.mlm.decode_logits``'s padded buffer passes as it is; anything else is copied."""
    B, Vr = logits.shape[0], -(-V // 4) * 4  # a row is read up to round_up(V, 4) columns
    if (logits.dtype == torch.float32 and logits.stride(1) == 1 and logits.data_ptr() % 16 == 0 and
            (B == 1 or (logits.stride(0) % 4 == 0 and logits.stride(0) >= Vr)) and
            logits.storage_offset() + (B - 1) * logits.stride(0) + Vr <= logits.untyped_storage().nbytes() // 4):
        return logits
    buf = torch.zeros(logits.shape[0], -(-V // 4) * 4, dtype=torch.float32, device=logits.device)
    buf[:, :V] = logits[:, :V]
    return buf


def sample_step(logits, V: int, state: SamplerState) -> None:
    """One sampling step on the GPU (``C.sample_step``): row b's next token from ``logits[b, :V]`` (fp32; columns
    past ``V`` may hold anything) into ``state.tokens[b, state.draws[b]]`` and ``state.next_ids[b]``, with the
    EOS / ``finished`` / ``lengths`` bookkeeping. One launch, no allocation, nothing read back."""
    require_native().sample_step(_sample_logits_operand(logits, V), V, state.params, state.draws, state.seq_ids,
                                 state.finished, state.lengths, state.tokens, state.next_ids, state.n_kept)


def sample_weights_reference(logits, V: int, inv_t_log2e: float):
    """(w int64 [B, V], argmax int64 [B], zc fp32 [B, V]): steps 1-2 of the definition in plain torch, the weights
    from ``torch.exp2`` in fp32 (the device's ``exp2f`` may differ from it in the last place: the tests feed the
    reference the device's own weights where they compare tokens)."""
    z = logits[:, :V].float()
    nan = torch.isnan(z)
    ninf = torch.full_like(z, float("-inf"))
    zc = torch.where(nan, ninf, z)
    zc = torch.where(zc == 0, torch.zeros_like(zc), zc)  # -0 counts as +0
    m = zc.max(-1, keepdim=True).values
    idx = torch.arange(V, device=z.device)
    a = torch.where(zc == m, idx, torch.full_like(idx, V)).min(-1).values  # the first index of the maximum
    s = torch.tensor(inv_t_log2e, dtype=torch.float32, device=z.device)
    e = torch.exp2((zc - m) * s).clamp(max=1.0)  # one fp32 subtract, one fp32 multiply
    w = torch.floor(e * 16777216.0)
    w = torch.where(zc == m, torch.full_like(w, float(SAMPLE_ONE)), w)
    w = torch.where(nan | torch.isnan(w), torch.zeros_like(w), w).to(torch.int64)
    return w, a, zc


def sample_step_reference(logits, V: int, state: SamplerState, weights=None) -> None:
    """``sample_step`` in plain torch, on any device (the CPU path and the oracle's subject). Per row b, with
    ``s = state.host["inv_t_log2e"]``:

    1. NaN logits count as -inf, -0 as +0; ``m`` = the maximum, ``a`` = the smallest index attaining it. ``s == 0``:
       the token is ``a`` (``n_kept`` = 1).
    2. ``w_i = 2^24`` where ``z_i == m``, else ``floor(min(exp2(s * (z_i - m)), 1) * 2^24)`` in fp32; NaN columns
       weigh 0. ``weights`` (int [B, V]) substitutes given ones. Everything below is int64 arithmetic.
    3. ``T_k`` = the k-th largest logit with multiplicity, ``K = {z_i >= T_k}`` (ties kept); k = 0 or k >= V: all.
    4. ``need = (p16 * W_K + 65535) >> 16``; ``T_p`` = the largest logit value t with ``sum_{K, z_i >= t} w_i >= need``;
       ``S = {i in K: z_i >= T_p}``; p16 = 65536: ``S = K``. The probability applied is ``p16 / 65536``.
    5. ``x`` = word 0 of philox4x32-10(counter (draws[b], seq_ids[b], 0x53414D50, 0), key = seed words),
       ``r = ((x >> 8) * W_S) >> 24``, the token is the smallest i in S with ``sum_{j in S, j <= i} w_j > r``.
    6. finished rows emit ``fill_id``; others add 1 to ``lengths`` and become finished on ``eos_id``; then
       ``tokens[b, draws[b]] = next_ids[b] = token`` and ``draws[b] += 1``."""
    from ml_trainer_amd.ops.dropout import philox4x32
    h = state.host
    dev = logits.device
    B = logits.shape[0]
    w, a, zc = sample_weights_reference(logits, V, h["inv_t_log2e"])
    if weights is not None:
        w = weights.to(device=dev, dtype=torch.int64)
    token = a
    kept = torch.ones(B, dtype=torch.int64, device=dev)
    if h["inv_t_log2e"] != 0:
        idx = torch.arange(V, device=dev)
        big = torch.full_like(idx, V)
        in_k = torch.ones_like(zc, dtype=torch.bool)
        if 0 < h["top_k"] < V:
            in_k = zc >= zc.topk(h["top_k"], dim=-1).values[:, -1:]
        in_s = in_k
        if h["p16"] < 65536:
            wk = torch.where(in_k, w, torch.zeros_like(w))
            need = (h["p16"] * wk.sum(-1, keepdim=True) + 65535) >> 16
            zs, order = torch.sort(zc, dim=-1, descending=True)
            cum = torch.cumsum(wk.gather(1, order), -1)
            n_ge = torch.searchsorted((-zs).contiguous(), (-zs).contiguous(), right=True)  # |{j: z_j >= zs[p]}|
            g = cum.gather(1, n_ge - 1)  # the weight of {i in K: z_i >= zs[p]}: non-decreasing in p
            first = torch.where(g >= need, idx, big).min(-1, keepdim=True).values
            t_p = zs.gather(1, first.clamp(max=V - 1))
            t_p = torch.where(need > 0, t_p, torch.full_like(t_p, float("-inf")))
            in_s = in_k & (zc >= t_p)
        ws = torch.where(in_s, w, torch.zeros_like(w))
        W = ws.sum(-1)
        counter = torch.stack((state.draws.long() & 0xFFFFFFFF, state.seq_ids.long() & 0xFFFFFFFF,
                               torch.full((B,), SAMPLE_SITE, dtype=torch.int64, device=dev),
                               torch.zeros(B, dtype=torch.int64, device=dev)), -1)
        key = torch.tensor([h["seed"] & 0xFFFFFFFF, h["seed"] >> 32], dtype=torch.int64, device=dev)
        u24 = philox4x32(counter, key)[:, 0] >> 8
        r = u24 * (W >> 24) + ((u24 * (W & 0xFFFFFF)) >> 24)  # (u24 * W) >> 24 without leaving int64
        hit = torch.where(torch.cumsum(ws, -1) > r[:, None], idx, big).min(-1).values
        token = torch.where(W > 0, hit, a)
        kept = in_s.sum(-1)
    fin = state.finished != 0
    out = torch.where(fin, torch.full_like(token, h["fill_id"]), token)
    state.lengths += (~fin).long()
    state.finished |= ((~fin) & (token == h["eos_id"])).to(state.finished.dtype)
    col = state.draws.long().clamp(0, state.tokens.shape[1] - 1)
    state.tokens[torch.arange(B, device=dev), col] = out
    state.next_ids.copy_(out)
    state.draws += 1
    state.n_kept.copy_(kept.to(state.n_kept.dtype))
