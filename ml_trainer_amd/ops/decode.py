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


def attn_decode(qkv_new, cache_layer, pos, H: int, scale: float = ATTN_SCALE, rope=None):
    """out [B, H * 64] bf16 = attention of the B new tokens' queries over their cached keys and themselves;
    rows ``pos[b]`` of ``cache_layer`` become the new tokens' k / v (the native kernel). ``qkv_new``
    [B, 3 * H * 64] bf16 may be a row-strided view (row stride a multiple of 8). ``rope`` (the fp32 table of
    ``ops.rope.rope_table``, at least Smax rows): the kernel's ROPE instantiation rotates q and the new k by
    ``pos[b]`` and rounds them to bf16 before the dot product and the append, so the cache holds the rotated keys
    the training path's QKV buffer holds. Without it the launch is the one before rotary positions existed."""
    C = require_native()
    out = torch.empty(qkv_new.shape[0], H * HEAD_DIM, dtype=torch.bfloat16, device=qkv_new.device)
    if rope is None:
        C.attn_decode(qkv_new, cache_layer, pos, out, H, scale)
    else:
        C.attn_decode(qkv_new, cache_layer, pos, out, H, scale, rope=rope)
    return out


def attn_decode_reference(qkv_new, cache_layer, pos, H: int, scale: float = ATTN_SCALE, rope=None):
    """``attn_decode`` in plain fp32 torch, on any device: appends into ``cache_layer`` (any float dtype) and
    returns out [B, H * 64] fp32. Stale rows are selected out (scores to -inf, values to 0), never multiplied
    by zero; nothing is read back from the device. ``rope`` (the table): q and the new k are rotated by
    ``pos[b]`` (clamped into the cache, as the kernel clamps it) before use, in ``qkv_new``'s own dtype (bf16 in:
    rounded to bf16 as the kernel rounds them; fp32 in: fp32)."""
    B = qkv_new.shape[0]
    Smax = cache_layer.shape[3]
    if rope is not None:
        from ml_trainer_amd.ops.rope import rope_qk_reference
        qkv_new = rope_qk_reference(qkv_new, rope, H, pos=pos.clamp(0, Smax - 1))
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
