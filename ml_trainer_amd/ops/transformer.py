"""Autograd blocks of the transformer path over the native gfx950 kernels.

Mixed precision: parameters are fp32 masters (in a FlatParams buffer when an
optimizer/DDP owns them); compute reads their bf16 *shadow* (refreshed by the
fused optimizer kernel in the same pass that updates the master, so there is
no separate cast per step). Weight / bias gradients come back in fp32.

Structure: an attention call is described by one ``AttnSpec`` (the Python side of the host layer's ``AttnProblem``),
which goes through ``_attn_fwd`` / ``_attn_bwd`` and onto ``ctx`` whole. The attention and the FFN are two *cores* of
one shape (``fwd(x, params, res) -> (y, saved)``, ``bwd(saved, params, dy, G, dbias_last, dres) -> grads``;
``attn_core`` / ``ffn_core``), and three autograd nodes take a core as an argument: ``block`` (core(x) + x),
``post_norm_block`` (x -> Norm(core(x) + x)) and ``pre_norm_block`` ((h, n) -> (h', Norm(h'))), the last two with the
hidden-dropout fork written once (``_sublayer_fwd``). Every block reaches the norm kernels through ``_norm_fwd`` /
``_dropout_add_norm_fwd`` / ``_norm_bwd`` (LayerNorm with ``beta``, RMSNorm without), and ``_check_bf16_only`` is the
one place that refuses a feature under the fp8 linears. The public blocks below keep their loose arguments and build
the spec and the core from them.

Blocks (one autograd node each, so the backward can fuse across ops):

* ``attention_block``: x -> QKV GEMM(+bias) -> fused flash attention -> out-proj
  GEMM (+bias +residual x). Backward: wgrad/colsum/dgrad of out-proj, attention
  backward into the packed dQKV, wgrad/colsum of QKV and dgrad with the residual
  gradient folded into the GEMM epilogue.
* ``ffn_block``: x -> FFN1 GEMM (+bias, GELU epilogue that also stores the
  pre-activation) -> FFN2 GEMM (+bias +residual). Backward: FFN2's dgrad GEMM
  applies gelu'(pre) in its epilogue (no separate elementwise pass). With ``act="swiglu"`` (every FFN block):
  FFN1 [2F, h] with the plain bias epilogue -> ``swiglu_fwd`` -> FFN2; backward FFN2 wgrad, plain dgrad,
  ``swiglu_bwd`` (dh1 and FFN1's bias gradient), FFN1 wgrad and dgrad (ops/swiglu.py, csrc/kernels/swiglu.hip).
* ``attention_ln_block`` / ``ffn_ln_block``: the block followed by its post-LayerNorm as one
  node; the LayerNorm backward kernel also produces the column sums of its dx, which are the
  bias gradient of the block's last linear layer (no separate pass over dy). With ``drop`` they
  apply hidden dropout to that linear's output: the LayerNorm forward kernel drops, adds the
  residual and normalises; the backward kernel also writes the masked, scaled dx (the linear's dY)
  and reduces the bias gradient from it. The mask is recomputed, never stored (ops/dropout.py).
  With ``attn_drop`` the attention blocks drop attention probabilities inside the flash kernels
  (forward, dQ, dK/dV), from a byte-per-element mask that is recomputed as well.
* ``pre_attention_block`` / ``pre_ffn_block`` / ``stream_norm``: the pre-norm blocks. A node maps the residual
  stream and its norm ``(h, n)`` to ``(h', n')`` with ``n'`` under the next sub-layer's norm weights, LayerNorm or
  RMSNorm (``beta=None``). The forward reuses the fusions above (residual in the GEMM epilogue, or the
  dropout_add norm kernel, which writes h' and n'); the norm backward takes the stream's gradient as DRES, so
  its dx is the total stream gradient: the residual's gradient, the last linear's dY (under dropout its masked
  copy DXM) and, through the fused column sums, that linear's bias gradient.
* ``layer_norm``, ``embeddings``, ``dropout`` (the embedding site).

Packed ("unpadded") batches: ``pack_batch`` drops the pad tokens of a right-padded [B, S] batch once
and the blocks then run on the T = sum(lens) real tokens as one [T, D] matrix. The attention blocks
take ``cu_seqlens`` (sequence b = rows cu[b] .. cu[b + 1]; ``S`` is then max_seqlen, the width of the
padded input, and ``lens`` is unused), ``embeddings`` takes explicit positions; everything else is
row-count agnostic.

The linear-layer arithmetic is pluggable (``impl``): ``BF16`` (bf16 operands) or
``ops.fp8.FP8`` (OCP fp8 forward / dgrad GEMMs with delayed per-tensor scaling; wgrad bf16).

Linear layout conventions (nn.Linear weight [out, in]):
  fwd   y  = x . W^T         gemm(x, W, a_mn=0, b_mn=0)
  dgrad dx = dy . W          gemm(dy, W, a_mn=0, b_mn=1)
  wgrad dW = dy^T . x        gemm(dy, x, a_mn=1, b_mn=1) -> fp32
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import NamedTuple, Optional

import torch

from ml_trainer_amd.ops._ext import require_native
from ml_trainer_amd.ops.gqa import gqa_expand, gqa_reduce, infer_kv_heads
from ml_trainer_amd.ops.swiglu import swiglu_bwd, swiglu_fwd
from ml_trainer_amd.utils.flat import FlatParams


def bf16_weight(p: torch.Tensor) -> torch.Tensor:
    """bf16 compute copy of an fp32 master parameter."""
    fp = FlatParams.owner(p)
    if fp is not None and fp.device.type == "cuda":
        return fp.shadow_view(p)
    cache = getattr(p, "_mlt_bf16", None)
    if cache is not None and cache[0] == p._version and cache[1] == p.data_ptr():
        return cache[2]
    w = p.detach().to(torch.bfloat16).contiguous()
    p._mlt_bf16 = (p._version, p.data_ptr(), w)
    return w


def bf16_weight_t(p: torch.Tensor) -> torch.Tensor:
    """W^T (bf16, contiguous [in, out]) of a weight [out, in], re-made once per optimizer update
    (FlatParams.generation) -- the k-contiguous B operand of the input-gradient GEMM."""
    fp = FlatParams.owner(p)
    # generation: optimizer updates; data._version: load_state_dict / manual edits of the masters
    key = ((fp.generation, fp.data._version) if fp is not None else p._version, p.data_ptr())
    cache = getattr(p, "_mlt_bf16_t", None)
    if cache is not None and cache[0] == key:
        return cache[1]
    w16 = bf16_weight(p)
    t = cache[1] if cache is not None else torch.empty(w16.shape[1], w16.shape[0], dtype=torch.bfloat16,
                                                        device=w16.device)
    require_native().transpose_bf16(w16, t)
    p._mlt_bf16_t = (key, t)
    return t


class Bf16Linear:
    """bf16 operands (bf16 shadows of the fp32 masters), fp32 accumulate, fused epilogues."""

    @staticmethod
    def fwd(x, w, bias=None, gelu_aux=None, res=None):
        return linear_fwd(x, bf16_weight(w), bias, gelu_aux=gelu_aux, res=res)

    @staticmethod
    def dgrad(dy, w, out, aux=None, res=None, colsum_out=None, colsum_acc=False):
        """out = dy . W  (* gelu'(aux) when aux is given) (+ res). Large token counts take W^T as
        a k-contiguous copy (one transpose per weight per step): the forward-layout tile runs
        8-11 % faster than the n-contiguous-B one on the BERT dgrad shapes. ``colsum_out``: the
        column sums of the dGELU output (the bias gradient of the layer before the GELU) from the
        GEMM epilogue (set or accumulated; see dgelu_colsum_ok)."""
        C = require_native()
        mode = 2 if aux is not None else 0
        if dy.shape[0] >= 4096 and os.environ.get("MLT_DGRAD_WT", "1") != "0":
            C.gemm(dy, bf16_weight_t(w), out, False, False, aux=aux, mode=mode, res=res,
                   colsum_out=colsum_out, colsum_accumulate=colsum_acc)
        else:
            C.gemm(dy, bf16_weight(w), out, False, True, aux=aux, mode=mode, res=res,
                   colsum_out=colsum_out, colsum_accumulate=colsum_acc)
        return out

    @staticmethod
    def dgelu_colsum_ok(dy, w) -> bool:
        """Whether dgrad(dy, w, aux=..., colsum_out=...) can fuse the column sums (ping-pong tiles
        over the whole output: tokens and W's input width multiples of 256)."""
        return dy.shape[0] % 256 == 0 and w.shape[1] % 256 == 0 and dy.shape[1] % 64 == 0


BF16 = Bf16Linear()


def linear_fwd(x, w16, bias=None, gelu_aux=None, res=None):
    C = require_native()
    y = torch.empty(x.shape[0], w16.shape[0], dtype=torch.bfloat16, device=x.device)
    C.gemm(x, w16, y, False, False, bias=bias, aux=gelu_aux, res=res, mode=1 if gelu_aux is not None else 0)
    return y


def linear_wgrad(dy, x):
    C = require_native()
    dw = torch.empty(dy.shape[1], x.shape[1], dtype=torch.float32, device=dy.device)
    C.gemm(dy, x, dw, True, True)
    return dw


def colsum(dy):
    C = require_native()
    db = torch.empty(dy.shape[1], dtype=torch.float32, device=dy.device)
    C.colsum(dy, db, False)
    return db


class _Grads:
    """Weight / bias gradients of one fused backward.

    When a parameter's ``.grad`` is a view into a FlatParams gradient buffer (fused optimizer /
    native DDP), the producing kernel accumulates straight into it (GEMM ``accumulate`` epilogue,
    reduction ``accmask``, embedding atomics): no fp32 temporary, no AccumulateGrad add kernel,
    and the autograd return value for that parameter is None. The owner is then told the
    gradient is ready (``FlatParams.notify_grad_ready``) so DDP bucket countdowns still fire.
    Parameters without a flat gradient get ordinary returned tensors."""

    def __init__(self):
        self.ready = []

    def sink(self, p):
        fp = FlatParams.owner(p)
        g = fp.grad_sink(p) if fp is not None else None
        if g is not None:
            self.ready.append(p)
        return g

    def out(self, p, n, device):
        """Where a kernel reduces the ``n``-float gradient of ``p``: (target, accumulate, result) --
        the flat-gradient sink, accumulated into (the autograd result is then None), or a fresh
        fp32 vector that is also the result."""
        g = self.sink(p)
        if g is not None:
            return g, True, None
        t = torch.empty(n, dtype=torch.float32, device=device)
        return t, False, t

    def wgrad(self, p, dy, x, impl=None):
        g = self.sink(p)
        if impl is not None and hasattr(impl, "wgrad"):  # fp8 weight gradient
            r = impl.wgrad(p, dy, x, g)
            if r is not None:
                return None if g is not None else r
        if g is None:
            return linear_wgrad(dy, x)
        require_native().gemm(dy, x, g, True, True, accumulate=True)
        return None

    def wgrad_bias(self, pw, pb, dy, x, impl=None):
        """(dW, db) of one linear. With an fp8 ``impl`` the bias gradient is reduced inside the
        dY cast the fp8 weight gradient needs anyway (one read of dY instead of two)."""
        if pb is None or impl is None or not getattr(impl, "wgrad_fuses_bias", False):
            return self.wgrad(pw, dy, x, impl), self.colsum(pb, dy)
        C = require_native()
        g = self.sink(pw)
        db, db_acc, db_ret = self.out(pb, dy.shape[1], dy.device)
        r = impl.wgrad(pw, dy, x, g, db_out=db, db_acc=db_acc)
        if r is not None:
            return (None if g is not None else r), db_ret
        # fp8 weight gradient not applicable here: separate kernels into the same sinks
        if g is None:
            dw = linear_wgrad(dy, x)
        else:
            C.gemm(dy, x, g, True, True, accumulate=True)
            dw = None
        C.colsum(dy, db, db_acc)
        return dw, db_ret

    def colsum(self, p, dy):
        g = self.sink(p)
        if g is None:
            return colsum(dy)
        require_native().colsum(dy, g, accumulate=True)
        return None

    def done(self):
        for p in self.ready:
            FlatParams.owner(p).notify_grad_ready(p)
        self.ready = []


@dataclass(frozen=True, eq=False)
class AttnSpec:
    """Everything of one attention call that is not an activation or a weight; the Python side of the host
    layer's ``AttnProblem``. ``lens`` int32 [B] or None. ``cu_seqlens`` (int32 [B + 1], device): packed batch, x is
    [T, D] with sequence b at rows cu[b] .. cu[b + 1]; S is then max_seqlen and ``lens`` is unused. ``causal``: key j
    is visible to query i of its sequence iff j <= i and j < len_b. ``rope`` = (table fp32 [P, 32, 2], pos int32
    [rows] or None: row % S), see ops/rope.py. ``attn_drop`` = (p, seed, site, rank): attention-probability dropout
    inside the flash kernels (the byte mask of ops/dropout.py, recomputed in the backward). ``kv_heads`` (None or H:
    none of this): grouped-query attention with the compact QKV layout of ops/gqa.py."""
    B: int
    S: int
    H: int
    lens: Optional[torch.Tensor] = None
    cu_seqlens: Optional[torch.Tensor] = None
    causal: bool = False
    rope: Optional[tuple] = None
    attn_drop: Optional[tuple] = None
    kv_heads: Optional[int] = None

    @property
    def gqa(self) -> bool:
        return self.kv_heads is not None and self.kv_heads != self.H

    def kernel_kw(self) -> dict:
        """Keyword arguments of C.attn_fwd / C.attn_bwd; a keyword goes out only when set."""
        kw = {}
        if self.attn_drop is not None:
            kw["p"], kw["seed"], kw["site"], kw["rank"] = self.attn_drop
        if self.causal:
            kw["causal"] = True
        if self.cu_seqlens is not None:
            kw["cu_seqlens"] = self.cu_seqlens
        return kw


def attn_spec(wqkv, lens, B, S, H, attn_drop=None, cu_seqlens=None, causal=False, rope=None) -> AttnSpec:
    """The spec of the public blocks' loose arguments. ``kv_heads`` comes from the QKV projection's own shape: None
    for the wide [3 * H * 64, h] weight (every launch as before), Hkv for the compact [(H + 2 Hkv) * 64, h] one."""
    return AttnSpec(B, S, H, lens, cu_seqlens, causal, rope, attn_drop, infer_kv_heads(wqkv.shape[0], H))


# What runs the bf16 linears only, in raising order: (feature, message).
_BF16_ONLY = (
    ("pre_norm", "pre-norm blocks run the bf16 linears only"),
    ("causal", "causal attention runs the bf16 linears only: the fp8 (q8) attention epilogue has no causal "
               "instantiation"),
    ("gqa", "grouped-query attention runs the bf16 linears only: the fp8 attention backward writes dQKV as e5m2 in "
            "the wide layout"),
    ("packed", "packed (cu_seqlens) attention runs the bf16 linears only: the fp8 attention epilogue writes at "
               "b * S offsets"),
    ("rotary", "rotary positions run the bf16 linears only: the fp8 attention backward writes dQKV as e5m2, which "
               "the inverse rotation cannot take"),
    ("swiglu", "the SwiGLU feed-forward runs the bf16 linears only: the fp8 FFN fusions are GELU epilogues"),
)


def _check_bf16_only(impl, **features):
    """Refuse the requested ``features`` (names of _BF16_ONLY) under any linear implementation but BF16."""
    if impl is not BF16:
        for name, message in _BF16_ONLY:
            if features.get(name):
                raise ValueError(message)


def _zero_packed_tail(t, cu_seqlens):
    """Packed batches may end in inert tail rows (``pack_batch``) that the attention kernels never write:
    zero the last rows before the launch, which then overwrites the real ones among them. T is not known
    on the host here, so the attention blocks support FEWER THAN PACK_ROW_MULTIPLE tail rows, which is
    what ``pack_batch`` produces; rows of a longer tail would keep uninitialised memory."""
    if cu_seqlens is not None:
        t[-min(PACK_ROW_MULTIPLE - 1, t.shape[0]):].zero_()


def _rope_qk(t, rope, S, H, sign=1):
    """Rotary positions: rotate the q and k columns of ``t`` (QKV, or dQKV with ``sign=-1``) in place.
    ``rope`` = (table fp32 [P, 32, 2], pos int32 [rows] or None: row % S), see ops/rope.py."""
    table, pos = rope
    require_native().rope_qk(t, table, H, S, pos=pos, sign=sign)


# The two sub-layer cores share one shape, which is all the block nodes below know of them:
#   fwd(x, params, res, what, impl) -> (y, saved)     res: what the last linear adds in its epilogue, or None
#   bwd(saved, params, dy, G, dbias_last, dres, what, impl) -> (dx, dw_first, db_first, dw_last, db_last)
# ``params`` = (w_first, b_first, w_last, b_last); ``what`` is the core's one non-tensor argument (an AttnSpec, or
# the FFN's ``act``). ``dbias_last``: "colsum" to reduce dy here, otherwise the last linear's bias gradient as the
# norm backward already produced it (tensor or None). ``dres``: what the first linear's dgrad adds in its epilogue:
# the gradient of the residual branch (``dy`` itself, or the norm backward's dx when hidden dropout sits between
# them), or None where the core's input is not its residual (pre-norm blocks).
def _attn_fwd(x, params, res, spec: AttnSpec, impl=BF16):
    """Under ``spec.rope`` q and k are rotated in place between the QKV GEMM and the attention kernel; the saved qkv
    is the rotated one, which the attention backward needs. Under ``spec.gqa`` ``wqkv`` projects to the compact
    layout q (H heads) | k (kv_heads) | v (kv_heads) and ``C.gqa_expand`` (ops/gqa.py) repeats every k / v head for
    its group into the wide [rows, 3 * H * 64] buffer, which the rotation and the attention kernel then take
    unchanged and which is what is saved."""
    _check_bf16_only(impl, causal=spec.causal, gqa=spec.gqa, packed=spec.cu_seqlens is not None,
                     rotary=spec.rope is not None)
    C = require_native()
    wqkv, bqkv, wo, bo = params
    B, S, H = spec.B, spec.S, spec.H
    qkv = impl.fwd(x, wqkv, bqkv)
    if spec.gqa:
        qkv = gqa_expand(qkv, H, spec.kv_heads)
    if spec.rope is not None:
        _rope_qk(qkv, spec.rope, S, H)
    attn = torch.empty(x.shape[0], H * 64, dtype=torch.bfloat16, device=x.device)
    lse = torch.empty(B * H * S, dtype=torch.float32, device=x.device)
    _zero_packed_tail(attn, spec.cu_seqlens)
    C.attn_fwd(qkv, attn, lse, spec.lens, B, S, H, _ATTN_SCALE, **{"cu_seqlens": None, **spec.kernel_kw()})
    # out-proj + bias + residual (under dropout the residual joins in the norm kernel instead)
    y = impl.fwd(attn, wo, bo, res=res)
    return y, (x, qkv, attn, lse)


def _attn_bwd(saved, params, dy, G, dbo, dres, spec: AttnSpec, impl=BF16):
    """Under ``spec.rope`` dQKV comes out of the attention backward in the rotated frame and is rotated back
    (``sign=-1``) before anything else reads it. The QKV bias gradient is then the column sum of the rotated-back
    dQKV: the attention kernels' own column sums are sums in the rotated frame, which differ row by row, so that
    fused branch is not taken under rotary. Under ``spec.gqa`` the wide dQKV (rotated back under rotary) is reduced
    to the compact layout by ``C.gqa_reduce`` (dk / dv summed over each group) before the weight gradient, the bias
    gradient and the dgrad read it. The attention kernels' own column sums are over wide columns, so that fused
    branch is not taken under grouped-query attention either."""
    C = require_native()
    B, S, H, lens, rope = spec.B, spec.S, spec.H, spec.lens, spec.rope
    akw = spec.kernel_kw()
    x, qkv, attn, lse = saved
    wqkv, bqkv, wo, bo = params
    dwo = G.wgrad(wo, dy, attn, impl)
    if isinstance(dbo, str):
        dbo = G.colsum(bo, dy)
    dattn = impl.dgrad(dy, wo, torch.empty_like(attn))
    dqkv = torch.empty_like(qkv)
    _zero_packed_tail(dqkv, spec.cu_seqlens)
    delta = torch.empty(qkv.shape[0] * H, dtype=torch.float32, device=dy.device)
    q8 = impl.attn_dy_q(wqkv, x, qkv.shape[0]) if (impl is not BF16 and hasattr(impl, "attn_dy_q")) else None
    if rope is not None or spec.gqa:
        C.attn_bwd(qkv, attn, dattn, lse, delta, lens, dqkv, B, S, H, _ATTN_SCALE, **akw)
        if rope is not None:
            _rope_qk(dqkv, rope, S, H, sign=-1)
        if spec.gqa:
            dqkv = gqa_reduce(dqkv, H, spec.kv_heads)
        dwqkv, dbqkv = G.wgrad_bias(wqkv, bqkv, dqkv, x, impl)
    elif q8 is not None or (impl is BF16 and bqkv is not None):
        # the QKV bias gradient (column sums of dQKV) from the backward kernels themselves
        db, db_acc, dbqkv = G.out(bqkv, qkv.shape[1], dy.device) if bqkv is not None else (None, False, None)
        if q8 is not None:
            # fp8: the kernels write dQKV as e5m2 + transpose + amax (no bf16 dQKV, no cast pass)
            d8, d8t, qs, qa = q8
            C.attn_bwd(qkv, attn, dattn, lse, delta, lens, dqkv, B, S, H, _ATTN_SCALE, colsum_out=db,
                       colsum_accumulate=db_acc, q8_y=d8, q8_yt=d8t, q8_scale=qs, q8_amax=qa, **akw)
            impl.attn_dy_q_done(wqkv, d8, d8t)
            dqkv = d8
        else:
            C.attn_bwd(qkv, attn, dattn, lse, delta, lens, dqkv, B, S, H, _ATTN_SCALE, colsum_out=db,
                       colsum_accumulate=db_acc, **akw)
        dwqkv = G.wgrad(wqkv, dqkv, x, impl)
    else:
        C.attn_bwd(qkv, attn, dattn, lse, delta, lens, dqkv, B, S, H, _ATTN_SCALE, **akw)
        dwqkv, dbqkv = G.wgrad_bias(wqkv, bqkv, dqkv, x, impl)
    dx = impl.dgrad(dqkv, wqkv, torch.empty_like(x), res=dres)  # dqkv . Wqkv + dres
    return dx, dwqkv, dbqkv, dwo, dbo


def _ffn_fwd(x, params, res, act="gelu", impl=BF16):
    """``act="swiglu"``: ``w1`` is [2F, h] (gate rows, then up rows); FFN1 runs with the plain bias epilogue into
    ``h1`` [rows, 2F], ``swiglu_fwd`` (ops/swiglu.py) makes ``a`` [rows, F], FFN2 as ever. Saves (x, h1, a)."""
    if act not in ("gelu", "swiglu"):
        raise ValueError(f"act must be 'gelu' or 'swiglu', got {act!r}")
    _check_bf16_only(impl, swiglu=act == "swiglu")
    w1, b1, w2, b2 = params
    if act == "swiglu":
        h1 = impl.fwd(x, w1, b1)
        a = swiglu_fwd(h1)
        return impl.fwd(a, w2, b2, res=res), (x, h1, a)
    pre = torch.empty(x.shape[0], w1.shape[0], dtype=torch.bfloat16, device=x.device)
    # fp8: FFN1's epilogue may emit FFN2's quantised input directly (Fp8Linear.fwd_gelu_q)
    a = impl.fwd_gelu_q(x, w1, b1, pre, w2) if hasattr(impl, "fwd_gelu_q") else None
    if a is None:
        a = impl.fwd(x, w1, b1, gelu_aux=pre)  # a = gelu(pre), pre saved
    return impl.fwd(a, w2, b2, res=res), (x, pre, a)


def _ffn_bwd(saved, params, dy, G, db2, dres, act="gelu", impl=BF16):
    """``act="swiglu"``: FFN2's plain dgrad gives ``da``, ``swiglu_bwd`` gives dh1 = dg | du and FFN1's bias gradient
    (the column sums of the rounded dh1, set or accumulated into the flat-gradient sink), then FFN1's wgrad and
    dgrad as the GELU branch ends."""
    x, pre, a = saved
    w1, b1, w2, b2 = params
    dw2 = G.wgrad(w2, dy, a, impl)
    if isinstance(db2, str):
        db2 = G.colsum(b2, dy)
    if act == "swiglu":
        da = impl.dgrad(dy, w2, torch.empty_like(a))
        db, db_acc, db1 = G.out(b1, w1.shape[0], dy.device)
        dh1 = swiglu_bwd(da, pre, db, db_acc)
        dw1 = G.wgrad(w1, dh1, x, impl)
        dx = impl.dgrad(dh1, w1, torch.empty_like(x), res=dres)
        return dx, dw1, db1, dw2, db2
    if a.dtype == torch.float8_e4m3fn and impl.dgrad_gelu_q_ready(w1, x):
        # fp8 FFN fusion: FFN2's dgrad epilogue emits FFN1's e5m2 dY, dY^T and bias gradient
        db, db_acc, db1 = G.out(b1, w1.shape[0], dy.device)
        d8 = impl.dgrad_gelu_q(dy, w2, pre, w1, db, db_acc)
        dw1 = G.wgrad(w1, d8, x, impl)
        dx = impl.dgrad(d8, w1, torch.empty_like(x), res=dres)
        return dx, dw1, db1, dw2, db2
    if impl is BF16 and impl.dgelu_colsum_ok(dy, w2):
        # FFN1's bias gradient from the dGELU epilogue (no separate pass over dpre)
        db, db_acc, db1 = G.out(b1, w1.shape[0], dy.device)
        dpre = impl.dgrad(dy, w2, torch.empty_like(pre), aux=pre, colsum_out=db, colsum_acc=db_acc)
        dw1 = G.wgrad(w1, dpre, x, impl)
        dx = impl.dgrad(dpre, w1, torch.empty_like(x), res=dres)
        return dx, dw1, db1, dw2, db2
    dpre = impl.dgrad(dy, w2, torch.empty_like(pre), aux=pre)  # (dy . W2) * gelu'(pre)
    dw1, db1 = G.wgrad_bias(w1, b1, dpre, x, impl)
    dx = impl.dgrad(dpre, w1, torch.empty_like(x), res=dres)
    return dx, dw1, db1, dw2, db2


class _Core(NamedTuple):
    """A sub-layer core bound to its non-tensor argument and linear implementation; ``n_saved`` tensors of what a
    node saves are the core's."""
    fwd_fn: object
    bwd_fn: object
    n_saved: int
    what: object
    impl: object

    def fwd(self, x, params, res):
        return self.fwd_fn(x, params, res, self.what, self.impl)

    def bwd(self, saved, params, dy, G, dbias_last, dres):
        return self.bwd_fn(saved, params, dy, G, dbias_last, dres, self.what, self.impl)


def attn_core(spec: AttnSpec, impl=BF16) -> _Core:
    return _Core(_attn_fwd, _attn_bwd, 4, spec, impl)


def ffn_core(act: str = "gelu", impl=BF16) -> _Core:
    return _Core(_ffn_fwd, _ffn_bwd, 3, act, impl)


def _ln_fwd(x, gamma, beta, eps):
    C = require_native()
    rows = x.shape[0]
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    C.ln_fwd(x, gamma, beta, y, mean, rstd, eps)
    return y, (x, gamma, mean, rstd)


def _dropout_add_ln_fwd(y0, res, gamma, beta, eps, drop):
    """LN(dropout(y0) + res) in one kernel; ``drop`` = (p, seed, site, rank). The bf16 sum z takes
    the saved slot the GEMM output (linear + residual) has without dropout."""
    C = require_native()
    rows = y0.shape[0]
    z = torch.empty_like(y0)
    y = torch.empty_like(y0)
    mean = torch.empty(rows, dtype=torch.float32, device=y0.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=y0.device)
    C.dropout_add_ln_fwd(y0, res, gamma, beta, z, y, mean, rstd, eps, *drop)
    return y, (z, gamma, mean, rstd)


def _ln_bwd(saved, beta, dy, G, dxsum_param=None, drop=None, dres=None):
    """LayerNorm backward; with ``dxsum_param`` also the column sums of dx (= that bias's grad).
    Returns (dx, dgamma|None, dbeta|None, dbias|None, dxm|None).
    ``drop`` = (p, seed, site, rank) (needs ``dxsum_param``): the input was dropout(linear) +
    residual. dx is then the residual's gradient, dxm = mask * scale * dx is the linear's dY (None without
    ``drop``), and dbias holds dxm's column sums. ``dres`` (pre-norm blocks): added into dx in the kernel,
    with ``drop`` as well (dxm is then the masked, scaled copy of that total)."""
    C = require_native()
    x, gamma, mean, rstd = saved
    D = gamma.numel()
    dev = x.device
    dx = torch.empty_like(x)
    want = dxsum_param is not None
    part = torch.empty(C.ln_partial_blocks(x.shape[0]) * (3 if want else 2) * D, dtype=torch.float32, device=dev)
    sg = FlatParams.owner(gamma)
    sg = sg.grad_sink(gamma) if sg is not None else None
    sb = FlatParams.owner(beta)
    sb = sb.grad_sink(beta) if sb is not None else None
    acc = sg is not None and sb is not None
    if acc:
        G.ready += [gamma, beta]
        dg = db = None
        dg_t, db_t = sg, sb
    else:
        dg = dg_t = torch.empty(D, dtype=torch.float32, device=dev)
        db = db_t = torch.empty(D, dtype=torch.float32, device=dev)
    dxs_t, dxs_acc, dxs = G.out(dxsum_param, D, dev) if want else (None, False, None)
    if drop is not None:
        dxm = torch.empty_like(x)
        p, seed, site, rank = drop
        if dres is not None:
            C.ln_bwd_dropout_res(dy, x, gamma, mean, rstd, dx, part, dg_t, db_t, acc, dres, dxs_t, dxs_acc, dxm, p,
                                 seed, site, rank)
        else:
            C.ln_bwd(dy, x, gamma, mean, rstd, dx, part, dg_t, db_t, acc, None, dxsum=dxs_t, dxsum_acc=dxs_acc,
                     dxm=dxm, p=p, seed=seed, site=site, rank=rank)
        return dx, dg, db, dxs, dxm
    C.ln_bwd(dy, x, gamma, mean, rstd, dx, part, dg_t, db_t, acc, dres, dxsum=dxs_t, dxsum_acc=dxs_acc)
    return dx, dg, db, dxs, None


def _rms_fwd(x, gamma, eps):
    C = require_native()
    y = torch.empty_like(x)
    rstd = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    C.rms_fwd(x, gamma, y, rstd, eps)
    return y, (x, gamma, None, rstd)


def _dropout_add_rms_fwd(y0, res, gamma, eps, drop):
    """RMSNorm(dropout(y0) + res) in one kernel, as _dropout_add_ln_fwd."""
    C = require_native()
    z = torch.empty_like(y0)
    y = torch.empty_like(y0)
    rstd = torch.empty(y0.shape[0], dtype=torch.float32, device=y0.device)
    C.dropout_add_rms_fwd(y0, res, gamma, z, y, rstd, eps, *drop)
    return y, (z, gamma, None, rstd)


def _rms_bwd(saved, dy, G, dxsum_param=None, drop=None, dres=None):
    """RMSNorm backward, the arguments of _ln_bwd without beta and its five results (dbeta is None)."""
    C = require_native()
    x, gamma, _, rstd = saved
    D = gamma.numel()
    dev = x.device
    dx = torch.empty_like(x)
    want = dxsum_param is not None
    part = torch.empty(C.ln_partial_blocks(x.shape[0]) * (2 if want else 1) * D, dtype=torch.float32, device=dev)
    dg_t, acc, dg = G.out(gamma, D, dev)
    dxs_t, dxs_acc, dxs = G.out(dxsum_param, D, dev) if want else (None, False, None)
    dxm, kw = None, {}
    if drop is not None:
        dxm = torch.empty_like(x)
        p, seed, site, rank = drop
        kw = dict(dxm=dxm, p=p, seed=seed, site=site, rank=rank)
    C.rms_bwd(dy, x, gamma, rstd, dx, part, dg_t, acc, dres, dxsum=dxs_t, dxsum_acc=dxs_acc, **kw)
    return dx, dg, None, dxs, dxm


# The norm every block calls: LayerNorm when ``beta`` is a tensor, RMSNorm when it is None. The saved
# tuple is (x, gamma, mean | None, rstd) for both.
def _norm_fwd(x, gamma, beta, eps):
    return _rms_fwd(x, gamma, eps) if beta is None else _ln_fwd(x, gamma, beta, eps)


def _dropout_add_norm_fwd(y0, res, gamma, beta, eps, drop):
    if beta is None:
        return _dropout_add_rms_fwd(y0, res, gamma, eps, drop)
    return _dropout_add_ln_fwd(y0, res, gamma, beta, eps, drop)


def _norm_bwd(saved, beta, dy, G, dxsum_param=None, drop=None, dres=None):
    """(dx, dgamma, dbeta (None under RMSNorm), dbias, dxm (None without ``drop``)) of either norm."""
    if beta is None:
        return _rms_bwd(saved, dy, G, dxsum_param, drop, dres)
    return _ln_bwd(saved, beta, dy, G, dxsum_param, drop, dres)


_ATTN_SCALE = 1.0 / 8.0  # 1/sqrt(head_dim = 64)


def _bf16_grad(g):
    return None if g is None else g.contiguous().to(torch.bfloat16)


def _input_grads(ctx, *grads):
    """A backward's result: ``grads`` for the leading inputs of the node's forward, None for all the others."""
    return grads + (None,) * (len(ctx.needs_input_grad) - len(grads))


class _Block(torch.autograd.Function):
    """core(x) + x, without a norm: ``attention_block`` / ``ffn_block``."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, core):
        y, saved = core.fwd(x, (w1, b1, w2, b2), x)
        ctx.save_for_backward(*saved)
        ctx.params, ctx.core = (w1, b1, w2, b2), core
        return y

    @staticmethod
    def backward(ctx, dy):
        G = _Grads()
        dy = _bf16_grad(dy)
        grads = ctx.core.bwd(ctx.saved_tensors, ctx.params, dy, G, "colsum", dy)
        G.done()
        return _input_grads(ctx, *grads)


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        y, saved = _ln_fwd(x, gamma, beta, eps)
        ctx.save_for_backward(*saved)
        ctx.beta = beta
        return y

    @staticmethod
    def backward(ctx, dy):
        G = _Grads()
        dx, dg, db, _, _ = _ln_bwd(ctx.saved_tensors, ctx.beta, _bf16_grad(dy), G)
        G.done()
        return _input_grads(ctx, dx, dg, db)


def _sublayer_fwd(core, x, res, params, gamma, beta, eps, drop):
    """z = drop(core(x)) + res and Norm(z), the forward of both block nodes: (z, Norm(z), what the core saves,
    what the norm saves). Without ``drop`` the core's last linear adds ``res`` in its epilogue and the norm kernel
    normalises; with ``drop`` = (p, seed, site, rank) the dropout_add norm kernel drops, adds and normalises, and
    its bf16 sum z takes the saved slot the GEMM output has without dropout."""
    if drop is None:
        z, s1 = core.fwd(x, params, res)
        y, s2 = _norm_fwd(z, gamma, beta, eps)
    else:
        y0, s1 = core.fwd(x, params, None)
        y, s2 = _dropout_add_norm_fwd(y0, res, gamma, beta, eps, drop)
    return s2[0], y, s1, s2


class _PostNormBlock(torch.autograd.Function):
    """x -> Norm(drop(core(x)) + x) as one node: the norm backward also emits the bias gradient of the core's last
    linear (column sums of its dx), so no separate pass over dy. Under ``drop`` its dx is the gradient of the
    residual x and its masked, scaled copy DXM the last linear's dY."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, gamma, beta, eps, core, drop):
        params = (w1, b1, w2, b2)
        _, y, s1, s2 = _sublayer_fwd(core, x, x, params, gamma, beta, eps, drop)
        ctx.save_for_backward(*s1, *s2)
        ctx.params, ctx.beta, ctx.core, ctx.drop = params, beta, core, drop
        return y

    @staticmethod
    def backward(ctx, dy):
        t, k = ctx.saved_tensors, ctx.core.n_saved
        G = _Grads()
        dz, dg, db, dbl, dxm = _norm_bwd(t[k:], ctx.beta, _bf16_grad(dy), G, dxsum_param=ctx.params[3], drop=ctx.drop)
        grads = ctx.core.bwd(t[:k], ctx.params, dz if ctx.drop is None else dxm, G, dbl, dz)
        G.done()
        return _input_grads(ctx, *grads, dg, db)


class _StreamNorm(torch.autograd.Function):
    """(h, Norm(h)): the entry of a pre-norm stack. The stream h is handed through, so that its two consumers
    (the first block's residual add and this norm) return one gradient: the norm backward adds dh as DRES."""

    @staticmethod
    def forward(ctx, h, gamma, beta, eps):
        n, saved = _norm_fwd(h, gamma, beta, eps)
        ctx.save_for_backward(*saved)
        ctx.beta = beta
        ctx.set_materialize_grads(False)
        return h.view_as(h), n

    @staticmethod
    def backward(ctx, dh, dn):
        if dn is None:
            return _input_grads(ctx, dh)
        G = _Grads()
        dx, dg, db, _, _ = _norm_bwd(ctx.saved_tensors, ctx.beta, _bf16_grad(dn), G, dres=_bf16_grad(dh))
        G.done()
        return _input_grads(ctx, dx, dg, db)


class _PreNormBlock(torch.autograd.Function):
    """One pre-norm sub-layer as a node (h, n) -> (h', n'): h' = h + drop(core(n)) and n' = Norm(h') under the NEXT
    sub-layer's norm weights. Forward: the core's last linear adds h in its epilogue and the norm kernel normalises
    (with ``drop``: the dropout_add norm kernel writes both h' and n'). Backward of (dh', dn'): the norm backward
    with DRES = dh' gives the total stream gradient, which is the residual's gradient and the last linear's dY (its
    masked copy DXM under dropout), with that linear's bias gradient as the fused column sums; the core's first
    dgrad then yields dn with nothing added."""

    @staticmethod
    def forward(ctx, h, n, w1, b1, w2, b2, gamma, beta, eps, core, drop):
        params = (w1, b1, w2, b2)
        h2, n2, s1, s2 = _sublayer_fwd(core, n, h, params, gamma, beta, eps, drop)
        ctx.save_for_backward(*s1, *s2)
        ctx.params, ctx.beta, ctx.core, ctx.drop = params, beta, core, drop
        ctx.set_materialize_grads(False)
        return h2, n2

    @staticmethod
    def backward(ctx, dh2, dn2):
        t, k = ctx.saved_tensors, ctx.core.n_saved
        G = _Grads()
        dn2 = torch.zeros_like(t[k]) if dn2 is None else _bf16_grad(dn2)
        dh, dg, db, dbl, dxm = _norm_bwd(t[k:], ctx.beta, dn2, G, dxsum_param=ctx.params[3], drop=ctx.drop,
                                         dres=_bf16_grad(dh2))
        dn, *grads = ctx.core.bwd(t[:k], ctx.params, dh if ctx.drop is None else dxm, G, dbl, None)
        G.done()
        return _input_grads(ctx, dh, dn, *grads, dg, db)


class _Embeddings(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, tt, ww, wp, wt, S, pos=None, cu_seqlens=None):
        C = require_native()
        ids = ids.contiguous().view(-1).to(torch.int64)
        ttf = tt.contiguous().view(-1).to(torch.int64) if tt is not None else None
        D = ww.shape[1]
        out = torch.empty(ids.numel(), D, dtype=torch.bfloat16, device=ids.device)
        if (pos is None) != (cu_seqlens is None):
            raise ValueError("packed embeddings take both pos and cu_seqlens")
        C.embed_fwd(ids, ttf, bf16_weight(ww), None if wp is None else bf16_weight(wp), bf16_weight(wt), out, S,
                    pos=pos)
        ctx.save_for_backward(ids, ttf if ttf is not None else torch.empty(0, dtype=torch.int64))
        ctx.cu = cu_seqlens
        ctx.meta = (tt is not None, S, ww.shape, None if wp is None else wp.shape, wt.shape)
        ctx.tables = (ww, wp, wt)
        return out

    @staticmethod
    def backward(ctx, dout):
        C = require_native()
        ids, ttf = ctx.saved_tensors
        has_tt, S, sw, sp, st = ctx.meta
        dout = dout.contiguous().to(torch.bfloat16)
        G = _Grads()
        ww, wp, wt = ctx.tables
        sinks = [None if p is None else G.sink(p) for p in (ww, wp, wt)]
        if all(s is not None or p is None for s, p in zip(sinks, (ww, wp, wt))):
            gw, gp, gt = sinks  # scatter-add straight into the flat gradients
            ret = (None, None, None)
        else:
            G.ready = []
            gw = torch.zeros(sw, dtype=torch.float32, device=dout.device)
            gp = None if wp is None else torch.zeros(sp, dtype=torch.float32, device=dout.device)
            gt = torch.zeros(st, dtype=torch.float32, device=dout.device)
            ret = (gw, gp, gt)
        D = sw[1]
        # stable sort of the ids: the word-table scatter then has one writer per row, summing its
        # tokens in order (no atomics, bitwise reproducible)
        sid, perm = torch.sort(ids.view(-1).clamp(0, sw[0] - 1), stable=True)
        part = torch.empty(S * 2 * D, dtype=torch.float32, device=dout.device)
        C.embed_bwd(sid, perm, ttf if has_tt else None, dout, gw, gp, gt, part, S, cu_seqlens=ctx.cu)
        G.done()
        return (None, None) + ret + (None, None, None)


class _ClassifierHead(torch.autograd.Function):
    """BERT pooler + classifier (reference criterion input, src/trainer.py:141-142) on the native
    kernels: pooled = tanh(cls . W_p^T + b_p) is the bf16 GEMM with the tanh epilogue (fp32 out),
    logits = pooled . W_c^T + b_c and its backward (dpre = (dlogits . W_c) * (1 - pooled^2), dW_c,
    db_c) run in head.hip; the pooler's wgrad / bias grad / dgrad are the native GEMMs / colsum."""

    @staticmethod
    def forward(ctx, cls, wp, bp, wc, bc):
        C = require_native()
        B, h = cls.shape
        pooled = torch.empty(B, wp.shape[0], dtype=torch.float32, device=cls.device)
        C.gemm(cls, bf16_weight(wp), pooled, False, False, bias=bp, mode=3)
        logits = torch.empty(B, wc.shape[0], dtype=torch.float32, device=cls.device)
        C.head_cls_fwd(pooled, wc.detach().float().contiguous(), bc.detach().float().contiguous(), logits)
        ctx.save_for_backward(cls, pooled)
        ctx.params = (wp, bp, wc, bc)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        C = require_native()
        cls, pooled = ctx.saved_tensors
        wp, bp, wc, bc = ctx.params
        G = _Grads()
        dpre = torch.empty(pooled.shape, dtype=torch.bfloat16, device=pooled.device)
        gwc, gbc = G.sink(wc), G.sink(bc)
        both = gwc is not None and gbc is not None
        dwc = gwc if both else torch.empty(wc.shape, dtype=torch.float32, device=wc.device)
        dbc = gbc if both else torch.empty(bc.shape, dtype=torch.float32, device=bc.device)
        if not both:
            G.ready = [p for p in G.ready if p is not wc and p is not bc]
        C.head_cls_bwd(dlogits.contiguous().float(), pooled, wc.detach().float().contiguous(), dpre, dwc, dbc,
                       accumulate=both)
        dwp = G.wgrad(wp, dpre, cls)
        dbp = G.colsum(bp, dpre)
        dcls = torch.empty(cls.shape, dtype=torch.bfloat16, device=cls.device)
        C.gemm(dpre, bf16_weight(wp), dcls, False, True)
        G.done()
        return dcls, dwp, dbp, (None if both else dwc), (None if both else dbc)


def classifier_head(cls, wp, bp, wc, bc):
    """cls [B, h] bf16 (may be a strided row view) -> logits [B, num_labels] fp32."""
    return _ClassifierHead.apply(cls, wp, bp, wc, bc)


def _mark_training(impl) -> None:
    # autograd runs Function.forward with grad mode off: tell the linear implementation here
    # whether a backward will follow (fp8 keeps transposed activations only then)
    if impl is not BF16:
        type(impl).training = torch.is_grad_enabled()


def block(core: _Core, x, params):
    """core(x) + x as one node; ``params`` = (w_first, b_first, w_last, b_last)."""
    _mark_training(core.impl)
    return _Block.apply(x, *params, core)


def post_norm_block(core: _Core, x, params, norm, drop=None):
    """Norm(drop(core(x)) + x) as one node. ``norm`` = (gamma, beta, eps) of the norm that closes the sub-layer.
    ``drop`` = (p, seed, site, rank): hidden dropout on the last linear's output, before the residual add, fused
    into the norm kernels (mask: ops/dropout.py; indexed by packed row for a packed batch). None: no dropout."""
    _mark_training(core.impl)
    return _PostNormBlock.apply(x, *params, *norm, core, drop)


def pre_norm_block(core: _Core, h, n, params, norm, drop=None):
    """(h, n) -> (h + drop(core(n)), Norm(that sum)) as one node; ``norm`` = (gamma, beta or None: RMSNorm, eps) of
    the norm that FOLLOWS. ``drop`` as in post_norm_block."""
    _check_bf16_only(core.impl, pre_norm=True)
    return _PreNormBlock.apply(h, n, *params, *norm, core, drop)


def attention_block(x, wqkv, bqkv, wo, bo, lens: Optional[torch.Tensor], B: int, S: int, H: int, impl=BF16,
                    attn_drop=None, cu_seqlens: Optional[torch.Tensor] = None, causal: bool = False, rope=None):
    """``attn_drop`` = (p, seed, site, rank): attention-probability dropout inside the flash attention
    kernels (the byte mask of ops/dropout.py: ``p`` is applied as round(p * 256) / 256). None: none.
    ``cu_seqlens`` (int32 [B + 1], device): x is a packed [T, D] batch (``pack_batch``), ``S`` is
    max_seqlen and ``lens`` is unused. The dropout mask of element (b, h, q, k) is the padded run's.
    x may end in tail rows past cu_seqlens[B] that belong to no sequence: fewer than PACK_ROW_MULTIPLE
    of them (``pack_batch`` keeps to that), since only that many trailing rows of the attention output
    and of dQKV are zeroed (``_zero_packed_tail``).
    ``causal``: key j is visible to query i of the same sequence iff j <= i and j < len_b (the causal
    instantiations of the three kernels, which skip the blocks above the diagonal); bf16 linears only.
    Composes with ``attn_drop`` (the non-causal run's keep mask, restricted) and ``cu_seqlens``.
    ``rope`` = (table fp32 [P, 32, 2], pos): rotary positions (ops/rope.py), q and k rotated in place after the
    QKV GEMM by ``C.rope_qk`` and dQKV rotated back in the backward; ``pos`` is None for a padded batch
    (position = row % S) or the packed batch's int32 positions, one per row of x. bf16 linears only."""
    spec = attn_spec(wqkv, lens, B, S, H, attn_drop, cu_seqlens, causal, rope)
    return block(attn_core(spec, impl), x, (wqkv, bqkv, wo, bo))


def ffn_block(x, w1, b1, w2, b2, impl=BF16, act: str = "gelu"):
    """``act``: ``"gelu"``, or ``"swiglu"`` (``w1`` [2F, h], ``b1`` [2F]: gate rows, then up rows; ops/swiglu.py;
    bf16 linears only)."""
    return block(ffn_core(act, impl), x, (w1, b1, w2, b2))


def attention_ln_block(x, wqkv, bqkv, wo, bo, gamma, beta, lens: Optional[torch.Tensor], B: int, S: int, H: int,
                       eps: float, impl=BF16, drop=None, attn_drop=None, cu_seqlens: Optional[torch.Tensor] = None,
                       causal: bool = False, rope=None):
    """post_norm_block around the attention core. ``drop``: hidden dropout on the out-projection's output.
    ``attn_drop``, ``causal``, ``rope``: see attention_block. ``cu_seqlens``: packed batch, with fewer than
    PACK_ROW_MULTIPLE tail rows (see attention_block)."""
    spec = attn_spec(wqkv, lens, B, S, H, attn_drop, cu_seqlens, causal, rope)
    return post_norm_block(attn_core(spec, impl), x, (wqkv, bqkv, wo, bo), (gamma, beta, eps), drop)


def ffn_ln_block(x, w1, b1, w2, b2, gamma, beta, eps: float, impl=BF16, drop=None, act: str = "gelu"):
    """post_norm_block around the FFN core. ``drop``: hidden dropout on FFN2's output. ``act``: see ffn_block."""
    return post_norm_block(ffn_core(act, impl), x, (w1, b1, w2, b2), (gamma, beta, eps), drop)


def layer_norm(x, gamma, beta, eps: float):
    return _LayerNorm.apply(x, gamma, beta, eps)


def stream_norm(h, gamma, beta, eps: float):
    """(h, Norm(h)) at the entry of a pre-norm stack, or wherever a stream meets a norm on its own: LayerNorm
    with ``beta``, RMSNorm (``rms_fwd`` / ``rms_bwd``) with ``beta=None``. Use both results: the node's
    backward adds the stream's gradient into the norm's in the kernel."""
    return _StreamNorm.apply(h, gamma, beta, eps)


def pre_attention_block(h, n, wqkv, bqkv, wo, bo, gamma, beta, lens: Optional[torch.Tensor], B: int, S: int, H: int,
                        eps: float, impl=BF16, drop=None, attn_drop=None, cu_seqlens: Optional[torch.Tensor] = None,
                        causal: bool = False, rope=None):
    """The pre-norm attention sub-layer: (h, n) -> (h + drop(Out(Attn(QKV(n)))), Norm(that sum)) where
    ``gamma`` / ``beta`` (None: RMSNorm) are the weights of the norm that FOLLOWS (the layer's ``ln2``).
    Every other argument as in attention_ln_block."""
    spec = attn_spec(wqkv, lens, B, S, H, attn_drop, cu_seqlens, causal, rope)
    return pre_norm_block(attn_core(spec, impl), h, n, (wqkv, bqkv, wo, bo), (gamma, beta, eps), drop)


def pre_ffn_block(h, n, w1, b1, w2, b2, gamma, beta, eps: float, impl=BF16, drop=None, act: str = "gelu"):
    """The pre-norm FFN sub-layer: (h, n) -> (h + drop(FFN2(gelu(FFN1(n)))), Norm(that sum)); ``gamma`` / ``beta``
    belong to the next layer's ``ln1``, or to the final norm after the last layer. ``act``: see ffn_block."""
    return pre_norm_block(ffn_core(act, impl), h, n, (w1, b1, w2, b2), (gamma, beta, eps), drop)


class _Dropout(torch.autograd.Function):
    """Stand-alone dropout of a bf16 [rows, D] tensor (the embedding site); the backward runs the
    same kernel on dy with the recomputed mask."""

    @staticmethod
    def forward(ctx, x, p, seed, site, rank):
        x = x.contiguous()
        out = torch.empty_like(x)
        require_native().dropout(x, out, p, seed, site, rank)
        ctx.drop = (p, seed, site, rank)
        return out

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous().to(torch.bfloat16)
        dx = torch.empty_like(dy)
        require_native().dropout(dy, dx, *ctx.drop)
        return dx, None, None, None, None


def dropout(x, p: float, seed: int, site: int, rank: int):
    """keep ? bf16(x * 1/(1-p)) : 0 with the mask of ops/dropout.py at (seed, site, rank)."""
    return _Dropout.apply(x, p, seed, site, rank)


def embeddings(ids, tt, ww, wp, wt, S: int, pos=None, cu_seqlens=None):
    """Padded form: ids / tt [B, S], position = column. Packed form (``pack_batch``): ids / tt [T],
    ``pos`` int32 [T] (index inside the token's own sequence), ``cu_seqlens`` int32 [B + 1], S = max_seqlen.
    ``wp`` None (rotary positions): no position table, the output is word + type."""
    return _Embeddings.apply(ids, tt, ww, wp, wt, S, pos, cu_seqlens)


class PackedBatch:
    """A right-padded [B, S] batch without its pads: ``ids`` / ``tt`` (or None) [T], ``pos`` int32 [T]
    (index inside the token's own sequence), ``cu_seqlens`` int32 [B + 1] (sequence b = rows cu[b] ..
    cu[b + 1]; ``cu_seqlens[:-1]`` are the CLS rows), ``index`` int64 [T] (the flat b * S + pos of every
    kept token), ``max_seqlen`` = S and ``tokens`` = T as a host int. ``rows`` >= T is the row count of
    ``ids`` / ``tt`` / ``pos``: with ``row_multiple`` the packed matrix ends in ``rows - T`` inert tail
    rows (token 0 at position 0) that belong to no sequence, see ``pack_batch``."""

    __slots__ = ("ids", "tt", "pos", "cu_seqlens", "index", "max_seqlen", "tokens", "batch", "rows")

    def __init__(self, ids, tt, pos, cu_seqlens, index, max_seqlen, tokens, batch, rows):
        self.ids, self.tt, self.pos, self.cu_seqlens, self.index = ids, tt, pos, cu_seqlens, index
        self.max_seqlen, self.tokens, self.batch, self.rows = max_seqlen, tokens, batch, rows

    @property
    def cls_rows(self):
        return self.cu_seqlens[:-1].to(torch.int64)


PACK_ROW_MULTIPLE = 256  # the row tile of the fast GEMM kernels (M of forward / dgrad, K of wgrad)


def pack_batch(ids, lens, token_type_ids=None, row_multiple: int = 1) -> PackedBatch:
    """Drop the pads of ``ids`` [B, S] given ``lens`` [B] (right padding: row b holds its tokens at
    columns 0 .. lens[b] - 1; lengths are clamped to 1 .. S). Runs on the device of ``ids`` with torch
    index ops; reading T = sum(lens) back to size the packed tensors is the one device-to-host read.

    ``row_multiple`` > 1 rounds the row count up to that multiple (when that still fits B * S) with
    inert tail rows: the 256-row GEMM tiles need it, an odd T sends every linear layer to the slow
    general kernels. The tail rows belong to no sequence (cu_seqlens[B] = T): attention neither reads
    nor writes them (the attention blocks zero them), they never reach a CLS row, and their gradients
    are exactly zero, so they add nothing to any weight gradient."""
    B, S = ids.shape
    lens = lens.to(device=ids.device, dtype=torch.int64).clamp(1, S)
    cu = torch.zeros(B + 1, dtype=torch.int32, device=ids.device)
    cu[1:] = torch.cumsum(lens, 0)
    keep = torch.arange(S, device=ids.device)[None, :] < lens[:, None]
    index = keep.view(-1).nonzero().view(-1)  # (the host read of T happens here)
    T = int(index.numel())
    pos = (index % S).to(torch.int32)
    pids = ids.reshape(-1).index_select(0, index)
    ptt = token_type_ids.reshape(-1).index_select(0, index) if token_type_ids is not None else None
    rows = -(-T // row_multiple) * row_multiple
    if rows > T and rows <= B * S:
        tail = rows - T
        pids = torch.cat((pids, pids.new_zeros(tail)))
        pos = torch.cat((pos, pos.new_zeros(tail)))
        ptt = torch.cat((ptt, ptt.new_zeros(tail))) if ptt is not None else None
    else:
        rows = T
    return PackedBatch(pids, ptt, pos, cu, index, S, T, B, rows)


def unpack_rows(x, packed: PackedBatch, fill=0):
    """The packed rows ``x`` [T, ...] back at their padded places: [B * S, ...] with ``fill`` at the pads."""
    out = x.new_full((packed.batch * packed.max_seqlen,) + tuple(x.shape[1:]), fill)
    out.index_copy_(0, packed.index, x[:packed.tokens])
    return out
