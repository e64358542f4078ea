"""Autograd blocks of the transformer path over the native gfx950 kernels.

Mixed precision: parameters are fp32 masters (in a FlatParams buffer when an
optimizer/DDP owns them); compute reads their bf16 *shadow* (refreshed by the
fused optimizer kernel in the same pass that updates the master, so there is
no separate cast per step). Weight / bias gradients come back in fp32.

Blocks (one autograd node each, so the backward can fuse across ops):

* ``attention_block``: x -> QKV GEMM(+bias) -> fused flash attention -> out-proj
  GEMM (+bias +residual x). Backward: wgrad/colsum/dgrad of out-proj, attention
  backward into the packed dQKV, wgrad/colsum of QKV and dgrad with the residual
  gradient folded into the GEMM epilogue.
* ``ffn_block``: x -> FFN1 GEMM (+bias, GELU epilogue that also stores the
  pre-activation) -> FFN2 GEMM (+bias +residual). Backward: FFN2's dgrad GEMM
  applies gelu'(pre) in its epilogue (no separate elementwise pass).
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
from typing import Optional

import torch

from ml_trainer_amd.ops._ext import require_native
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


def _attn_drop_kw(attn_drop):
    """Keyword arguments of C.attn_fwd / C.attn_bwd for ``attn_drop`` = (p, seed, site, rank) or None."""
    if attn_drop is None:
        return {}
    p, seed, site, rank = attn_drop
    return dict(p=p, seed=seed, site=site, rank=rank)


def _zero_packed_tail(t, cu_seqlens):
    """Packed batches may end in inert tail rows (``pack_batch``) that the attention kernels never write:
    zero the last rows before the launch, which then overwrites the real ones among them. T is not known
    on the host here, so the attention blocks support FEWER THAN PACK_ROW_MULTIPLE tail rows, which is
    what ``pack_batch`` produces; rows of a longer tail would keep uninitialised memory."""
    if cu_seqlens is not None:
        t[-min(PACK_ROW_MULTIPLE - 1, t.shape[0]):].zero_()


def _causal_kw(causal, impl):
    """Keyword arguments of C.attn_fwd / C.attn_bwd for ``causal``; the keyword goes out only when set."""
    if not causal:
        return {}
    if impl is not BF16:
        raise ValueError("causal attention runs the bf16 linears only: the fp8 (q8) attention epilogue has no "
                         "causal instantiation")
    return dict(causal=True)


def _rope_qk(t, rope, S, H, sign=1):
    """Rotary positions: rotate the q and k columns of ``t`` (QKV, or dQKV with ``sign=-1``) in place.
    ``rope`` = (table fp32 [P, 32, 2], pos int32 [rows] or None: row % S), see ops/rope.py."""
    table, pos = rope
    require_native().rope_qk(t, table, H, S, pos=pos, sign=sign)


def _attn_fwd(x, wqkv, bqkv, wo, bo, lens, B, S, H, impl=BF16, residual=True, attn_drop=None, cu_seqlens=None,
              causal: bool = False, rope=None, res=None):
    """``attn_drop`` = (p, seed, site, rank): attention-probability dropout inside the flash kernels
    (the byte mask of ops/dropout.py, recomputed in the backward); None: no dropout.
    ``cu_seqlens`` (int32 [B + 1], device): packed batch, x is [T, D] with sequence b at rows
    cu[b] .. cu[b + 1]; S is max_seqlen and ``lens`` is unused.
    ``causal``: key j is visible to query i of its sequence iff j <= i and j < len_b.
    ``rope`` = (table, pos or None): rotary positions, q and k rotated in place between the QKV GEMM and the
    attention kernel (``pos`` for packed batches); the saved qkv is the rotated one, which the attention
    backward needs. ``res``: the residual the out-projection adds instead of ``x`` (pre-norm blocks: x is the
    norm of the stream, ``res`` the stream)."""
    C = require_native()
    ckw = _causal_kw(causal, impl)
    if cu_seqlens is not None and impl is not BF16:
        raise ValueError("packed (cu_seqlens) attention runs the bf16 linears only: the fp8 attention epilogue "
                         "writes at b * S offsets")
    if rope is not None and impl is not BF16:
        raise ValueError("rotary positions run the bf16 linears only: the fp8 attention backward writes dQKV as "
                         "e5m2, which the inverse rotation cannot take")
    qkv = impl.fwd(x, wqkv, bqkv)
    if rope is not None:
        _rope_qk(qkv, rope, S, H)
    attn = torch.empty(x.shape[0], H * 64, dtype=torch.bfloat16, device=x.device)
    lse = torch.empty(B * H * S, dtype=torch.float32, device=x.device)
    _zero_packed_tail(attn, cu_seqlens)
    C.attn_fwd(qkv, attn, lse, lens, B, S, H, _ATTN_SCALE, cu_seqlens=cu_seqlens, **_attn_drop_kw(attn_drop), **ckw)
    # out-proj + bias + residual (under dropout the residual joins in the LayerNorm kernel instead)
    y = impl.fwd(attn, wo, bo, res=(x if res is None else res) if residual else None)
    return y, (x, qkv, attn, lse)


def _attn_bwd(saved, params, lens, B, S, H, dy, G, dbo="colsum", impl=BF16, dres=None, attn_drop=None,
              cu_seqlens=None, causal: bool = False, rope=None, residual=True):
    """Backward of the attention block. ``dbo``: "colsum" to reduce dy here, otherwise the
    out-proj bias gradient already produced by the LayerNorm backward (tensor or None).
    ``dres``: the gradient of the residual branch when it differs from the out-proj's ``dy``
    (hidden dropout sits between them); defaults to ``dy``. ``attn_drop``, ``cu_seqlens``, ``causal``: the
    forward's. ``rope``: the forward's; dQKV comes out of the attention backward in the rotated frame and is
    rotated back (``sign=-1``) before anything else reads it. The QKV bias gradient is then the column sum of the
    rotated-back dQKV: the attention kernels' own column sums are sums in the rotated frame, which differ row by
    row, so that fused branch is not taken under rotary. ``residual=False`` (pre-norm blocks): the block's input
    is not its residual, the QKV dgrad adds nothing."""
    C = require_native()
    akw = _attn_drop_kw(attn_drop)
    akw.update(_causal_kw(causal, impl))
    if cu_seqlens is not None:
        akw["cu_seqlens"] = cu_seqlens
    x, qkv, attn, lse = saved
    wqkv, bqkv, wo, bo = params
    dres = dy if dres is None else dres
    dwo = G.wgrad(wo, dy, attn, impl)
    if isinstance(dbo, str):
        dbo = G.colsum(bo, dy)
    dattn = impl.dgrad(dy, wo, torch.empty_like(attn))
    dqkv = torch.empty_like(qkv)
    _zero_packed_tail(dqkv, cu_seqlens)
    delta = torch.empty(qkv.shape[0] * H, dtype=torch.float32, device=dy.device)
    q8 = impl.attn_dy_q(wqkv, x, qkv.shape[0]) if (impl is not BF16 and hasattr(impl, "attn_dy_q")) else None
    if rope is not None:
        C.attn_bwd(qkv, attn, dattn, lse, delta, lens, dqkv, B, S, H, _ATTN_SCALE, **akw)
        _rope_qk(dqkv, rope, S, H, sign=-1)
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
    dx = impl.dgrad(dqkv, wqkv, torch.empty_like(x), res=dres if residual else None)  # dqkv . Wqkv + dres
    return dx, dwqkv, dbqkv, dwo, dbo


def _ffn_fwd(x, w1, b1, w2, b2, impl=BF16, residual=True, res=None):
    pre = torch.empty(x.shape[0], w1.shape[0], dtype=torch.bfloat16, device=x.device)
    # fp8: FFN1's epilogue may emit FFN2's quantised input directly (Fp8Linear.fwd_gelu_q)
    a = impl.fwd_gelu_q(x, w1, b1, pre, w2) if hasattr(impl, "fwd_gelu_q") else None
    if a is None:
        a = impl.fwd(x, w1, b1, gelu_aux=pre)  # a = gelu(pre), pre saved
    y = impl.fwd(a, w2, b2, res=(x if res is None else res) if residual else None)  # (res: as in _attn_fwd)
    return y, (x, pre, a)


def _ffn_bwd(saved, params, dy, G, db2="colsum", impl=BF16, dres=None, residual=True):
    """``dres``: the residual branch's gradient when hidden dropout separates it from FFN2's ``dy``.
    ``residual=False`` (pre-norm blocks): FFN1's dgrad adds no residual gradient."""
    x, pre, a = saved
    w1, b1, w2, b2 = params
    dres = (dy if dres is None else dres) if residual else None
    dw2 = G.wgrad(w2, dy, a, impl)
    if isinstance(db2, str):
        db2 = G.colsum(b2, dy)
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
    Returns (dx, dgamma|None, dbeta|None, dbias|None).
    ``drop`` = (p, seed, site, rank) (needs ``dxsum_param``): the input was dropout(linear) +
    residual. dx is then the residual's gradient, a fifth result dxm = mask * scale * dx is the
    linear's dY, and dbias holds dxm's column sums. ``dres`` (pre-norm blocks): added into dx in the kernel,
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
    return dx, dg, db, dxs


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
    """RMSNorm backward, the arguments of _ln_bwd without beta. Returns (dx, dgamma|None, dbias|None, dxm|None)."""
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
    return dx, dg, dxs, dxm


# The norm of a pre-norm block: LayerNorm when ``beta`` is a tensor, RMSNorm when it is None. The saved
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
        dx, dg, dxs, dxm = _rms_bwd(saved, dy, G, dxsum_param, drop, dres)
        return dx, dg, None, dxs, dxm
    r = _ln_bwd(saved, beta, dy, G, dxsum_param, drop, dres)
    return r if drop is not None else r + (None,)


_ATTN_SCALE = 1.0 / 8.0  # 1/sqrt(head_dim = 64)


class _AttentionBlock(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wqkv, bqkv, wo, bo, lens, B, S, H, impl, attn_drop=None, cu_seqlens=None, causal=False,
                rope=None):
        y, saved = _attn_fwd(x, wqkv, bqkv, wo, bo, lens, B, S, H, impl, attn_drop=attn_drop, cu_seqlens=cu_seqlens,
                             causal=causal, rope=rope)
        ctx.save_for_backward(*saved)
        ctx.params, ctx.impl, ctx.rope = (wqkv, bqkv, wo, bo), impl, rope
        ctx.lens, ctx.dims, ctx.attn_drop, ctx.cu, ctx.causal = lens, (B, S, H), attn_drop, cu_seqlens, causal
        return y

    @staticmethod
    def backward(ctx, dy):
        G = _Grads()
        grads = _attn_bwd(ctx.saved_tensors, ctx.params, ctx.lens, *ctx.dims, dy.contiguous().to(torch.bfloat16), G,
                          impl=ctx.impl, attn_drop=ctx.attn_drop, cu_seqlens=ctx.cu, causal=ctx.causal,
                          rope=ctx.rope)
        G.done()
        return grads + (None, None, None, None, None, None, None, None, None)


class _FFNBlock(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, impl):
        y, saved = _ffn_fwd(x, w1, b1, w2, b2, impl)
        ctx.save_for_backward(*saved)
        ctx.params, ctx.impl = (w1, b1, w2, b2), impl
        return y

    @staticmethod
    def backward(ctx, dy):
        G = _Grads()
        grads = _ffn_bwd(ctx.saved_tensors, ctx.params, dy.contiguous().to(torch.bfloat16), G, impl=ctx.impl)
        G.done()
        return grads + (None,)


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
        dx, dg, db, _ = _ln_bwd(ctx.saved_tensors, ctx.beta, dy.contiguous().to(torch.bfloat16), G)
        G.done()
        return dx, dg, db, None


class _AttentionLNBlock(torch.autograd.Function):
    """LN(attention_block(x)) as one node: the LayerNorm backward also emits the out-proj bias
    gradient (column sums of its dx), so no separate pass over dy."""

    @staticmethod
    def forward(ctx, x, wqkv, bqkv, wo, bo, gamma, beta, lens, B, S, H, eps, impl, drop=None, attn_drop=None,
                cu_seqlens=None, causal=False, rope=None):
        if drop is None:
            a, s1 = _attn_fwd(x, wqkv, bqkv, wo, bo, lens, B, S, H, impl, attn_drop=attn_drop, cu_seqlens=cu_seqlens,
                              causal=causal, rope=rope)
            y, s2 = _ln_fwd(a, gamma, beta, eps)
        else:  # LN(dropout(out-proj) + x): dropout and the residual add inside the LayerNorm kernel
            a, s1 = _attn_fwd(x, wqkv, bqkv, wo, bo, lens, B, S, H, impl, residual=False, attn_drop=attn_drop,
                              cu_seqlens=cu_seqlens, causal=causal, rope=rope)
            y, s2 = _dropout_add_ln_fwd(a, x, gamma, beta, eps, drop)
        ctx.save_for_backward(*s1, *s2)
        ctx.params, ctx.beta, ctx.impl = (wqkv, bqkv, wo, bo), beta, impl
        ctx.lens, ctx.dims, ctx.drop, ctx.attn_drop, ctx.cu = lens, (B, S, H), drop, attn_drop, cu_seqlens
        ctx.causal, ctx.rope = causal, rope
        return y

    @staticmethod
    def backward(ctx, dy):
        t = ctx.saved_tensors
        G = _Grads()
        if ctx.drop is None:
            da, dg, db, dbo = _ln_bwd(t[4:], ctx.beta, dy.contiguous().to(torch.bfloat16), G,
                                      dxsum_param=ctx.params[3])  # da = out-proj dY
            dres = None
        else:  # dres: gradient of the residual x; da = its masked, scaled copy, the out-proj dY
            dres, dg, db, dbo, da = _ln_bwd(t[4:], ctx.beta, dy.contiguous().to(torch.bfloat16), G,
                                            dxsum_param=ctx.params[3], drop=ctx.drop)
        dx, dwqkv, dbqkv, dwo, dbo = _attn_bwd(t[:4], ctx.params, ctx.lens, *ctx.dims, da, G, dbo=dbo,
                                               impl=ctx.impl, dres=dres, attn_drop=ctx.attn_drop, cu_seqlens=ctx.cu,
                                               causal=ctx.causal, rope=ctx.rope)
        G.done()
        return dx, dwqkv, dbqkv, dwo, dbo, dg, db, None, None, None, None, None, None, None, None, None, None, None


class _FFNLNBlock(torch.autograd.Function):
    """LN(ffn_block(x)) as one node (FFN2 bias gradient fused into the LayerNorm backward)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, gamma, beta, eps, impl, drop=None):
        if drop is None:
            f, s1 = _ffn_fwd(x, w1, b1, w2, b2, impl)
            y, s2 = _ln_fwd(f, gamma, beta, eps)
        else:  # LN(dropout(FFN2) + x)
            f, s1 = _ffn_fwd(x, w1, b1, w2, b2, impl, residual=False)
            y, s2 = _dropout_add_ln_fwd(f, x, gamma, beta, eps, drop)
        ctx.save_for_backward(*s1, *s2)
        ctx.params, ctx.beta, ctx.impl, ctx.drop = (w1, b1, w2, b2), beta, impl, drop
        return y

    @staticmethod
    def backward(ctx, dy):
        t = ctx.saved_tensors
        G = _Grads()
        if ctx.drop is None:
            df, dg, db, db2 = _ln_bwd(t[3:], ctx.beta, dy.contiguous().to(torch.bfloat16), G,
                                      dxsum_param=ctx.params[3])  # df = FFN2 dY
            dres = None
        else:
            dres, dg, db, db2, df = _ln_bwd(t[3:], ctx.beta, dy.contiguous().to(torch.bfloat16), G,
                                            dxsum_param=ctx.params[3], drop=ctx.drop)
        dx, dw1, db1, dw2, db2 = _ffn_bwd(t[:3], ctx.params, df, G, db2=db2, impl=ctx.impl, dres=dres)
        G.done()
        return dx, dw1, db1, dw2, db2, dg, db, None, None, None


def _bf16_grad(g):
    return None if g is None else g.contiguous().to(torch.bfloat16)


def _zero_grad_like(saved_norm):
    x = saved_norm[0]
    return torch.zeros_like(x)


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
            return dh, None, None, None
        G = _Grads()
        dx, dg, db, _, _ = _norm_bwd(ctx.saved_tensors, ctx.beta, _bf16_grad(dn), G, dres=_bf16_grad(dh))
        G.done()
        return dx, dg, db, None


class _PreAttentionBlock(torch.autograd.Function):
    """One pre-norm attention sub-layer as a node (h, n) -> (h', n'): h' = h + drop(Out(Attn(QKV(n)))) and
    n' = Norm(h') under the NEXT sub-layer's norm weights. Forward: the out-projection adds h in its epilogue
    and the norm kernel normalises (with ``drop``: the dropout_add norm kernel writes both h' and n').
    Backward of (dh', dn'): the norm backward with DRES = dh' gives the total stream gradient, which is the
    residual's gradient and the out-projection's dY (its masked copy DXM under dropout), with that linear's
    bias gradient as the fused column sums; the QKV dgrad then yields dn with nothing added."""

    @staticmethod
    def forward(ctx, h, n, wqkv, bqkv, wo, bo, gamma, beta, lens, B, S, H, eps, impl, drop=None, attn_drop=None,
                cu_seqlens=None, causal=False, rope=None):
        if drop is None:
            h2, s1 = _attn_fwd(n, wqkv, bqkv, wo, bo, lens, B, S, H, impl, attn_drop=attn_drop, cu_seqlens=cu_seqlens,
                               causal=causal, rope=rope, res=h)
            n2, s2 = _norm_fwd(h2, gamma, beta, eps)
        else:
            a, s1 = _attn_fwd(n, wqkv, bqkv, wo, bo, lens, B, S, H, impl, residual=False, attn_drop=attn_drop,
                              cu_seqlens=cu_seqlens, causal=causal, rope=rope)
            n2, s2 = _dropout_add_norm_fwd(a, h, gamma, beta, eps, drop)
            h2 = s2[0]
        ctx.save_for_backward(*s1, *s2)
        ctx.params, ctx.beta, ctx.impl = (wqkv, bqkv, wo, bo), beta, impl
        ctx.lens, ctx.dims, ctx.drop, ctx.attn_drop, ctx.cu = lens, (B, S, H), drop, attn_drop, cu_seqlens
        ctx.causal, ctx.rope = causal, rope
        ctx.set_materialize_grads(False)
        return h2, n2

    @staticmethod
    def backward(ctx, dh2, dn2):
        t = ctx.saved_tensors
        G = _Grads()
        dn2 = _zero_grad_like(t[4:]) if dn2 is None else _bf16_grad(dn2)
        dh, dg, db, dbo, dxm = _norm_bwd(t[4:], ctx.beta, dn2, G, dxsum_param=ctx.params[3], drop=ctx.drop,
                                         dres=_bf16_grad(dh2))
        da = dh if ctx.drop is None else dxm
        dn, dwqkv, dbqkv, dwo, dbo = _attn_bwd(t[:4], ctx.params, ctx.lens, *ctx.dims, da, G, dbo=dbo, impl=ctx.impl,
                                               attn_drop=ctx.attn_drop, cu_seqlens=ctx.cu, causal=ctx.causal,
                                               rope=ctx.rope, residual=False)
        G.done()
        return (dh, dn, dwqkv, dbqkv, dwo, dbo, dg, db) + (None,) * 11


class _PreFFNBlock(torch.autograd.Function):
    """The pre-norm FFN sub-layer (h, n) -> (h', n'), see _PreAttentionBlock."""

    @staticmethod
    def forward(ctx, h, n, w1, b1, w2, b2, gamma, beta, eps, impl, drop=None):
        if drop is None:
            h2, s1 = _ffn_fwd(n, w1, b1, w2, b2, impl, res=h)
            n2, s2 = _norm_fwd(h2, gamma, beta, eps)
        else:
            f, s1 = _ffn_fwd(n, w1, b1, w2, b2, impl, residual=False)
            n2, s2 = _dropout_add_norm_fwd(f, h, gamma, beta, eps, drop)
            h2 = s2[0]
        ctx.save_for_backward(*s1, *s2)
        ctx.params, ctx.beta, ctx.impl, ctx.drop = (w1, b1, w2, b2), beta, impl, drop
        ctx.set_materialize_grads(False)
        return h2, n2

    @staticmethod
    def backward(ctx, dh2, dn2):
        t = ctx.saved_tensors
        G = _Grads()
        dn2 = _zero_grad_like(t[3:]) if dn2 is None else _bf16_grad(dn2)
        dh, dg, db, db2, dxm = _norm_bwd(t[3:], ctx.beta, dn2, G, dxsum_param=ctx.params[3], drop=ctx.drop,
                                         dres=_bf16_grad(dh2))
        df = dh if ctx.drop is None else dxm
        dn, dw1, db1, dw2, db2 = _ffn_bwd(t[:3], ctx.params, df, G, db2=db2, impl=ctx.impl, residual=False)
        G.done()
        return (dh, dn, dw1, db1, dw2, db2, dg, db) + (None,) * 3


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
    _mark_training(impl)
    return _AttentionBlock.apply(x, wqkv, bqkv, wo, bo, lens, B, S, H, impl, attn_drop, cu_seqlens, causal, rope)


def ffn_block(x, w1, b1, w2, b2, impl=BF16):
    _mark_training(impl)
    return _FFNBlock.apply(x, w1, b1, w2, b2, impl)


def attention_ln_block(x, wqkv, bqkv, wo, bo, gamma, beta, lens: Optional[torch.Tensor], B: int, S: int, H: int,
                       eps: float, impl=BF16, drop=None, attn_drop=None, cu_seqlens: Optional[torch.Tensor] = None,
                       causal: bool = False, rope=None):
    """``drop`` = (p, seed, site, rank): hidden dropout on the out-projection's output, before the
    residual add, fused into the LayerNorm kernels (mask: ops/dropout.py). None: no dropout.
    ``attn_drop`` = (p, seed, site, rank): attention-probability dropout (see attention_block).
    ``cu_seqlens``: packed batch, with fewer than PACK_ROW_MULTIPLE tail rows (see attention_block);
    hidden-dropout masks are indexed by packed row. ``causal``, ``rope``: see attention_block."""
    _mark_training(impl)
    return _AttentionLNBlock.apply(x, wqkv, bqkv, wo, bo, gamma, beta, lens, B, S, H, eps, impl, drop, attn_drop,
                                   cu_seqlens, causal, rope)


def ffn_ln_block(x, w1, b1, w2, b2, gamma, beta, eps: float, impl=BF16, drop=None):
    """``drop`` = (p, seed, site, rank): hidden dropout on FFN2's output (see attention_ln_block)."""
    _mark_training(impl)
    return _FFNLNBlock.apply(x, w1, b1, w2, b2, gamma, beta, eps, impl, drop)


def layer_norm(x, gamma, beta, eps: float):
    return _LayerNorm.apply(x, gamma, beta, eps)


def _pre_norm_impl(impl):
    if impl is not BF16:
        raise ValueError("pre-norm blocks run the bf16 linears only")


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
    _pre_norm_impl(impl)
    return _PreAttentionBlock.apply(h, n, wqkv, bqkv, wo, bo, gamma, beta, lens, B, S, H, eps, impl, drop, attn_drop,
                                    cu_seqlens, causal, rope)


def pre_ffn_block(h, n, w1, b1, w2, b2, gamma, beta, eps: float, impl=BF16, drop=None):
    """The pre-norm FFN sub-layer: (h, n) -> (h + drop(FFN2(gelu(FFN1(n)))), Norm(that sum)); ``gamma`` / ``beta``
    belong to the next layer's ``ln1``, or to the final norm after the last layer."""
    _pre_norm_impl(impl)
    return _PreFFNBlock.apply(h, n, w1, b1, w2, b2, gamma, beta, eps, impl, drop)


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
