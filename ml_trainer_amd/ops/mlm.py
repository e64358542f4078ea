"""BERT's masked-language-model head over the native gfx950 kernels (csrc/kernels/mlm.hip).

``mlm_head`` computes the pre-training objective from the encoder's last hidden states and HF-style
``labels`` [B, S] (-100 = not a target): select the target positions -> gather their rows -> transform
(dense + GELU + LayerNorm) -> project onto the vocabulary with the word-embedding table (tied weights)
plus an output bias -> softmax cross-entropy, mean over the valid targets.

Static shapes, no device-to-host read: every sequence gets ``P`` slots (``max_predictions``), so the
head always runs on ``R = B * P`` rounded up to 256 rows; empty slots carry row -1 / label -100, are
gathered as zeros and ignored by the loss. Targets past the P-th of a sequence (or past its length)
are dropped and counted in a device ``overflow`` counter.

The vocabulary logits never exist beyond one chunk of rows. The fused decoder loops over chunks of
``chunk_rows`` rows: logits GEMM (+ bias) into one reusable bf16 ``[chunk_rows, Vp]`` buffer (``Vp`` = V
rounded up to 256, so the fast GEMM tiles run; the table and bias are read through cached zero-padded
copies, the parameters keep their shapes), ``vocab_ce`` in place (loss, log-sum-exp, hit per row, and
the unscaled gradient softmax - onehot over the logits), then -- when a backward will follow -- the
chunk's dgrad GEMM, its wgrad GEMM accumulated into an fp32 ``[Vp, h]`` temporary and its column sums.
The backward scales those small results by ``grad_out / max(n_valid, 1)`` (a device scalar).

Tied weights: the word table receives the decoder's weight gradient here (first in the backward) and
the embedding rows from ``embed_bwd`` (last). Only the embedding backward notifies the table's owner
(``FlatParams.notify_grad_ready``): a DDP bucket must not be reduced before both have landed.

The plain-torch functions (``select_reference``, ``gather_reference``, ``scatter_reference``,
``vocab_ce_reference``, ``mlm_head_reference``) define what the kernels compute; they are the CPU
path and the oracle of the tests.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

from ml_trainer_amd.ops._ext import require_native
from ml_trainer_amd.utils.flat import FlatParams

IGNORE_INDEX = -100
ROW_MULTIPLE = 256      # row tile of the fast GEMM kernels
VOCAB_MULTIPLE = 256    # column tile: the logits buffer and the padded table are this wide a multiple
# rows of logits alive at once (a [chunk_rows, Vp] bf16 buffer: 1.0 GB at a 30,720-wide vocabulary). Swept at
# the bench shape (122,880 rows, h 768, V 30522; head forward + backward, medians of 3, alternated):
# 2048 30.5 ms, 4096 32.0, 8192 27.8, 16384 26.3 (profiles/mlm/mlm_head_bench_r122880.jsonl).
DEFAULT_CHUNK_ROWS = 16384
# vocab_ce keeps rows of up to this many columns (62 KB of bf16) in LDS between the statistics and the
# gradient write, so the logits are read from memory once; wider rows are read a second time
# (kVocabCeResidentCols in csrc/include/mlt_kernels.h).
VOCAB_CE_RESIDENT_COLS = 31744


class MLMParams(NamedTuple):
    """The head's parameters: transform dense [h, h] + bias, transform LayerNorm, the word table
    [V, h] (tied decoder weight) and the output bias [V]."""
    dense_w: torch.Tensor
    dense_b: torch.Tensor
    ln_w: torch.Tensor
    ln_b: torch.Tensor
    word_w: torch.Tensor
    out_bias: torch.Tensor
    ln_eps: float = 1e-12


class MLMOutput(NamedTuple):
    loss: torch.Tensor        # mean over the valid targets (0 for an all-ignored batch), differentiable
    accuracy: torch.Tensor    # share of valid targets whose first arg-max is the label
    overflow: torch.Tensor    # int32: targets dropped (past the P-th of a sequence, or past its length)
    row_loss: torch.Tensor    # fp32 [R]: per-slot loss, 0 for empty slots


def default_max_predictions(seq_len: int, mask_prob: float = 0.15) -> int:
    """ceil(mask_prob * S) rounded up to 8: 80 at S = 512."""
    return -(-math.ceil(mask_prob * seq_len) // 8) * 8


def _round_up(x: int, m: int) -> int:
    return -(-x // m) * m


def slot_rows(B: int, P: int) -> int:
    """R: the head's static row count, B * P rounded up to the GEMM row tile."""
    return _round_up(B * P, ROW_MULTIPLE)


# ----------------------------------------------------------------------------- torch oracle
def select_reference(labels, P: int, lens=None, cu_seqlens=None, rows: Optional[int] = None):
    """(slot_row int32 [R], slot_label int64 [R], overflow int32 scalar): the targets of each sequence
    compacted in order into its P slots. slot_row = b * S + s, or cu_seqlens[b] + s when packed; empty
    slots -1 / -100. Targets past the P-th, or at s >= len_b (lens, or the lengths cu_seqlens implies),
    are dropped and counted. No host read."""
    B, S = labels.shape
    dev = labels.device
    R = slot_rows(B, P) if rows is None else rows
    target = labels != IGNORE_INDEX
    base = torch.arange(B, device=dev, dtype=torch.int64) * S
    valid = target
    if cu_seqlens is not None:
        cu = cu_seqlens.to(device=dev, dtype=torch.int64)
        base = cu[:-1]
        lens = cu[1:] - cu[:-1]
    if lens is not None:
        ln = lens.to(device=dev, dtype=torch.int64).clamp(max=S)
        valid = target & (torch.arange(S, device=dev)[None, :] < ln[:, None])
    rank = torch.cumsum(valid.to(torch.int64), 1) - 1
    keep = valid & (rank < P)
    overflow = (target.sum() - keep.sum()).to(torch.int32)
    dst = torch.where(keep, torch.arange(B, device=dev)[:, None] * P + rank, torch.full_like(rank, R)).view(-1)
    src = (base[:, None] + torch.arange(S, device=dev)[None, :]).view(-1)
    slot_row = torch.full((R + 1,), -1, dtype=torch.int64, device=dev).scatter_(0, dst, src)
    slot_label = torch.full((R + 1,), IGNORE_INDEX, dtype=torch.int64, device=dev).scatter_(0, dst, labels.reshape(-1))
    slot_row[R] = -1  # (the dump slot of everything not kept)
    return slot_row[:R].to(torch.int32), slot_label[:R].contiguous(), overflow


def gather_reference(x, slot_row):
    """out[r] = x[slot_row[r]], zeros for the empty slots."""
    idx = slot_row.to(torch.int64)
    out = x.index_select(0, idx.clamp(min=0))
    return out * (idx >= 0).to(out.dtype)[:, None]


def scatter_reference(g, slot_row, n_rows: int):
    """dx [n_rows, h]: zeros, then dx[slot_row[r]] = g[r] for the non-empty slots."""
    idx = slot_row.to(torch.int64)
    dx = g.new_zeros(n_rows + 1, g.shape[1])
    dx.index_copy_(0, torch.where(idx >= 0, idx, torch.full_like(idx, n_rows)), g)
    return dx[:n_rows]


def vocab_ce_reference(Z, V: int, labels, write_grad: bool = True, ignore_index: int = IGNORE_INDEX):
    """(row_loss, row_lse, row_hit, grad): what ``vocab_ce`` computes from Z [R, ldz] over its first V
    columns, in fp32 torch. grad (None without write_grad) is a new [R, ldz] tensor of Z's dtype:
    softmax - onehot, zeros at the padding columns and in ignored rows (label == ignore_index or
    outside [0, V))."""
    z = Z[:, :V].float()
    ok = (labels != ignore_index) & (labels >= 0) & (labels < V)
    t = labels.clamp(0, V - 1)
    lse = torch.logsumexp(z, 1)
    zt = z.gather(1, t[:, None])[:, 0]
    okf = ok.to(torch.float32)
    row_loss = torch.where(ok, lse - zt, torch.zeros_like(lse))
    row_lse = torch.where(ok, lse, torch.zeros_like(lse))
    row_hit = (z.argmax(1) == t).to(torch.float32) * okf  # torch's argmax returns the first maximum on ties
    grad = None
    if write_grad:
        g = torch.softmax(z, 1)
        g.scatter_add_(1, t[:, None], -torch.ones_like(zt)[:, None])
        grad = torch.zeros(Z.shape, dtype=Z.dtype, device=Z.device)
        grad[:, :V] = torch.where(ok[:, None], g, torch.zeros_like(g)).to(Z.dtype)
    return row_loss, row_lse, row_hit, grad


def transform_reference(x, p: MLMParams):
    """dense + GELU (erf) + LayerNorm in x's dtype."""
    a = F.gelu(F.linear(x, p.dense_w.to(x.dtype), p.dense_b.to(x.dtype)))
    return F.layer_norm(a, (a.shape[1],), p.ln_w.to(x.dtype), p.ln_b.to(x.dtype), p.ln_eps)


def mlm_head_reference(hidden, labels, P: int, params: MLMParams, cu_seqlens=None, lens=None) -> MLMOutput:
    """The head in plain differentiable fp32 torch (the CPU path and the numerics oracle)."""
    V = params.word_w.shape[0]
    slot_row, slot_label, overflow = select_reference(labels, P, lens, cu_seqlens)
    x = gather_reference(hidden.float(), slot_row)
    t = transform_reference(x, params)
    logits = F.linear(t, params.word_w.float(), params.out_bias.float())
    ok = (slot_label != IGNORE_INDEX) & (slot_label >= 0) & (slot_label < V)
    tgt = torch.where(ok, slot_label, torch.full_like(slot_label, IGNORE_INDEX))
    row_loss = F.cross_entropy(logits, tgt, ignore_index=IGNORE_INDEX, reduction="none")
    n = ok.sum().clamp(min=1).to(torch.float32)
    loss = row_loss.sum() / n
    hit = (logits.detach().argmax(1) == slot_label) & ok
    return MLMOutput(loss, hit.sum().to(torch.float32) / n, overflow, row_loss.detach())


# ----------------------------------------------------------------------------- native kernels
def select(labels, P: int, lens=None, cu_seqlens=None, rows: Optional[int] = None):
    """``select_reference`` on the ``mlm_select`` kernel (labels on the GPU)."""
    C = require_native()
    B, S = labels.shape
    R = slot_rows(B, P) if rows is None else rows
    dev = labels.device
    labels = labels.contiguous().to(torch.int64)
    slot_row = torch.empty(R, dtype=torch.int32, device=dev)
    slot_label = torch.empty(R, dtype=torch.int64, device=dev)
    seq_overflow = torch.empty(B, dtype=torch.int32, device=dev)
    overflow = torch.empty((), dtype=torch.int32, device=dev)
    if cu_seqlens is not None:
        lens = None
        cu_seqlens = cu_seqlens.to(torch.int32).contiguous()
    elif lens is not None:
        lens = lens.to(device=dev, dtype=torch.int32).contiguous()
    C.mlm_select(labels, P, slot_row, slot_label, seq_overflow, overflow.view(1), lens=lens, cu_seqlens=cu_seqlens)
    return slot_row, slot_label, overflow


def gather_rows(x, slot_row):
    out = torch.empty(slot_row.numel(), x.shape[1], dtype=torch.bfloat16, device=x.device)
    require_native().gather_rows(x, slot_row, out)
    return out


def scatter_rows(g, slot_row, n_rows: int):
    dx = torch.empty(n_rows, g.shape[1], dtype=torch.bfloat16, device=g.device)
    require_native().scatter_rows(g, slot_row, dx)
    return dx


def vocab_ce(Z, V: int, labels, write_grad: bool = True):
    """(row_loss, row_lse, row_hit) of bf16 logits Z [R, ldz]; with ``write_grad`` Z becomes the
    unscaled gradient in place."""
    R = Z.shape[0]
    out = torch.empty(3, R, dtype=torch.float32, device=Z.device)
    require_native().vocab_ce(Z, V, labels, out[0], out[1], out[2], write_grad)
    return out[0], out[1], out[2]


def _cache_key(p):
    fp = FlatParams.owner(p)
    # generation: optimizer updates; the version counters: load_state_dict / manual edits of the masters
    return ((fp.generation, fp.data._version, p._version) if fp is not None else p._version, p.data_ptr())


def padded_decoder(word_w, out_bias):
    """(table bf16 [Vp, h], bias fp32 [Vp]): zero-padded compute copies of the word table's bf16 shadow
    and of the output bias, re-made once per optimizer update (keyed as ``bf16_weight_t``). The
    parameters and their checkpoints keep the true vocabulary size."""
    V, h = word_w.shape
    Vp = _round_up(V, VOCAB_MULTIPLE)
    key = _cache_key(word_w)
    cache = getattr(word_w, "_mlt_mlm_table", None)
    if cache is None or cache[0] != key:
        w = cache[1] if cache is not None else torch.zeros(Vp, h, dtype=torch.bfloat16, device=word_w.device)
        fp = FlatParams.owner(word_w)
        # the flat buffer's bf16 shadow, or the same round-to-nearest cast straight from the master
        w[:V].copy_(fp.shadow_view(word_w) if fp is not None and fp.device.type == "cuda" else word_w.detach())
        word_w._mlt_mlm_table = cache = (key, w)
    keyb = _cache_key(out_bias)
    cb = getattr(out_bias, "_mlt_mlm_bias", None)
    if cb is None or cb[0] != keyb:
        b = cb[1] if cb is not None else torch.zeros(Vp, dtype=torch.float32, device=out_bias.device)
        b[:V].copy_(out_bias.detach())
        out_bias._mlt_mlm_bias = cb = (keyb, b)
    return cache[1], cb[1]


def _transform_fwd(x, p: MLMParams):
    """x [R, h] bf16 -> (t, pre, a, ln_saved): dense GEMM with the GELU epilogue, LayerNorm kernel."""
    from ml_trainer_amd.ops import transformer as T
    pre = torch.empty_like(x)
    a = T.linear_fwd(x, T.bf16_weight(p.dense_w), p.dense_b, gelu_aux=pre)
    t, ln_saved = T._ln_fwd(a, p.ln_w, p.ln_b, p.ln_eps)
    return t, pre, ln_saved


def _dgelu(da, pre):
    """da * gelu'(pre) (erf GELU) in fp32 torch, bf16 out: it sits between the LayerNorm backward and
    the dense layer's own GEMMs, so no GEMM epilogue can take it."""
    x = pre.float()
    d = 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0)))) + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))
    return (da.float() * d).to(torch.bfloat16)


class _MLMHead(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hidden, dense_w, dense_b, ln_w, ln_b, word_w, out_bias, slot_row, slot_label, eps, chunk_rows,
                need_grad):
        C = require_native()
        p = MLMParams(dense_w, dense_b, ln_w, ln_b, word_w, out_bias, eps)
        V, h = word_w.shape
        R = slot_row.numel()
        dev = hidden.device
        wp, bp = padded_decoder(word_w, out_bias)
        Vp = wp.shape[0]
        x = gather_rows(hidden, slot_row)
        t, pre, ln_saved = _transform_fwd(x, p)
        stats = torch.empty(3, R, dtype=torch.float32, device=dev)
        chunk = max(ROW_MULTIPLE, min(_round_up(chunk_rows, ROW_MULTIPLE), R))
        Z = torch.empty(chunk, Vp, dtype=torch.bfloat16, device=dev)
        if need_grad:
            dt = torch.empty(R, h, dtype=torch.bfloat16, device=dev)
            dw = torch.empty(Vp, h, dtype=torch.float32, device=dev)
            db = torch.empty(Vp, dtype=torch.float32, device=dev)
        for r0 in range(0, R, chunk):
            r1 = min(r0 + chunk, R)
            Zc, tc = Z[:r1 - r0], t[r0:r1]
            C.gemm(tc, wp, Zc, False, False, bias=bp)
            C.vocab_ce(Zc, V, slot_label[r0:r1], stats[0, r0:r1], stats[1, r0:r1], stats[2, r0:r1], need_grad)
            if need_grad:  # Zc now holds softmax - onehot (unscaled)
                C.gemm(Zc, wp, dt[r0:r1], False, True)
                C.gemm(Zc, tc, dw, True, True, accumulate=r0 > 0)
                C.colsum(Zc, db, r0 > 0)
        del Z
        ok = (slot_label != IGNORE_INDEX) & (slot_label >= 0) & (slot_label < V)
        n = ok.sum().clamp(min=1).to(torch.float32)
        loss = stats[0].sum() / n
        acc = stats[2].sum() / n
        row_loss = stats[0].clone()
        if need_grad:
            ctx.save_for_backward(x, pre, *ln_saved, dt, dw, db, slot_row, n)
            ctx.params = p
            ctx.n_rows = hidden.shape[0]
            ctx.spent = False
        ctx.mark_non_differentiable(acc, row_loss)
        return loss, acc, row_loss

    @staticmethod
    def backward(ctx, gloss, _gacc, _grow):
        from ml_trainer_amd.ops import transformer as T
        x, pre, a, gamma, mean, rstd, dt, dw, db, slot_row, n = ctx.saved_tensors
        p = ctx.params
        V = p.word_w.shape[0]
        if ctx.spent:
            raise RuntimeError("the MLM head's backward ran already: its unscaled decoder gradients are scaled in "
                               "place (no second [V, h] buffer), so it cannot run a second time")
        ctx.spent = True
        scale = (gloss.float() / n).reshape(())  # device scalar: no sync
        G = T._Grads()
        # tied table: accumulate, but leave the notification to the embedding backward (see module docstring)
        fp = FlatParams.owner(p.word_w)
        sink = fp.grad_sink(p.word_w) if fp is not None else None
        if sink is not None:
            sink.addcmul_(dw[:V], scale)
            gw = None
        else:
            gw = dw.mul_(scale)[:V]
        sb = G.sink(p.out_bias)
        if sb is not None:
            sb.addcmul_(db[:V], scale)
            gb = None
        else:
            gb = db.mul_(scale)[:V]
        dts = (dt.float() * scale).to(torch.bfloat16)
        da, dg, dbeta, _ = T._ln_bwd((a, gamma, mean, rstd), p.ln_b, dts, G)
        dpre = _dgelu(da, pre)
        dwd, dbd = G.wgrad_bias(p.dense_w, p.dense_b, dpre, x)
        dx = T.BF16.dgrad(dpre, p.dense_w, torch.empty_like(x))
        dh = scatter_rows(dx, slot_row, ctx.n_rows)
        G.done()
        return dh, dwd, dbd, dg, dbeta, gw, gb, None, None, None, None, None


def mlm_head(hidden, labels, P: int, params: MLMParams, cu_seqlens=None, chunk_rows: int = DEFAULT_CHUNK_ROWS,
             lens=None) -> MLMOutput:
    """The masked-LM objective of ``hidden`` [N, h] (bf16 on the GPU: the encoder's last hidden states,
    row b * S + s, or the packed rows with ``cu_seqlens``) for ``labels`` [B, S]; one autograd node.
    ``P`` slots per sequence; ``lens`` [B] drops targets at s >= len_b. On the CPU (or for an fp32
    ``hidden``) the plain-torch reference runs."""
    if not hidden.is_cuda:
        return mlm_head_reference(hidden, labels, P, params, cu_seqlens, lens)
    h = hidden.shape[1]
    if hidden.dtype != torch.bfloat16 or h % 256 or not 256 <= h <= 1024:
        raise ValueError("the native MLM head takes bf16 hidden states of width 256 / 512 / 768 / 1024")
    labels = labels.to(hidden.device)
    slot_row, slot_label, overflow = select(labels, P, lens, cu_seqlens)
    need_grad = torch.is_grad_enabled() and (hidden.requires_grad or any(
        isinstance(t, torch.Tensor) and t.requires_grad for t in params))
    loss, acc, row_loss = _MLMHead.apply(hidden.contiguous(), params.dense_w, params.dense_b, params.ln_w,
                                         params.ln_b, params.word_w, params.out_bias, slot_row, slot_label,
                                         params.ln_eps, chunk_rows, need_grad)
    return MLMOutput(loss, acc, overflow, row_loss)


def mlm_logits(hidden, rows, params: MLMParams):
    """fp32 [len(rows), V]: the vocabulary logits of the given hidden rows (inspection and tests).
    bf16 hidden states on the GPU go through the same kernels as ``mlm_head`` (row count padded to the
    GEMM tile); anything else through plain fp32 torch."""
    rows = torch.as_tensor(rows, dtype=torch.int64, device=hidden.device).view(-1)
    V = params.word_w.shape[0]
    if not hidden.is_cuda or hidden.dtype != torch.bfloat16:  # CPU, or the fp32 reference's hidden states
        t = transform_reference(hidden.float().index_select(0, rows), params)
        return F.linear(t, params.word_w.float(), params.out_bias.float())
    C = require_native()
    n = rows.numel()
    slot_row = torch.full((_round_up(max(n, 1), ROW_MULTIPLE),), -1, dtype=torch.int32, device=hidden.device)
    slot_row[:n] = rows.to(torch.int32)
    with torch.no_grad():
        wp, bp = padded_decoder(params.word_w, params.out_bias)
        t, _, _ = _transform_fwd(gather_rows(hidden.contiguous(), slot_row), params)
        out = torch.empty(slot_row.numel(), wp.shape[0], dtype=torch.float32, device=hidden.device)
        C.gemm(t, wp, out, False, False, bias=bp)
    return out[:n, :V]


def decode_logits(hidden, params: MLMParams):
    """fp32 [B, V]: the vocabulary logits of every row of ``hidden`` [B, h] (bf16, on the GPU), for the few rows
    of a decode step: the transform's dense + GELU and the tied decoder through ``ops.decode.linear_small`` (the
    weight-streaming kernel where ``decode_linear_path`` says so), the LayerNorm kernel of ``_transform_fwd``
    between them. B rows in, B rows out: no gather into a 256-row tile, no [256, Vp] logits matrix."""
    from ml_trainer_amd.ops import decode as DC
    from ml_trainer_amd.ops import transformer as T
    V = params.word_w.shape[0]
    with torch.no_grad():
        wp, bp = padded_decoder(params.word_w, params.out_bias)
        x = hidden.contiguous()
        pre = torch.empty_like(x)
        a = DC.linear_small(x, T.bf16_weight(params.dense_w), params.dense_b, gelu_aux=pre)
        t, _ = T._ln_fwd(a, params.ln_w, params.ln_b, params.ln_eps)
        out = torch.empty(x.shape[0], wp.shape[0], dtype=torch.float32, device=x.device)
        DC.linear_small(t, wp, bp, out=out)
    return out[:, :V]
