"""BERT encoder classifier -- BASELINE.json config 4 ("BERT-base classifier via
src/model.py, seq_len=512 bf16 DDP=8") and config 5 ("large config fp8").

Not part of the reference (its only model is the LeNet of src/model.py); the
model-config decision is recorded in SURVEY.md §7.1 and the README:

* ``bert-base``  12 layers, hidden 768, 12 heads, FFN 3072, vocab 30522, 512 positions
* ``large``      24 layers, hidden 1024, 16 heads, FFN 4096 (fp8 GEMMs, ops/fp8.py)
* ``bert-tiny``  2 layers, hidden 256, 4 heads, FFN 1024 (tests / CPU plumbing)

Post-LN BERT: embeddings(word+pos+type) -> LN -> N x [attention block -> LN -> FFN
block -> LN] -> pooler tanh(W h_CLS) -> classifier. On the GPU every heavy op runs
on the native kernels (ops/transformer.py: MFMA GEMMs with fused epilogues,
flash attention, LayerNorm, embedding gather/scatter, and the classifier head: pooler
GEMM with a tanh epilogue + the num_labels-wide classifier layer of head.hip) with fp32
master weights and bf16 activations. On CPU the
same math runs in plain torch (and serves as the numerics oracle in tests).

Hidden dropout (``BertConfig.hidden_dropout``, default 0: the benchmark measures the compute
path) is BERT's standard one: on the embedding output after its LayerNorm, and on the output of
the attention out-projection and of FFN2 before the residual add. It is active in ``train()``
mode only. On the GPU it runs inside the LayerNorm kernels (plus one small kernel for the
embedding site); the mask is a counter-based Philox stream recomputed in the backward, so nothing
is stored. One 62-bit seed per forward comes from torch's default CPU generator (no device sync,
reproducible under ``torch.manual_seed``, saved and restored with the trainer's RNG state) or from
``dropout_seed=``; ``ops/dropout.py`` defines the mask and the site numbering, and the torch paths
here apply the same masks.

Attention-probability dropout (``BertConfig.attention_dropout``, default 0) drops softmax
probabilities inside the flash attention kernels (forward, dQ, dK/dV): the S x S matrix is still
never materialised and the mask is recomputed, never stored. It spends one random byte per
probability, so the probability applied is ``p_eff = round(p * 256) / 256`` (0.1 -> 26/256 =
0.1015625) and kept probabilities are scaled by ``1 / (1 - p_eff)``. It shares the forward's one
seed with hidden dropout (sites ``0x40000000 + layer``) and is active in ``train()`` mode only.
Not covered: the LeNet models (the reference model has no dropout).

Unpadded execution (``BertConfig.unpad``, default False) drops the pad tokens of a right-padded
``[B, S]`` batch once, before the embeddings, and runs the whole encoder on the ``T = sum(len_b)`` real
tokens as one ``[T, hidden]`` matrix (``ops.transformer.pack_batch``). GEMMs, LayerNorm, GELU and
hidden dropout are row-count agnostic. The native path rounds the row count up to the GEMMs' 256-row
tile with inert tail rows that belong to no sequence and get zero gradients. The flash attention
kernels find sequence ``b`` at rows ``cu_seqlens[b] .. cu_seqlens[b + 1]`` (their packed
instantiations) and the embedding kernels take
explicit positions (the index inside the token's own sequence). The CLS rows are ``cu_seqlens[:-1]``,
so the logits equal the padded model's: pads never reach the CLS loss. It needs lengths
(``attention_mask`` or ``pad_id``; without them the padded path runs unchanged) and assumes right
padding, as ``_lengths`` does. Packing needs ``T`` on the host to size the packed tensors: one small
device-to-host read per forward. Attention-probability dropout draws the bytes of the padded run
(element ``(b, h, q, k)`` is indexed with the padded width ``S``); hidden dropout is indexed by packed
row, so its masks differ from a padded run's with the same seed. ``unpad`` with ``fp8`` is rejected: the
fp8 attention epilogue writes 16-row transposed runs at ``b * S`` offsets.

Masked-LM pre-training: ``BertForMaskedLM`` is the same encoder (same state-dict keys) without the pooler
and classifier, under the MLM head of ``ops/mlm.py`` (transform dense + GELU + LayerNorm, vocabulary
projection tied to the word table, fused chunked softmax cross-entropy). Hidden dropout, attention
dropout and ``unpad`` work unchanged; fp8 is rejected.

Causal attention (``BertConfig.causal``, default False): key ``j`` of a sequence is visible to query ``i``
of the same sequence iff ``j <= i`` and ``j < len_b``, inside the flash attention kernels (their causal
instantiations skip the key blocks above the diagonal; no S x S mask exists anywhere). It composes with
hidden dropout, attention dropout and ``unpad``; with ``fp8`` it is rejected. ``BertLMHeadModel`` is the
encoder run as a next-token decoder (post-LN, learned positions -- or rotary ones, below --, tied word table:
GPT-1's block) under
the MLM prediction head with one slot per position.

Incremental decoding (``BertLMHeadModel`` only; the bidirectional models have no use for a key/value cache):
``prefill(input_ids, attention_mask)`` runs the padded causal forward once, keeps every layer's K / V in a
head-major cache (``ops.decode.KVCache``: ``[2, B, H, Smax, 64]`` per layer) and returns a ``DecodeState``;
``decode_step(state, token_ids)`` runs one token per sequence through the stack (per layer QKV GEMM, the
``attn_decode`` kernel over the cache with the append fused in, out-projection + residual, LayerNorm, FFN,
LayerNorm) and returns fp32 logits; ``generate`` loops it with greedy, temperature / top-k sampling and an EOS
mask. The position of every sequence lives on the device (ragged prompts continue at their own length) and no
step reads anything back. Over a cache of ``ops.decode.DECODE_SPLIT_MIN_SMAX`` rows or more the attention of a step is
``C.attn_decode_split`` (the cached keys of a head split over workgroups, then a merge launch:
``ops.decode.decode_attn_path``; ``MLT_DECODE_SPLIT=0`` keeps the single kernel). On the CPU the same runs in fp32
torch with an fp32 cache;
``generate_reference`` / ``decode_logits_reference`` are the uncached oracle. Opt-in: ``sampler="device"`` (the
``sample_step`` kernel of ``ops.decode``: top-k / top-p and the EOS bookkeeping in one launch, integer-defined,
independent of the batch), ``top_p``, and ``graph=True`` (``GraphedDecoder``: one captured graph of ``decode_step`` +
``sample_step`` replayed per token). Not built: paged caches, beam search, repetition penalties,
``return_logits`` under a graph, a graph for ``prefill``.

Rotary positions (``BertConfig.rotary``, default False; ``rope_base``): instead of a learned position table added at
the embedding, queries and keys are rotated by an angle proportional to their position (``ops/rope.py`` has the
definition: interleaved pairs, an fp32 cos / sin table of ``max_position`` rows built once on the host, uncontracted
fp32 arithmetic, bf16 results), so attention scores depend on ``i - j`` only. The model then has no
``position_embeddings`` module and no such state-dict key; the table is a non-persistent buffer ``rope_table``. On the
GPU the ``rope_qk`` kernel rotates the q and k columns of the QKV buffer in place between the QKV GEMM and the flash
attention kernel and rotates dQKV back in the backward; the key/value cache holds rotated keys and the ROPE
instantiation of ``attn_decode`` rotates the one new row per sequence. ``max_position`` only sizes the table: it may
exceed every length seen in training, which is the point (a model trained at 32 tokens can be run past them). It
composes with ``causal``, ``unpad`` and both dropouts and with all three model classes; with ``fp8`` it is rejected.

Pre-norm blocks (``BertConfig.pre_ln``, default False) and RMSNorm (``BertConfig.norm = "rmsnorm"``, default
``"layernorm"``; needs ``pre_ln``): the layer keeps its module names and becomes
``n = ln1(h); h = h + drop(out(attn(qkv(n)))); n = ln2(h); h = h + drop(ffn2(gelu(ffn1(n))))`` (the hidden-dropout
sites of the post-LN layer), and one more norm of the same kind, ``final_ln``, follows the last layer: its output is
what the pooler, the MLM head and the LM head consume. ``norm`` selects the kind of ``ln1``, ``ln2`` and ``final_ln``
only; ``emb_ln`` and the MLM head's ``mlm_ln`` stay LayerNorm. RMSNorm is ``x * rsqrt(mean(x^2) + ln_eps) * weight``
with fp32 statistics, no centring and no bias (no ``.bias`` keys). On the GPU a sub-layer is one autograd node
``(h, n) -> (h', n')`` (``ops.transformer.pre_attention_block`` / ``pre_ffn_block``): the residual stream ``h`` is
stored in bf16 after every add, the norm of the new stream comes from the kernel that closes the sub-layer, and the
norm backward adds the stream's gradient in the kernel. The key/value cache and ``attn_decode`` are unchanged
(``prefill`` caches the QKV of ``n``); ``decode_step`` keeps the normed rows in ``state.hidden``. Composes with
``causal``, ``unpad``, ``rotary``, both dropouts and all three model classes; with ``fp8`` it is rejected. Not built:
post-norm RMSNorm, RMSNorm for ``emb_ln`` / ``mlm_ln``, the norm fused into a GEMM prologue.

Grouped-query attention (``BertConfig.kv_heads``, default None = ``heads``): ``Hkv = kv_heads`` key/value heads, each
shared by the ``G = heads / Hkv`` query heads ``hkv * G .. hkv * G + G - 1`` (query head h reads KV head ``h // G``);
``kv_heads`` must divide ``heads``. With ``kv_heads < heads`` ``layers.N.qkv`` is ``nn.Linear(h, (H + 2 Hkv) * 64)``
with the compact column layout q (H heads) | k (Hkv) | v (Hkv) (ops/gqa.py); no other parameter changes, and with
``kv_heads`` None or ``heads`` nothing changes at all. Training and prefill expand the compact rows to the wide
layout in front of the unchanged rotation and flash attention kernels (``C.gqa_expand``) and reduce the wide dQKV
behind them (``C.gqa_reduce``); the key/value cache is ``[2, B, Hkv, Smax, 64]`` and a decode step's attention is
``C.attn_decode_gqa``, which streams every cached row once for its whole group. Composes with ``rotary``, ``pre_ln`` /
``rmsnorm``, ``unpad`` and both dropouts; with ``fp8`` it is rejected. Not built: ``h // G`` indexing inside the
flash kernels, the rotation fused into expand / reduce, paged caches.

SwiGLU feed-forward (``BertConfig.ffn = "swiglu"``, default ``"gelu"``): ``layers.N.ffn1`` becomes
``nn.Linear(h, 2 * intermediate)`` whose output columns ``[0, F)`` are the gate ``g`` and ``[F, 2F)`` the up-projection
``u`` (``F = intermediate``), the block computes ``ffn2(bf16((g * s) * u))`` with ``s = 1 / (1 + exp(-g))`` (ops/swiglu.py
has the definition, its gradient and the rounding points), and no other parameter changes; with ``"gelu"`` nothing
changes at all. Training and prefill run FFN1 with the plain bias epilogue, then the streaming kernel ``C.swiglu_fwd``;
the backward's ``C.swiglu_bwd`` writes dg | du and FFN1's bias gradient in one pass. A decode step runs FFN1 and the
gate as ONE launch, ``C.gemm_skinny_glu`` (two weight streams of the one [2F, h] weight, the activation in the
epilogue), bit for bit the unfused pair (``MLT_DECODE_GLU=0``). Parameter parity with a GELU FFN of width 4h needs
``intermediate = 8h / 3`` (2048 for ``bert-base``). Composes with ``rotary``, ``pre_ln`` / ``rmsnorm``, ``kv_heads``,
``unpad`` and both dropouts and with all three model classes; with ``fp8`` it is rejected. Not built: the gate fused
into the FFN1 tile-GEMM epilogue (interleaved gate / up weight rows), GeGLU / ReGLU, recomputing ``a`` in the backward.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from ml_trainer_amd.ops.transformer import AttnSpec, _norm_fwd


@dataclass
class BertConfig:
    vocab_size: int = 30522
    hidden: int = 768
    layers: int = 12
    heads: int = 12
    intermediate: int = 3072
    max_position: int = 512
    type_vocab: int = 2
    num_labels: int = 2
    ln_eps: float = 1e-12
    init_std: float = 0.02
    fp8: bool = False
    hidden_dropout: float = 0.0  # embedding / attention-output / FFN-output dropout (train() only)
    attention_dropout: float = 0.0  # attention-probability dropout, applied as round(p * 256) / 256
    pad_id: Optional[int] = None  # when set, key lengths are derived from trailing pad tokens
    unpad: bool = False  # run the encoder on the real tokens only (needs lengths; not with fp8)
    max_predictions: Optional[int] = None  # MLM slots per sequence; None: ceil(0.15 * S) rounded up to 8
    causal: bool = False  # key j visible to query i iff j <= i (and j < len_b); not with fp8
    rotary: bool = False  # rotary positions on q and k instead of a learned position table; not with fp8
    rope_base: float = 10000.0  # the angle of position p, pair i is p * rope_base ** (-2 i / 64)
    pre_ln: bool = False  # pre-norm blocks h + f(norm(h)) and a final norm (final_ln); not with fp8
    norm: str = "layernorm"  # the kind of ln1 / ln2 / final_ln: "layernorm", or "rmsnorm" (needs pre_ln)
    kv_heads: Optional[int] = None  # grouped-query attention: key/value heads (a divisor of heads); None = heads
    ffn: str = "gelu"  # the feed-forward: "gelu", or "swiglu" (ffn1 is [2 * intermediate, hidden]); not with fp8

    @property
    def num_kv_heads(self) -> int:
        return self.heads if self.kv_heads is None else self.kv_heads


_PRESETS = {
    "bert-base": BertConfig(),
    "bert": BertConfig(),
    "bert_base": BertConfig(),
    "large": BertConfig(hidden=1024, layers=24, heads=16, intermediate=4096, fp8=True),
    "bert-large": BertConfig(hidden=1024, layers=24, heads=16, intermediate=4096),
    "bert-tiny": BertConfig(vocab_size=1000, hidden=256, layers=2, heads=4, intermediate=1024, max_position=128),
}


def bert_config(name: str = "bert-base", **overrides) -> BertConfig:
    cfg = _PRESETS[name.lower()]
    return replace(cfg, **overrides) if overrides else cfg


class RMSNorm(nn.Module):
    """``x * rsqrt(mean(x^2, -1) + eps) * weight``: no centring, no bias. Computed in fp32, returned in the
    dtype of ``x``."""

    def __init__(self, hidden: int, eps: float):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden))
        self.register_parameter("bias", None)
        self.eps = eps

    def forward(self, x):
        xf = x.float()
        return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.eps) * self.weight.float()).to(x.dtype)


def block_norm(c: BertConfig) -> nn.Module:
    """A norm of the kind ``c.norm`` selects for ``ln1`` / ``ln2`` / ``final_ln``."""
    return RMSNorm(c.hidden, c.ln_eps) if c.norm == "rmsnorm" else nn.LayerNorm(c.hidden, eps=c.ln_eps)


def _norm_args(m):
    """(gamma, beta or None, eps) of a LayerNorm / RMSNorm module for the native norm kernels."""
    return m.weight, m.bias, m.eps


def _norm_native(x, m):
    """The norm module ``m`` of bf16 rows ``x`` on its native forward kernel, nothing kept for a backward."""
    return _norm_fwd(x, m.weight, m.bias, m.eps)[0]


def _fp8_exclusions(c: BertConfig):
    """(the switch is on, the refusal) for everything that runs the bf16 linears only."""
    return (
        (c.unpad, "unpad=True with fp8=True is not supported: the fp8 attention epilogue writes 16-row transposed "
                  "runs at b * S offsets and cannot take packed row offsets"),
        (c.causal, "causal=True with fp8=True is not supported: the fp8 (q8) attention epilogue has no causal "
                   "instantiation"),
        (c.rotary, "rotary=True with fp8=True is not supported: the fp8 attention backward writes dQKV as e5m2, "
                   "which the inverse rotation cannot take"),
        (c.pre_ln or c.norm != "layernorm", "pre_ln=True / norm='rmsnorm' with fp8=True is not supported: the "
                                            "pre-norm blocks run the bf16 linears only"),
        (c.ffn == "swiglu", "ffn='swiglu' with fp8=True is not supported: the fp8 FFN fusions are GELU epilogues"),
        (c.num_kv_heads != c.heads, "kv_heads < heads with fp8=True is not supported: the fp8 attention backward "
                                    "writes dQKV as e5m2 in the wide layout, which the group reduction cannot take"),
    )


def _sites(l: int):
    """The dropout sites of layer ``l`` (ops/dropout.py): hidden dropout of its attention and of its FFN sub-layer,
    and its attention probabilities. Site 0 is the embedding output."""
    from ml_trainer_amd.ops.dropout import attention_site
    return 1 + 2 * l, 2 + 2 * l, attention_site(l)


@dataclass
class _Batch:
    """What the encoder needs to know of its input, padded or packed. Padded: ``ids`` / ``tt`` (or None) [B, S],
    ``pos`` and ``cu`` None, rows are b * S + s. Packed (``packed``, the ``PackedBatch``): ``ids`` / ``tt`` / ``pos``
    [rows], ``cu`` = cu_seqlens, ``S`` = max_seqlen. ``lens`` [B] or None either way."""
    ids: torch.Tensor
    tt: Optional[torch.Tensor]
    lens: Optional[torch.Tensor]
    B: int
    S: int
    pos: Optional[torch.Tensor] = None
    cu: Optional[torch.Tensor] = None
    packed: object = None

    @classmethod
    def of(cls, input_ids, lens, token_type_ids, pk=None):
        B, S = input_ids.shape
        if pk is None:
            return cls(input_ids, token_type_ids, lens, B, S)
        return cls(pk.ids, pk.tt, lens, B, S, pk.pos, pk.cu_seqlens, pk)

    def attn_spec(self, c: BertConfig, rope_table, attn_drop=None):
        """The ``AttnSpec`` of a layer of the model ``c`` on this batch (a packed batch has no use for ``lens``)."""
        return AttnSpec(self.B, self.S, c.heads, self.lens if self.cu is None else None, self.cu, c.causal,
                        (rope_table, self.pos) if c.rotary else None, attn_drop, c.kv_heads)

    def key_mask(self, device):
        """[B, S] bool, True = a real key; None without lengths."""
        if self.lens is None:
            return None
        lens = self.lens.to(device)
        if self.packed is not None:
            lens = lens.clamp(1, self.S)
        return torch.arange(self.S, device=device)[None, :] < lens[:, None]

    def cls_rows(self, x):
        """The CLS rows [B, h] of hidden states ``x`` [rows, h]; for a padded batch a strided view."""
        return x.view(self.B, self.S, -1)[:, 0] if self.packed is None else x.index_select(0, self.packed.cls_rows)

    def last_batch(self):
        """(B, S, lens, cu_seqlens) as the MLM head takes them: ``lens`` only without ``cu_seqlens``."""
        return self.B, self.S, self.lens if self.cu is None else None, self.cu


class BertLayer(nn.Module):
    def __init__(self, c: BertConfig):
        super().__init__()
        h = c.hidden
        self.c = c
        self.qkv = nn.Linear(h, h + 2 * c.num_kv_heads * (h // c.heads))  # 3 h, or compact under kv_heads
        self.out = nn.Linear(h, h)
        self.ln1 = block_norm(c)
        self.ffn1 = nn.Linear(h, (2 if c.ffn == "swiglu" else 1) * c.intermediate)  # swiglu: gate rows | up rows
        self.ffn2 = nn.Linear(c.intermediate, h)
        self.ln2 = block_norm(c)

    def attn_params(self):
        return self.qkv.weight, self.qkv.bias, self.out.weight, self.out.bias

    def ffn_params(self):
        return self.ffn1.weight, self.ffn1.bias, self.ffn2.weight, self.ffn2.bias

    def forward_native(self, x, n, spec, closing, drops=(None, None)):
        """The layer on the native kernels, attention then FFN sub-layer, each one block node of
        ``ops.transformer``. Post-LN: ``x -> closing(core(x) + x)``, ``n`` is None and stays so. Pre-norm: ``x`` is
        the residual stream and ``n`` its norm, ``(x, n) -> (x + core(n), closing(that sum))``. ``closing``: the two
        norm modules that close the sub-layers: the layer's own ``(ln1, ln2)`` for post-LN; ``ln2`` and the next
        layer's ``ln1`` (the model's ``final_ln`` after the last layer) for pre-norm. ``spec``: the layer's
        ``AttnSpec``. ``drops``: hidden dropout (p, seed, site, rank) of the two sub-layers. Returns ``(x, n)``."""
        from ml_trainer_amd.ops import transformer as T
        if self.c.fp8:
            from ml_trainer_amd.ops.fp8 import FP8 as impl
        else:
            impl = T.BF16
        cores = ((T.attn_core(spec, impl), self.attn_params()), (T.ffn_core(self.c.ffn, impl), self.ffn_params()))
        for (core, params), norm, drop in zip(cores, closing, drops):
            if self.c.pre_ln:
                x, n = T.pre_norm_block(core, x, n, params, _norm_args(norm), drop)
            else:
                x = T.post_norm_block(core, x, params, _norm_args(norm), drop)
        return x, n

    def ffn_torch(self, x, round_bf16=False, lin=None):
        """``ffn2(act(ffn1(x)))`` in plain torch: GELU, or the SwiGLU of ops/swiglu.py on ffn1's gate | up columns.
        ``round_bf16`` (the eager bf16 baseline): h1 and a rounded to bf16, as the native path stores them.
        ``lin(module, x)`` (default: call the module) applies the two linears: the decode steps on fp8 weights."""
        if lin is None:
            lin = lambda m, v: m(v)
        h1 = lin(self.ffn1, x)
        if self.c.ffn != "swiglu":
            return lin(self.ffn2, F.gelu(h1))
        from ml_trainer_amd.ops.swiglu import swiglu
        return lin(self.ffn2, swiglu(h1.to(torch.bfloat16) if round_bf16 else h1))

    def forward_reference(self, x, mask, B, S, drop=None, attn_drop=None, packed=None, rope=None):
        """fp32 torch reference. x [B*S, h]; mask [B, S] bool (True = valid key); drop and attn_drop
        as in forward_native (the same masks, through ops.dropout). ``packed`` (a PackedBatch): x is
        [T, h]; the linears, LayerNorms and hidden dropout run on the packed rows, attention on a
        padded scratch of the QKV rows (so its dropout mask is the padded run's). With ``config.causal``
        the lower-triangular mask (key <= query) joins the key mask. ``rope`` (the table): q and k are rotated in
        the dtype of the activations (fp32) at position = column of the padded layout. With ``config.pre_ln``
        x is the residual stream and so is the result (the model applies ``final_ln`` after the last layer)."""
        from ml_trainer_amd.ops import dropout as D
        c = self.c
        H, dh = c.heads, c.hidden // c.heads
        res = x
        if c.pre_ln:
            x = self.ln1(x)
        qkv = self.qkv(x)
        if packed is not None:
            from ml_trainer_amd.ops.transformer import unpack_rows
            qkv = unpack_rows(qkv, packed)
        if c.num_kv_heads != H:  # compact q | k | v: every KV head repeated for the query heads of its group
            Hkv = c.num_kv_heads
            q, k, v = qkv.split((H * dh, Hkv * dh, Hkv * dh), dim=-1)
            q = q.view(B, S, H, dh).permute(0, 2, 1, 3)
            k = k.view(B, S, Hkv, dh).permute(0, 2, 1, 3).repeat_interleave(H // Hkv, dim=1)
            v = v.view(B, S, Hkv, dh).permute(0, 2, 1, 3).repeat_interleave(H // Hkv, dim=1)
        else:
            qkv = qkv.view(B, S, 3, H, dh).permute(2, 0, 3, 1, 4)
            q, k, v = qkv[0], qkv[1], qkv[2]
        if rope is not None:
            from ml_trainer_amd.ops.rope import rotate
            q, k = rotate(q, rope[:S]).to(q.dtype), rotate(k, rope[:S]).to(k.dtype)
        s = (q @ k.transpose(-1, -2)) / math.sqrt(dh)
        if mask is not None:
            s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
        if c.causal:
            s = s.masked_fill(~torch.ones(S, S, dtype=torch.bool, device=s.device).tril(), float("-inf"))
        pr = s.softmax(-1)
        if attn_drop is not None:
            p, seed, site, rank = attn_drop
            keep = D.attention_keep_mask(seed, site, rank, B, H, S, p, x.device)
            pr = pr * keep * D.attention_scale(p)
        ctx = (pr @ v).permute(0, 2, 1, 3).reshape(B * S, c.hidden)
        if packed is not None:
            ctx = ctx.index_select(0, packed.index)
        a = self.out(ctx)
        if drop is not None:
            a = D.apply(a, *drop)
        x = a + res if c.pre_ln else self.ln1(a + x)
        f = self.ffn_torch(self.ln2(x) if c.pre_ln else x)
        if drop is not None:
            f = D.apply(f, drop[0], drop[1], drop[2] + 1, drop[3])
        return f + x if c.pre_ln else self.ln2(f + x)


class BertClassifier(nn.Module):
    def __init__(self, c: Optional[BertConfig] = None):
        super().__init__()
        c = c or BertConfig()
        if c.hidden % c.heads or c.hidden // c.heads != 64:
            raise ValueError("the native attention kernel needs head dim 64")
        if not 0.0 <= c.hidden_dropout < 1.0:
            raise ValueError(f"hidden_dropout must satisfy 0 <= p < 1, got {c.hidden_dropout}")
        if not 0.0 <= c.attention_dropout < 1.0:
            raise ValueError(f"attention_dropout must satisfy 0 <= p < 1, got {c.attention_dropout}")
        if c.attention_dropout > 0:
            from ml_trainer_amd.ops.dropout import attention_threshold
            attention_threshold(c.attention_dropout)  # a p that rounds to 0/256 (or 256/256) is an error
        if c.norm not in ("layernorm", "rmsnorm"):
            raise ValueError(f"norm must be 'layernorm' or 'rmsnorm', got {c.norm!r}")
        if c.norm == "rmsnorm" and not c.pre_ln:
            raise ValueError("norm='rmsnorm' needs pre_ln=True: post-norm RMSNorm blocks are not built")
        if c.ffn not in ("gelu", "swiglu"):
            raise ValueError(f"ffn must be 'gelu' or 'swiglu', got {c.ffn!r}")
        from ml_trainer_amd.ops.gqa import check_kv_heads
        check_kv_heads(c.heads, c.kv_heads)
        for on, message in _fp8_exclusions(c):
            if on and c.fp8:
                raise ValueError(message)
        self.config = c
        self.last_dropout_seed = None  # the seed of the last forward that dropped
        self.word_embeddings = nn.Embedding(c.vocab_size, c.hidden)
        if c.rotary:  # no position table to train: the cos / sin table of ops/rope.py, not part of the state dict
            from ml_trainer_amd.ops.rope import rope_table
            self.position_embeddings = None
            self.register_buffer("rope_table", rope_table(c.max_position, c.rope_base).clone(), persistent=False)
        else:
            self.position_embeddings = nn.Embedding(c.max_position, c.hidden)
            self.rope_table = None
        self.token_type_embeddings = nn.Embedding(c.type_vocab, c.hidden)
        self.emb_ln = nn.LayerNorm(c.hidden, eps=c.ln_eps)
        self.layers = nn.ModuleList([BertLayer(c) for _ in range(c.layers)])
        if c.pre_ln:  # the norm of the last layer's stream: what every head consumes
            self.final_ln = block_norm(c)
        self._build_head(c)
        self.apply(self._init)

    def _build_head(self, c):
        self.pooler = nn.Linear(c.hidden, c.hidden)
        self.classifier = nn.Linear(c.hidden, c.num_labels)

    def _init(self, m):
        std = self.config.init_std
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, std=std)
            nn.init.zeros_(m.bias)
        elif isinstance(m, nn.Embedding):
            nn.init.normal_(m.weight, std=std)
        elif isinstance(m, nn.LayerNorm):
            nn.init.ones_(m.weight)
            nn.init.zeros_(m.bias)

    def _pos_weight(self):
        """The learned position table, or None under rotary positions (the embedding kernels then add none)."""
        return None if self.position_embeddings is None else self.position_embeddings.weight

    def _embed_torch(self, ids, tt, pos, per_batch=False):
        """word (+ learned position, ``pos`` indexing the table; ``per_batch``: one [S] row of positions for every
        sequence) + type in plain torch."""
        x = self.word_embeddings(ids)
        if self.position_embeddings is not None:
            p = self.position_embeddings(pos)
            x = x + (p[None] if per_batch else p)
        return x + self.token_type_embeddings(tt)

    def _final_norm(self, x):
        """``final_ln`` of a pre-norm model on the stream ``x`` in plain torch; the identity for post-LN."""
        return self.final_ln(x) if self.config.pre_ln else x

    def _lengths(self, input_ids, attention_mask):
        B, S = input_ids.shape
        if attention_mask is not None:
            return attention_mask.to(torch.int32).sum(1).clamp(min=1).to(torch.int32)
        if self.config.pad_id is not None:
            return (input_ids != self.config.pad_id).to(torch.int32).sum(1).clamp(min=1).to(torch.int32)
        return None

    def _dropout(self, dropout_seed=None):
        """(hidden, attention) of this forward: each (p, seed, rank) when that dropout is active
        (train() mode and its p > 0), else None. One seed serves both. Without ``dropout_seed`` one
        62-bit seed is drawn from torch's default CPU generator when either is active: no device
        sync, reproducible under torch.manual_seed / set_rng_state."""
        ph, pa = self.config.hidden_dropout, self.config.attention_dropout
        if not (self.training and (ph > 0 or pa > 0)):
            return None, None
        if dropout_seed is None:
            dropout_seed = torch.randint(0, 2 ** 62, (), dtype=torch.int64)
        from ml_trainer_amd.ops.dropout import data_parallel_rank
        self.last_dropout_seed = int(dropout_seed)
        rank = data_parallel_rank()
        return ((ph, self.last_dropout_seed, rank) if ph > 0 else None,
                (pa, self.last_dropout_seed, rank) if pa > 0 else None)

    @staticmethod
    def _site(drop, site):
        return None if drop is None else (drop[0], drop[1], site, drop[2])

    @classmethod
    def _layer_drops(cls, drop, adrop, l):
        """(p, seed, site, rank) or None of layer ``l``'s three sites, in the order of ``_sites``."""
        s_attn, s_ffn, s_prob = _sites(l)
        return cls._site(drop, s_attn), cls._site(drop, s_ffn), cls._site(adrop, s_prob)

    def _batch(self, input_ids, lens, token_type_ids, native=False) -> _Batch:
        """The ``_Batch`` of this forward: packed when ``unpad`` is on and lengths are known (``native``: with the
        row count rounded up to the GEMM tile), else padded."""
        from ml_trainer_amd.ops.transformer import PACK_ROW_MULTIPLE
        pk = self._pack(input_ids, lens, token_type_ids, PACK_ROW_MULTIPLE if native else 1)
        return _Batch.of(input_ids, lens, token_type_ids, pk)

    def _embed_batch_torch(self, bt):
        """``_embed_torch`` of a ``_Batch``: [B, S, h], or [T, h] for a packed one."""
        tt = bt.tt if bt.tt is not None else torch.zeros_like(bt.ids)
        if bt.packed is None:
            return self._embed_torch(bt.ids, tt, torch.arange(bt.S, device=bt.ids.device), per_batch=True)
        return self._embed_torch(bt.ids, tt, bt.pos.long())

    def _pack(self, input_ids, lens, token_type_ids, row_multiple=1):
        """The PackedBatch of this forward when ``unpad`` is on and lengths are known, else None."""
        if not self.config.unpad or lens is None:
            return None
        from ml_trainer_amd.ops.transformer import pack_batch
        return pack_batch(input_ids, lens, token_type_ids, row_multiple)

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, dropout_seed=None):
        """Logits [B, num_labels]. With ``config.unpad`` and lengths known (``attention_mask`` or
        ``pad_id``; right padding assumed) the batch is packed on the device and the encoder runs on
        the real tokens only; sizing the packed tensors costs one small device-to-host read (the
        token count) per forward. Without lengths the padded path runs."""
        if isinstance(input_ids, (tuple, list)):
            input_ids, attention_mask = input_ids[0], input_ids[1] if len(input_ids) > 1 else None
        lens = self._lengths(input_ids, attention_mask)
        drop, adrop = self._dropout(dropout_seed)
        if input_ids.is_cuda:
            from ml_trainer_amd.ops import transformer as T
            if self.config.fp8 and torch.is_grad_enabled():
                from ml_trainer_amd.ops.fp8 import context
                context(input_ids.device).update()  # delayed scaling: fold last step's amaxes
            bt = self._batch(input_ids, lens, token_type_ids, native=True)
            # (padded: a strided row view, which the pooler GEMM reads in place; packed: rows cu_seqlens[:-1])
            cls = bt.cls_rows(self._encode_native(bt, drop, adrop))
            if cls.shape[1] % 8 == 0 and self.pooler.weight.shape[0] % 8 == 0:
                return T.classifier_head(cls, self.pooler.weight, self.pooler.bias, self.classifier.weight,
                                         self.classifier.bias)
            cls = cls.float()
        else:
            cls = self.forward_reference_hidden(input_ids, lens, token_type_ids, drop, adrop)
        pooled = torch.tanh(self.pooler(cls))
        return self.classifier(pooled)

    def _encode_native(self, bt, drop, adrop):
        """The native encoder on a ``_Batch``: the hidden states every head consumes, [rows, h] bf16 (padded:
        B * S rows; packed: the T tokens, then the inert tail rows that round the count up to the GEMMs' 256-row
        tile). Post-LN: the last layer's output; pre-norm: ``final_ln`` of the last stream."""
        from ml_trainer_amd.ops import transformer as T
        c, layers = self.config, self.layers
        x = T.embeddings(bt.ids, bt.tt, self.word_embeddings.weight, self._pos_weight(),
                         self.token_type_embeddings.weight, bt.S, pos=bt.pos, cu_seqlens=bt.cu)
        x = T.layer_norm(x, self.emb_ln.weight, self.emb_ln.bias, c.ln_eps)
        if drop is not None:
            x = T.dropout(x, *self._site(drop, 0))
        n = None
        if c.pre_ln:  # x becomes the residual stream, n its norm under the next sub-layer's weights
            x, n = T.stream_norm(x, *_norm_args(layers[0].ln1))
        for l, layer in enumerate(layers):
            d_attn, d_ffn, d_prob = self._layer_drops(drop, adrop, l)
            closing = (layer.ln1, layer.ln2)
            if c.pre_ln:
                closing = (layer.ln2, layers[l + 1].ln1 if l + 1 < len(layers) else self.final_ln)
            x, n = layer.forward_native(x, n, bt.attn_spec(c, self.rope_table, d_prob), closing, (d_attn, d_ffn))
        return n if c.pre_ln else x

    def forward_reference_hidden(self, input_ids, lens=None, token_type_ids=None, drop=None, adrop=None, full=False):
        """The CLS rows [B, h] of the fp32 torch encoder; ``full``: every row, [B * S, h] (packed: [T, h])."""
        return self._reference_hidden(self._batch(input_ids, lens, token_type_ids), drop, adrop, full)

    def _reference_hidden(self, bt, drop, adrop, full=False):
        x = self.emb_ln(self._embed_batch_torch(bt)).view(-1, self.config.hidden)
        if drop is not None:
            from ml_trainer_amd.ops import dropout as D
            x = D.apply(x, *self._site(drop, 0))
        mask = bt.key_mask(x.device)
        for l, layer in enumerate(self.layers):
            d_attn, _, d_prob = self._layer_drops(drop, adrop, l)
            x = layer.forward_reference(x, mask, bt.B, bt.S, d_attn, d_prob, bt.packed, self.rope_table)
        x = self._final_norm(x)
        return x if full else bt.cls_rows(x)

    def forward_reference(self, input_ids, attention_mask=None, token_type_ids=None, dropout_seed=None):
        lens = self._lengths(input_ids, attention_mask)
        cls = self.forward_reference_hidden(input_ids, lens, token_type_ids, *self._dropout(dropout_seed))
        return self.classifier(torch.tanh(self.pooler(cls)))

    def forward_torch_bf16(self, input_ids, attention_mask=None, token_type_ids=None, dropout_seed=None):
        with torch.autocast(input_ids.device.type, dtype=torch.bfloat16):
            x, bt = self._hidden_torch_bf16(input_ids, attention_mask, token_type_ids, dropout_seed)
            cls = bt.cls_rows(x.reshape(-1, x.shape[-1]))
            return self.classifier(torch.tanh(self.pooler(cls.float())))

    def _hidden_torch_bf16(self, input_ids, attention_mask=None, token_type_ids=None, dropout_seed=None):
        """PyTorch-eager bf16 path on the same weights (torch.autocast + SDPA + hipBLASLt): the
        baseline the native kernels are benchmarked and error-budgeted against. Hidden dropout
        uses the native path's masks (ops.dropout), each applied in the dtype autocast gives the
        tensor it drops. With attention dropout active the attention is computed explicitly under
        autocast (softmax -> * keep * scale -> @ v) instead of through SDPA, which cannot take our mask.
        Under ``pre_ln`` the residual stream is rounded to bf16 after every add, as the native path stores it.
        Returns (hidden [B, S, h] -- packed: [1, T, h] --, the ``_Batch``); the callers add their head."""
        from ml_trainer_amd.ops import dropout as D
        c = self.config
        drop, adrop = self._dropout(dropout_seed)

        def dropped(t, site):  # t [B, S, h] (unpad: [1, T, h]), masks indexed by row
            return t if drop is None else D.apply(t.reshape(-1, t.shape[-1]), *self._site(drop, site)).view(t.shape)

        B, S = input_ids.shape
        lens = self._lengths(input_ids, attention_mask)
        bt = self._batch(input_ids, lens, token_type_ids)
        pk = bt.packed
        if pk is not None:
            from ml_trainer_amd.ops.transformer import unpack_rows
        mask = None
        if lens is not None:
            mask = (torch.arange(S, device=input_ids.device)[None, :] < lens[:, None])[:, None, None, :]
        causal = c.causal
        if causal and (mask is not None or adrop is not None):  # one boolean mask: key < len and key <= query
            tril = torch.ones(S, S, dtype=torch.bool, device=input_ids.device).tril()[None, None]
            mask = tril if mask is None else mask & tril
            causal = False
        with torch.autocast(input_ids.device.type, dtype=torch.bfloat16):
            x = self._embed_batch_torch(bt)
            if pk is not None:  # the packed rows as a batch of one, [1, T, h]; attention on a padded scratch of QKV
                x = x[None]
            x = dropped(self.emb_ln(x), 0)
            if c.pre_ln:
                x = x.to(torch.bfloat16)
            for l, L in enumerate(self.layers):
                s_attn, s_ffn, s_prob = _sites(l)
                qkv = L.qkv(L.ln1(x) if c.pre_ln else x)
                if pk is not None:
                    qkv = unpack_rows(qkv[0], pk)
                if c.num_kv_heads != c.heads:  # compact rows: the wide layout, k / v repeated per group
                    from ml_trainer_amd.ops.gqa import gqa_expand_reference
                    qkv = gqa_expand_reference(qkv.reshape(B * S, -1), c.heads, c.num_kv_heads)
                qkv = qkv.view(B, S, 3, c.heads, 64).permute(2, 0, 3, 1, 4)
                if c.rotary:  # fp32 rotation of the (bf16) q and k, rounded back as the native path stores them
                    from ml_trainer_amd.ops.rope import rotate
                    cs = self.rope_table[:S]
                    qkv = torch.stack((rotate(qkv[0], cs).to(qkv.dtype), rotate(qkv[1], cs).to(qkv.dtype), qkv[2]))
                if adrop is None:
                    ctx = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2], attn_mask=mask, is_causal=causal)
                else:
                    pa, seed, site, rank = self._site(adrop, s_prob)
                    sc = (qkv[0] @ qkv[1].transpose(-1, -2)) / 8.0
                    if mask is not None:
                        sc = sc.masked_fill(~mask, float("-inf"))
                    keep = D.attention_keep_mask(seed, site, rank, B, c.heads, S, pa, x.device)
                    pr = sc.softmax(-1)
                    ctx = (pr * keep * D.attention_scale(pa)).to(qkv[2].dtype) @ qkv[2]
                ctx = ctx.transpose(1, 2).reshape(B, S, -1)
                if pk is not None:
                    ctx = ctx.reshape(B * S, -1).index_select(0, pk.index)[None]
                if c.pre_ln:
                    x = (dropped(L.out(ctx), s_attn) + x).to(torch.bfloat16)
                    x = (dropped(L.ffn_torch(L.ln2(x), True), s_ffn) + x).to(torch.bfloat16)
                    continue
                x = L.ln1(dropped(L.out(ctx), s_attn) + x)
                x = L.ln2(dropped(L.ffn_torch(x, True), s_ffn) + x)
            return self._final_norm(x), bt

    def num_parameters(self) -> int:
        return sum(p.numel() for p in self.parameters())

    def flops_per_token(self, seq_len: int) -> float:
        """Training FLOPs per token (fwd + bwd = 3x fwd) of the encoder stack."""
        c = self.config
        h, f = c.hidden, c.intermediate
        if c.ffn == "swiglu":
            f = 3 * f // 2  # three h x f matrices instead of two
        per_layer = 2 * (3 * h * h + h * h + 2 * h * f) + 2 * 2 * seq_len * h  # linears + QK^T / PV
        return 3.0 * c.layers * per_layer


class BertForMaskedLM(BertClassifier):
    """The same encoder (same state-dict keys as ``BertClassifier``) under BERT's masked-language-model
    head instead of the pooler and classifier: transform ``mlm_dense`` + GELU + ``mlm_ln``, then the
    vocabulary projection with ``word_embeddings.weight`` itself (tied: no second module, no duplicate
    key) plus the output bias ``mlm_bias`` [V]. An MLM-pretrained state dict loads into a
    ``BertClassifier`` with ``strict=False`` (the fine-tune flow) and vice versa.

    ``forward`` returns the last layer's hidden states ([B * S, h]; bf16 on the GPU; the packed rows
    under ``unpad``) and remembers B, S and cu_seqlens of that forward; ``mlm_loss(hidden, labels)``
    runs ``ops.mlm.mlm_head`` on them (labels [B, S], -100 = not a target) and sets
    ``last_mlm_accuracy`` / ``last_mlm_overflow`` (device scalars). The vocabulary logits never exist
    beyond one chunk of ``mlm_chunk_rows`` rows. Every sequence gets ``config.max_predictions`` slots
    (default ceil(0.15 * S) rounded up to 8); targets past that are dropped and counted in the overflow.
    On the CPU, and in ``forward_reference``, everything runs in plain fp32 torch."""

    def __init__(self, c: Optional[BertConfig] = None):
        c = c or BertConfig()
        if c.fp8:
            raise ValueError("fp8=True with the masked-LM head is not supported: the fp8 linears are wired for "
                             "the classifier model only")
        if c.max_predictions is not None and c.max_predictions < 1:
            raise ValueError(f"max_predictions must be >= 1, got {c.max_predictions}")
        super().__init__(c)
        from ml_trainer_amd.ops.mlm import DEFAULT_CHUNK_ROWS
        self.mlm_chunk_rows = DEFAULT_CHUNK_ROWS
        self.last_mlm_accuracy = None
        self.last_mlm_overflow = None
        self._last_batch = None  # (B, S, lens, cu_seqlens) of the last forward

    def _build_head(self, c):
        self.mlm_dense = nn.Linear(c.hidden, c.hidden)
        self.mlm_ln = nn.LayerNorm(c.hidden, eps=c.ln_eps)
        self.mlm_bias = nn.Parameter(torch.zeros(c.vocab_size))

    def mlm_params(self):
        from ml_trainer_amd.ops.mlm import MLMParams
        return MLMParams(self.mlm_dense.weight, self.mlm_dense.bias, self.mlm_ln.weight, self.mlm_ln.bias,
                         self.word_embeddings.weight, self.mlm_bias, self.config.ln_eps)

    def max_predictions(self, S: int) -> int:
        from ml_trainer_amd.ops.mlm import default_max_predictions
        P = self.config.max_predictions
        return P if P is not None else default_max_predictions(S)

    def forward(self, input_ids, attention_mask=None, token_type_ids=None, dropout_seed=None):
        if isinstance(input_ids, (tuple, list)):
            input_ids, attention_mask = input_ids[0], input_ids[1] if len(input_ids) > 1 else None
        lens = self._lengths(input_ids, attention_mask)
        drop, adrop = self._dropout(dropout_seed)
        if not input_ids.is_cuda:
            return self._hidden_reference(input_ids, lens, token_type_ids, drop, adrop)
        bt = self._remember(self._batch(input_ids, lens, token_type_ids, native=True))
        return self._encode_native(bt, drop, adrop)

    def _remember(self, bt):
        self._last_batch = bt.last_batch()  # what mlm_loss needs of this forward
        return bt

    def _hidden_reference(self, input_ids, lens, token_type_ids, drop, adrop):
        bt = self._remember(self._batch(input_ids, lens, token_type_ids))
        return self._reference_hidden(bt, drop, adrop, full=True)

    def forward_reference(self, input_ids, attention_mask=None, token_type_ids=None, dropout_seed=None):
        """The hidden states in fp32 torch on any device (the numerics oracle of ``forward``)."""
        lens = self._lengths(input_ids, attention_mask)
        return self._hidden_reference(input_ids, lens, token_type_ids, *self._dropout(dropout_seed))

    def forward_torch_bf16(self, input_ids, attention_mask=None, token_type_ids=None, dropout_seed=None):
        """The hidden states of the PyTorch-eager bf16 baseline, [B * S, h] (packed: [T, h])."""
        with torch.autocast(input_ids.device.type, dtype=torch.bfloat16):
            x, bt = self._hidden_torch_bf16(input_ids, attention_mask, token_type_ids, dropout_seed)
        self._remember(bt)
        return x.reshape(-1, x.shape[-1])

    def _head(self, fn, hidden, labels, **kw):
        if self._last_batch is None:
            raise RuntimeError("mlm_loss needs the hidden states of a forward of this model")
        B, S, lens, cu = self._last_batch
        if tuple(labels.shape) != (B, S):
            raise ValueError(f"labels must be [B, S] = [{B}, {S}] as the last forward's input_ids, got "
                             f"{tuple(labels.shape)}")
        out = fn(hidden, labels.to(hidden.device), self.max_predictions(S), self.mlm_params(), cu_seqlens=cu,
                 lens=lens, **kw)
        self.last_mlm_accuracy = out.accuracy.detach()
        self.last_mlm_overflow = out.overflow
        self.last_mlm_row_loss = out.row_loss
        return out.loss

    def mlm_loss(self, hidden, labels):
        """Mean masked-LM loss (device scalar; 0 for a batch without targets) of ``hidden`` = this model's
        last forward output and ``labels`` [B, S]. Targets at pad positions are dropped."""
        from ml_trainer_amd.ops import mlm as M
        if hidden.is_cuda and hidden.dtype == torch.bfloat16:
            return self._head(M.mlm_head, hidden, labels, chunk_rows=self.mlm_chunk_rows)
        return self._head(M.mlm_head_reference, hidden, labels)

    def mlm_loss_reference(self, hidden, labels):
        from ml_trainer_amd.ops import mlm as M
        return self._head(M.mlm_head_reference, hidden, labels)

    def mlm_loss_torch_bf16(self, hidden, labels):
        """The eager bf16 head on the same weights (torch.autocast: F.linear + F.cross_entropy over the
        full [R, V] logits): the baseline next to ``forward_torch_bf16``."""
        from ml_trainer_amd.ops import mlm as M
        if self._last_batch is None:
            raise RuntimeError("mlm_loss_torch_bf16 needs the hidden states of a forward of this model")
        B, S, lens, cu = self._last_batch
        p = self.mlm_params()
        slot_row, slot_label, _ = M.select_reference(labels.to(hidden.device), self.max_predictions(S), lens, cu)
        with torch.autocast(hidden.device.type, dtype=torch.bfloat16):
            x = M.gather_reference(hidden, slot_row)
            t = self.mlm_ln(F.gelu(self.mlm_dense(x)))
            logits = F.linear(t, p.word_w, p.out_bias)
            n = (slot_label != M.IGNORE_INDEX).sum().clamp(min=1)
            return F.cross_entropy(logits.float(), slot_label, ignore_index=M.IGNORE_INDEX, reduction="sum") / n

    def mlm_logits(self, hidden, rows):
        """fp32 [len(rows), V]: the vocabulary logits of the given rows of ``hidden`` (inspection, tests)."""
        from ml_trainer_amd.ops import mlm as M
        return M.mlm_logits(hidden, rows, self.mlm_params())


def shift_labels(input_ids, lens=None):
    """Next-token labels of ``input_ids`` [B, S]: labels[b, s] = input_ids[b, s + 1] where s + 1 < len_b
    (``lens`` [B], or S without it), else -100. Pads and each sequence's last real token have no target."""
    B, S = input_ids.shape
    labels = torch.full_like(input_ids, -100)
    labels[:, :-1] = input_ids[:, 1:]
    if lens is not None:
        pos = torch.arange(S, device=input_ids.device)[None, :]
        labels = labels.masked_fill(pos + 1 >= lens.to(input_ids.device).long()[:, None], -100)
    return labels


class BertLMHeadModel(BertForMaskedLM):
    """The encoder run as a next-token decoder: ``causal`` forced on, under the MLM prediction head (the
    state-dict keys of ``BertForMaskedLM``). Every position has a prediction slot (``max_predictions(S)``
    is S), so ``ops.mlm.mlm_head`` (select, gather, transform, chunked tied decoder, ``vocab_ce``) is the
    LM head unchanged and nothing overflows. ``lm_loss(hidden, labels)`` is that head on next-token
    labels (``shift_labels``); ``last_mlm_accuracy`` is then the next-token accuracy."""

    def __init__(self, c: Optional[BertConfig] = None):
        c = c or BertConfig()
        super().__init__(c if c.causal else replace(c, causal=True))

    def max_predictions(self, S: int) -> int:
        return S

    def lm_loss(self, hidden, labels):
        """Mean next-token loss of ``hidden`` = this model's last forward output and the already shifted
        ``labels`` [B, S] (-100 = no target)."""
        return self.mlm_loss(hidden, labels)

    def lm_loss_reference(self, hidden, labels):
        return self.mlm_loss_reference(hidden, labels)

    # ------------------------------------------------------------------ incremental decoding (ops/decode.py)
    def _last_rows(self, lens, B, S, device):
        """Flat row b * S + len_b - 1 of every sequence's last real token (S - 1 without lengths)."""
        last = (lens.to(device).long() - 1) if lens is not None else torch.full((B,), S - 1, device=device)
        return torch.arange(B, device=device) * S + last

    @torch.no_grad()
    def prefill(self, input_ids, attention_mask=None, max_len: Optional[int] = None, cache=None, kv_cache=None,
                pool=None, weights=None):
        """Run the prompt ``input_ids`` [B, S] (right-padded; lengths from ``attention_mask`` or ``pad_id``)
        through the padded causal forward, layer by layer, keep every layer's K / V in a cache of ``max_len``
        rows per sequence (default ``config.max_position``) and return the ``DecodeState``: the cache with
        ``pos = lens`` and the hidden row of each sequence's last real token. No gradients and no dropout,
        whatever mode the model is in; ``config.unpad`` has no effect (prompts are short). ``cache``: an existing
        ``KVCache`` of this shape to fill in place (its ``pos`` is overwritten with ``pos.copy_``, its tensors keep
        their addresses: what a captured decode step needs) instead of a new one. ``kv_cache``: ``None`` / ``"bf16"``
        (the cache as it is) or ``"fp8"`` (e4m3 codes and one scale per cached row, ``ops.decode.KVCache``); a given
        ``cache`` must be of that format. ``decode_step`` takes the format from the cache. ``pool`` (an
        ``ops.decode.PagePool`` of this model's layers and KV heads on the prompts' device): the state's cache is a
        ``PagedKVCache`` over it with a table of ``ceil(max(max_len or S, S) / 64)`` pages, of which it owns those of
        the S prompt rows; ``decode_step`` reserves more as the sequences grow, past ``max_len`` too, and
        ``state.release()`` returns them. Not with ``cache=`` or ``kv_cache="fp8"``. ``weights``: ``None`` /
        ``"bf16"`` or ``"fp8"``, recorded in the state for ``decode_step`` and ``extend`` (``generate`` documents the
        option); the prompt itself always runs on the bf16 tile GEMMs and the full weights."""
        from ml_trainer_amd.ops import decode as DC
        c = self.config
        fp8 = DC.check_kv_cache(kv_cache)
        DC.check_weights(weights)
        B, S = input_ids.shape
        if pool is not None:
            self._check_pool(pool, input_ids.device, fp8, cache)
        Smax = c.max_position if max_len is None else int(max_len)
        if not S <= Smax <= c.max_position:
            raise ValueError(f"prefill: prompt width {S} <= max_len {Smax} <= max_position {c.max_position} "
                             f"does not hold")
        dev = input_ids.device
        lens = self._lengths(input_ids, attention_mask)
        if pool is not None:
            cache = DC.PagedKVCache(pool, B, -(-max(int(max_len or S), S) // DC.PAGE_ROWS))
            cache.reserve(S)
        elif cache is None:
            cache = DC.KVCache.allocate(c.layers, B, c.num_kv_heads, Smax, dev, kv_cache=kv_cache)
        elif (cache.Smax != Smax or len(cache.kv) != c.layers or cache.pos.device != dev or
              tuple(cache.kv[0].shape) != (2, B, c.num_kv_heads, Smax, DC.HEAD_DIM)):
            raise ValueError(f"prefill: the given cache does not hold {c.layers} layers of [2, {B}, {c.num_kv_heads}, {Smax}, "
                             f"{DC.HEAD_DIM}] on {dev}")
        elif (cache.scales is not None) != fp8:
            raise ValueError(f"prefill: the given cache is {cache.kv_cache}, kv_cache = {kv_cache!r}")
        if input_ids.is_cuda:
            from ml_trainer_amd.ops import transformer as T
            x = T.embeddings(input_ids, None, self.word_embeddings.weight, self._pos_weight(),
                             self.token_type_embeddings.weight, S)
            x = _norm_native(x, self.emb_ln)
            spec = _Batch.of(input_ids, lens, None).attn_spec(c, self.rope_table)
            for l, L in enumerate(self.layers):
                # pre-norm: x is the stream, a sub-layer reads its norm (the cache holds the K / V of that norm) and
                # its sum is the new stream; post-LN: a sub-layer reads x and its normed sum is the new x
                n = _norm_native(x, L.ln1) if c.pre_ln else x
                y, (_, qkv, _, _) = T._attn_fwd(n, L.attn_params(), x, spec)
                # (qkv: rotated under rotary, the wide buffer under kv_heads)
                DC.fill_from_prefill(cache, l, qkv, lens, B, S, heads=c.heads)
                x = y if c.pre_ln else _norm_native(y, L.ln1)
                n = _norm_native(x, L.ln2) if c.pre_ln else x
                y, _ = T._ffn_fwd(n, L.ffn_params(), x, c.ffn)
                x = y if c.pre_ln else _norm_native(y, L.ln2)
        else:
            pos = torch.arange(S, device=dev)
            x = self._embed_torch(input_ids, torch.zeros_like(input_ids), pos, per_batch=True)
            x = self.emb_ln(x).view(B * S, -1)
            mask = None if lens is None else pos[None, :] < lens[:, None]
            for l, L in enumerate(self.layers):
                qkv = L.qkv(L.ln1(x) if c.pre_ln else x)
                if c.num_kv_heads != c.heads:
                    from ml_trainer_amd.ops.gqa import gqa_expand_reference
                    qkv = gqa_expand_reference(qkv, c.heads, c.num_kv_heads)
                if c.rotary:  # the cache holds rotated keys
                    from ml_trainer_amd.ops.rope import rope_qk_reference
                    qkv = rope_qk_reference(qkv, self.rope_table, c.heads, S)
                DC.fill_from_prefill(cache, l, qkv, lens, B, S, heads=c.heads)
                x = L.forward_reference(x, mask, B, S, rope=self.rope_table)
        cache.pos.copy_(lens if lens is not None else torch.full((B,), S, dtype=torch.int32, device=dev))
        x = x.index_select(0, self._last_rows(lens, B, S, dev))
        if c.pre_ln:  # rows are independent: the final norm of the last real rows only
            x = _norm_native(x, self.final_ln) if x.is_cuda else self.final_ln(x)
        return DC.DecodeState(cache, x, width=S, weights=weights)

    def _check_pool(self, pool, dev, fp8=False, cache=None):
        """The ``ValueError`` cases of ``prefill(pool=)`` / ``generate(pool=)``."""
        c = self.config
        if fp8:
            raise ValueError("pool= takes a bf16 cache: there are no fp8 pages (kv_cache='fp8' cannot be given with it)")
        if cache is not None:
            raise ValueError("pool= builds its own PagedKVCache: cache= cannot be given with it")
        if len(pool.kv) != c.layers or pool.Hkv != c.num_kv_heads or pool.device != dev:
            raise ValueError(f"the page pool holds {len(pool.kv)} layers of {pool.Hkv} KV heads on {pool.device}, the "
                             f"model needs {c.layers} layers of {c.num_kv_heads} on {dev}")

    def _reserve_paged(self, state, rows: int):
        """Before a step over a paged state: pages for ``rows`` rows per sequence, by the host bound ``state.width``."""
        c = self.config
        if rows > c.max_position:
            raise ValueError(f"a paged state of {rows} rows exceeds max_position {c.max_position}")
        state.cache.reserve(rows)
        if self.rope_table is not None and state.cache.Smax > self.rope_table.shape[0]:
            raise ValueError(f"a block table of {state.cache.max_pages} pages names {state.cache.Smax} rows, the rotary "
                             f"table has max_position = {self.rope_table.shape[0]}: make it a multiple of 64")

    def _state_logits(self, state):
        from ml_trainer_amd.ops import decode as DC
        from ml_trainer_amd.ops import mlm as M
        B, h = state.hidden.shape
        Vp = M._round_up(self.config.vocab_size, M.VOCAB_MULTIPLE)
        if (state.hidden.is_cuda and state.hidden.dtype == torch.bfloat16 and
                DC.decode_linear_path(B, h, h) == "skinny" and DC.decode_linear_path(B, Vp, h) == "skinny"):
            return M.decode_logits(state.hidden, self.mlm_params())  # B rows, no gather into a 256-row tile
        return self.mlm_logits(state.hidden, torch.arange(B, device=state.hidden.device))

    def _ffn1_decode(self, L, x, fp8=False):
        """act(ffn1(x)) [B, F] bf16 of a native decode step: FFN1 with the GELU epilogue, or under SwiGLU the gated
        skinny GEMM (``ops.decode.linear_small_glu``). ``fp8``: on the fp8 weight rows."""
        from ml_trainer_amd.ops import decode as DC
        from ml_trainer_amd.ops.transformer import bf16_weight
        w8 = DC.fp8_weight_rows(L.ffn1.weight) if fp8 else None
        if self.config.ffn == "swiglu":
            return DC.linear_small_glu(x, bf16_weight(L.ffn1.weight), L.ffn1.bias, w8=w8)
        pre = torch.empty(x.shape[0], L.ffn1.weight.shape[0], dtype=torch.bfloat16, device=x.device)
        return DC.linear_small(x, bf16_weight(L.ffn1.weight), L.ffn1.bias, gelu_aux=pre, w8=w8)

    @torch.no_grad()
    def decode_step(self, state, token_ids=None):
        """fp32 logits [B, V] of the next token. Without ``token_ids``: those of the prompt's last token, nothing
        new is run. With ``token_ids`` [B]: token b enters sequence b at position ``state.pos[b]`` and runs
        through the stack on one row per sequence (embedding at explicit positions, per layer QKV GEMM ->
        ``attn_decode`` over the cache, which under rotary positions rotates q and the new k by ``state.pos[b]`` first
        -> out-projection + residual -> LayerNorm -> FFN -> LayerNorm; pre-norm: norm -> QKV -> ``attn_decode`` ->
        out-projection + stream -> norm -> FFN + stream per layer, then ``final_ln``), then
        ``state.pos`` advances by 1 on the device. Nothing is read back from the device. The caller keeps
        ``state.pos[b]`` below the cache's ``Smax`` (``generate`` does by construction)."""
        if token_ids is None:
            return self._state_logits(state)
        from ml_trainer_amd.ops import decode as DC
        c = self.config
        cache = state.cache
        fp8w = DC.check_weights(state.weights)
        ids = token_ids.reshape(-1).to(torch.int64).contiguous()
        B = ids.numel()
        paged = isinstance(cache, DC.PagedKVCache)
        if paged:  # pages for the row this step appends; the table may be a new, wider tensor afterwards
            if state.width is None:
                raise ValueError("a paged state needs its width (the host bound pages are reserved by)")
            self._reserve_paged(state, state.width + 1)
        if ids.is_cuda:
            from ml_trainer_amd.ops import transformer as T
            C = T.require_native()
            x = torch.empty(B, c.hidden, dtype=torch.bfloat16, device=ids.device)
            C.embed_fwd(ids, None, T.bf16_weight(self.word_embeddings.weight),
                        None if c.rotary else T.bf16_weight(self.position_embeddings.weight),
                        T.bf16_weight(self.token_type_embeddings.weight), x,
                        min(cache.Smax, c.max_position) if paged else cache.Smax, pos=cache.pos)
            if paged:
                x = self._decode_layers(x, lambda l, qkv: DC.attn_decode(
                    qkv, cache.kv[l], cache.pos, c.heads, rope=self.rope_table, block_table=cache.block_table), fp8w)
            else:
                x = self._decode_layers(x, lambda l, qkv: DC.attn_decode(
                    qkv, cache.kv[l], cache.pos, c.heads, rope=self.rope_table, kv_scale=cache.scale(l)), fp8w)
        else:
            x = self._embed_torch(ids, torch.zeros_like(ids), cache.pos.long())
            if paged:
                x = self._decode_layers_torch(x, lambda l, qkv: DC.attn_decode_paged_reference(
                    qkv, cache.kv[l], cache.block_table, cache.pos, c.heads, rope=self.rope_table), fp8w)
            else:
                x = self._decode_layers_torch(x, lambda l, qkv: DC.attn_decode_reference(
                    qkv, cache.kv[l], cache.pos, c.heads, rope=self.rope_table, kv_scale=cache.scale(l)), fp8w)
        cache.pos.add_(1)
        state.hidden = x
        if state.width is not None:
            state.width += 1
        return self._state_logits(state)

    def _decode_layers(self, x, attn, fp8=False):
        """The native layer walk of ``decode_step`` and ``extend`` on the embedded bf16 rows ``x`` [M, h]: every kernel
        works row by row except ``attn(l, qkv)``, the attention of layer l over the cache. Returns the rows
        ``state.hidden`` holds (normed, as after a post-LN layer). ``fp8`` (``DecodeState.weights == "fp8"``): the four
        layer linears read ``ops.decode.fp8_weight_rows`` of their weights; the attention call is untouched."""
        from ml_trainer_amd.ops import decode as DC
        from ml_trainer_amd.ops import transformer as T
        c = self.config
        w8 = (lambda m: DC.fp8_weight_rows(m.weight)) if fp8 else (lambda m: None)
        x = _norm_native(x, self.emb_ln)
        for l, L in enumerate(self.layers):  # (x, n and the sums as in prefill)
            n = _norm_native(x, L.ln1) if c.pre_ln else x
            qkv = DC.linear_small(n, T.bf16_weight(L.qkv.weight), L.qkv.bias, w8=w8(L.qkv))
            ctx = attn(l, qkv)
            y = DC.linear_small(ctx, T.bf16_weight(L.out.weight), L.out.bias, res=x, w8=w8(L.out))
            x = y if c.pre_ln else _norm_native(y, L.ln1)
            n = _norm_native(x, L.ln2) if c.pre_ln else x
            y = DC.linear_small(self._ffn1_decode(L, n, fp8), T.bf16_weight(L.ffn2.weight), L.ffn2.bias, res=x,
                                w8=w8(L.ffn2))
            x = y if c.pre_ln else _norm_native(y, L.ln2)
        if c.pre_ln:
            x = _norm_native(x, self.final_ln)
        return x

    def _decode_layers_torch(self, x, attn, fp8=False):
        """``_decode_layers`` on the modules (the CPU path), from the embedding sum ``x``. ``fp8``: the four layer
        linears as ``F.linear`` on their dequantised fp8 weight rows, otherwise the same operations in the same order."""
        c = self.config
        if fp8:
            from ml_trainer_amd.ops import decode as DC

            def lin(m, v):
                return F.linear(v, DC.w8_dequantized(DC.fp8_weight_rows(m.weight), v.dtype), m.bias)
        else:
            def lin(m, v):
                return m(v)
        x = self.emb_ln(x)
        for l, L in enumerate(self.layers):
            n = L.ln1(x) if c.pre_ln else x
            y = lin(L.out, attn(l, lin(L.qkv, n))) + x
            x = y if c.pre_ln else L.ln1(y)
            y = L.ffn_torch(L.ln2(x) if c.pre_ln else x, lin=lin) + x
            x = y if c.pre_ln else L.ln2(y)
        return self._final_norm(x)

    def _rows_logits(self, x):
        """fp32 [M, V] of the hidden rows ``x`` [M, h]: ``decode_logits`` where both its linears route "skinny"."""
        from ml_trainer_amd.ops import decode as DC
        from ml_trainer_amd.ops import mlm as M
        rows, h = x.shape
        Vp = M._round_up(self.config.vocab_size, M.VOCAB_MULTIPLE)
        if (x.is_cuda and x.dtype == torch.bfloat16 and DC.decode_linear_path(rows, h, h) == "skinny" and
                DC.decode_linear_path(rows, Vp, h) == "skinny"):
            return M.decode_logits(x, self.mlm_params())
        return self.mlm_logits(x, torch.arange(rows, device=x.device))

    @torch.no_grad()
    def extend(self, state, token_ids, counts=None):
        """fp32 logits [B, T, V] of ``token_ids`` [B, T] pushed into a live cache in one pass: token t of sequence b
        enters at position ``state.pos[b] + t`` and sees the cache and the tokens before it (a new chat turn, a
        prompt fed in pieces, the verification pass of speculative decoding). The walk is ``decode_step``'s on
        ``B * T`` rows with ``ops.decode.attn_append`` as the attention; ``T > 16`` runs in pieces of at most 16
        tokens, each seeing the previous ones in the cache. Then ``state.pos += counts`` (int32 [B] on the device,
        ``0 <= counts[b] <= T``, default T): rows past ``counts[b]`` were written but stay above ``pos``, stale by
        definition, so accepting fewer tokens than were scored costs nothing. ``state.hidden`` becomes the row of
        token ``counts[b] - 1`` (unchanged where ``counts[b] == 0``). Nothing is read back from the device. The
        caller keeps ``state.pos[b] + T <= Smax``, as with ``decode_step``. An fp8 cache and ``T < 1`` raise
        ``ValueError``."""
        from ml_trainer_amd.ops import decode as DC
        c = self.config
        cache = state.cache
        fp8w = DC.check_weights(state.weights)
        if cache.scales is not None:
            raise ValueError("extend takes a bf16 cache: the fp8 cache has no multi-token attention kernel")
        if isinstance(cache, DC.PagedKVCache):
            raise ValueError("extend takes a contiguous cache: the paged cache has no multi-token attention kernel")
        if token_ids.dim() != 2 or token_ids.shape[1] < 1 or token_ids.shape[0] != cache.pos.numel():
            raise ValueError(f"extend takes token_ids [B = {cache.pos.numel()}, T >= 1], got {tuple(token_ids.shape)}")
        B, T = token_ids.shape
        dev = token_ids.device
        counts = (torch.full((B,), T, dtype=torch.int32, device=dev) if counts is None
                  else counts.to(device=dev, dtype=torch.int32).clamp(0, T))
        ar = torch.arange(B, device=dev)
        logits = []
        for t0 in range(0, T, DC.APPEND_MAX_TOKENS):
            ids = token_ids[:, t0:t0 + DC.APPEND_MAX_TOKENS].to(torch.int64)
            Tp = ids.shape[1]
            ids = ids.reshape(-1).contiguous()
            # every piece sits at pos + t0 whatever counts says, so all T rows of logits are those of their positions;
            # pos itself moves once, at the end, by counts
            base = cache.pos + t0
            tpos = (base[:, None] + torch.arange(Tp, dtype=torch.int32, device=dev)[None, :]).reshape(-1)
            if ids.is_cuda:
                from ml_trainer_amd.ops import transformer as TR
                x = torch.empty(B * Tp, c.hidden, dtype=torch.bfloat16, device=dev)
                TR.require_native().embed_fwd(ids, None, TR.bf16_weight(self.word_embeddings.weight),
                                              None if c.rotary else TR.bf16_weight(self.position_embeddings.weight),
                                              TR.bf16_weight(self.token_type_embeddings.weight), x, cache.Smax,
                                              pos=tpos.contiguous())
                x = self._decode_layers(x, lambda l, qkv: DC.attn_append(qkv, cache.kv[l], base, B, c.heads,
                                                                         rope=self.rope_table), fp8w)
            else:
                x = self._embed_torch(ids, torch.zeros_like(ids), tpos.long())
                x = self._decode_layers_torch(x, lambda l, qkv: DC.attn_append_reference(
                    qkv, cache.kv[l], base, B, c.heads, rope=self.rope_table), fp8w)
            sel = (counts.long() - 1 - t0)  # token counts - 1, where it falls in this piece (on the device)
            last = x.view(B, Tp, -1)[ar, sel.clamp(0, Tp - 1)]
            state.hidden = torch.where(((sel >= 0) & (sel < Tp))[:, None], last, state.hidden.to(last.dtype))
            logits.append(self._rows_logits(x).float().reshape(B, Tp, -1))
        cache.pos.add_(counts)
        if state.width is not None:
            state.width += T
        return logits[0] if len(logits) == 1 else torch.cat(logits, 1)

    def _feed_paged(self, state, token_ids, counts):
        """What ``extend`` does for ``generate(past=)``, over a paged state: the columns of ``token_ids`` [B, T] one
        ``decode_step`` each (the paged cache has no multi-token kernel). A sequence with ``counts[b] <= t`` takes
        column t back: its ``pos`` and hidden row stay, and the row it wrote lies at ``pos[b]``, stale by definition."""
        counts = counts.to(device=token_ids.device, dtype=torch.int32)
        for t in range(token_ids.shape[1]):
            hidden = state.hidden
            self.decode_step(state, token_ids[:, t])
            live = counts > t
            state.cache.pos.sub_((~live).to(torch.int32))
            state.hidden = torch.where(live[:, None], state.hidden, hidden.to(state.hidden.dtype))

    def _check_generate(self, input_ids, max_new_tokens, temperature, top_k, top_p=None, sampler=None, graph=False,
                        return_logits=False, kv_cache=None, weights=None):
        from ml_trainer_amd.ops.decode import check_kv_cache, check_weights
        S = input_ids.shape[1]
        check_kv_cache(kv_cache)
        check_weights(weights)
        if sampler not in (None, "device"):
            raise ValueError(f"sampler must be None (the torch sampler) or 'device', got {sampler!r}")
        if top_p is not None:
            from ml_trainer_amd.ops.decode import top_p_to_p16
            if sampler != "device":
                raise ValueError("top_p needs sampler='device' (the torch sampler has no nucleus sampling)")
            top_p_to_p16(top_p)  # raises outside (0, 1] and where it rounds to 0 / 65536
        if graph:
            if sampler != "device":
                raise ValueError("graph=True needs sampler='device': the torch sampler cannot be captured")
            if return_logits:
                raise ValueError("graph=True cannot return per-step logits (they live in the graph's buffers)")
            if not input_ids.is_cuda:
                raise ValueError("graph=True needs the prompts on a GPU")
        if max_new_tokens < 1:
            raise ValueError(f"max_new_tokens must be >= 1, got {max_new_tokens}")
        if temperature < 0:
            raise ValueError(f"temperature must be >= 0, got {temperature}")
        if top_k is not None and top_k < 1:
            raise ValueError(f"top_k must be >= 1, got {top_k}")
        if S + max_new_tokens > self.config.max_position:
            raise ValueError(f"prompt width {S} + max_new_tokens {max_new_tokens} exceeds max_position "
                             f"{self.config.max_position}")

    def _generate_loop(self, first_logits, step, B, dev, max_new_tokens, temperature, top_k, eos_id, seed,
                       return_logits):
        """The token loop shared by ``generate`` and ``generate_reference``: ``first_logits()`` are the prompt's,
        ``step(tokens)`` feeds [B] tokens and returns the next logits. Always ``max_new_tokens`` steps; EOS is a
        device-side mask, nothing is read back."""
        from ml_trainer_amd.ops.decode import sample_tokens
        gen = None
        if temperature > 0:
            gen = torch.Generator(device=dev)
            if seed is not None:
                gen.manual_seed(seed)
        fill = None
        if eos_id is not None:
            fill = self.config.pad_id if self.config.pad_id is not None else eos_id
        finished = torch.zeros(B, dtype=torch.bool, device=dev)
        lengths = torch.zeros(B, dtype=torch.int64, device=dev)
        tokens, kept = [], []
        logits = first_logits()
        for t in range(max_new_tokens):
            tok = sample_tokens(logits, temperature, top_k, gen)
            if eos_id is not None:
                tok = torch.where(finished, torch.full_like(tok, fill), tok)
                lengths += (~finished).long()
                finished = finished | (tok == eos_id)
            else:
                lengths += 1
            tokens.append(tok)
            if return_logits:
                kept.append(logits)
            if t + 1 < max_new_tokens:
                logits = step(tok)
        out = (torch.stack(tokens, 1), lengths)
        return out + (torch.stack(kept, 1),) if return_logits else out

    def _new_sampler(self, B, T, dev, temperature, top_k, top_p, eos_id, seed):
        from ml_trainer_amd.ops.decode import SamplerState
        return SamplerState.allocate(B, T, dev, **self._sampler_params(temperature, top_k, top_p, eos_id, seed))

    def _sampler_params(self, temperature, top_k, top_p, eos_id, seed):
        """``SamplerState.set_params`` arguments of a ``generate`` call: the fill token is ``config.pad_id``
        (``eos_id`` without one), an unseeded sampling run draws its seed from torch's host generator."""
        fill = 0
        if eos_id is not None:
            fill = self.config.pad_id if self.config.pad_id is not None else eos_id
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if temperature > 0 else 0
        return dict(seed=seed, temperature=temperature, top_k=top_k, top_p=top_p, eos_id=eos_id, fill_id=fill)

    def _device_sampler_loop(self, first_logits, step, sampler, max_new_tokens, return_logits):
        """``_generate_loop`` with the on-device sampler: ``sample_step`` (its torch reference on the CPU) draws
        into ``sampler`` and does the EOS bookkeeping, ``step(sampler.next_ids)`` returns the next logits."""
        from ml_trainer_amd.ops import decode as DC
        sample = DC.sample_step if sampler.tokens.is_cuda else DC.sample_step_reference
        V = self.config.vocab_size
        kept = []
        logits = first_logits()
        for t in range(max_new_tokens):
            sample(logits, V, sampler)
            if return_logits:
                kept.append(logits)
            if t + 1 < max_new_tokens:
                logits = step(sampler.next_ids)
        out = (sampler.tokens, sampler.lengths)
        return out + (torch.stack(kept, 1),) if return_logits else out

    def _decode_signature(self, weights=None):
        """What a captured decode step baked in of the parameters: an in-place edit bumps ``_version`` (and makes
        ``bf16_weight`` / ``padded_decoder`` / ``fp8_weight_rows`` hand out new tensors), a re-allocation moves
        ``data_ptr``. ``weights="fp8"`` adds the format (which linears a step launches); without it no value changes."""
        c = self.config  # (the block kind decides which kernels a step launches)
        gqa = (c.kv_heads,) if c.num_kv_heads != c.heads else ()  # (the attention launch and the cache shape)
        ffn = (c.ffn,) if c.ffn != "gelu" else ()  # (which FFN1 launch a step makes)
        w8 = ("w-fp8",) if weights == "fp8" else ()
        return (c.pre_ln, c.norm) + gqa + ffn + w8 + tuple((p._version, p.data_ptr()) for p in self.parameters())

    def _graphed_decoder(self, B, Smax, T, dev, kv_cache=None, weights=None):
        key = (B, Smax, T, str(dev)) + (("fp8",) if kv_cache == "fp8" else ())  # (the cache a capture baked in)
        key += ("w-fp8",) if weights == "fp8" else ()  # (and the weight tensors its linears read)
        decoders = self.__dict__.setdefault("_graphed_decoders", {})
        dec = decoders.get(key)
        sig = self._decode_signature(weights)
        if dec is None or dec.signature != sig:
            decoders.pop(key, None)  # free the stale graph's buffers before the new capture
            del dec
            dec = decoders[key] = GraphedDecoder(self, B, Smax, T, dev, sig, kv_cache, weights)
            self._decode_graph_captures = self.decode_graph_captures + 1
        return dec

    @property
    def decode_graph_captures(self) -> int:
        """How many decode graphs this model has captured (``generate(graph=True)``)."""
        return getattr(self, "_decode_graph_captures", 0)

    @torch.no_grad()
    def generate(self, input_ids, max_new_tokens: int, attention_mask=None, temperature: float = 0.0,
                 top_k: Optional[int] = None, eos_id: Optional[int] = None, seed: Optional[int] = None,
                 return_logits: bool = False, top_p: Optional[float] = None, sampler: Optional[str] = None,
                 graph: bool = False, kv_cache: Optional[str] = None, past=None, pool=None,
                 weights: Optional[str] = None):
        """Continue the prompts ``input_ids`` [B, S] (right-padded, ragged lengths allowed: sequence b's new
        tokens continue at position ``len_b``) by ``max_new_tokens`` tokens with a key/value cache: one
        ``prefill``, then one ``decode_step`` per token. Returns ``(tokens [B, max_new_tokens], lengths [B])``,
        plus the per-step logits [B, max_new_tokens, V] with ``return_logits``.

        ``temperature == 0``: greedy argmax. Otherwise a draw from softmax(logits / temperature), restricted to
        the ``top_k`` largest when given, from a device ``torch.Generator`` seeded with ``seed``. With ``eos_id`` a
        sequence that has emitted it produces ``config.pad_id`` (``eos_id`` without a pad id) from then on and
        ``lengths[b]`` counts its tokens up to and including the EOS; the loop still runs every step and never
        reads from the device. Runs without gradients and without dropout in any mode.

        ``sampler="device"`` (opt-in; ``None`` keeps the torch sampler and its random stream): every token comes
        from ``ops.decode.sample_step``, one launch that samples and does the EOS bookkeeping on the device, with
        an integer-defined result: seeded runs repeat bit for bit and a sequence's tokens do not depend on the batch
        it is decoded in. ``top_p`` (nucleus sampling inside the top-k set, applied as ``round(top_p * 65536) /
        65536``) needs it. ``graph=True`` (GPU, device sampler, no ``return_logits``) replays one captured graph
        of ``decode_step`` + ``sample_step`` per token (``GraphedDecoder``); the graph is captured on the first call
        of a shape and again after a parameter changed, and ``MLT_DECODE_GEMM`` / ``MLT_DECODE_SPLIT`` are read when it is
        captured.

        ``kv_cache="fp8"`` (opt-in; ``None`` / ``"bf16"`` change nothing): the cache holds OCP e4m3 codes and one
        power-of-two scale per cached row (``ops.decode.kv_quantize_reference``), 0.53 x the bytes; a step's attention
        is ``C.attn_decode_f8`` over the dequantised rows, the prompt is quantised by ``C.kv_fill_f8``. Works eager and
        graph-replayed, with every block kind, ``rotary`` and ``kv_heads``.

        ``weights="fp8"`` (opt-in; ``None`` / ``"bf16"`` change nothing): weight-only quantisation of the decode steps.
        The four layer linears of every step (QKV, out-projection, FFN1 including the gated form, FFN2) read e4m3
        codes and one power-of-two scale per output row (``ops.decode.weight_quantize_reference``, made once per
        weight version by ``fp8_weight_rows``) through ``C.gemm_skinny_f8`` / ``C.gemm_skinny_glu_f8``: half the
        bytes of a step's largest stream, activations bf16, accumulation fp32. A step is exactly the bf16 step on
        the dequantised weights. Not covered: the prompt (compute-bound: the bf16 tile GEMMs on the full weights),
        the head (the transform and the tied vocabulary decoder stay bf16; the decoder shares its table with the
        embedding lookup) and memory (the fp32 and bf16 weights remain, the codes are a third copy). Works eager and
        graph-replayed, with every cache kind, ``past=`` (``None`` keeps the state's own setting) and ``pool=``.

        ``past`` (a ``DecodeState`` of an earlier ``prefill`` / ``generate`` turn over the same batch): ``input_ids``
        are then the NEW turn only; they enter ``past``'s cache through ``extend`` instead of ``prefill``, the first
        logits are those of each sequence's last real new token, and decoding continues into ``past``'s cache (the
        state is advanced in place and can be passed again). Not with ``graph=True`` (the captured decoder owns its
        cache) or an fp8 cache. The cache must have room for ``pos[b] + S + max_new_tokens`` rows: checked against
        ``past.width`` where the state records it, otherwise the caller's duty, as with ``decode_step``.

        ``pool`` (an ``ops.decode.PagePool``; eager, either sampler, bf16): the cache is a ``PagedKVCache`` over it
        (``prefill(pool=)``) that owns pages for the rows it holds and takes more as it grows; its pages go back to the
        pool before this returns. A paged ``past`` (from ``prefill(pool=)``) simply grows, past the ``max_len`` it was
        made with: the new turn enters it one ``decode_step`` per column, the "does not fit" error is the contiguous
        cache's alone, and the state stays the caller's to ``release()``. Tokens and logits are those of the
        contiguous cache, bit for bit while fewer than 256 rows are cached (one active split)."""
        self._check_generate(input_ids, max_new_tokens, temperature, top_k, top_p, sampler, graph, return_logits,
                             kv_cache, weights)
        B, S = input_ids.shape
        dev = input_ids.device
        from ml_trainer_amd.ops.decode import PagedKVCache
        if pool is not None:
            if graph:
                raise ValueError("generate(pool=) runs eager: a captured decoder bakes in its cache's addresses")
            self._check_pool(pool, dev, kv_cache == "fp8")
            if past is not None and (not isinstance(past.cache, PagedKVCache) or past.cache.pool is not pool):
                raise ValueError("generate(past=, pool=): the state's cache is not a paged cache over that pool")
        if past is not None:
            if graph:
                raise ValueError("generate(past=) cannot run graph=True: the captured decoder owns its cache")
            if kv_cache == "fp8" or past.cache.scales is not None:
                raise ValueError("generate(past=) takes a bf16 cache: extend has no fp8 form")
            if weights is not None:
                past.weights = weights
            if isinstance(past.cache, PagedKVCache):
                lens = self._lengths(input_ids, attention_mask)
                self._feed_paged(past, input_ids, torch.full((B,), S, device=dev) if lens is None else lens)
            elif (past.width if past.width is not None else 0) + S + max_new_tokens > past.cache.Smax:
                raise ValueError(f"generate(past=): {S} new columns + {max_new_tokens} tokens do not fit the cache of "
                                 f"{past.cache.Smax} rows after {past.width or 0} cached columns")
            else:
                self.extend(past, input_ids, counts=self._lengths(input_ids, attention_mask))
            state = past
        elif graph:
            dec = self._graphed_decoder(B, S + max_new_tokens, max_new_tokens, dev, kv_cache, weights)
            return dec.generate(self, input_ids, attention_mask,
                                self._sampler_params(temperature, top_k, top_p, eos_id, seed))
        else:
            state = self.prefill(input_ids, attention_mask, max_len=S + max_new_tokens, kv_cache=kv_cache, pool=pool,
                                 weights=weights)
        try:
            if sampler == "device":
                st = self._new_sampler(B, max_new_tokens, dev, temperature, top_k, top_p, eos_id, seed)
                return self._device_sampler_loop(lambda: self.decode_step(state),
                                                 lambda tok: self.decode_step(state, tok), st, max_new_tokens,
                                                 return_logits)
            return self._generate_loop(lambda: self.decode_step(state), lambda tok: self.decode_step(state, tok), B,
                                       dev, max_new_tokens, temperature, top_k, eos_id, seed, return_logits)
        finally:
            if pool is not None and past is None:  # the state made here; a caller's state stays the caller's
                state.release()

    @torch.no_grad()
    def decode_logits_reference(self, ids, lens):
        """fp32 logits [B, V] at every sequence's last real token from the uncached fp32 ``forward_reference``
        over the whole ``ids`` [B, W] (``lens`` [B]): the oracle of ``decode_step``."""
        B, W = ids.shape
        lens = lens.to(ids.device)
        hidden = self.forward_reference_hidden(ids, lens.to(torch.int32), None, None, None, full=True)
        if self._pack(ids, lens, None) is not None:  # unpad: packed rows, sequence b ends at cumsum(lens)[b] - 1
            rows = torch.cumsum(lens.long().clamp(1, W), 0) - 1
        else:
            rows = self._last_rows(lens, B, W, ids.device)
        return self.mlm_logits(hidden.float(), rows)

    @torch.no_grad()
    def generate_reference(self, input_ids, max_new_tokens: int, attention_mask=None, temperature: float = 0.0,
                           top_k: Optional[int] = None, eos_id: Optional[int] = None, seed: Optional[int] = None,
                           return_logits: bool = False, top_p: Optional[float] = None, sampler: Optional[str] = None,
                           kv_cache: Optional[str] = None, weights: Optional[str] = None):
        """``generate`` without any cache: ``forward_reference`` over the growing sequence, once per token.
        ``kv_cache`` and ``weights`` are checked as ``generate`` checks them and change nothing here: there is no
        cache and no decode step to quantise, so this stays the unquantised oracle of every format."""
        self._check_generate(input_ids, max_new_tokens, temperature, top_k, top_p, sampler, kv_cache=kv_cache,
                             weights=weights)
        B, S = input_ids.shape
        dev = input_ids.device
        lens = self._lengths(input_ids, attention_mask)
        lens = torch.full((B,), S, dtype=torch.int64, device=dev) if lens is None else lens.long()
        ids = torch.cat((input_ids, torch.zeros(B, max_new_tokens, dtype=input_ids.dtype, device=dev)), 1)
        ar = torch.arange(B, device=dev)
        grown = [0]

        def step(tok):
            ids[ar, lens + grown[0]] = tok.to(ids.dtype)
            grown[0] += 1
            return self.decode_logits_reference(ids[:, :S + grown[0]], lens + grown[0])

        if sampler == "device":
            st = self._new_sampler(B, max_new_tokens, dev, temperature, top_k, top_p, eos_id, seed)
            return self._device_sampler_loop(lambda: self.decode_logits_reference(input_ids, lens), step, st,
                                             max_new_tokens, return_logits)
        return self._generate_loop(lambda: self.decode_logits_reference(input_ids, lens), step, B, dev,
                                   max_new_tokens, temperature, top_k, eos_id, seed, return_logits)


class GraphedDecoder:
    """One captured decode loop body of a ``BertLMHeadModel`` for a fixed ``(B, Smax, T, device)``, and everything
    the capture baked addresses of: the key/value cache (bf16, or codes + scales under ``kv_cache="fp8"``, which is
    part of the decoder's key; ``prefill(cache=)`` refills it in place), the
    ``SamplerState`` (``set_params`` / ``reset`` rewrite it in place) and, inside the graph's own memory pool, the
    hidden rows and the logits buffer of a step. The body is ``decode_step(state, sampler.next_ids)`` followed by
    ``sample_step`` on the logits it returns: token t's sampling closes replay t, so a generation is one eager
    ``sample_step`` on the prompt's logits and ``T - 1`` replays. Captured on ONE side stream after one eager run
    of the body on it: the graph is a linear chain of kernel nodes, no branches. ``signature`` is the model's
    ``_decode_signature()`` at capture; the model recaptures when it no longer matches. ``MLT_DECODE_GEMM`` and
    ``MLT_DECODE_SPLIT`` (``ops.decode.decode_attn_path``: the split attention's two launches and its workspace are then
    nodes and pool memory of the graph) are read while capturing. Not supported: ``return_logits``, a graph for ``prefill``."""

    def __init__(self, model, B, Smax, T, dev, signature, kv_cache=None, weights=None):
        import time
        from ml_trainer_amd.ops import decode as DC
        c = model.config
        self.signature = signature
        self.B, self.Smax, self.T = B, Smax, T
        self.kv_cache, self.weights = kv_cache, weights
        self.cache = DC.KVCache.allocate(c.layers, B, c.num_kv_heads, Smax, dev, kv_cache=kv_cache)
        self.sampler = DC.SamplerState.allocate(B, T, dev)
        self.state = DC.DecodeState(self.cache, None, weights=weights)
        self.graph = None
        self.capture_seconds = 0.0
        if T < 2:
            return  # a single token is the eager sample_step alone
        V = c.vocab_size

        def body():
            DC.sample_step(model.decode_step(self.state, self.sampler.next_ids), V, self.sampler)

        # The zeroed cache and sampler are a valid state (token 0 at position 0, column 0): the eager run warms the
        # bf16 weight copies (the fp8 weight rows under weights="fp8", whose quantiser copies between host and device
        # and must not run inside a capture) and the allocator, the capture records the same launches. Both leave marks in the
        # state; every generation starts by resetting it.
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            body()
        torch.cuda.current_stream(dev).wait_stream(stream)
        self.sampler.reset()
        self.cache.pos.zero_()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=stream):
            body()
        torch.cuda.synchronize(dev)
        self.capture_seconds = time.perf_counter() - t0

    def start(self, model, input_ids, attention_mask, params):
        """Everything before the token loop: the sampler reset and given ``params`` (``SamplerState.set_params``
        arguments), the prompt prefilled into the captured cache. Returns the prompt's logits."""
        self.sampler.reset()
        self.sampler.set_params(**params)
        return model.decode_step(model.prefill(input_ids, attention_mask, max_len=self.Smax, cache=self.cache,
                                               kv_cache=self.kv_cache, weights=self.weights))

    def run(self, model, first_logits):
        """The token loop: one eager ``sample_step`` on the prompt's logits, then ``T - 1`` replays. Results are in
        ``self.sampler`` (``tokens``, ``lengths``), which the next generation overwrites."""
        from ml_trainer_amd.ops import decode as DC
        DC.sample_step(first_logits, model.config.vocab_size, self.sampler)
        for _ in range(self.T - 1):
            self.graph.replay()

    def generate(self, model, input_ids, attention_mask, params):
        self.run(model, self.start(model, input_ids, attention_mask, params))
        return self.sampler.tokens.clone(), self.sampler.lengths.clone()
