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
step reads anything back. On the CPU the same runs in fp32 torch with an fp32 cache;
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
post-norm RMSNorm, RMSNorm for ``emb_ln`` / ``mlm_ln``, gated FFNs, the norm fused into a GEMM prologue.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn


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


class BertLayer(nn.Module):
    def __init__(self, c: BertConfig):
        super().__init__()
        h = c.hidden
        self.c = c
        self.qkv = nn.Linear(h, 3 * h)
        self.out = nn.Linear(h, h)
        self.ln1 = block_norm(c)
        self.ffn1 = nn.Linear(h, c.intermediate)
        self.ffn2 = nn.Linear(c.intermediate, h)
        self.ln2 = block_norm(c)

    def forward_native(self, x, lens, B, S, drop=None, attn_drop=None, cu_seqlens=None, rope=None):
        """``drop`` = (p, seed, site of the attention sub-layer, rank); the FFN takes the next site.
        ``attn_drop`` = (p, seed, attention site of this layer, rank): attention-probability dropout.
        ``cu_seqlens``: x is a packed [T, h] batch (S = max_seqlen, lens unused).
        ``rope`` = (table, pos or None): rotary positions (``ops.transformer.attention_block``)."""
        from ml_trainer_amd.ops import transformer as T
        if self.c.fp8:
            from ml_trainer_amd.ops.fp8 import FP8 as impl
        else:
            impl = T.BF16
        x = T.attention_ln_block(x, self.qkv.weight, self.qkv.bias, self.out.weight, self.out.bias, self.ln1.weight,
                                 self.ln1.bias, lens, B, S, self.c.heads, self.c.ln_eps, impl, drop, attn_drop,
                                 cu_seqlens, self.c.causal, rope)
        if drop is not None:
            drop = (drop[0], drop[1], drop[2] + 1, drop[3])
        return T.ffn_ln_block(x, self.ffn1.weight, self.ffn1.bias, self.ffn2.weight, self.ffn2.bias, self.ln2.weight,
                              self.ln2.bias, self.c.ln_eps, impl, drop)

    def forward_native_pre(self, h, n, next_norm, lens, B, S, drop=None, attn_drop=None, cu_seqlens=None, rope=None):
        """The pre-norm layer on the native kernels: (h, n = ln1(h)) -> (h', n' = next_norm(h')), where
        ``next_norm`` is the next layer's ``ln1`` or the model's ``final_ln``. Arguments as in forward_native."""
        from ml_trainer_amd.ops import transformer as T
        eps = self.c.ln_eps
        h, n = T.pre_attention_block(h, n, self.qkv.weight, self.qkv.bias, self.out.weight, self.out.bias,
                                     self.ln2.weight, self.ln2.bias, lens, B, S, self.c.heads, eps, T.BF16, drop,
                                     attn_drop, cu_seqlens, self.c.causal, rope)
        if drop is not None:
            drop = (drop[0], drop[1], drop[2] + 1, drop[3])
        return T.pre_ffn_block(h, n, self.ffn1.weight, self.ffn1.bias, self.ffn2.weight, self.ffn2.bias,
                               next_norm.weight, next_norm.bias, eps, T.BF16, drop)

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
        f = self.ffn2(F.gelu(self.ffn1(self.ln2(x) if c.pre_ln else x)))
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
        if c.unpad and c.fp8:
            raise ValueError("unpad=True with fp8=True is not supported: the fp8 attention epilogue writes 16-row "
                             "transposed runs at b * S offsets and cannot take packed row offsets")
        if c.causal and c.fp8:
            raise ValueError("causal=True with fp8=True is not supported: the fp8 (q8) attention epilogue has no "
                             "causal instantiation")
        if c.rotary and c.fp8:
            raise ValueError("rotary=True with fp8=True is not supported: the fp8 attention backward writes dQKV as "
                             "e5m2, which the inverse rotation cannot take")
        if c.norm not in ("layernorm", "rmsnorm"):
            raise ValueError(f"norm must be 'layernorm' or 'rmsnorm', got {c.norm!r}")
        if c.norm == "rmsnorm" and not c.pre_ln:
            raise ValueError("norm='rmsnorm' needs pre_ln=True: post-norm RMSNorm blocks are not built")
        if (c.pre_ln or c.norm != "layernorm") and c.fp8:
            raise ValueError("pre_ln=True / norm='rmsnorm' with fp8=True is not supported: the pre-norm blocks run "
                             "the bf16 linears only")
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

    def _rope(self, pos=None):
        """The ``rope`` argument of the native attention blocks: (table, packed positions or None), or None."""
        return (self.rope_table, pos) if self.config.rotary else None

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

    def _pre_stack_native(self, x, lens, B, S, drop, adrop, cu=None, rope=None):
        """The pre-norm layers on the native kernels from the embedding output ``x`` (the first stream):
        ``final_ln`` of the last stream, [rows, h] bf16."""
        from ml_trainer_amd.ops import transformer as T
        h, n = T.stream_norm(x, *_norm_args(self.layers[0].ln1))
        last = len(self.layers) - 1
        for l, layer in enumerate(self.layers):
            nxt = self.final_ln if l == last else self.layers[l + 1].ln1
            h, n = layer.forward_native_pre(h, n, nxt, lens, B, S, self._site(drop, 1 + 2 * l),
                                            self._attn_site(adrop, l), cu, rope)
        return n

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
    def _attn_site(cls, adrop, l):
        from ml_trainer_amd.ops.dropout import attention_site
        return cls._site(adrop, attention_site(l))

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
        B, S = input_ids.shape
        lens = self._lengths(input_ids, attention_mask)
        drop, adrop = self._dropout(dropout_seed)
        if input_ids.is_cuda:
            from ml_trainer_amd.ops import transformer as T
            if self.config.fp8 and torch.is_grad_enabled():
                from ml_trainer_amd.ops.fp8 import context
                context(input_ids.device).update()  # delayed scaling: fold last step's amaxes
            pk = self._pack(input_ids, lens, token_type_ids, T.PACK_ROW_MULTIPLE)
            if pk is not None:
                return self._forward_native_packed(pk, drop, adrop)
            x = self._encode_native(input_ids, lens, token_type_ids, drop, adrop)
            cls = x.view(B, S, -1)[:, 0]  # strided row view: the pooler GEMM reads it in place
            if cls.shape[1] % 8 == 0 and self.pooler.weight.shape[0] % 8 == 0:
                return T.classifier_head(cls, self.pooler.weight, self.pooler.bias, self.classifier.weight,
                                         self.classifier.bias)
            cls = cls.float()
        else:
            cls = self.forward_reference_hidden(input_ids, lens, token_type_ids, drop, adrop)
        pooled = torch.tanh(self.pooler(cls))
        return self.classifier(pooled)

    def _encode_native(self, input_ids, lens, token_type_ids, drop, adrop):
        """The native encoder on a padded [B, S] batch: the last layer's hidden states [B * S, h] bf16."""
        from ml_trainer_amd.ops import transformer as T
        B, S = input_ids.shape
        x = T.embeddings(input_ids, token_type_ids, self.word_embeddings.weight, self._pos_weight(),
                         self.token_type_embeddings.weight, S)
        x = T.layer_norm(x, self.emb_ln.weight, self.emb_ln.bias, self.config.ln_eps)
        if drop is not None:
            x = T.dropout(x, *self._site(drop, 0))
        rope = self._rope()
        if self.config.pre_ln:
            return self._pre_stack_native(x, lens, B, S, drop, adrop, None, rope)
        for l, layer in enumerate(self.layers):
            x = layer.forward_native(x, lens, B, S, self._site(drop, 1 + 2 * l), self._attn_site(adrop, l), rope=rope)
        return x

    def _encode_native_packed(self, pk, drop, adrop):
        """The native encoder on a PackedBatch: [rows, h] throughout (the T tokens, then the inert tail rows
        that round the count up to the GEMMs' 256-row tile)."""
        from ml_trainer_amd.ops import transformer as T
        B, S, cu = pk.batch, pk.max_seqlen, pk.cu_seqlens
        x = T.embeddings(pk.ids, pk.tt, self.word_embeddings.weight, self._pos_weight(),
                         self.token_type_embeddings.weight, S, pos=pk.pos, cu_seqlens=cu)
        x = T.layer_norm(x, self.emb_ln.weight, self.emb_ln.bias, self.config.ln_eps)
        if drop is not None:
            x = T.dropout(x, *self._site(drop, 0))
        rope = self._rope(pk.pos)
        if self.config.pre_ln:
            return self._pre_stack_native(x, None, B, S, drop, adrop, cu, rope)
        for l, layer in enumerate(self.layers):
            x = layer.forward_native(x, None, B, S, self._site(drop, 1 + 2 * l), self._attn_site(adrop, l), cu, rope)
        return x

    def _forward_native_packed(self, pk, drop, adrop):
        """The native path on a PackedBatch, CLS rows at cu_seqlens[:-1]."""
        from ml_trainer_amd.ops import transformer as T
        x = self._encode_native_packed(pk, drop, adrop)
        cls = x.index_select(0, pk.cls_rows)  # contiguous [B, h]
        if cls.shape[1] % 8 == 0 and self.pooler.weight.shape[0] % 8 == 0:
            return T.classifier_head(cls, self.pooler.weight, self.pooler.bias, self.classifier.weight,
                                     self.classifier.bias)
        return self.classifier(torch.tanh(self.pooler(cls.float())))

    def _reference_hidden_packed(self, pk, lens, drop, adrop, full=False):
        B, S = pk.batch, pk.max_seqlen
        tt = pk.tt if pk.tt is not None else torch.zeros_like(pk.ids)
        x = self.emb_ln(self._embed_torch(pk.ids, tt, pk.pos.long()))
        if drop is not None:
            from ml_trainer_amd.ops import dropout as D
            x = D.apply(x, *self._site(drop, 0))
        mask = torch.arange(S, device=x.device)[None, :] < lens.to(x.device).clamp(1, S)[:, None]
        for l, layer in enumerate(self.layers):
            x = layer.forward_reference(x, mask, B, S, self._site(drop, 1 + 2 * l), self._attn_site(adrop, l), pk,
                                        self.rope_table)
        x = self._final_norm(x)
        return x if full else x.index_select(0, pk.cls_rows)

    def forward_reference_hidden(self, input_ids, lens=None, token_type_ids=None, drop=None, adrop=None, full=False):
        """The CLS rows [B, h] of the fp32 torch encoder; ``full``: every row, [B * S, h] (packed: [T, h])."""
        B, S = input_ids.shape
        pk = self._pack(input_ids, lens, token_type_ids)
        if pk is not None:
            return self._reference_hidden_packed(pk, lens, drop, adrop, full)
        pos = torch.arange(S, device=input_ids.device)
        tt = token_type_ids if token_type_ids is not None else torch.zeros_like(input_ids)
        x = self.emb_ln(self._embed_torch(input_ids, tt, pos, per_batch=True)).view(B * S, -1)
        if drop is not None:
            from ml_trainer_amd.ops import dropout as D
            x = D.apply(x, *self._site(drop, 0))
        mask = None
        if lens is not None:
            mask = torch.arange(S, device=input_ids.device)[None, :] < lens.to(input_ids.device)[:, None]
        for l, layer in enumerate(self.layers):
            x = layer.forward_reference(x, mask, B, S, self._site(drop, 1 + 2 * l), self._attn_site(adrop, l),
                                        rope=self.rope_table)
        x = self._final_norm(x)
        return x if full else x.view(B, S, -1)[:, 0]

    def forward_reference(self, input_ids, attention_mask=None, token_type_ids=None, dropout_seed=None):
        lens = self._lengths(input_ids, attention_mask)
        cls = self.forward_reference_hidden(input_ids, lens, token_type_ids, *self._dropout(dropout_seed))
        return self.classifier(torch.tanh(self.pooler(cls)))

    def forward_torch_bf16(self, input_ids, attention_mask=None, token_type_ids=None, dropout_seed=None):
        with torch.autocast(input_ids.device.type, dtype=torch.bfloat16):
            x, pk = self._hidden_torch_bf16(input_ids, attention_mask, token_type_ids, dropout_seed)
            cls = x[:, 0] if pk is None else x[0].index_select(0, pk.cls_rows)
            return self.classifier(torch.tanh(self.pooler(cls.float())))

    def _hidden_torch_bf16(self, input_ids, attention_mask=None, token_type_ids=None, dropout_seed=None):
        """PyTorch-eager bf16 path on the same weights (torch.autocast + SDPA + hipBLASLt): the
        baseline the native kernels are benchmarked and error-budgeted against. Hidden dropout
        uses the native path's masks (ops.dropout), each applied in the dtype autocast gives the
        tensor it drops. With attention dropout active the attention is computed explicitly under
        autocast (softmax -> * keep * scale -> @ v) instead of through SDPA, which cannot take our mask.
        Under ``pre_ln`` the residual stream is rounded to bf16 after every add, as the native path stores it.
        Returns (hidden [B, S, h] -- packed: [1, T, h] --, the PackedBatch or None); the callers add their head."""
        from ml_trainer_amd.ops import dropout as D
        c = self.config
        drop, adrop = self._dropout(dropout_seed)

        def dropped(t, site):  # t [B, S, h] (unpad: [1, T, h]), masks indexed by row
            return t if drop is None else D.apply(t.reshape(-1, t.shape[-1]), *self._site(drop, site)).view(t.shape)

        B, S = input_ids.shape
        lens = self._lengths(input_ids, attention_mask)
        pk = self._pack(input_ids, lens, token_type_ids)
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
            if pk is None:
                pos = torch.arange(S, device=input_ids.device)
                tt = token_type_ids if token_type_ids is not None else torch.zeros_like(input_ids)
                x = self._embed_torch(input_ids, tt, pos, per_batch=True)
            else:  # the packed rows as a batch of one: x [1, T, h]; attention on a padded scratch of the QKV rows
                tt = pk.tt if pk.tt is not None else torch.zeros_like(pk.ids)
                x = self._embed_torch(pk.ids, tt, pk.pos.long())[None]
            x = dropped(self.emb_ln(x), 0)
            if c.pre_ln:
                x = x.to(torch.bfloat16)
            for l, L in enumerate(self.layers):
                qkv = L.qkv(L.ln1(x) if c.pre_ln else x)
                if pk is not None:
                    qkv = unpack_rows(qkv[0], pk)
                qkv = qkv.view(B, S, 3, c.heads, 64).permute(2, 0, 3, 1, 4)
                if c.rotary:  # fp32 rotation of the (bf16) q and k, rounded back as the native path stores them
                    from ml_trainer_amd.ops.rope import rotate
                    cs = self.rope_table[:S]
                    qkv = torch.stack((rotate(qkv[0], cs).to(qkv.dtype), rotate(qkv[1], cs).to(qkv.dtype), qkv[2]))
                if adrop is None:
                    ctx = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2], attn_mask=mask, is_causal=causal)
                else:
                    pa, seed, site, rank = self._attn_site(adrop, l)
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
                    x = (dropped(L.out(ctx), 1 + 2 * l) + x).to(torch.bfloat16)
                    x = (dropped(L.ffn2(F.gelu(L.ffn1(L.ln2(x)))), 2 + 2 * l) + x).to(torch.bfloat16)
                    continue
                x = L.ln1(dropped(L.out(ctx), 1 + 2 * l) + x)
                x = L.ln2(dropped(L.ffn2(F.gelu(L.ffn1(x))), 2 + 2 * l) + x)
            return self._final_norm(x), pk

    def num_parameters(self) -> int:
        return sum(p.numel() for p in self.parameters())

    def flops_per_token(self, seq_len: int) -> float:
        """Training FLOPs per token (fwd + bwd = 3x fwd) of the encoder stack."""
        c = self.config
        h, f = c.hidden, c.intermediate
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
        B, S = input_ids.shape
        lens = self._lengths(input_ids, attention_mask)
        drop, adrop = self._dropout(dropout_seed)
        if not input_ids.is_cuda:
            return self._hidden_reference(input_ids, lens, token_type_ids, drop, adrop)
        from ml_trainer_amd.ops import transformer as T
        pk = self._pack(input_ids, lens, token_type_ids, T.PACK_ROW_MULTIPLE)
        if pk is not None:
            self._last_batch = (B, S, None, pk.cu_seqlens)
            return self._encode_native_packed(pk, drop, adrop)
        self._last_batch = (B, S, lens, None)
        return self._encode_native(input_ids, lens, token_type_ids, drop, adrop)

    def _hidden_reference(self, input_ids, lens, token_type_ids, drop, adrop):
        B, S = input_ids.shape
        pk = self._pack(input_ids, lens, token_type_ids)
        self._last_batch = (B, S, lens if pk is None else None, None if pk is None else pk.cu_seqlens)
        return self.forward_reference_hidden(input_ids, lens, token_type_ids, drop, adrop, full=True)

    def forward_reference(self, input_ids, attention_mask=None, token_type_ids=None, dropout_seed=None):
        """The hidden states in fp32 torch on any device (the numerics oracle of ``forward``)."""
        lens = self._lengths(input_ids, attention_mask)
        return self._hidden_reference(input_ids, lens, token_type_ids, *self._dropout(dropout_seed))

    def forward_torch_bf16(self, input_ids, attention_mask=None, token_type_ids=None, dropout_seed=None):
        """The hidden states of the PyTorch-eager bf16 baseline, [B * S, h] (packed: [T, h])."""
        B, S = input_ids.shape
        with torch.autocast(input_ids.device.type, dtype=torch.bfloat16):
            x, pk = self._hidden_torch_bf16(input_ids, attention_mask, token_type_ids, dropout_seed)
        lens = self._lengths(input_ids, attention_mask)
        self._last_batch = (B, S, lens if pk is None else None, None if pk is None else pk.cu_seqlens)
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
    def prefill(self, input_ids, attention_mask=None, max_len: Optional[int] = None, cache=None):
        """Run the prompt ``input_ids`` [B, S] (right-padded; lengths from ``attention_mask`` or ``pad_id``)
        through the padded causal forward, layer by layer, keep every layer's K / V in a cache of ``max_len``
        rows per sequence (default ``config.max_position``) and return the ``DecodeState``: the cache with
        ``pos = lens`` and the hidden row of each sequence's last real token. No gradients and no dropout,
        whatever mode the model is in; ``config.unpad`` has no effect (prompts are short). ``cache``: an existing
        ``KVCache`` of this shape to fill in place (its ``pos`` is overwritten with ``pos.copy_``, its tensors keep
        their addresses: what a captured decode step needs) instead of a new one."""
        from ml_trainer_amd.ops import decode as DC
        c = self.config
        B, S = input_ids.shape
        Smax = c.max_position if max_len is None else int(max_len)
        if not S <= Smax <= c.max_position:
            raise ValueError(f"prefill: prompt width {S} <= max_len {Smax} <= max_position {c.max_position} "
                             f"does not hold")
        dev = input_ids.device
        lens = self._lengths(input_ids, attention_mask)
        if cache is None:
            cache = DC.KVCache.allocate(c.layers, B, c.heads, Smax, dev)
        elif (cache.Smax != Smax or len(cache.kv) != c.layers or cache.pos.device != dev or
              tuple(cache.kv[0].shape) != (2, B, c.heads, Smax, DC.HEAD_DIM)):
            raise ValueError(f"prefill: the given cache does not hold {c.layers} layers of [2, {B}, {c.heads}, {Smax}, "
                             f"{DC.HEAD_DIM}] on {dev}")
        if input_ids.is_cuda:
            from ml_trainer_amd.ops import transformer as T
            x = T.embeddings(input_ids, None, self.word_embeddings.weight, self._pos_weight(),
                             self.token_type_embeddings.weight, S)
            x, _ = T._ln_fwd(x, self.emb_ln.weight, self.emb_ln.bias, c.ln_eps)
            for l, L in enumerate(self.layers):
                if c.pre_ln:  # x is the stream; the cache holds the K / V of its norm
                    n, _ = T._norm_fwd(x, *_norm_args(L.ln1))
                    x, (_, qkv, _, _) = T._attn_fwd(n, L.qkv.weight, L.qkv.bias, L.out.weight, L.out.bias, lens, B, S,
                                                    c.heads, causal=True, rope=self._rope(), res=x)
                    DC.fill_from_prefill(cache, l, qkv, lens, B, S)
                    n, _ = T._norm_fwd(x, *_norm_args(L.ln2))
                    x, _ = T._ffn_fwd(n, L.ffn1.weight, L.ffn1.bias, L.ffn2.weight, L.ffn2.bias, res=x)
                    continue
                a, (_, qkv, _, _) = T._attn_fwd(x, L.qkv.weight, L.qkv.bias, L.out.weight, L.out.bias, lens, B, S,
                                                c.heads, causal=True, rope=self._rope())  # (qkv: rotated under rotary)
                DC.fill_from_prefill(cache, l, qkv, lens, B, S)
                x, _ = T._ln_fwd(a, L.ln1.weight, L.ln1.bias, c.ln_eps)
                f, _ = T._ffn_fwd(x, L.ffn1.weight, L.ffn1.bias, L.ffn2.weight, L.ffn2.bias)
                x, _ = T._ln_fwd(f, L.ln2.weight, L.ln2.bias, c.ln_eps)
        else:
            pos = torch.arange(S, device=dev)
            x = self._embed_torch(input_ids, torch.zeros_like(input_ids), pos, per_batch=True)
            x = self.emb_ln(x).view(B * S, -1)
            mask = None if lens is None else pos[None, :] < lens[:, None]
            for l, L in enumerate(self.layers):
                qkv = L.qkv(L.ln1(x) if c.pre_ln else x)
                if c.rotary:  # the cache holds rotated keys
                    from ml_trainer_amd.ops.rope import rope_qk_reference
                    qkv = rope_qk_reference(qkv, self.rope_table, c.heads, S)
                DC.fill_from_prefill(cache, l, qkv, lens, B, S)
                x = L.forward_reference(x, mask, B, S, rope=self.rope_table)
        cache.pos.copy_(lens if lens is not None else torch.full((B,), S, dtype=torch.int32, device=dev))
        x = x.index_select(0, self._last_rows(lens, B, S, dev))
        if c.pre_ln:  # rows are independent: the final norm of the last real rows only
            if x.is_cuda:
                from ml_trainer_amd.ops import transformer as T
                x, _ = T._norm_fwd(x, *_norm_args(self.final_ln))
            else:
                x = self.final_ln(x)
        return DC.DecodeState(cache, x)

    def _state_logits(self, state):
        from ml_trainer_amd.ops import decode as DC
        from ml_trainer_amd.ops import mlm as M
        B, h = state.hidden.shape
        Vp = M._round_up(self.config.vocab_size, M.VOCAB_MULTIPLE)
        if (state.hidden.is_cuda and state.hidden.dtype == torch.bfloat16 and
                DC.decode_linear_path(B, h, h) == "skinny" and DC.decode_linear_path(B, Vp, h) == "skinny"):
            return M.decode_logits(state.hidden, self.mlm_params())  # B rows, no gather into a 256-row tile
        return self.mlm_logits(state.hidden, torch.arange(B, device=state.hidden.device))

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
        ids = token_ids.reshape(-1).to(torch.int64).contiguous()
        B = ids.numel()
        if ids.is_cuda:
            from ml_trainer_amd.ops import transformer as T
            C = T.require_native()
            x = torch.empty(B, c.hidden, dtype=torch.bfloat16, device=ids.device)
            C.embed_fwd(ids, None, T.bf16_weight(self.word_embeddings.weight),
                        None if c.rotary else T.bf16_weight(self.position_embeddings.weight),
                        T.bf16_weight(self.token_type_embeddings.weight), x, cache.Smax, pos=cache.pos)
            x, _ = T._ln_fwd(x, self.emb_ln.weight, self.emb_ln.bias, c.ln_eps)
            for l, L in enumerate(self.layers):
                if c.pre_ln:  # x is the stream
                    n, _ = T._norm_fwd(x, *_norm_args(L.ln1))
                    qkv = DC.linear_small(n, T.bf16_weight(L.qkv.weight), L.qkv.bias)
                    ctx = DC.attn_decode(qkv, cache.kv[l], cache.pos, c.heads, rope=self.rope_table)
                    x = DC.linear_small(ctx, T.bf16_weight(L.out.weight), L.out.bias, res=x)
                    n, _ = T._norm_fwd(x, *_norm_args(L.ln2))
                    pre = torch.empty(B, L.ffn1.weight.shape[0], dtype=torch.bfloat16, device=x.device)
                    g = DC.linear_small(n, T.bf16_weight(L.ffn1.weight), L.ffn1.bias, gelu_aux=pre)
                    x = DC.linear_small(g, T.bf16_weight(L.ffn2.weight), L.ffn2.bias, res=x)
                    continue
                qkv = DC.linear_small(x, T.bf16_weight(L.qkv.weight), L.qkv.bias)
                ctx = DC.attn_decode(qkv, cache.kv[l], cache.pos, c.heads, rope=self.rope_table)
                a = DC.linear_small(ctx, T.bf16_weight(L.out.weight), L.out.bias, res=x)
                x, _ = T._ln_fwd(a, L.ln1.weight, L.ln1.bias, c.ln_eps)
                pre = torch.empty(B, L.ffn1.weight.shape[0], dtype=torch.bfloat16, device=x.device)
                g = DC.linear_small(x, T.bf16_weight(L.ffn1.weight), L.ffn1.bias, gelu_aux=pre)
                f = DC.linear_small(g, T.bf16_weight(L.ffn2.weight), L.ffn2.bias, res=x)
                x, _ = T._ln_fwd(f, L.ln2.weight, L.ln2.bias, c.ln_eps)
            if c.pre_ln:  # state.hidden holds the normed rows, as after a post-LN layer
                x, _ = T._norm_fwd(x, *_norm_args(self.final_ln))
        else:
            x = self.emb_ln(self._embed_torch(ids, torch.zeros_like(ids), cache.pos.long()))
            for l, L in enumerate(self.layers):
                if c.pre_ln:
                    ctx = DC.attn_decode_reference(L.qkv(L.ln1(x)), cache.kv[l], cache.pos, c.heads,
                                                   rope=self.rope_table)
                    x = L.out(ctx) + x
                    x = L.ffn2(F.gelu(L.ffn1(L.ln2(x)))) + x
                    continue
                ctx = DC.attn_decode_reference(L.qkv(x), cache.kv[l], cache.pos, c.heads, rope=self.rope_table)
                x = L.ln1(L.out(ctx) + x)
                x = L.ln2(L.ffn2(F.gelu(L.ffn1(x))) + x)
            x = self._final_norm(x)
        cache.pos.add_(1)
        state.hidden = x
        return self._state_logits(state)

    def _check_generate(self, input_ids, max_new_tokens, temperature, top_k, top_p=None, sampler=None, graph=False,
                        return_logits=False):
        S = input_ids.shape[1]
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

    def _decode_signature(self):
        """What a captured decode step baked in of the parameters: an in-place edit bumps ``_version`` (and makes
        ``bf16_weight`` / ``padded_decoder`` hand out new tensors), a re-allocation moves ``data_ptr``."""
        c = self.config  # (the block kind decides which kernels a step launches)
        return (c.pre_ln, c.norm) + tuple((p._version, p.data_ptr()) for p in self.parameters())

    def _graphed_decoder(self, B, Smax, T, dev):
        key = (B, Smax, T, str(dev))
        decoders = self.__dict__.setdefault("_graphed_decoders", {})
        dec = decoders.get(key)
        sig = self._decode_signature()
        if dec is None or dec.signature != sig:
            decoders.pop(key, None)  # free the stale graph's buffers before the new capture
            del dec
            dec = decoders[key] = GraphedDecoder(self, B, Smax, T, dev, sig)
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
                 graph: bool = False):
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
        of a shape and again after a parameter changed, and ``MLT_DECODE_GEMM`` is read when it is captured."""
        self._check_generate(input_ids, max_new_tokens, temperature, top_k, top_p, sampler, graph, return_logits)
        B, S = input_ids.shape
        dev = input_ids.device
        if graph:
            dec = self._graphed_decoder(B, S + max_new_tokens, max_new_tokens, dev)
            return dec.generate(self, input_ids, attention_mask,
                                self._sampler_params(temperature, top_k, top_p, eos_id, seed))
        state = self.prefill(input_ids, attention_mask, max_len=S + max_new_tokens)
        if sampler == "device":
            st = self._new_sampler(B, max_new_tokens, dev, temperature, top_k, top_p, eos_id, seed)
            return self._device_sampler_loop(lambda: self.decode_step(state), lambda tok: self.decode_step(state, tok),
                                             st, max_new_tokens, return_logits)
        return self._generate_loop(lambda: self.decode_step(state), lambda tok: self.decode_step(state, tok), B,
                                   dev, max_new_tokens, temperature, top_k, eos_id, seed, return_logits)

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
                           return_logits: bool = False, top_p: Optional[float] = None, sampler: Optional[str] = None):
        """``generate`` without any cache: ``forward_reference`` over the growing sequence, once per token."""
        self._check_generate(input_ids, max_new_tokens, temperature, top_k, top_p, sampler)
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
    the capture baked addresses of: the key/value cache (``prefill(cache=)`` refills it in place), the
    ``SamplerState`` (``set_params`` / ``reset`` rewrite it in place) and, inside the graph's own memory pool, the
    hidden rows and the logits buffer of a step. The body is ``decode_step(state, sampler.next_ids)`` followed by
    ``sample_step`` on the logits it returns: token t's sampling closes replay t, so a generation is one eager
    ``sample_step`` on the prompt's logits and ``T - 1`` replays. Captured on ONE side stream after one eager run
    of the body on it: the graph is a linear chain of kernel nodes, no branches. ``signature`` is the model's
    ``_decode_signature()`` at capture; the model recaptures when it no longer matches. ``MLT_DECODE_GEMM`` is
    read while capturing. Not supported: ``return_logits``, a graph for ``prefill``."""

    def __init__(self, model, B, Smax, T, dev, signature):
        import time
        from ml_trainer_amd.ops import decode as DC
        c = model.config
        self.signature = signature
        self.B, self.Smax, self.T = B, Smax, T
        self.cache = DC.KVCache.allocate(c.layers, B, c.heads, Smax, dev)
        self.sampler = DC.SamplerState.allocate(B, T, dev)
        self.state = DC.DecodeState(self.cache, None)
        self.graph = None
        self.capture_seconds = 0.0
        if T < 2:
            return  # a single token is the eager sample_step alone
        V = c.vocab_size

        def body():
            DC.sample_step(model.decode_step(self.state, self.sampler.next_ids), V, self.sampler)

        # The zeroed cache and sampler are a valid state (token 0 at position 0, column 0): the eager run warms the
        # bf16 weight copies and the allocator, the capture records the same launches. Both leave marks in the
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
        return model.decode_step(model.prefill(input_ids, attention_mask, max_len=self.Smax, cache=self.cache))

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
