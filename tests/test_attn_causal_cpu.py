"""Causal attention on the CPU: the masked bounds of tests/attn_causal_ref.py pinned to tests/helpers.py, a causal
emulation of the kernels inside them, off-by-one mutations of the diagonal outside them, the fp32 / fp64 reference
with ``BertConfig.causal``, and the causal language-model task (BertLMHeadModel, shift_labels, SyntheticCausalLM,
build_model / Trainer / main.py ``clm``).

The definition under test: key j of a sequence is visible to query i of the same sequence iff j <= i and j < len_b."""
import os
import pickle
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from ml_trainer_amd.data.text import SyntheticCausalLM, SyntheticMaskedLM
from ml_trainer_amd.models import build_model
from ml_trainer_amd.models.bert import (BertClassifier, BertConfig, BertForMaskedLM, BertLayer, BertLMHeadModel,
                                        bert_config, shift_labels)
from ml_trainer_amd.ops import dropout as D
from tests.attn_causal_ref import (attn_bwd_bound_masked, attn_fwd_bound_masked, causal_edge_inputs, causal_valid,
                                   emulate_masked, key_valid)
from tests.helpers import (ATTN_EDGE_DROPOUT_S, ATTN_EDGE_SHAPES, assert_within, attn_bwd_bound, attn_edge_inputs,
                           attn_fwd_bound, attn_heads, attn_split, store_bound)
from tests.test_attn_bound_cpu import CASES, RANK, SEED, SITE, emulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


# ------------------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("si", range(len(ATTN_EDGE_SHAPES)))
def test_masked_bounds_equal_the_helpers_with_the_key_padding_mask(si):
    """With `valid` = the plain key-padding mask the masked bounds ARE helpers.attn_fwd_bound / attn_bwd_bound:
    every returned tensor is torch.equal, without and (where the edge tests run it) with dropout."""
    B, S, H, lens, scale = ATTN_EDGE_SHAPES[si]
    qkv, dout = attn_edge_inputs(B, S, H, lens, scale, seed=100 + si)
    q, k, v = attn_split(qkv, B, S, H)
    do = attn_heads(dout, B, S, H)
    valid = key_valid(lens, B, S)
    for p in (0.0, 0.1) if S in ATTN_EDGE_DROPOUT_S else (0.0,):
        keep = D.attention_keep_mask(SEED, SITE, RANK, B, H, S, p) if p else None
        c = D.attention_scale(p) if p else 1.0
        e = emulate(qkv, dout, B, S, H, lens, scale, keep, c)
        want = attn_fwd_bound(q, k, v, lens, scale, keep, c)
        got = attn_fwd_bound_masked(q, k, v, valid, scale, keep, c)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        wb = attn_bwd_bound(q, k, v, do, e["o_b"].double(), e["lse"].double(), lens, scale, keep, c)
        gb = attn_bwd_bound_masked(q, k, v, do, e["o_b"].double(), e["lse"].double(), valid, scale, keep, c)
        assert set(wb) == set(gb)
        for name in wb:
            assert torch.equal(gb[name], wb[name]), name


_DATA = {}


def _case(si, p):
    """Inputs, keep mask, mask and forward reference of a causal case: made once, never modified."""
    if (si, p) not in _DATA:
        B, S, H, lens, scale = ATTN_EDGE_SHAPES[si]
        qkv, dout = causal_edge_inputs(B, S, H, lens, scale, seed=100 + si)
        keep = D.attention_keep_mask(SEED, SITE, RANK, B, H, S, p) if p else None
        c = D.attention_scale(p) if p else 1.0
        q, k, v = attn_split(qkv, B, S, H)
        valid = causal_valid(lens, B, S)
        _DATA[si, p] = (qkv, dout, keep, c, valid, attn_fwd_bound_masked(q, k, v, valid, scale, keep, c))
    return _DATA[si, p]


def _refs(si, p, e):
    B, S, H, lens, scale = ATTN_EDGE_SHAPES[si]
    qkv, dout, keep, c, valid, (O, tO, L, tL) = _case(si, p)
    q, k, v = attn_split(qkv, B, S, H)
    bw = attn_bwd_bound_masked(q, k, v, attn_heads(dout, B, S, H), e["o_b"].double(), e["lse"].double(), valid, scale,
                               keep, c)
    return dict(o=(O, tO), lse=(L, tL), delta=(bw["delta"], bw["t_delta"]), dq=(bw["dq"], bw["t_dq"]),
                dk=(bw["dk"], bw["t_dk"]), dv=(bw["dv"], bw["t_dv"]))


def _emulate_case(si, p, mut=None, off=None):
    B, S, H, lens, scale = ATTN_EDGE_SHAPES[si]
    qkv, dout, keep, c, valid, _ = _case(si, p)
    if mut is not None:
        valid = causal_valid(lens, B, S, mut)
    return emulate_masked(qkv, dout, B, S, H, valid, scale, keep, c, off=off)


@pytest.mark.parametrize("stale", [False, True])
@pytest.mark.parametrize("si,p", CASES)
def test_causal_emulation_within_bounds(si, p, stale):
    """Every element of every output of the causal emulation is within its masked bound, with the exact row
    maximum and with one stale by a random 0 .. 8 per row, at every edge shape (p = 0.1 at ATTN_EDGE_DROPOUT_S)."""
    B, S, H, lens, scale = ATTN_EDGE_SHAPES[si]
    off = 8.0 * torch.rand(B, H, S, 1, generator=torch.Generator().manual_seed(si)) if stale else None
    e = _emulate_case(si, p, off=off)
    ref = _refs(si, p, e)
    fig = {n: float(((e[n].double() - x).abs() / t).max()) for n, (x, t) in ref.items()}
    print(f"S={S} p={p} stale={stale}: " + " ".join(f"{n} {r:.3f}" for n, r in fig.items()))
    for name, (x, t) in ref.items():
        assert_within(e[name], x, t, f"emulated {name} (fp32)")
        if name + "_b" in e:
            assert_within(e[name + "_b"], x, store_bound(x, t, BF16), f"emulated {name} (bf16 store)")
    # what no query sees gets exact zeros: the keys at or past each length
    n = torch.full((B,), S) if lens is None else torch.tensor(lens)
    masked = (torch.arange(S)[None, :] >= n[:, None])[:, None, :, None]
    assert (e["dk_b"].float()[masked.expand_as(e["dk"])] == 0).all()
    assert (e["dv_b"].float()[masked.expand_as(e["dv"])] == 0).all()


@pytest.mark.parametrize("mut", ["causal_plus_1", "causal_minus_1"])
@pytest.mark.parametrize("si,p", [(si, p) for si, p in CASES if ATTN_EDGE_SHAPES[si][1] >= 2])
def test_diagonal_off_by_one_violates_a_bound(si, p, mut):
    """causal_plus_1 (key i + 1 visible) and causal_minus_1 (key i hidden for i >= 1), built into the emulation,
    each put at least one element of one STORED output outside its tolerance at every shape with S >= 2."""
    B, S, H, lens, scale = ATTN_EDGE_SHAPES[si]
    e = _emulate_case(si, p, mut=mut)
    ref = _refs(si, p, e)
    stored = {}
    for name, (x, t) in ref.items():
        if name in ("lse", "delta"):
            stored[name] = float(((e[name].double() - x).abs() / t).max())
        else:
            stored[name + "_b"] = float(((e[name + "_b"].double() - x).abs() / store_bound(x, t, BF16)).max())
    print(f"S={S} p={p} {mut}: " + " ".join(f"{n} {x:.3g}" for n, x in stored.items()))
    assert max(stored.values()) > 1.0, stored


@pytest.mark.parametrize("mut", ["causal_plus_1", "causal_minus_1"])
def test_diagonal_off_by_one_shows_at_the_sentinel_rows(mut):
    """At S = 192 the off-by-one shows at the sentinel rows themselves (attn_causal_ref.causal_edge_inputs): a
    leaked key i + 1 carries row i in {15, 63, 127}; a hidden diagonal key loses what carries row i + 1."""
    si = [s[1] for s in ATTN_EDGE_SHAPES].index(192)
    e = _emulate_case(si, 0.0, mut=mut)
    O, tO = _refs(si, 0.0, e)["o"]
    bad = ((e["o_b"].double() - O).abs() > store_bound(O, tO, BF16)).any(-1)  # [B, H, S]
    rows = (15, 63, 127) if mut == "causal_plus_1" else (16, 64, 128)
    assert bool(bad[0, :, list(rows)].all()), bad[0, :, list(rows)]


# ------------------------------------------------------------------------------------- reference
def _naive_causal_attention(layer, x, lens, B, S):
    """Hand-written masked softmax, one (b, h, i) at a time."""
    c = layer.c
    H, dh = c.heads, c.hidden // c.heads
    qkv = layer.qkv(x).view(B, S, 3, H, dh)
    ctx = torch.zeros(B, S, H, dh, dtype=x.dtype)
    for b in range(B):
        for h in range(H):
            for i in range(S):
                keys = [j for j in range(S) if j <= i and j < lens[b]]
                s = torch.stack([(qkv[b, i, 0, h] * qkv[b, j, 1, h]).sum() for j in keys]) / dh ** 0.5
                w = torch.exp(s - s.max())
                w = w / w.sum()
                ctx[b, i, h] = sum(w[n] * qkv[b, j, 2, h] for n, j in enumerate(keys))
    a = layer.out(ctx.view(B * S, c.hidden))
    y = layer.ln1(a + x)
    return layer.ln2(layer.ffn2(F.gelu(layer.ffn1(y))) + y)


def test_reference_layer_is_the_hand_written_masked_softmax_f64():
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size=50, hidden=128, layers=1, heads=2, intermediate=256, max_position=16, causal=True)
    layer = BertLayer(cfg).double()
    B, S, lens = 2, 9, [9, 4]
    x = torch.randn(B * S, 128, dtype=torch.float64)
    mask = torch.arange(S)[None, :] < torch.tensor(lens)[:, None]
    with torch.no_grad():
        got = layer.forward_reference(x, mask, B, S)
        want = _naive_causal_attention(layer, x, lens, B, S)
        full = layer.forward_reference(x, None, B, S)
        want_full = _naive_causal_attention(layer, x, [S, S], B, S)
    assert float((got - want).abs().max()) <= 1e-12
    assert float((full - want_full).abs().max()) <= 1e-12
    cfg_nc = BertConfig(vocab_size=50, hidden=128, layers=1, heads=2, intermediate=256, max_position=16)
    plain = BertLayer(cfg_nc).double()
    plain.load_state_dict(layer.state_dict())
    with torch.no_grad():
        assert float((plain.forward_reference(x, mask, B, S) - got).abs().max()) > 1e-3  # the mask is live


def test_reference_hidden_is_the_hand_written_model_f64_and_ignores_the_future():
    """forward_reference_hidden with causal=True: layer by layer the hand-written attention; and changing the
    input ids at positions >= t leaves the hidden states of positions < t unchanged (1e-6)."""
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size=50, hidden=128, layers=2, heads=2, intermediate=256, max_position=16, causal=True)
    m = BertLMHeadModel(cfg).double()
    B, S, lens = 2, 9, torch.tensor([9, 4])
    ids = torch.randint(5, 50, (B, S))
    with torch.no_grad():
        got = m.forward_reference_hidden(ids, lens, full=True)
        x = m.emb_ln(m.word_embeddings(ids) + m.position_embeddings(torch.arange(S))[None] +
                     m.token_type_embeddings(torch.zeros_like(ids))).view(B * S, -1)
        for layer in m.layers:
            x = _naive_causal_attention(layer, x, lens.tolist(), B, S)
        assert float((got - x).abs().max()) <= 1e-12
        for t in (1, 3, 8):
            ids2 = ids.clone()
            ids2[:, t:] = torch.randint(5, 50, (B, S - t))
            h2 = m.forward_reference_hidden(ids2, None, full=True).view(B, S, -1)
            h1 = m.forward_reference_hidden(ids, None, full=True).view(B, S, -1)
            assert torch.allclose(h2[:, :t], h1[:, :t], rtol=0, atol=1e-6)
            assert float((h2[:, t:] - h1[:, t:]).abs().max()) > 1e-3
        nc = BertForMaskedLM(BertConfig(vocab_size=50, hidden=128, layers=2, heads=2, intermediate=256,
                                        max_position=16)).double()
        nc.load_state_dict(m.state_dict())
        ids2 = ids.clone()
        ids2[:, 3:] = torch.randint(5, 50, (B, S - 3))
        a = nc.forward_reference_hidden(ids, None, full=True).view(B, S, -1)
        b = nc.forward_reference_hidden(ids2, None, full=True).view(B, S, -1)
        assert float((a[:, :3] - b[:, :3]).abs().max()) > 1e-3  # the non-causal encoder does look ahead


@pytest.mark.parametrize("attention_dropout", [0.0, 0.1])
def test_packed_causal_reference_equals_padded_reference_f64(attention_dropout):
    """As tests/test_unpad_cpu.py for the non-causal model: the packed and the padded causal reference are the same
    function of the weights; the LM loss and every parameter gradient agree to float64 rounding."""
    torch.manual_seed(0)
    over = {"attention_dropout": attention_dropout} if attention_dropout else {}
    pad = BertLMHeadModel(bert_config("bert-tiny", pad_id=0, **over)).double()
    unp = BertLMHeadModel(bert_config("bert-tiny", pad_id=0, unpad=True, **over)).double()
    unp.load_state_dict(pad.state_dict())
    B, S, lens = 4, 24, torch.tensor([24, 7, 1, 16])
    ids = torch.randint(5, 1000, (B, S), generator=torch.Generator().manual_seed(1))
    ids[torch.arange(S)[None, :] >= lens[:, None]] = 0
    labels = shift_labels(ids, lens)
    seed = 1234 if attention_dropout else None
    res = []
    for m in (pad, unp):
        m.train()
        h = m.forward_reference(ids, dropout_seed=seed)
        loss = m.lm_loss_reference(h, labels)
        loss.backward()
        res.append((loss.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}))
    (lp, gp), (lu, gu) = res
    assert unp._last_batch[3] is not None and pad._last_batch[3] is None
    assert abs(float(lu - lp)) <= 1e-9 * abs(float(lp))
    for n in gp:
        assert float((gu[n] - gp[n]).abs().max()) <= 1e-9 * max(float(gp[n].abs().max()), 1e-300), n


def test_eager_bf16_baseline_honours_causal():
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny"))
    ids = torch.randint(5, 1000, (2, 16))
    ids2 = ids.clone()
    ids2[:, 8:] = torch.randint(5, 1000, (2, 8))
    lens = torch.tensor([16, 11])
    for mask in (None, torch.arange(16)[None, :] < lens[:, None]):
        with torch.no_grad():
            a = m.forward_torch_bf16(ids, mask).view(2, 16, -1).float()
            b = m.forward_torch_bf16(ids2, mask).view(2, 16, -1).float()
            r = m.forward_reference(ids, mask).view(2, 16, -1)
        assert torch.equal(a[:, :8], b[:, :8]) or float((a[:, :8] - b[:, :8]).abs().max()) < 1e-6
        assert float((a - r).abs().max()) < 0.1  # bf16 autocast against fp32 on O(1) LayerNorm outputs


# ------------------------------------------------------------------------------------- model, data
def test_config_and_model_errors():
    assert BertConfig().causal is False
    assert BertLMHeadModel(bert_config("bert-tiny")).config.causal is True
    assert BertClassifier(bert_config("bert-tiny", causal=True)).config.causal is True
    with pytest.raises(ValueError, match="causal"):
        BertClassifier(bert_config("bert-tiny", causal=True, fp8=True))
    with pytest.raises(ValueError, match="fp8"):
        BertLMHeadModel(bert_config("large"))
    with pytest.raises(ValueError, match="fp8"):
        build_model("large", task="clm")
    with pytest.raises(ValueError, match="BERT models"):
        build_model("default", task="clm")
    with pytest.raises(ValueError, match="unknown task"):
        build_model("bert-tiny", task="lm")
    m = build_model("bert-tiny", task="clm")
    assert isinstance(m, BertLMHeadModel) and m.config.causal and m.max_predictions(77) == 77
    assert set(m.state_dict()) == set(BertForMaskedLM(bert_config("bert-tiny")).state_dict())


def test_cpu_lm_loss_equals_cross_entropy_of_the_reference_logits():
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny"))
    with torch.no_grad():
        m.mlm_bias.normal_(std=0.5)
    B, S, lens = 3, 40, torch.tensor([40, 17, 1])
    ids = torch.randint(5, 1000, (B, S))
    mask = torch.arange(S)[None, :] < lens[:, None]
    labels = shift_labels(ids, lens)
    hidden = m(ids, mask)
    loss = m.lm_loss(hidden, labels)
    rows = (labels.view(-1) != -100).nonzero().view(-1)
    assert rows.numel() == int((lens - 1).sum())
    logits = m.mlm_logits(hidden, rows)
    torch.testing.assert_close(loss, F.cross_entropy(logits, labels.view(-1)[rows]), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(m.last_mlm_accuracy, (logits.argmax(1) == labels.view(-1)[rows]).float().mean())
    assert int(m.last_mlm_overflow) == 0  # one slot per position: nothing is dropped
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


@pytest.mark.parametrize("min_len", [None, 1])
def test_shift_labels_and_dataset_agree(min_len):
    S = 24
    ds = SyntheticCausalLM(64, seq_len=S, vocab_size=1000, seed=3, min_len=min_len, pad_id=0)
    assert ds.ids.shape == ds.labels.shape == (64, S) and len(ds) == 64
    assert torch.equal(shift_labels(ds.ids, ds.lengths), ds.labels)
    if min_len is None:
        assert bool((ds.lengths == S).all()) and ds.pad_id is None
        assert torch.equal(shift_labels(ds.ids), ds.labels)
    else:
        assert ds.pad_id == 0 and int(ds.lengths.min()) >= 1 and int(ds.lengths.max()) <= S
        assert len(set(ds.lengths.tolist())) > 4
    for i in range(len(ds)):
        n = int(ds.lengths[i])
        ids, lab = ds[i]
        assert bool((ids[:n] >= 5).all()) and bool((ids[n:] == 0).all())
        assert torch.equal(lab[:n - 1], ids[1:n]) and bool((lab[n - 1:] == -100).all())
        d = (ids[1:n] - ids[:n - 1]) % 995
        assert n < 2 or (len(set(d.tolist())) == 1 and int(d[0]) in (1, 2, 3))  # the next token follows from two
    same = SyntheticMaskedLM(64, seq_len=S, vocab_size=1000, seed=3)
    if min_len is None:
        assert torch.equal(same.original, ds.ids)  # the MLM set's progressions, unmasked


def test_shift_labels_length_edges():
    ids = torch.arange(10, 22).view(2, 6)
    assert torch.equal(shift_labels(ids), torch.tensor([[11, 12, 13, 14, 15, -100], [17, 18, 19, 20, 21, -100]]))
    lab = shift_labels(ids, torch.tensor([1, 6]))
    assert bool((lab[0] == -100).all())  # len 1: no target at all
    assert torch.equal(lab[1], torch.tensor([17, 18, 19, 20, 21, -100]))  # len S
    lab = shift_labels(ids, torch.tensor([3, 2]))
    assert torch.equal(lab, torch.tensor([[11, 12, -100, -100, -100, -100], [17, -100, -100, -100, -100, -100]]))
    ds = SyntheticCausalLM(4, seq_len=1, vocab_size=100, seed=0)
    assert bool((ds.labels == -100).all())
    with pytest.raises(ValueError, match="min_len"):
        SyntheticCausalLM(4, seq_len=8, vocab_size=100, min_len=9)


def test_trainer_clm_criterion_trains_on_the_cpu():
    from ml_trainer_amd.trainer import Trainer
    torch.manual_seed(0)
    m = build_model("bert-tiny", task="clm")
    ds = SyntheticCausalLM(8, seq_len=32, vocab_size=1000, seed=0)
    tr = Trainer(m, datasets=(ds, ds), epochs=1, batch_size=4, optimizer="adamw", lr=1e-3, criterion="clm",
                 metric="accuracy", options={"progress": False})
    losses = [float(tr.train_step((ds.ids[:4], ds.labels[:4]))) for _ in range(6)]
    assert all(x == x for x in losses) and losses[-1] < losses[0], losses
    ev_loss, ev_acc = tr.evaluate()
    assert ev_loss == ev_loss and 0.0 <= ev_acc <= 1.0
    with pytest.raises(ValueError, match="lm_loss"):
        Trainer(BertForMaskedLM(bert_config("bert-tiny")), datasets=(ds, ds), epochs=1, batch_size=4, criterion="clm",
                options={"progress": False})


# ------------------------------------------------------------------------------------- CLI
def _cli(tmp_path, *flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--synthetic", "--synthetic_size", "16",
                           "--seq_len", "32", "--epochs", "1", "--batch_size", "8", "--optimizer", "adamw",
                           "--no_parallel", "--no_progress", "--model_dir", str(tmp_path / "mo"), *flags],
                          capture_output=True, text=True, timeout=600, cwd=str(tmp_path))


def test_cli_clm_bert_tiny_cpu(tmp_path):
    r = _cli(tmp_path, "--model", "bert-tiny", "--task", "clm", "--metric", "accuracy", "--min_seq_len", "4")
    assert r.returncode == 0, r.stderr[-2000:]
    out = tmp_path / "mo"
    sd = torch.load(out / "model.pth", weights_only=True)
    assert "mlm_bias" in sd and "layers.0.qkv.weight" in sd and "pooler.weight" not in sd
    with open(out / "history.pkl", "rb") as f:
        hist = pickle.load(f)
    losses = [v for k, v in hist.items() if "loss" in k and isinstance(v, list)]
    assert losses and all(len(v) == 1 and v[0] == v[0] and abs(v[0]) < float("inf") for v in losses), hist
    metrics = [v for k, v in hist.items() if "loss" not in k and isinstance(v, list) and v]
    assert metrics and all(0.0 <= float(v[0]) <= 1.0 for v in metrics), hist  # the next-token accuracy is reported


def test_cli_clm_error_cases(tmp_path):
    r = _cli(tmp_path, "--model", "default", "--task", "clm")
    assert r.returncode != 0 and "--task clm applies to the BERT models" in r.stderr
    r = _cli(tmp_path, "--model", "large", "--task", "clm")
    assert r.returncode != 0 and "fp8" in r.stderr
    r = _cli(tmp_path, "--model", "bert-tiny", "--task", "clm", "--mask_prob", "0.2")
    assert r.returncode != 0 and "--mask_prob" in r.stderr
    r = _cli(tmp_path, "--model", "bert-tiny", "--task", "clm", "--max_predictions", "8")
    assert r.returncode != 0 and "--max_predictions" in r.stderr
