"""Masked-LM pre-training on the CPU: the synthetic masked dataset, the torch oracle of the selection
kernel, BertForMaskedLM's loss against F.cross_entropy over hand-gathered logits, state-dict
compatibility with BertClassifier, and the CLI."""
import os
import pickle
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from ml_trainer_amd.data.text import SyntheticMaskedLM
from ml_trainer_amd.models.bert import BertClassifier, BertForMaskedLM, bert_config
from ml_trainer_amd.ops import mlm as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------- dataset
@pytest.mark.parametrize("min_len", [None, 9])
def test_dataset_invariants(min_len):
    n, S, V, P, prob = 64, 96, 500, 8, 0.15
    kw = {} if min_len is None else {"min_len": min_len, "pad_id": 0}
    ds = SyntheticMaskedLM(n, seq_len=S, vocab_size=V, mask_prob=prob, max_predictions=P, seed=3, **kw)
    assert len(ds) == n and ds.max_predictions == P
    again = SyntheticMaskedLM(n, seq_len=S, vocab_size=V, mask_prob=prob, max_predictions=P, seed=3, **kw)
    assert torch.equal(ds.ids, again.ids) and torch.equal(ds.labels, again.labels)
    other = SyntheticMaskedLM(n, seq_len=S, vocab_size=V, mask_prob=prob, max_predictions=P, seed=4, **kw)
    assert not torch.equal(ds.labels, other.labels)
    for i in range(n):
        ids, labels = ds[i]
        assert ids.shape == (S,) and labels.shape == (S,) and labels.dtype == torch.int64
        ln = int(ds.lengths[i])
        k = min(P, max(1, round(prob * ln)))
        target = labels != -100
        assert int(target.sum()) == k <= P
        assert not bool(target[ln:].any())  # no target at a pad
        # the unmasked text: the row's arithmetic progression (d in {1, 2, 3}), pads after its length
        orig = ds.original[i]
        d = int((orig[1] - orig[0]) % (V - 5)) if ln > 1 else 1
        assert d in (1, 2, 3)
        t = torch.arange(S)
        expect = 5 + (int(orig[0]) - 5 + t * d) % (V - 5)
        assert torch.equal(orig[:ln], expect[:ln])
        if min_len is not None:
            assert bool((orig[ln:] == 0).all()) and bool((ids[ln:] == 0).all())
        assert torch.equal(labels[target], orig[target])
        assert torch.equal(ids[~target], orig[~target])  # only targets are ever replaced
        assert bool((ids[target] >= 4).all())


def test_dataset_default_slots_and_mask_share():
    """P defaults to ceil(0.15 * S) rounded up to 8; over 2000 rows of S = 128 the share of targets set
    to mask_id lies in [0.77, 0.83] (the seeded generator makes this deterministic), about a tenth
    keep their token."""
    assert M.default_max_predictions(512) == 80 and M.default_max_predictions(128) == 24
    ds = SyntheticMaskedLM(2000, seq_len=128, vocab_size=30522)
    assert ds.max_predictions == 24
    target = ds.labels != -100
    assert int(target.sum()) == 2000 * 19  # round(0.15 * 128) = 19 per row
    share = float((ds.ids[target] == ds.mask_id).float().mean())
    assert 0.77 <= share <= 0.83, share
    kept = float((ds.ids[target] == ds.labels[target]).float().mean())
    assert 0.07 <= kept <= 0.13, kept


# ------------------------------------------------------------------------------------- selection oracle
def _select_naive(labels, P, lens=None, cu=None):
    B, S = labels.shape
    R = -(-B * P // 256) * 256
    rows, labs, overflow = [-1] * R, [-100] * R, 0
    for b in range(B):
        base = b * S if cu is None else int(cu[b])
        ln = S if (lens is None and cu is None) else (int(lens[b]) if cu is None else int(cu[b + 1] - cu[b]))
        k = 0
        for s in range(S):
            if int(labels[b, s]) == -100:
                continue
            if s >= ln or k >= P:
                overflow += 1
                continue
            rows[b * P + k], labs[b * P + k] = base + s, int(labels[b, s])
            k += 1
    return torch.tensor(rows, dtype=torch.int32), torch.tensor(labs), overflow


def _select_case():
    g = torch.Generator().manual_seed(0)
    B, S, P = 3, 70, 8
    labels = torch.full((B, S), -100, dtype=torch.int64)
    pos0 = torch.randperm(S, generator=g)[:13]  # more than P targets: overflow
    labels[0, pos0] = torch.randint(5, 1000, (13,), generator=g)
    pos2 = torch.tensor([0, 3, 40, 64, 69])     # (sequence 1 has none)
    labels[2, pos2] = torch.randint(5, 1000, (5,), generator=g)
    lens = torch.tensor([70, 33, 66])           # sequence 2: the target at 69 lies past its length
    return labels, P, lens


def test_select_reference_matches_naive_loop():
    labels, P, lens = _select_case()
    row, lab, ov = M.select_reference(labels, P)
    nrow, nlab, nov = _select_naive(labels, P)
    assert torch.equal(row, nrow) and torch.equal(lab, nlab) and int(ov) == nov == 5
    assert row.dtype == torch.int32 and row.numel() == 256
    assert bool((row[8:16] == -1).all()) and bool((lab[8:16] == -100).all())  # the empty sequence
    row, lab, ov = M.select_reference(labels, P, lens=lens)
    nrow, nlab, nov = _select_naive(labels, P, lens=lens)
    assert torch.equal(row, nrow) and torch.equal(lab, nlab) and int(ov) == nov == 6
    cu = torch.zeros(4, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    row, lab, ov = M.select_reference(labels, P, cu_seqlens=cu)
    nrow, nlab, nov = _select_naive(labels, P, cu=cu)
    assert torch.equal(row, nrow) and torch.equal(lab, nlab) and int(ov) == nov == 6
    assert int(row.max()) < int(cu[-1])


def test_gather_scatter_reference_roundtrip():
    labels, P, _ = _select_case()
    row, _, _ = M.select_reference(labels, P)
    x = torch.randn(3 * 70, 16)
    g = M.gather_reference(x, row)
    sel = row[row >= 0].long()
    assert torch.equal(g[row >= 0], x[sel]) and bool((g[row < 0] == 0).all())
    back = M.scatter_reference(g, row, x.shape[0])
    expect = torch.zeros_like(x)
    expect[sel] = x[sel]
    assert torch.equal(back, expect)


def test_vocab_ce_reference_matches_torch():
    torch.manual_seed(0)
    V, ld = 37, 40
    Z = torch.randn(5, ld) * 3
    Z[:, V:] = float("nan")
    labels = torch.tensor([0, V - 1, -100, V, 7])
    loss, lse, hit, grad = M.vocab_ce_reference(Z, V, labels)
    z = Z[:, :V].clone().requires_grad_()
    tgt = torch.where(labels < V, labels, torch.full_like(labels, -100))
    ref = F.cross_entropy(z, tgt, ignore_index=-100, reduction="none")
    ref.sum().backward()
    torch.testing.assert_close(loss, ref.detach())
    torch.testing.assert_close(grad[:, :V], z.grad)
    assert bool((grad[:, V:] == 0).all()) and bool((grad[2] == 0).all()) and bool((grad[3] == 0).all())
    assert float(lse[2]) == 0 and float(lse[3]) == 0 and float(hit[2]) == 0


# ------------------------------------------------------------------------------------- model
def _tiny(**kw):
    torch.manual_seed(0)
    return BertForMaskedLM(bert_config("bert-tiny", **kw))


def test_cpu_mlm_loss_equals_cross_entropy_over_gathered_logits():
    m = _tiny(max_predictions=8)
    with torch.no_grad():
        m.mlm_bias.normal_(std=0.5)
    ds = SyntheticMaskedLM(3, seq_len=64, vocab_size=1000, max_predictions=8, seed=1, min_len=30)
    ids, labels = ds.ids, ds.labels
    hidden = m(ids, ids != 0)
    assert hidden.shape == (3 * 64, 256)
    loss = m.mlm_loss(hidden, labels)
    rows = (labels.view(-1) != -100).nonzero().view(-1)
    logits = m.mlm_logits(hidden, rows)
    assert logits.shape == (rows.numel(), 1000) and logits.dtype == torch.float32
    ref = F.cross_entropy(logits, labels.view(-1)[rows])
    torch.testing.assert_close(loss, ref, rtol=1e-5, atol=1e-6)
    acc = (logits.argmax(1) == labels.view(-1)[rows]).float().mean()
    torch.testing.assert_close(m.last_mlm_accuracy, acc)
    assert int(m.last_mlm_overflow) == 0
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    assert float(m.word_embeddings.weight.grad.abs().sum()) > 0


def test_cpu_unpad_gives_the_same_loss_and_all_ignored_is_zero():
    m = _tiny(max_predictions=8)
    ds = SyntheticMaskedLM(3, seq_len=64, vocab_size=1000, max_predictions=8, seed=2, min_len=30)
    mask = ds.ids != 0
    a = m.mlm_loss(m(ds.ids, mask), ds.labels)
    mu = BertForMaskedLM(bert_config("bert-tiny", max_predictions=8, unpad=True))
    mu.load_state_dict(m.state_dict())
    hu = mu(ds.ids, mask)
    assert hu.shape[0] == int(mask.sum())
    torch.testing.assert_close(mu.mlm_loss(hu, ds.labels), a, rtol=1e-4, atol=1e-5)
    none = m.mlm_loss(m(ds.ids, mask), torch.full_like(ds.labels, -100))
    assert float(none.detach()) == 0.0
    none.backward()
    assert all(float(p.grad.abs().sum()) == 0 for p in m.parameters() if p.grad is not None)


def test_overflow_is_counted_and_fp8_is_rejected():
    m = _tiny(max_predictions=2)
    ids = torch.randint(5, 1000, (2, 32))
    labels = torch.full((2, 32), -100)
    labels[0, :5] = ids[0, :5]
    m.mlm_loss(m(ids), labels)
    assert int(m.last_mlm_overflow) == 3
    with pytest.raises(ValueError, match="fp8"):
        BertForMaskedLM(bert_config("large"))
    with pytest.raises(ValueError, match="labels must be"):
        m.mlm_loss(m(ids), labels[:, :8])


def test_state_dict_keys_are_compatible_with_the_classifier():
    cfg = bert_config("bert-tiny")
    mlm, cls = BertForMaskedLM(cfg), BertClassifier(cfg)
    km, kc = set(mlm.state_dict()), set(cls.state_dict())
    head_c = {"pooler.weight", "pooler.bias", "classifier.weight", "classifier.bias"}
    head_m = {"mlm_dense.weight", "mlm_dense.bias", "mlm_ln.weight", "mlm_ln.bias", "mlm_bias"}
    assert kc - km == head_c and km - kc == head_m  # same encoder keys; no pooler, no second decoder weight
    assert mlm.mlm_bias.shape == (cfg.vocab_size,) and mlm.word_embeddings.weight.shape[0] == cfg.vocab_size
    r = cls.load_state_dict(mlm.state_dict(), strict=False)  # the fine-tune flow
    assert set(r.missing_keys) == head_c and set(r.unexpected_keys) == head_m
    for k in km & kc:
        assert torch.equal(cls.state_dict()[k], mlm.state_dict()[k]), k
    r = mlm.load_state_dict(cls.state_dict(), strict=False)
    assert set(r.missing_keys) == head_m and set(r.unexpected_keys) == head_c


def test_trainer_mlm_criterion_cpu():
    from ml_trainer_amd.trainer import Trainer
    m = _tiny(max_predictions=8)
    ds = SyntheticMaskedLM(8, seq_len=32, vocab_size=1000, max_predictions=8, seed=0)
    tr = Trainer(m, datasets=(ds, ds), epochs=1, batch_size=4, optimizer="adamw", lr=1e-3, criterion="mlm",
                 metric="accuracy", options={"progress": False})
    loss = tr.train_step((ds.ids[:4], ds.labels[:4]))
    assert bool(torch.isfinite(loss))
    ev_loss, ev_acc = tr.evaluate()
    assert ev_loss == ev_loss and 0.0 <= ev_acc <= 1.0


# ------------------------------------------------------------------------------------- CLI
def _cli(tmp_path, *flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--synthetic", "--synthetic_size", "16",
                           "--seq_len", "32", "--epochs", "1", "--batch_size", "8", "--optimizer", "adamw",
                           "--no_parallel", "--no_progress", "--model_dir", str(tmp_path / "mo"), *flags],
                          capture_output=True, text=True, timeout=600, cwd=str(tmp_path))


def test_cli_mlm_bert_tiny_cpu(tmp_path):
    r = _cli(tmp_path, "--model", "bert-tiny", "--task", "mlm", "--metric", "accuracy")
    assert r.returncode == 0, r.stderr[-2000:]
    out = tmp_path / "mo"
    assert (out / "model.pth").exists() and (out / "history.pkl").exists()
    sd = torch.load(out / "model.pth", weights_only=True)
    assert "mlm_bias" in sd and "layers.0.qkv.weight" in sd and "pooler.weight" not in sd
    with open(out / "history.pkl", "rb") as f:
        hist = pickle.load(f)
    losses = [v for k, v in hist.items() if "loss" in k and isinstance(v, list)]
    assert losses and all(len(v) == 1 and v[0] == v[0] and abs(v[0]) < float("inf") for v in losses), hist


def test_cli_mlm_is_an_error_on_the_lenet_models(tmp_path):
    r = _cli(tmp_path, "--model", "default", "--task", "mlm")
    assert r.returncode != 0 and "--task mlm applies to the BERT models" in r.stderr
    r = _cli(tmp_path, "--model", "default", "--mask_prob", "0.2")
    assert r.returncode != 0 and "--mask_prob" in r.stderr
