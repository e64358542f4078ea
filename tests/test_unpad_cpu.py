"""Unpadded (packed) BERT execution, the parts that need no GPU: the pack helpers, the packed torch
reference against the padded one in float64, the construction errors / CLI flags and the
variable-length synthetic dataset."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ml_trainer_amd.data.text import SyntheticTextClassification
from ml_trainer_amd.models.bert import BertClassifier, bert_config


# ---------------------------------------------------------------- pack helpers
def test_pack_batch_layout():
    from ml_trainer_amd.ops.transformer import pack_batch
    S = 8
    lens = torch.tensor([5, 1, 8])
    ids = torch.arange(3 * S).view(3, S) + 100
    tt = (torch.arange(3 * S).view(3, S) % 2)
    pk = pack_batch(ids, lens, tt)
    assert pk.cu_seqlens.dtype == torch.int32 and pk.cu_seqlens.tolist() == [0, 5, 6, 14]
    assert pk.pos.dtype == torch.int32 and pk.pos.tolist() == [0, 1, 2, 3, 4, 0, 0, 1, 2, 3, 4, 5, 6, 7]
    assert pk.ids.tolist() == [100, 101, 102, 103, 104, 108] + list(range(116, 124))
    assert pk.tt.tolist() == [int(tt.view(-1)[i]) for i in pk.index.tolist()]
    assert pk.cls_rows.tolist() == [0, 5, 6] and pk.cls_rows.dtype == torch.int64
    assert (pk.tokens, pk.max_seqlen, pk.batch) == (14, S, 3)
    assert pack_batch(ids, lens).tt is None


def test_pack_then_unpack_restores_valid_entries():
    from ml_trainer_amd.ops.transformer import pack_batch, unpack_rows
    g = torch.Generator().manual_seed(0)
    B, S = 4, 16
    lens = torch.tensor([16, 1, 9, 12])
    ids = torch.randint(5, 100, (B, S), generator=g)
    pk = pack_batch(ids, lens)
    valid = torch.arange(S)[None, :] < lens[:, None]
    back = unpack_rows(pk.ids, pk, fill=-1).view(B, S)
    assert torch.equal(back[valid], ids[valid]) and (back[~valid] == -1).all()
    x = torch.randn(pk.tokens, 3, generator=g)
    xb = unpack_rows(x, pk).view(B, S, 3)
    assert torch.equal(xb[valid], x) and (xb[~valid] == 0).all()
    # lengths are clamped to 1 .. S, as BertClassifier._lengths clamps them
    assert pack_batch(ids, torch.tensor([0, 99, 3, 3])).cu_seqlens.tolist() == [0, 1, 17, 20, 23]


def test_pack_batch_row_multiple_adds_inert_tail_rows():
    """row_multiple rounds the row count up (the GEMMs' 256-row tile) with tail rows after cu[B] = T,
    unless that would exceed B * S; the real rows and cu_seqlens are those of the plain packing."""
    from ml_trainer_amd.ops.transformer import pack_batch, unpack_rows
    g = torch.Generator().manual_seed(0)
    B, S = 4, 16
    lens = torch.tensor([16, 1, 9, 12])
    ids = torch.randint(5, 100, (B, S), generator=g)
    tt = torch.randint(0, 2, (B, S), generator=g)
    a, b = pack_batch(ids, lens, tt), pack_batch(ids, lens, tt, row_multiple=8)
    assert (a.tokens, a.rows) == (38, 38) and (b.tokens, b.rows) == (38, 40)
    assert torch.equal(b.cu_seqlens, a.cu_seqlens) and torch.equal(b.index, a.index)
    for name in ("ids", "tt", "pos"):
        x, y = getattr(a, name), getattr(b, name)
        assert y.shape == (40,) and y.dtype == x.dtype and torch.equal(y[:38], x) and (y[38:] == 0).all()
    x = torch.randn(40, 3, generator=g)
    assert torch.equal(unpack_rows(x, b), unpack_rows(x[:38], a))
    c = pack_batch(ids, lens, tt, row_multiple=48)  # 48 <= B * S = 64: fits
    assert c.rows == 48
    d = pack_batch(ids, torch.tensor([16, 16, 16, 15]), row_multiple=48)  # 63 -> 96 > 64: left as it is
    assert (d.tokens, d.rows) == (63, 63)


# ---------------------------------------------------------------- reference equivalence (float64)
B, S, LENS = 4, 32, [32, 1, 17, 20]


def _pair(**over):
    torch.manual_seed(0)
    pad = BertClassifier(bert_config("bert-tiny", pad_id=0, **over)).double()
    unp = BertClassifier(bert_config("bert-tiny", pad_id=0, unpad=True, **over)).double()
    unp.load_state_dict(pad.state_dict())
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(5, 1000, (B, S), generator=g)
    ids[torch.arange(S)[None, :] >= torch.tensor(LENS)[:, None]] = 0
    tt = torch.randint(0, 2, (B, S), generator=g)
    y = torch.tensor([0, 1, 1, 0])
    return pad, unp, ids, tt, y


def _run(m, ids, tt, y, seed=None):
    m.zero_grad(set_to_none=True)
    logits = m.forward_reference(ids, token_type_ids=tt, dropout_seed=seed)
    F.cross_entropy(logits, y).backward()
    return logits.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def _assert_f64_equal(a, b, name):
    tol = 1e-9 * max(b.abs().max().item(), 1e-300)
    err = (a - b).abs().max().item()
    assert err <= tol, f"{name}: max abs diff {err:.3g} > {tol:.3g}"


@pytest.mark.parametrize("attention_dropout", [0.0, 0.1])
def test_packed_reference_equals_padded_reference_f64(attention_dropout):
    """Pads cannot reach the CLS loss, so the packed and the padded reference are the same function of
    the weights: logits and every parameter gradient agree to float64 rounding (1e-9 of each tensor's
    max). With attention dropout the masks are identical by construction (indexed with the padded S)."""
    over = {"attention_dropout": attention_dropout} if attention_dropout else {}
    pad, unp, ids, tt, y = _pair(**over)
    pad.train()
    unp.train()
    seed = 1234 if attention_dropout else None
    lp, gp = _run(pad, ids, tt, y, seed)
    lu, gu = _run(unp, ids, tt, y, seed)
    _assert_f64_equal(lu, lp, "logits")
    assert set(gp) == set(gu)
    for n in gp:
        _assert_f64_equal(gu[n], gp[n], n)
    if attention_dropout:  # the dropout is live: another seed moves the logits
        lo, _ = _run(unp, ids, tt, y, seed + 1)
        assert (lo - lu).abs().max().item() > 1e-6
    # rows of the position table past the longest sequence get no gradient, the used ones do
    assert gu["position_embeddings.weight"][:S].abs().sum() > 0
    assert gu["position_embeddings.weight"][S:].abs().sum() == 0


def test_packed_reference_hidden_dropout_is_seed_reproducible():
    """Hidden-dropout masks are indexed by packed row, so they differ from the padded run's by design:
    only the packed reference's own reproducibility is checked."""
    _, unp, ids, tt, y = _pair(hidden_dropout=0.1)
    unp.train()
    l1, g1 = _run(unp, ids, tt, y, 77)
    l2, g2 = _run(unp, ids, tt, y, 77)
    assert torch.equal(l1, l2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    l3, _ = _run(unp, ids, tt, y, 78)
    assert not torch.equal(l1, l3)
    unp.eval()  # eval(): no dropout, whatever the seed
    assert torch.equal(unp.forward_reference(ids, dropout_seed=1), unp.forward_reference(ids, dropout_seed=2))


def test_unpad_without_lengths_runs_the_padded_path():
    torch.manual_seed(0)
    a = BertClassifier(bert_config("bert-tiny"))
    b = BertClassifier(bert_config("bert-tiny", unpad=True))
    b.load_state_dict(a.state_dict())
    ids = torch.randint(5, 1000, (2, 16), generator=torch.Generator().manual_seed(2))
    assert b._pack(ids, b._lengths(ids, None), None) is None
    assert torch.equal(a.forward_reference(ids), b.forward_reference(ids))
    mask = torch.ones(2, 16, dtype=torch.long)
    mask[1, 9:] = 0
    torch.testing.assert_close(b.forward_reference(ids, mask), a.forward_reference(ids, mask), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(b(ids, mask), a(ids, mask), rtol=1e-5, atol=1e-6)  # the CPU forward


# ---------------------------------------------------------------- construction errors, CLI
def test_unpad_config_and_errors():
    assert bert_config("bert-base").unpad is False
    assert BertClassifier(bert_config("bert-tiny", unpad=True)).config.unpad is True
    with pytest.raises(ValueError, match="fp8"):
        BertClassifier(bert_config("bert-tiny", unpad=True, fp8=True))


def test_cli_unpad_flags():
    import main
    parser = main.build_parser()
    a = parser.parse_args([])
    assert a.unpad is False and a.min_seq_len is None and a.pad_id is None
    for lenet in ("default", "tiny"):
        with pytest.raises(ValueError, match="unpad"):
            main.main(parser.parse_args(["--model", lenet, "--unpad", "--synthetic"]))
    args = parser.parse_args(["--unpad", "--min_seq_len", "16", "--model", "bert-tiny", "--synthetic",
                              "--synthetic_size", "64", "--seq_len", "48"])
    model, (train, val) = main.build_model_and_datasets(args)
    assert model.config.unpad is True and model.config.pad_id == 0
    assert len(train) == 64 and train.seq_len == 48 and train.pad_id == 0
    assert 16 <= int(train.lengths.min()) and int(train.lengths.max()) <= 48 and int(train.lengths.min()) < 48
    assert val.pad_id == 0 and int(val.lengths.min()) >= 16
    # without the new flags: the fixed-length data and no pad id, as before
    model, (train, _) = main.build_model_and_datasets(parser.parse_args(
        ["--model", "bert-tiny", "--synthetic", "--synthetic_size", "8", "--seq_len", "32"]))
    assert model.config.unpad is False and model.config.pad_id is None and (train.lengths == 32).all()
    assert parser.parse_args(["--pad_id", "1", "--min_seq_len", "4"]).pad_id == 1


# ---------------------------------------------------------------- dataset
def test_variable_length_dataset():
    n, L, lo = 200, 40, 7
    d = SyntheticTextClassification(n, seq_len=L, vocab_size=1000, seed=3, learnable=True, min_len=lo, pad_id=0)
    assert int(d.lengths.min()) >= lo and int(d.lengths.max()) <= L and d.lengths.unique().numel() > 5
    col = torch.arange(L)[None, :]
    assert (d.ids[col >= d.lengths[:, None]] == 0).all()  # trailing pads only ...
    assert (d.ids[col < d.lengths[:, None]] != 0).all()  # ... and none inside a sequence
    has = d.targets == 1  # the marker lands inside the sequence, and only in rows labelled 1
    marked = ((d.ids == 3) & (col < d.lengths[:, None])).any(1)
    assert torch.equal(marked, has)
    e = SyntheticTextClassification(n, seq_len=L, vocab_size=1000, seed=3, learnable=True, min_len=lo, pad_id=0)
    assert torch.equal(d.ids, e.ids) and torch.equal(d.targets, e.targets) and torch.equal(d.lengths, e.lengths)
    f = SyntheticTextClassification(n, seq_len=L, vocab_size=1000, seed=4, learnable=True, min_len=lo, pad_id=0)
    assert not torch.equal(d.lengths, f.lengths)
    x, y = d[0]
    assert x.shape == (L,) and isinstance(y, int)
    with pytest.raises(ValueError):
        SyntheticTextClassification(4, seq_len=8, min_len=9)
    # another pad id
    p = SyntheticTextClassification(16, seq_len=L, vocab_size=1000, seed=3, min_len=lo, pad_id=1)
    assert (p.ids[col >= p.lengths[:, None]] == 1).all()


@pytest.mark.parametrize("learnable", [False, True])
def test_fixed_length_dataset_is_unchanged(learnable):
    """min_len=None: bit for bit the dataset the generator gave before the option existed (written out
    here draw by draw), and the variable-length one shares its tokens inside the sequences."""
    n, L, V = 50, 24, 1000
    d = SyntheticTextClassification(n, seq_len=L, vocab_size=V, seed=9, learnable=learnable)
    rng = np.random.default_rng(9)
    ids = torch.from_numpy(rng.integers(5, V, size=(n, L), dtype=np.int64))
    targets = torch.from_numpy(rng.integers(0, 2, size=n, dtype=np.int64))
    if learnable:
        pos = torch.from_numpy(rng.integers(1, max(L // 2, 2), size=n))
        ids[targets == 1, pos[targets == 1]] = 3
    assert torch.equal(d.ids, ids) and torch.equal(d.targets, targets)
    assert (d.lengths == L).all() and d.pad_id is None
    v = SyntheticTextClassification(n, seq_len=L, vocab_size=V, seed=9, learnable=False, min_len=4)
    keep = torch.arange(L)[None, :] < v.lengths[:, None]
    if not learnable:
        assert torch.equal(v.ids[keep], d.ids[keep]) and torch.equal(v.targets, d.targets)
