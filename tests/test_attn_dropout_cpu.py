"""Attention-probability dropout on the CPU: the byte-mask oracle (ops/dropout.py) against a
per-element evaluation of its rule, and the BERT model's CPU paths with attention dropout."""
import math

import pytest
import torch

from ml_trainer_amd.models.bert import BertClassifier, bert_config
from ml_trainer_amd.ops import dropout as D

SEED = 0x1234_5678_9ABC_DEF
SITE = D.ATTENTION_SITE0 + 3


def _element_keep(seed, site, rank, H, S, p, b, h, q, k):
    """The rule, one element at a time."""
    T = (S + 3) // 4
    vec = ((b * H + h) * T + (q >> 2)) * T + (k >> 2)
    counter = torch.tensor([vec & 0xFFFFFFFF, vec >> 32, site, rank], dtype=torch.int64)
    key = torch.tensor([seed & 0xFFFFFFFF, seed >> 32], dtype=torch.int64)
    word = int(D.philox4x32(counter, key)[q & 3])
    return ((word >> (8 * (k & 3))) & 0xFF) >= int(p * 256 + 0.5)


@pytest.mark.parametrize("B,H,S", [(2, 3, 10), (1, 2, 64), (2, 4, 128)])  # S = 10: partial edge tiles
def test_oracle_matches_element_rule(B, H, S):
    p, rank = 0.1, 5
    m = D.attention_keep_mask(SEED, SITE, rank, B, H, S, p)
    assert m.shape == (B, H, S, S) and m.dtype == torch.bool
    g = torch.Generator().manual_seed(S)
    idx = torch.stack([torch.randint(0, n, (300,), generator=g) for n in (B, H, S, S)], 1).tolist()
    idx += [[B - 1, H - 1, S - 1, S - 1], [0, 0, 0, S - 1], [B - 1, 0, S - 1, 0]]
    for b, h, q, k in idx:
        assert bool(m[b, h, q, k]) == _element_keep(SEED, SITE, rank, H, S, p, b, h, q, k), (b, h, q, k)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropped_fraction(p):
    m = D.attention_keep_mask(SEED, D.attention_site(0), 0, 2, 4, 128, p)
    pe = D.attention_p(p)
    sigma = math.sqrt(pe * (1 - pe) / m.numel())
    frac = 1.0 - m.float().mean().item()
    print(f"p {p}: dropped {frac:.5f}, p_eff {pe:.5f}, 2 sigma {2 * sigma:.5f}")
    assert abs(frac - pe) <= 2 * sigma


def test_streams():
    B, H, S, p = 2, 2, 32, 0.5
    base = D.attention_keep_mask(SEED, SITE, 0, B, H, S, p)
    assert torch.equal(base, D.attention_keep_mask(SEED, SITE, 0, B, H, S, p))
    for seed, site, rank in ((SEED, SITE + 1, 0), (SEED, SITE, 1), (SEED ^ 1, SITE, 0), (SEED ^ (1 << 32), SITE, 0)):
        assert not torch.equal(base, D.attention_keep_mask(seed, site, rank, B, H, S, p))
    # a larger batch extends the same stream
    assert torch.equal(D.attention_keep_mask(SEED, SITE, 0, B + 2, H, S, p)[:B], base)


def test_sites_and_hidden_masks_untouched():
    assert D.attention_site(0) == 0x40000000 and D.attention_site(7) == 0x40000007
    L = 24
    assert all(D.attention_site(l) > 2 * L for l in range(L))  # disjoint from the hidden sites 0 .. 2L
    for site in range(5):  # the hidden rule keeps its numbering and its masks
        a = D.keep_mask(SEED, site, 0, 8, 16, 0.1)
        assert torch.equal(a, D.keep_mask(SEED, site, 0, 8, 16, 0.1))
        w = D.philox4x32(torch.tensor([[0, 0, site, 0]], dtype=torch.int64),
                         torch.tensor([SEED & 0xFFFFFFFF, SEED >> 32], dtype=torch.int64))[0]
        assert a.view(-1)[:4].tolist() == [int(x) >= D.threshold(0.1) for x in w]


def test_threshold_scale_and_bad_p():
    assert D.attention_threshold(0.1) == 26 and D.attention_p(0.1) == 26 / 256
    assert D.attention_threshold(0.5) == 128 and D.attention_scale(0.5) == 2.0
    assert D.attention_threshold(0.0) == 0 and D.attention_scale(0.0) == 1.0
    assert D.attention_scale(0.1) == torch.tensor(256.0 / 230.0, dtype=torch.float64).float().item()
    for bad in (-0.1, 1.0, 1.5, 0.001, 0.999):  # 0.001 rounds to 0/256, 0.999 to 256/256
        with pytest.raises(ValueError):
            D.attention_threshold(bad)
        with pytest.raises(ValueError):
            D.attention_keep_mask(0, SITE, 0, 1, 1, 4, bad)
    for bad in (1.0, -0.5, 0.001):
        with pytest.raises(ValueError):
            BertClassifier(bert_config("bert-tiny", attention_dropout=bad))


def _tiny_pair(**kw):
    torch.manual_seed(0)
    m0 = BertClassifier(bert_config("bert-tiny"))
    md = BertClassifier(bert_config("bert-tiny", **kw))
    md.load_state_dict(m0.state_dict())
    ids = torch.randint(5, 1000, (2, 32))
    return m0, md, ids


def test_model_attention_dropout_cpu():
    assert bert_config("bert-tiny").attention_dropout == 0.0 and bert_config("bert-base").attention_dropout == 0.0
    m0, md, ids = _tiny_pair(attention_dropout=0.1)
    md.train()
    with torch.no_grad():
        a = md(ids, dropout_seed=9)
        assert md.last_dropout_seed == 9
        assert torch.equal(md.forward_reference(ids, dropout_seed=9), a)
        assert not torch.equal(md(ids, dropout_seed=10), a)
        m0.train()
        assert not torch.equal(m0(ids), a)  # something was dropped
        torch.manual_seed(7)
        c = md(ids)
        s = md.last_dropout_seed
        torch.manual_seed(7)
        assert torch.equal(md(ids), c) and md.last_dropout_seed == s
        assert not torch.equal(md(ids), c)  # a fresh seed per forward
        # the padding-mask path drops too and matches the reference
        mask = torch.ones(2, 32, dtype=torch.long)
        mask[1, 20:] = 0
        assert torch.equal(md(ids, mask, dropout_seed=9), md.forward_reference(ids, mask, dropout_seed=9))
        md.eval()
        m0.eval()
        assert torch.equal(md(ids), m0(ids)) and torch.equal(md(ids, dropout_seed=5), m0(ids))


def test_attention_dropout_reference_is_the_rule():
    """forward_reference applies softmax -> * keep * scale -> @ v with layer l's attention site."""
    _, md, ids = _tiny_pair(attention_dropout=0.5)
    md.train()
    layer, B, S, H = md.layers[1], 2, 32, md.config.heads
    x = torch.randn(B * S, md.config.hidden)
    drop = (0.5, SEED, D.attention_site(1), 0)
    with torch.no_grad():
        got = layer.forward_reference(x, None, B, S, None, drop)
        qkv = layer.qkv(x).view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
        pr = ((qkv[0] @ qkv[1].transpose(-1, -2)) / 8.0).softmax(-1)
        pr = pr * D.attention_keep_mask(SEED, D.attention_site(1), 0, B, H, S, 0.5) * 2.0
        a = layer.out((pr @ qkv[2]).permute(0, 2, 1, 3).reshape(B * S, -1))
        x1 = layer.ln1(a + x)
        want = layer.ln2(layer.ffn2(torch.nn.functional.gelu(layer.ffn1(x1))) + x1)
    torch.testing.assert_close(got, want, rtol=0, atol=0)


def test_hidden_only_seed_draw_unchanged():
    """With only hidden dropout active the draw is the one 62-bit randint per forward it always was."""
    _, md, ids = _tiny_pair(hidden_dropout=0.1)
    md.train()
    torch.manual_seed(7)
    want = [int(torch.randint(0, 2 ** 62, (), dtype=torch.int64)) for _ in range(2)]
    torch.manual_seed(7)
    got = []
    with torch.no_grad():
        for _ in range(2):
            md(ids)
            got.append(md.last_dropout_seed)
    assert got == want
    # both kinds active: still one draw per forward, shared by the two
    _, mb, _ = _tiny_pair(hidden_dropout=0.1, attention_dropout=0.1)
    mb.train()
    torch.manual_seed(7)
    with torch.no_grad():
        mb(ids)
    assert mb.last_dropout_seed == want[0]


def test_cli_attention_dropout_flag():
    import main
    parser = main.build_parser()
    assert parser.parse_args([]).attention_dropout == 0.0
    assert parser.parse_args(["--attention_dropout", "0.1"]).attention_dropout == 0.1
    for lenet in ("default", "tiny"):
        with pytest.raises(ValueError):
            main.main(parser.parse_args(["--model", lenet, "--attention_dropout", "0.1", "--synthetic"]))
