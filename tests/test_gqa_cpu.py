"""Grouped-query attention on the CPU: the configuration surface, the fp32 reference against a float64 GQA
attention written out independently, cached against uncached decode, and the ops/gqa.py oracles."""
import math

import pytest
import torch

from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
from ml_trainer_amd.ops import gqa as Q


def _model(**over):
    torch.manual_seed(0)
    return BertLMHeadModel(bert_config("bert-tiny", **over)).eval()


@pytest.mark.parametrize("kv", [None, 4])
def test_default_kv_heads_changes_no_state_dict_entry(kv):
    a, b = _model().state_dict(), _model(kv_heads=kv).state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)
    assert _model(kv_heads=kv)._decode_signature()[:2] == _model()._decode_signature()[:2]
    assert len(_model(kv_heads=kv)._decode_signature()) == len(_model()._decode_signature())


@pytest.mark.parametrize("kv", [2, 1])
def test_compact_qkv_shape_and_nothing_else(kv):
    a, b = _model().state_dict(), _model(kv_heads=kv).state_dict()
    assert list(a) == list(b)
    for k in a:
        if k.endswith(".qkv.weight"):
            assert tuple(b[k].shape) == ((4 + 2 * kv) * 64, 256)
        elif k.endswith(".qkv.bias"):
            assert tuple(b[k].shape) == ((4 + 2 * kv) * 64,)
        else:
            assert a[k].shape == b[k].shape, k
    assert kv in _model(kv_heads=kv)._decode_signature()


@pytest.mark.parametrize("bad", [3, 0, 8, -1])
def test_non_divisor_is_refused(bad):
    with pytest.raises(ValueError, match="kv_heads"):
        _model(kv_heads=bad)


def test_fp8_is_refused():
    from ml_trainer_amd.models.bert import BertClassifier
    with pytest.raises(ValueError, match="kv_heads"):
        BertClassifier(bert_config("large", layers=1, kv_heads=4))


@pytest.mark.parametrize("kv,rotary", [(2, False), (1, True)])
def test_layer_reference_against_float64_gqa(kv, rotary):
    """One layer of ``forward_reference`` against a GQA attention in float64 that indexes KV head h // G per query
    head (no repeat of k / v), around the layer's own linears and norms."""
    m = _model(kv_heads=kv, rotary=rotary).double()
    L, c = m.layers[0], m.config
    B, S, H, G = 2, 9, c.heads, c.heads // kv
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B * S, c.hidden, generator=g, dtype=torch.float64)
    table = m.rope_table.double() if rotary else None
    got = L.forward_reference(x, None, B, S, rope=table)

    qkv = (x @ L.qkv.weight.T + L.qkv.bias).view(B, S, H + 2 * kv, 64)
    if rotary:
        cs = table[:S]  # [S, 32, 2]
        def rot(t):  # t [B, S, heads, 64], interleaved pairs
            a, b = t[..., 0::2], t[..., 1::2]
            co, si = cs[None, :, None, :, 0], cs[None, :, None, :, 1]
            return torch.stack((a * co - b * si, a * si + b * co), -1).flatten(-2)
        qkv = torch.cat((rot(qkv[:, :, :H + kv]), qkv[:, :, H + kv:]), 2)
    ctx = torch.zeros(B, S, H, 64, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            q, k, v = qkv[b, :, h], qkv[b, :, H + h // G], qkv[b, :, H + kv + h // G]
            s = (q @ k.T) / math.sqrt(64)
            s = s.masked_fill(~torch.ones(S, S, dtype=torch.bool).tril(), float("-inf"))
            ctx[b, :, h] = s.softmax(-1) @ v
    y = L.ln1(L.out(ctx.view(B * S, -1)) + x)
    want = L.ln2(L.ffn2(torch.nn.functional.gelu(L.ffn1(y))) + y)
    assert torch.allclose(got, want, rtol=1e-9, atol=1e-9), float((got - want).abs().max())


@pytest.mark.parametrize("over", [dict(kv_heads=2), dict(kv_heads=1, rotary=True, pre_ln=True, norm="rmsnorm")],
                         ids=["kv2", "kv1-rotary-preln-rms"])
def test_cached_decode_equals_uncached_on_the_cpu(over):
    m = _model(**over)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(5, 1000, (2, 12), generator=g)
    with torch.no_grad():
        state = m.prefill(ids[:, :7], max_len=12)
        assert tuple(state.cache.kv[0].shape) == (2, 2, over["kv_heads"], 12, 64)
        logits = [m.decode_step(state)] + [m.decode_step(state, ids[:, t]) for t in range(7, 12)]
        ref = m.mlm_logits(m.forward_reference(ids), torch.arange(24)).view(2, 12, -1)
    for k, z in enumerate(logits):
        assert torch.allclose(z, ref[:, 6 + k], rtol=1e-4, atol=1e-4), (k, float((z - ref[:, 6 + k]).abs().max()))


@pytest.mark.parametrize("H,Hkv", [(4, 2), (3, 1), (12, 4)])
def test_expand_then_reduce_of_a_one_hot_gradient(H, Hkv):
    """d(sum of the wide buffer) / d(compact entry): G for a k / v entry, 1 for a q entry; and the infer helper."""
    G, W = H // Hkv, Q.compact_width(H, Hkv)
    assert Q.infer_kv_heads(W, H) == Hkv and Q.infer_kv_heads(3 * H * 64, H) is None
    for col in (5, H * 64 + 3, (H + Hkv) * 64 + 63, W - 1):
        e = torch.zeros(2, W)
        e[1, col] = 1.0
        back = Q.gqa_reduce_reference(Q.gqa_expand_reference(e, H, Hkv), H, Hkv)
        assert torch.equal(back, e * (1 if col < H * 64 else G))
