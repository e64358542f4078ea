"""``BertConfig.ffn = "swiglu"`` on the CPU: the model's fp32 torch path (``forward_reference``, whose SwiGLU node has
the written-out backward of ops/swiglu.py) against a post-norm and a pre-norm layer stack written out here in float64
with ``silu`` and autograd, the state dict, the refusals, and cached against uncached decoding."""
import pytest
import torch
import torch.nn.functional as F

from ml_trainer_amd.models.bert import BertClassifier, BertLMHeadModel, bert_config

B, S = 2, 12


def _independent_logits(m, ids):
    """The classifier written out from the state dict alone, in the dtype of the weights."""
    c, p = m.config, dict(m.named_parameters())
    lin = lambda x, n: x @ p[n + ".weight"].T + p[n + ".bias"]
    ln = lambda x, n: F.layer_norm(x, (c.hidden,), p[n + ".weight"], p[n + ".bias"], c.ln_eps)
    x = p["word_embeddings.weight"][ids] + p["position_embeddings.weight"][:S] + p["token_type_embeddings.weight"][0]
    x = ln(x, "emb_ln")
    for l in range(c.layers):
        L = f"layers.{l}."
        q, k, v = (t.view(B, S, c.heads, 64).transpose(1, 2) for t in lin(ln(x, L + "ln1") if c.pre_ln else x,
                                                                           L + "qkv").chunk(3, -1))
        ctx = (torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1) @ v).transpose(1, 2).reshape(B, S, c.hidden)
        a = lin(ctx, L + "out")
        x = a + x if c.pre_ln else ln(a + x, L + "ln1")
        g, u = lin(ln(x, L + "ln2") if c.pre_ln else x, L + "ffn1").split(c.intermediate, -1)
        f = lin(F.silu(g) * u, L + "ffn2")
        x = f + x if c.pre_ln else ln(f + x, L + "ln2")
    if c.pre_ln:
        x = ln(x, "final_ln")
    return lin(torch.tanh(lin(x[:, 0], "pooler")), "classifier")


@pytest.mark.parametrize("pre_ln", [False, True], ids=["post_ln", "pre_ln"])
def test_swiglu_model_matches_independent_float64(pre_ln):
    torch.manual_seed(0)
    m = BertClassifier(bert_config("bert-tiny", ffn="swiglu", pre_ln=pre_ln, init_std=0.2)).double()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith(".bias"):
                p.normal_(std=0.2)
    ids = torch.randint(5, 1000, (B, S))
    y = torch.tensor([0, 1])
    grads = []
    for fn in (m, lambda i: _independent_logits(m, i)):
        m.zero_grad()
        logits = fn(ids)
        F.cross_entropy(logits, y).backward()
        grads.append((logits.detach(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    (la, ga), (lb, gb) = grads
    assert torch.allclose(la, lb, rtol=1e-11, atol=1e-12)
    assert set(ga) == set(gb) and "layers.1.ffn1.bias" in ga
    for n in ga:
        assert float(gb[n].abs().max()) > 0, n
        assert torch.allclose(ga[n], gb[n], rtol=1e-9, atol=1e-12 * float(gb[n].abs().max()) + 1e-300), n


def test_swiglu_state_dict_and_refusals():
    c = bert_config("bert-tiny", ffn="swiglu", intermediate=680)
    sd = BertClassifier(c).state_dict()
    assert tuple(sd["layers.0.ffn1.weight"].shape) == (1360, 256) and tuple(sd["layers.0.ffn1.bias"].shape) == (1360,)
    assert tuple(sd["layers.1.ffn2.weight"].shape) == (256, 680)
    dflt, old = BertClassifier(bert_config("bert-tiny")).state_dict(), BertClassifier(bert_config("bert-tiny", ffn="gelu"))
    assert bert_config("bert-tiny").ffn == "gelu" and tuple(dflt["layers.0.ffn1.weight"].shape) == (1024, 256)
    assert {k: tuple(v.shape) for k, v in dflt.items()} == {k: tuple(v.shape) for k, v in old.state_dict().items()}
    assert set(sd) == set(dflt)  # no key appears or leaves
    with pytest.raises(ValueError, match="ffn must be"):
        BertClassifier(bert_config("bert-tiny", ffn="geglu"))
    with pytest.raises(ValueError, match="fp8"):
        BertClassifier(bert_config("bert-tiny", ffn="swiglu", fp8=True))
    lm = BertLMHeadModel(bert_config("bert-tiny"))
    assert "swiglu" not in lm._decode_signature() and lm._decode_signature()[:2] == (False, "layernorm")
    assert BertLMHeadModel(c)._decode_signature()[2] == "swiglu"


def test_swiglu_ends_of_the_range():
    """exp(-g) overflows below g ~ -88.7: s = 0, a = +-0, dg = 0; large g: a = g u, dg = da u. Never NaN."""
    from ml_trainer_amd.ops.swiglu import swiglu, swiglu_bwd_reference, swiglu_reference
    g = torch.tensor([-200.0, -89.0, -0.0, 0.0, 30.0, 200.0])
    h1 = torch.cat((g, torch.full_like(g, 3.0)))[None]
    for t in (h1, h1.bfloat16()):
        a, d = swiglu_reference(t).float(), swiglu_bwd_reference(torch.ones(1, 6, dtype=t.dtype), t).float()
        assert bool(torch.isfinite(a).all() and torch.isfinite(d).all())
        assert a[0].tolist() == [0.0, 0.0, 0.0, 0.0, 90.0, 600.0] and d[0, :2].tolist() == [0.0, 0.0]
        assert d[0, 2:6].tolist() == [1.5, 1.5, 3.0, 3.0] and d[0, 10:].tolist() == [30.0, 200.0]
    x = h1.clone().requires_grad_()
    swiglu(x).sum().backward()
    assert bool(torch.isfinite(x.grad).all())


@pytest.mark.parametrize("over", [dict(), dict(pre_ln=True, norm="rmsnorm", rotary=True, kv_heads=2)],
                         ids=["post_ln", "pre_rms_rope_gqa"])
def test_swiglu_cached_decode_matches_uncached(over):
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny", ffn="swiglu", **over)).eval()
    with torch.no_grad():
        m.mlm_bias.normal_(std=0.1)
    ids = torch.randint(5, 1000, (3, 10))
    mask = (torch.arange(10)[None, :] < torch.tensor([10, 6, 1])[:, None]).long()
    tok, n, logits = m.generate(ids, 8, attention_mask=mask, return_logits=True)
    rtok, rn, rlogits = m.generate_reference(ids, 8, attention_mask=mask, return_logits=True)
    assert torch.equal(tok, rtok) and torch.equal(n, rn)
    assert torch.allclose(logits, rlogits, rtol=1e-4, atol=1e-4)
