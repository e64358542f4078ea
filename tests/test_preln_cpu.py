"""Pre-norm blocks and RMSNorm on the CPU paths.

``forward_reference`` is the oracle of the native path (tests/test_preln_gpu.py), so it is held here to a pre-norm
model written out in this file in plain torch from the state dict alone (``_independent_hidden``: ``nn.LayerNorm``
/ the explicit RMS formula, an explicit attention with its masks; nothing shared with models/bert.py), to fp32
round-off: that is what keeps native and reference from being wrong in the same way. Then: the state-dict keys,
cached decoding against the uncached rows, ``generate_reference``, the dropout sites, ``--no_decay_1d``, and the
config / command-line rejections with one short training run."""
import math
import pickle

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests.test_attn_causal_cpu import _cli
from tests.test_rope_cpu import LEARNED_KEYS

KINDS = [("layernorm"), ("rmsnorm")]


def _models():
    from ml_trainer_amd.models.bert import BertClassifier, BertForMaskedLM, BertLMHeadModel
    return BertClassifier, BertForMaskedLM, BertLMHeadModel


def _spread(m, seed=3):
    """Every norm weight / bias and linear bias away from its initial 1 / 0, so that a misplaced norm shows."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.ndim == 1:
                p.add_(0.2 * torch.randn(p.shape, generator=g))


def _norm(sd, name, x, kind, eps):
    if kind == "rmsnorm":
        assert name + ".bias" not in sd
        return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * sd[name + ".weight"]
    ln = nn.LayerNorm(x.shape[-1], eps=eps)
    with torch.no_grad():
        ln.weight.copy_(sd[name + ".weight"])
        ln.bias.copy_(sd[name + ".bias"])
    return ln(x)


def _independent_hidden(sd, c, ids, lens, causal):
    """[B, S, h]: the pre-norm encoder from the state dict: emb_ln(word + position + type 0), then per layer
    h += out(attn(qkv(ln1 h))); h += ffn2(gelu(ffn1(ln2 h))), then final_ln."""
    B, S = ids.shape
    H, dh, eps, kind = c.heads, c.hidden // c.heads, c.ln_eps, c.norm
    lin = lambda x, n: x @ sd[n + ".weight"].T + sd[n + ".bias"]
    h = sd["word_embeddings.weight"][ids] + sd["position_embeddings.weight"][:S][None] + sd["token_type_embeddings.weight"][0]
    h = _norm(sd, "emb_ln", h, "layernorm", eps)
    allowed = torch.ones(B, 1, S, S, dtype=torch.bool)
    if lens is not None:
        allowed = allowed & (torch.arange(S)[None, :] < lens[:, None])[:, None, None, :]
    if causal:
        allowed = allowed & (torch.arange(S)[None, :] <= torch.arange(S)[:, None])
    for l in range(c.layers):
        p = f"layers.{l}."
        q, k, v = lin(_norm(sd, p + "ln1", h, kind, eps), p + "qkv").split(c.hidden, dim=-1)
        heads = lambda t: t.view(B, S, H, dh).transpose(1, 2)
        sc = heads(q) @ heads(k).transpose(-1, -2) / math.sqrt(dh)
        pr = sc.masked_fill(~allowed, float("-inf")).softmax(-1)
        h = h + lin((pr @ heads(v)).transpose(1, 2).reshape(B, S, c.hidden), p + "out")
        h = h + lin(F.gelu(lin(_norm(sd, p + "ln2", h, kind, eps), p + "ffn1")), p + "ffn2")
    return _norm(sd, "final_ln", h, kind, eps)


@pytest.mark.parametrize("with_lens", [False, True], ids=["full", "lens"])
@pytest.mark.parametrize("kind", KINDS)
def test_forward_reference_equals_an_independent_pre_norm_model(kind, with_lens):
    from ml_trainer_amd.models.bert import bert_config
    B, S = 3, 24
    ids = torch.randint(5, 1000, (B, S), generator=torch.Generator().manual_seed(1))
    lens = torch.tensor([24, 9, 1]) if with_lens else None
    mask = None if lens is None else (torch.arange(S)[None, :] < lens[:, None]).long()
    for cls in _models():
        torch.manual_seed(0)
        m = cls(bert_config("bert-tiny", pre_ln=True, norm=kind)).eval()
        _spread(m)
        sd = m.state_dict()
        with torch.no_grad():
            out = m.forward_reference(ids, mask)
            hid = _independent_hidden(sd, m.config, ids, lens, m.config.causal)
            if cls.__name__ == "BertClassifier":
                pooled = torch.tanh(hid[:, 0] @ sd["pooler.weight"].T + sd["pooler.bias"])
                exp = pooled @ sd["classifier.weight"].T + sd["classifier.bias"]
            else:
                exp = hid.reshape(B * S, -1)
                assert m.config.causal == (cls.__name__ == "BertLMHeadModel")
        real = torch.ones(B * S, dtype=torch.bool) if lens is None else (torch.arange(S)[None, :] < lens[:, None]).view(-1)
        if exp.shape[0] == B * S:  # (pad rows of the padded layout are not compared: no caller reads them)
            out, exp = out[real], exp[real]
        assert torch.allclose(out, exp, rtol=1e-5, atol=1e-5 * float(exp.abs().max())), (cls.__name__, float((out - exp).abs().max()))
        # and the packed path computes the same rows
        u = cls(bert_config("bert-tiny", pre_ln=True, norm=kind, unpad=True, pad_id=0)).eval()
        u.load_state_dict(sd)
        if lens is not None:
            with torch.no_grad():
                pu = u.forward_reference(ids, mask)
            assert torch.allclose(pu, out, rtol=1e-5, atol=1e-5 * float(exp.abs().max()))


def test_the_independent_model_tells_post_norm_apart():
    """The check above is not vacuous: the post-LN model with the same weights is far from the pre-norm one."""
    from ml_trainer_amd.models.bert import BertForMaskedLM, bert_config
    torch.manual_seed(0)
    pre = BertForMaskedLM(bert_config("bert-tiny", pre_ln=True)).eval()
    _spread(pre)
    post = BertForMaskedLM(bert_config("bert-tiny")).eval()
    post.load_state_dict(pre.state_dict(), strict=False)
    ids = torch.randint(5, 1000, (2, 16), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        assert float((pre.forward_reference(ids) - post.forward_reference(ids)).abs().max()) > 0.1


def test_state_dict_keys():
    from ml_trainer_amd.models.bert import BertConfig, BertLMHeadModel, RMSNorm, bert_config
    assert BertConfig().pre_ln is False and BertConfig().norm == "layernorm"
    assert list(BertLMHeadModel(bert_config("bert-tiny")).state_dict()) == LEARNED_KEYS  # the default: unchanged
    for cls in _models():
        base = set(cls(bert_config("bert-tiny")).state_dict())
        ln = set(cls(bert_config("bert-tiny", pre_ln=True)).state_dict())
        assert ln - base == {"final_ln.weight", "final_ln.bias"} and base <= ln
        rms = cls(bert_config("bert-tiny", pre_ln=True, norm="rmsnorm"))
        gone = {f"layers.{l}.{n}.bias" for l in range(2) for n in ("ln1", "ln2")}
        assert set(rms.state_dict()) == (base - gone) | {"final_ln.weight"}
        assert isinstance(rms.final_ln, RMSNorm) and isinstance(rms.layers[1].ln2, RMSNorm)
        assert isinstance(rms.emb_ln, nn.LayerNorm) and rms.final_ln.eps == rms.config.ln_eps
        assert bool((rms.final_ln.weight == 1).all())
        if hasattr(rms, "mlm_ln"):
            assert isinstance(rms.mlm_ln, nn.LayerNorm)
    x = torch.randn(3, 256).to(torch.bfloat16)
    y = RMSNorm(256, 1e-5)(x)
    assert y.dtype == torch.bfloat16
    xf = x.float()
    assert torch.equal(y, (xf * torch.rsqrt((xf * xf).mean(-1, keepdim=True) + 1e-5)).to(torch.bfloat16))
    assert bool((RMSNorm(256, 1e-12)(torch.zeros(2, 256)) == 0).all())


def test_config_rejections():
    from ml_trainer_amd.models.bert import BertClassifier, BertLMHeadModel, bert_config
    with pytest.raises(ValueError, match="norm must be"):
        BertClassifier(bert_config("bert-tiny", pre_ln=True, norm="scalenorm"))
    with pytest.raises(ValueError, match="needs pre_ln=True"):
        BertLMHeadModel(bert_config("bert-tiny", norm="rmsnorm"))
    with pytest.raises(ValueError, match="fp8"):
        BertClassifier(bert_config("bert-tiny", pre_ln=True, fp8=True))
    with pytest.raises(ValueError, match="fp8|pre_ln"):
        BertClassifier(bert_config("bert-tiny", norm="rmsnorm", fp8=True))


S, PW, STEPS = 80, 48, 32
PLENS = [48, 33, 1]


@pytest.mark.parametrize("kind", KINDS)
def test_cached_decode_equals_uncached(kind):
    """As tests/test_rope_cpu.py: prompts [48, 33, 1], 32 teacher-forced steps, logits within 2e-5 (relative to the
    row's largest magnitude) of forward_reference over the full sequences; then generate against generate_reference."""
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny", pre_ln=True, norm=kind)).eval()
    _spread(m)
    ids = torch.randint(5, 1000, (3, S), generator=torch.Generator().manual_seed(11))
    pl = torch.tensor(PLENS)
    pmask = (torch.arange(PW)[None, :] < pl[:, None]).long()
    fmask = (torch.arange(S)[None, :] < (pl + STEPS)[:, None]).long()
    with torch.no_grad():
        hid = m.forward_reference(ids, fmask)
        ref = m.mlm_logits(hid, torch.arange(3 * S)).view(3, S, -1)
    state = m.prefill(ids[:, :PW].clone(), pmask, max_len=S)
    assert state.pos.tolist() == PLENS
    assert torch.allclose(state.hidden, hid.view(3, S, -1)[torch.arange(3), pl - 1], rtol=1e-4, atol=1e-5)  # normed rows
    worst = 0.0
    logits = m.decode_step(state)
    for t in range(STEPS + 1):
        if t > 0:
            logits = m.decode_step(state, torch.stack([ids[b, PLENS[b] + t - 1] for b in range(3)]))
        for b, n in enumerate(PLENS):
            r = ref[b, n - 1 + t]
            worst = max(worst, float((logits[b] - r).abs().max() / r.abs().max()))
    print(f"pre-norm {kind} cached vs uncached logits: worst relative error {worst:.3g}")
    assert state.pos.tolist() == [n + STEPS for n in PLENS]
    assert worst <= 2e-5
    tok, n = m.generate(ids[:, :PW].clone(), 8, attention_mask=pmask)
    rtok, rn = m.generate_reference(ids[:, :PW].clone(), 8, attention_mask=pmask)
    assert tok.shape == (3, 8) and torch.equal(tok, rtok) and torch.equal(n, rn)


def test_dropout_sites_on_the_cpu_path():
    """train() mode with hidden dropout: emb_ln's output at site 0, layer l's attention output at site 1 + 2 l and
    its FFN output at 2 + 2 l, each BEFORE the residual add (ops/dropout.py masks, indexed by row)."""
    from ml_trainer_amd.models.bert import BertForMaskedLM, bert_config
    from ml_trainer_amd.ops import dropout as D
    torch.manual_seed(0)
    p, seed = 0.25, 77
    m = BertForMaskedLM(bert_config("bert-tiny", pre_ln=True, norm="rmsnorm", hidden_dropout=p)).train()
    _spread(m)
    ids = torch.randint(5, 1000, (2, 16), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        got = m(ids, dropout_seed=seed)
        c, sd = m.config, m.state_dict()
        B, S = ids.shape
        lin = lambda x, n: x @ sd[n + ".weight"].T + sd[n + ".bias"]
        drop = lambda x, site: D.apply(x, p, seed, site, 0)
        h = sd["word_embeddings.weight"][ids] + sd["position_embeddings.weight"][:S][None] + sd["token_type_embeddings.weight"][0]
        h = drop(_norm(sd, "emb_ln", h, "layernorm", c.ln_eps).view(B * S, -1), 0)
        for l in range(c.layers):
            pre = f"layers.{l}."
            q, k, v = lin(_norm(sd, pre + "ln1", h, "rmsnorm", c.ln_eps), pre + "qkv").view(B, S, -1).split(c.hidden, dim=-1)
            heads = lambda t: t.reshape(B, S, c.heads, 64).transpose(1, 2)
            pr = (heads(q) @ heads(k).transpose(-1, -2) / 8.0).softmax(-1)
            h = h + drop(lin((pr @ heads(v)).transpose(1, 2).reshape(B * S, c.hidden), pre + "out"), 1 + 2 * l)
            h = h + drop(lin(F.gelu(lin(_norm(sd, pre + "ln2", h, "rmsnorm", c.ln_eps), pre + "ffn1")), pre + "ffn2"), 2 + 2 * l)
        exp = _norm(sd, "final_ln", h, "rmsnorm", c.ln_eps)
        assert torch.allclose(got, exp, rtol=1e-5, atol=1e-5 * float(exp.abs().max()))
        assert not torch.allclose(got, m.eval()(ids), rtol=1e-3, atol=1e-3)


def test_no_decay_1d_excludes_the_rms_weights():
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    m = BertLMHeadModel(bert_config("bert-tiny", pre_ln=True, norm="rmsnorm"))
    names = {n for n, p in m.named_parameters() if p.requires_grad and p.ndim <= 1}  # the rule of ops/optim.py
    assert {"final_ln.weight", "layers.0.ln1.weight", "layers.1.ln2.weight", "emb_ln.bias"} <= names
    assert not any(n.endswith("ln1.bias") or n.endswith("ln2.bias") for n in names)
    import inspect
    from ml_trainer_amd.ops import optim
    assert "p.ndim <= 1" in inspect.getsource(optim.build_optimizer)


def test_main_argument_errors():
    import main

    def build(*flags):
        return main.build_model_and_datasets(main.build_parser().parse_args(["--synthetic", "--synthetic_size", "16",
                                                                             "--seq_len", "32", *flags]))

    with pytest.raises(ValueError, match="--pre_ln / --norm apply to the BERT models"):
        build("--model", "default", "--pre_ln")
    with pytest.raises(ValueError, match="--pre_ln / --norm apply to the BERT models"):
        build("--model", "tiny", "--norm", "rmsnorm")
    with pytest.raises(ValueError, match="fp8"):
        build("--model", "large", "--pre_ln")
    with pytest.raises(ValueError, match="--norm rmsnorm needs --pre_ln"):
        build("--model", "bert-tiny", "--norm", "rmsnorm")
    with pytest.raises(SystemExit):
        main.build_parser().parse_args(["--norm", "scalenorm"])
    for task in ("classify", "mlm", "clm"):
        model, _ = build("--model", "bert-tiny", "--pre_ln", "--norm", "rmsnorm", "--task", task)
        assert model.config.pre_ln and model.config.norm == "rmsnorm" and "final_ln.weight" in model.state_dict()
    model, _ = build("--model", "bert-tiny", "--pre_ln")
    assert model.config.pre_ln and model.config.norm == "layernorm"
    model, _ = build("--model", "bert-tiny")
    assert not model.config.pre_ln and not hasattr(model, "final_ln")


def test_cli_pre_norm_rmsnorm_clm_trains(tmp_path):
    r = _cli(tmp_path, "--model", "bert-tiny", "--task", "clm", "--pre_ln", "--norm", "rmsnorm", "--epochs", "3",
             "--lr", "1e-3")
    assert r.returncode == 0, r.stderr[-2000:]
    out = tmp_path / "mo"
    sd = torch.load(out / "model.pth", weights_only=True)
    assert "final_ln.weight" in sd and "final_ln.bias" not in sd and "layers.0.ln1.bias" not in sd
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    BertLMHeadModel(bert_config("bert-tiny", pre_ln=True, norm="rmsnorm")).load_state_dict(sd)  # strict
    with open(out / "history.pkl", "rb") as f:
        hist = pickle.load(f)
    losses = [v for k, v in hist.items() if "loss" in k and "train" in k and isinstance(v, list)]
    assert losses and all(len(v) == 3 and v[-1] < v[0] for v in losses), hist
