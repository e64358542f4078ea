"""Pre-norm blocks and RMSNorm through the native model on the GPU: bert-tiny with the fixtures and thresholds of
tests/test_clm_gpu.py (training: hidden states within 5e-2 of the fp32 ``forward_reference``'s largest magnitude,
the loss within 5e-2 relative, every parameter gradient within max(2 x the eager autocast baseline's error, 0.02))
and the decode fixture of tests/test_generate_gpu.py as tests/test_rope_gpu.py reuses it (prompts [48, 33, 1], 32
fed steps, TOL = 5e-2). No tolerance is new.

The compared gradient names must include ``final_ln.weight``, ``layers.0.ln1.weight``, ``layers.1.ln2.weight`` and
the biases ``layers.0.out.bias`` / ``layers.1.ffn2.bias``, which are the fused column sums of the stream gradient
(under dropout: of its masked copy DXM) from the norm backward kernels. ``forward_reference`` itself is held to a
model written out independently in tests/test_preln_cpu.py."""
import pytest
import torch

from tests.test_clm_gpu import LENS, S, _batch, _grads
from tests.test_unpad_gpu import _close

pytestmark = pytest.mark.gpu

NORMS = ("layernorm", "rmsnorm")
MUST_CHECK = {"final_ln.weight", "layers.0.ln1.weight", "layers.1.ln2.weight", "layers.0.out.bias", "layers.1.ffn2.bias"}


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def _spread_norm_weights(m, seed=5):
    """Norm weights away from 1 (and biases from 0), so that a norm applied with another norm's weights shows."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if ".ln1." in n or ".ln2." in n or n.startswith("final_ln."):
                p.copy_((1.0 if n.endswith("weight") else 0.0) + 0.2 * torch.randn(p.shape, generator=g).to(p.device))


def _compare_grads(gn, gr, ga):
    checked = set()
    for n in gr:
        nr = gr[n].norm().item()
        if nr < 1e-8:
            continue
        e_nat = (gn[n] - gr[n]).norm().item() / nr
        e_ac = (ga[n] - gr[n]).norm().item() / nr
        print(f"{n}: native rel err {e_nat:.4f} vs autocast {e_ac:.4f}")
        assert e_nat <= max(2.0 * e_ac, 0.02), f"{n}: native rel err {e_nat:.4f} vs autocast {e_ac:.4f}"
        checked.add(n)
    assert MUST_CHECK <= checked, MUST_CHECK - checked
    return checked


@pytest.mark.parametrize("dropout", [False, True], ids=["plain", "dropout"])
@pytest.mark.parametrize("unpad", [False, True], ids=["padded", "unpad"])
@pytest.mark.parametrize("norm", NORMS)
def test_bert_tiny_preln_clm_matches_reference(dev, norm, unpad, dropout, rotary=False):
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    over = dict(hidden_dropout=0.1, attention_dropout=0.1) if dropout else {}
    m = BertLMHeadModel(bert_config("bert-tiny", pre_ln=True, norm=norm, unpad=unpad, rotary=rotary, **over)).to(dev)
    assert m.config.pre_ln and m.config.causal and ("final_ln.bias" in m.state_dict()) == (norm == "layernorm")
    m.train()
    with torch.no_grad():
        m.mlm_bias.normal_(std=0.1)
    _spread_norm_weights(m)
    ids, mask, labels = _batch(dev)
    kw = dict(dropout_seed=4242) if dropout else {}
    hn, ln, gn = _grads(m, m, m.lm_loss, ids, mask, labels, **kw)
    assert int(m.last_mlm_overflow) == 0
    hr, lr, gr = _grads(m, m.forward_reference, m.lm_loss_reference, ids, mask, labels, **kw)
    _, la, ga = _grads(m, m.forward_torch_bf16, m.mlm_loss_torch_bf16, ids, mask, labels, **kw)
    rows = hr.shape[0]
    assert rows == (sum(LENS) if unpad else len(LENS) * S)
    assert bool(torch.isfinite(hn.float()).all())  # the inert tail rows of a packed batch included
    _close(hn[:rows], hr, 5e-2)
    print(f"pre-norm {norm} clm loss native {float(ln):.5f} reference {float(lr):.5f} autocast {float(la):.5f}")
    assert abs(float(ln) - float(lr)) <= 5e-2 * abs(float(lr))
    _compare_grads(gn, gr, ga)


def test_preln_rmsnorm_with_rotary(dev):
    test_bert_tiny_preln_clm_matches_reference(dev, "rmsnorm", True, True, rotary=True)


def test_preln_rmsnorm_classifier(dev):
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    torch.manual_seed(0)
    m = BertClassifier(bert_config("bert-tiny", pre_ln=True, norm="rmsnorm")).to(dev).train()
    _spread_norm_weights(m)
    ids, mask, _ = _batch(dev)
    y = torch.tensor([0, 1, 1], device=dev)
    ce = lambda logits, t: torch.nn.functional.cross_entropy(logits.float(), t)
    on, ln, gn = _grads(m, m, ce, ids, mask, y)
    orf, lr, gr = _grads(m, m.forward_reference, ce, ids, mask, y)
    _, la, ga = _grads(m, m.forward_torch_bf16, ce, ids, mask, y)
    _close(on, orf, 5e-2)
    assert abs(float(ln) - float(lr)) <= 5e-2 * abs(float(lr))
    _compare_grads(gn, gr, ga)


def test_preln_rmsnorm_mlm(dev):
    from ml_trainer_amd.models.bert import BertForMaskedLM, bert_config
    torch.manual_seed(0)
    m = BertForMaskedLM(bert_config("bert-tiny", pre_ln=True, norm="rmsnorm")).to(dev).train()
    with torch.no_grad():
        m.mlm_bias.normal_(std=0.1)
    _spread_norm_weights(m)
    ids, mask, _ = _batch(dev)
    g = torch.Generator().manual_seed(2)
    labels = torch.where((torch.rand(ids.shape, generator=g) < 0.12).to(dev) & mask.bool(), ids, torch.full_like(ids, -100))
    hn, ln, gn = _grads(m, m, m.mlm_loss, ids, mask, labels)
    hr, lr, gr = _grads(m, m.forward_reference, m.mlm_loss_reference, ids, mask, labels)
    _, la, ga = _grads(m, m.forward_torch_bf16, m.mlm_loss_torch_bf16, ids, mask, labels)
    _close(hn, hr, 5e-2)
    assert abs(float(ln) - float(lr)) <= 5e-2 * abs(float(lr))
    _compare_grads(gn, gr, ga)


# ------------------------------------------------------------------------------------------------ decoding
PW, STEPS = 48, 32
PLENS = [48, 33, 1]
TOL = 5e-2


class _Fixture:
    def __init__(self, dev, norm):
        from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
        torch.manual_seed(0)
        self.m = m = BertLMHeadModel(bert_config("bert-tiny", pre_ln=True, norm=norm)).to(dev).eval()
        with torch.no_grad():
            m.mlm_bias.normal_(std=0.1)
        _spread_norm_weights(m)
        g = torch.Generator().manual_seed(11)
        self.ids = ids = torch.randint(5, 1000, (3, S), generator=g).to(dev)
        self.plens = pl = torch.tensor(PLENS, device=dev)
        self.prompt = ids[:, :PW].clone()
        self.pmask = (torch.arange(PW, device=dev)[None, :] < pl[:, None]).long()
        self.feed = torch.stack([ids[b, PLENS[b]:PLENS[b] + STEPS] for b in range(3)])  # [3, STEPS]
        fmask = (torch.arange(S, device=dev)[None, :] < (pl + STEPS)[:, None]).long()
        self.rows = torch.stack([torch.arange(3, device=dev) * S + pl - 1 + k for k in range(STEPS + 1)])
        with torch.no_grad():
            hr = m.forward_reference(ids, fmask)  # fp32 torch, uncached: once per norm kind
            self.ref_hidden = hr.view(3 * S, -1)
            self.ref_logits = m.mlm_logits(hr, torch.arange(3 * S, device=dev))
            self.hidden, self.logits, self.state = self.decode(self.prefill(), self.feed)

    def prefill(self, poison=False):
        state = self.m.prefill(self.prompt, self.pmask, max_len=S)
        if poison:
            for kv in state.cache.kv:
                for b, n in enumerate(PLENS):
                    kv[:, b, :, n:] = float("nan")
        return state

    def decode(self, state, feed):
        m = self.m
        hs, ls = [state.hidden.clone()], [m.decode_step(state)]
        for t in range(feed.shape[1]):
            ls.append(m.decode_step(state, feed[:, t]))
            hs.append(state.hidden.clone())
        return torch.stack(hs), torch.stack(ls), state


_FX = {}


@pytest.fixture(params=NORMS)
def fx(request):
    if request.param not in _FX:
        _FX[request.param] = _Fixture(torch.device("cuda", 0), request.param)
    return _FX[request.param]


def test_preln_decode_matches_fp32_reference(fx):
    assert fx.state.pos.tolist() == [n + STEPS for n in PLENS]
    assert fx.logits.dtype == torch.float32 and fx.logits.shape == (STEPS + 1, 3, fx.m.config.vocab_size)
    for k in range(STEPS + 1):
        _close(fx.hidden[k], fx.ref_hidden[fx.rows[k]], TOL)
        _close(fx.logits[k], fx.ref_logits[fx.rows[k]], TOL)


def test_preln_stale_cache_rows_never_read(fx):
    _, logits, _ = fx.decode(fx.prefill(poison=True), fx.feed)
    assert bool(torch.isfinite(logits).all())
    assert torch.equal(logits, fx.logits)


def test_preln_alone_equals_its_row_of_the_batch_bitwise(fx, monkeypatch):
    from ml_trainer_amd.ops.decode import DecodeState, KVCache
    monkeypatch.delenv("MLT_DECODE_GEMM", raising=False)
    batch = fx.prefill()
    alone = DecodeState(KVCache([kv[:, 1:2].clone() for kv in batch.cache.kv], batch.cache.pos[1:2].clone(), S),
                        batch.hidden[1:2].clone())
    steps = 8
    hb, lb, _ = fx.decode(batch, fx.feed[:, :steps])
    ha, la, _ = fx.decode(alone, fx.feed[1:2, :steps])
    assert alone.pos.tolist() == [PLENS[1] + steps] and bool(torch.isfinite(la).all())
    for k in range(steps + 1):
        assert torch.equal(_bits(ha[k, 0]), _bits(hb[k, 1])), f"hidden, step {k}"
        assert torch.equal(_bits(la[k, 0]), _bits(lb[k, 1])), f"logits, step {k}"
    for l in range(len(batch.cache.kv)):
        assert torch.equal(_bits(alone.cache.kv[l][:, 0]), _bits(batch.cache.kv[l][:, 1]))


def test_preln_graph_equals_eager(fx):
    kw = dict(attention_mask=fx.pmask, sampler="device", temperature=0.8, top_k=5, top_p=0.9, seed=21)
    eager = fx.m.generate(fx.prompt, STEPS, **kw)
    graph = fx.m.generate(fx.prompt, STEPS, graph=True, **kw)
    assert torch.equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1])
    captures = fx.m.decode_graph_captures
    g2 = fx.m.generate(fx.prompt, STEPS, graph=True, **kw)  # a replay of the captured graph
    assert torch.equal(eager[0], g2[0]) and fx.m.decode_graph_captures == captures


def test_block_kind_is_part_of_the_decode_signature(dev):
    """Two models that differ in pre_ln / norm only have different decode signatures, and a decoder whose signature
    no longer matches the model's is captured again, not replayed."""
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    sigs = []
    for over in (dict(), dict(pre_ln=True), dict(pre_ln=True, norm="rmsnorm")):
        torch.manual_seed(0)
        m = BertLMHeadModel(bert_config("bert-tiny", **over)).to(dev).eval()
        sigs.append(m._decode_signature()[:2])
    assert sigs == [(False, "layernorm"), (True, "layernorm"), (True, "rmsnorm")]
    ids = torch.randint(5, 1000, (2, 8), generator=torch.Generator().manual_seed(1)).to(dev)
    kw = dict(sampler="device", graph=True)
    a = m.generate(ids, 4, **kw)
    assert m.decode_graph_captures == 1
    for dec in m._graphed_decoders.values():  # as if captured for a model of another block kind
        dec.signature = (True, "layernorm") + dec.signature[2:]
    b = m.generate(ids, 4, **kw)
    assert m.decode_graph_captures == 2 and torch.equal(a[0], b[0])


def test_trainer_preln_rmsnorm_flat_gradients(dev):
    """Through the Trainer: the norm backward kernels accumulate dgamma and the fused bias gradients straight into
    the flat gradient buffer of the fused optimizer; the loss falls."""
    from ml_trainer_amd.data.text import SyntheticCausalLM
    from ml_trainer_amd.models import build_model
    from ml_trainer_amd.trainer import Trainer
    torch.manual_seed(0)
    m = build_model("bert-tiny", task="clm", pad_id=0, pre_ln=True, norm="rmsnorm", hidden_dropout=0.1)
    assert m.config.pre_ln and m.config.norm == "rmsnorm"
    ds = SyntheticCausalLM(8, seq_len=64, vocab_size=1000, seed=0, min_len=8, pad_id=0)
    tr = Trainer(m, datasets=(ds, ds), epochs=1, batch_size=4, optimizer="adamw", lr=1e-3, criterion="clm",
                 metric="accuracy", options={"progress": False, "no_decay_1d": True})
    w0 = m.final_ln.weight.detach().clone()
    losses = [float(tr.train_step((ds.ids[:4], ds.labels[:4]))) for _ in range(6)]
    assert tr.device.type == "cuda"
    assert all(x == x for x in losses) and losses[-1] < losses[0], losses
    assert not torch.equal(m.final_ln.weight.detach().cpu(), w0.cpu())  # its gradient arrived
