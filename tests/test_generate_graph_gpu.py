"""``generate(sampler="device", graph=True)`` on the GPU: one captured graph of decode_step + sample_step replayed
per token must return bit for bit what the eager loop of the same kernels returns. bert-tiny, prompts [3, 48] with
lens [48, 33, 1], 32 new tokens: the shape of tests/test_generate_gpu.py, whose sequences cross the 64-key boundary
of the decode attention kernel."""
import pytest
import torch

pytestmark = pytest.mark.gpu

PW, NEW = 48, 32
PLENS = [48, 33, 1]
SAMPLED = dict(temperature=0.8, top_k=5, top_p=0.9, seed=21)


class _Fixture:
    def __init__(self, dev):
        from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
        torch.manual_seed(0)
        self.m = m = BertLMHeadModel(bert_config("bert-tiny")).to(dev).eval()
        with torch.no_grad():
            m.mlm_bias.normal_(std=0.1)
        g = torch.Generator().manual_seed(11)
        self.prompt = torch.randint(5, 1000, (3, PW), generator=g).to(dev)
        self.other = torch.randint(5, 1000, (3, PW), generator=g).to(dev)
        self.mask = (torch.arange(PW, device=dev)[None, :] < torch.tensor(PLENS, device=dev)[:, None]).long()

    def both(self, prompt=None, **kw):
        prompt = self.prompt if prompt is None else prompt
        eager = self.m.generate(prompt, NEW, attention_mask=self.mask, sampler="device", **kw)
        graph = self.m.generate(prompt, NEW, attention_mask=self.mask, sampler="device", graph=True, **kw)
        return eager, graph


@pytest.fixture(scope="module")
def fx():
    return _Fixture(torch.device("cuda", 0))


def _same(eager, graph):
    assert torch.equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1])


def test_graph_equals_eager(fx):
    eager, graph = fx.both()
    _same(eager, graph)
    assert eager[0].shape == (3, NEW) and eager[1].tolist() == [NEW] * 3
    e2, g2 = fx.both(**SAMPLED)
    _same(e2, g2)
    assert not torch.equal(e2[0], eager[0])  # the sampled run is not the greedy one
    # an EOS that sequence 0's greedy run emits mid-way: it finishes there, pads after it, the others go on
    eos = int(eager[0][0, NEW // 2])
    e3, g3 = fx.both(eos_id=eos)
    _same(e3, g3)
    first = eager[0][0].tolist().index(eos)
    assert first <= NEW // 2 and int(e3[1][0]) == first + 1
    assert torch.equal(e3[0][0, :first + 1], eager[0][0, :first + 1])
    assert e3[0][0, first + 1:].tolist() == [fx.m.config.pad_id if fx.m.config.pad_id is not None else eos] * (NEW - first - 1)


def test_second_call_reuses_the_graph(fx):
    fx.both()  # the shape is captured (by this call or an earlier test)
    n = fx.m.decode_graph_captures
    assert n >= 1
    eager, graph = fx.both(prompt=fx.other, temperature=1.1, top_k=9, seed=4)
    _same(eager, graph)
    eager, graph = fx.both(prompt=fx.other, temperature=0.6, top_p=0.7, seed=5, eos_id=17)
    _same(eager, graph)
    assert fx.m.decode_graph_captures == n


def test_weight_edit_recaptures(fx):
    before, _ = fx.both(**SAMPLED)
    n = fx.m.decode_graph_captures
    with torch.no_grad():
        fx.m.layers[1].ffn1.weight.mul_(1.01)
    try:
        eager, graph = fx.both(**SAMPLED)
        _same(eager, graph)  # a stale graph would still read the old bf16 copy of the weight
        assert fx.m.decode_graph_captures == n + 1
        fx.both(**SAMPLED)
        assert fx.m.decode_graph_captures == n + 1
    finally:
        with torch.no_grad():
            fx.m.layers[1].ffn1.weight.div_(1.01)


def test_device_greedy_equals_default_greedy(fx):
    dflt = fx.m.generate(fx.prompt, NEW, attention_mask=fx.mask)
    devs = fx.m.generate(fx.prompt, NEW, attention_mask=fx.mask, sampler="device")
    _same(dflt, devs)


def test_graph_argument_errors(fx):
    with pytest.raises(ValueError):
        fx.m.generate(fx.prompt, 4, attention_mask=fx.mask, sampler="device", graph=True, return_logits=True)
    with pytest.raises(ValueError):
        fx.m.generate(fx.prompt, 4, attention_mask=fx.mask, graph=True)
    with pytest.raises(ValueError):
        fx.m.generate(fx.prompt, 4, attention_mask=fx.mask, temperature=1.0, top_p=0.9)
