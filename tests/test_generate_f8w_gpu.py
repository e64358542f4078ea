"""``generate(weights="fp8")`` on the GPU against the CPU fp32 run of the same call, and under graph replay.

Tolerance: ``_close(..., 5e-2)``, the comparison tests/test_generate_gpu.py makes between the bf16 path and its fp32
reference (both sides run on the same dequantised weights: the error sources are the bf16 path's). The logits of step
t belong to the tokens before it, so a sequence is compared through the first step at which the two greedy runs pick
different tokens, and always at step 0."""
import copy

import pytest
import torch

from tests.test_unpad_gpu import _close

pytestmark = pytest.mark.gpu

TOL = 5e-2


def _model(over):
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny", **over)).eval()
    ids = torch.randint(5, 1000, (3, 12), generator=torch.Generator().manual_seed(3))
    mask = (torch.arange(12)[None, :] < torch.tensor([12, 7, 1])[:, None]).long()
    return m, ids, mask


@pytest.mark.parametrize("over", [dict(), dict(kv_heads=1, ffn="swiglu")], ids=["plain", "gqa-swiglu"])
def test_generate_fp8_weights_against_the_cpu_run(dev, over):
    m, ids, mask = _model(over)
    tok_c, _, log_c = m.generate(ids, 8, attention_mask=mask, weights="fp8", return_logits=True)
    g = copy.deepcopy(m).to(dev)
    tok_g, _, log_g = g.generate(ids.to(dev), 8, attention_mask=mask.to(dev), weights="fp8", return_logits=True)
    same = (tok_g.cpu() == tok_c).long().cumprod(1)  # 1 while every token so far agreed
    upto = torch.cat((torch.ones(3, 1, dtype=torch.long), same[:, :-1]), 1).bool()  # steps fed the same tokens
    print(f"steps compared: {upto.sum(1).tolist()} of 8")
    _close(log_g.cpu()[upto], log_c[upto], TOL)
    assert not torch.equal(log_g, g.generate(ids.to(dev), 8, attention_mask=mask.to(dev), return_logits=True)[2])


def test_graph_replay_with_fp8_weights(dev):
    m, ids, mask = _model(dict())
    m = m.to(dev)
    kw = dict(attention_mask=mask.to(dev), sampler="device", temperature=0.8, top_k=20, seed=5, weights="fp8")
    eager, n = m.generate(ids.to(dev), 8, **kw)
    before = m.decode_graph_captures
    replayed, nr = m.generate(ids.to(dev), 8, graph=True, **kw)
    assert torch.equal(replayed, eager) and torch.equal(nr, n) and m.decode_graph_captures == before + 1
    again, _ = m.generate(ids.to(dev), 8, graph=True, **kw)
    assert torch.equal(again, eager) and m.decode_graph_captures == before + 1  # nothing new captured
