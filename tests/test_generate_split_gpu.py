"""Cached decoding over a cache long enough for the split attention kernels (ops.decode.decode_attn_path): a rotary
bert-tiny against its fp32 reference at the tolerance of tests/test_generate_gpu.py, sequence 0 crossing the first
split boundary; NaN in the stale rows; the captured graph; and MLT_DECODE_SPLIT=0."""
import pytest
import torch

from tests.test_unpad_gpu import _close

pytestmark = pytest.mark.gpu
STEPS, TOL = 6, 5e-2


def _decode(m, state, feed):
    hs, ls = [state.hidden.clone()], [m.decode_step(state)]
    for t in range(feed.shape[1]):
        ls.append(m.decode_step(state, feed[:, t]))
        hs.append(state.hidden.clone())
    return torch.stack(hs), torch.stack(ls)


def test_decode_over_a_split_cache(dev, monkeypatch):
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    from ml_trainer_amd.ops import decode as DC
    from ml_trainer_amd.ops._ext import require_native
    monkeypatch.delenv("MLT_DECODE_SPLIT", raising=False)
    monkeypatch.delenv("MLT_DECODE_GEMM", raising=False)
    Ck = require_native().attn_decode_split_keys()
    Smax = max(DC.DECODE_SPLIT_MIN_SMAX, 2 * Ck) + 8
    assert DC.decode_attn_path(Smax) == "split"
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny", rotary=True, max_position=Smax)).to(dev).eval()
    with torch.no_grad():
        m.mlm_bias.normal_(std=0.1)
    plens, W, PW = [Ck - 2, 20], Ck + STEPS, Smax - STEPS  # sequence 0 crosses Ck at its third token
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(5, 1000, (2, W), generator=g).to(dev)
    pl = torch.tensor(plens, device=dev)
    prompt = torch.zeros(2, PW, dtype=ids.dtype, device=dev)  # as wide as generate() needs for a cache of Smax rows
    prompt[:, :Ck - 2] = ids[:, :Ck - 2]
    pmask = (torch.arange(PW, device=dev)[None, :] < pl[:, None]).long()
    feed = torch.stack([ids[b, plens[b]:plens[b] + STEPS] for b in range(2)])
    fmask = (torch.arange(W, device=dev)[None, :] < (pl + STEPS)[:, None]).long()
    rows = torch.stack([torch.arange(2, device=dev) * W + pl - 1 + k for k in range(STEPS + 1)])

    def run(poison):
        state = m.prefill(prompt, pmask, max_len=Smax)
        if poison:  # rows at and above pos[b]: the append rewrites row pos[b], nothing reads the others
            for kv in state.cache.kv:
                for b, n in enumerate(plens):
                    kv[:, b, :, n:] = float("nan")
        return _decode(m, state, feed)

    with torch.no_grad():
        hr = m.forward_reference(ids, fmask)
        ref_logits = m.mlm_logits(hr, torch.arange(2 * W, device=dev))
        hidden, logits = run(False)
        _, poisoned = run(True)
        monkeypatch.setenv("MLT_DECODE_SPLIT", "0")
        assert DC.decode_attn_path(Smax) == "single"
        _, single = run(False)
        monkeypatch.delenv("MLT_DECODE_SPLIT")
    for k in range(STEPS + 1):
        _close(hidden[k], hr.view(2 * W, -1)[rows[k]], TOL)
        _close(logits[k], ref_logits[rows[k]], TOL)
        _close(single[k], ref_logits[rows[k]], TOL)
    assert torch.equal(poisoned.view(torch.int32), logits.view(torch.int32))
    kw = dict(attention_mask=pmask, sampler="device", temperature=0.8, top_k=5, top_p=0.9, seed=21)
    eager = m.generate(prompt, STEPS, **kw)
    for _ in range(2):
        graph = m.generate(prompt, STEPS, graph=True, **kw)
        assert torch.equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1])
