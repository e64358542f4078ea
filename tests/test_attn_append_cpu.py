"""Multi-token append on the CPU: ``attn_append_reference`` against T successive ``attn_decode_reference`` calls, and
``BertLMHeadModel.extend`` against T ``decode_step``s, in fp32 (the two differ in summation order only: 1e-5)."""
import pytest
import torch

from ml_trainer_amd.ops import decode as DC
from ml_trainer_amd.ops.rope import rope_table


@pytest.mark.parametrize("H,Hkv,rope", [(2, 2, False), (4, 2, True), (6, 1, True)])
@pytest.mark.parametrize("T", [1, 5, 16])
def test_reference_equals_successive_decode_steps(H, Hkv, rope, T):
    B, Smax = 3, 40
    g = torch.Generator().manual_seed(H * 100 + T)
    pos = torch.tensor([0, 7, Smax - T], dtype=torch.int32)
    qkv = torch.randn(B * T, (H + 2 * Hkv) * 64, generator=g)
    kv = torch.randn(2, B, Hkv, Smax, 64, generator=g)
    for b in range(B):
        kv[:, b, :, int(pos[b]):] = float("nan")  # stale rows: selected out by both
    table = rope_table(Smax) if rope else None
    kv_a, kv_d, p = kv.clone(), kv.clone(), pos.clone()
    out = DC.attn_append_reference(qkv, kv_a, pos, B, H, rope=table).view(B, T, -1)
    for t in range(T):
        step = DC.attn_decode_reference(qkv.view(B, T, -1)[:, t], kv_d, p, H, rope=table)
        torch.testing.assert_close(out[:, t], step, rtol=1e-5, atol=1e-5 * float(step.abs().max()))
        p += 1
    assert torch.equal(pos, torch.tensor([0, 7, Smax - T], dtype=torch.int32))
    assert torch.equal(kv_a.nan_to_num(nan=7.0), kv_d.nan_to_num(nan=7.0))  # the same rows appended, the rest untouched


@pytest.mark.parametrize("kw", [{}, dict(kv_heads=1, rotary=True, pre_ln=True, ffn="swiglu")], ids=["plain", "gqa-rope"])
def test_extend_equals_decode_steps(kw):
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny", **kw)).eval()
    ids = torch.randint(5, 1000, (2, 30), generator=torch.Generator().manual_seed(3))
    mask = (torch.arange(9)[None, :] < torch.tensor([9, 4])[:, None]).long()
    new = ids[:, 9:29]  # T = 20: two pieces
    a, d = (m.prefill(ids[:, :9], mask, max_len=40) for _ in range(2))
    counts = torch.tensor([20, 7], dtype=torch.int32)
    logits = m.extend(a, new, counts=counts)
    assert logits.shape == (2, 20, m.config.vocab_size) and a.pos.tolist() == [29, 11]
    steps = torch.stack([m.decode_step(d, new[:, t]) for t in range(20)], 1)
    assert d.pos.tolist() == [29, 24]
    tol = 1e-5 * float(steps.abs().max())
    torch.testing.assert_close(logits, steps, rtol=1e-5, atol=tol)
    torch.testing.assert_close(a.hidden[0], d.hidden[0], rtol=1e-5, atol=1e-5)  # the row of token counts - 1
    d.cache.pos.copy_(a.pos)  # sequence 1 accepted 7: its next token must not see the 13 stale rows
    torch.testing.assert_close(m.decode_step(a, ids[:, 29]), m.decode_step(d, ids[:, 29]), rtol=1e-5, atol=tol)


def test_refused():
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    kv = torch.zeros(2, 1, 2, 32, 64)
    pos = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError):
        DC.attn_append_reference(torch.zeros(17, 6 * 64), kv, pos, 1, 2)
    with pytest.raises(ValueError):
        DC.attn_append_reference(torch.zeros(4, 6 * 64), kv.to(torch.uint8), pos, 1, 2)
    with pytest.raises(ValueError):
        DC.attn_append_reference(torch.zeros(4, 6 * 64), kv, pos, 1, 2, kv_scale=torch.ones(2, 1, 2, 32))
    m = BertLMHeadModel(bert_config("bert-tiny")).eval()
    ids = torch.randint(5, 1000, (1, 4))
    with pytest.raises(ValueError):
        m.extend(m.prefill(ids, max_len=16, kv_cache="fp8"), ids)
    with pytest.raises(ValueError):
        m.extend(m.prefill(ids, max_len=16), ids[:, :0])
    with pytest.raises(ValueError):
        m.generate(ids, 4, past=m.prefill(ids, max_len=8))  # 4 cached + 4 new + 4 generated > 8 rows
