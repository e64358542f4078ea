"""The fp8 key/value cache on the CPU: the oracle quantiser of ops/decode.py against tests/fp8_ref.py, and
``generate(kv_cache="fp8")`` through the torch path of the model."""
import pytest
import torch

from ml_trainer_amd.ops import decode as DC
from tests import fp8_ref

BF16 = torch.bfloat16


def _rows():
    """Hand-picked rows [13, 64] and 64 random ones, bf16. Entry 0 of a hand-picked row carries its amax."""
    def bits(b):  # one bf16 from its bit pattern
        return torch.tensor([b], dtype=torch.int16).view(BF16)[0]
    small = (torch.randn(64, generator=torch.Generator().manual_seed(1)) * 0.01).to(BF16)
    hand = []
    for top in (0.0, 1.0, bits(0x3F7F), bits(0x3F81), 2.0 ** -20, 2.0 ** 100, bits(0x7F7F),  # zero; 1 and its
                2.0 ** -120, 2.0 ** -126, bits(0x0001), -3.0):  # neighbours; largest finite; e clamps at -126 (x 3)
        r = small.clone() * float(top)
        r[0] = top
        hand.append(r)
    sub = torch.zeros(64, dtype=BF16)  # amax 240 -> e = 0: 2^-7, 3 * 2^-9, 2^-10 (a tie) and 2^-11 are subnormal / zero
    sub[:6] = torch.tensor([240.0, 2.0 ** -7, 3 * 2.0 ** -9, -2.0 ** -9, 2.0 ** -10, 2.0 ** -11])
    mixed = small.clone()
    mixed[5] = -1.75
    g = torch.Generator().manual_seed(2)
    rnd = (torch.randn(64, 64, generator=g) * torch.exp2(torch.randint(-30, 30, (64, 1), generator=g).float())).to(BF16)
    return torch.cat([torch.stack(hand + [sub, mixed]), rnd])


def test_oracle_quantiser():
    """Row by row: the scale is 2^max(E - 7, -126) (1 for the zero row), the codes are fp8_ref.quantize(row, 2^-e),
    and |x - deq| <= max(2^-4 |x|, 2^-10 d): half an ulp of a 3-bit mantissa above e4m3's minimum normal 2^-6, half a
    subnormal step 2^-9 below it."""
    x = _rows()
    codes, scales = DC.kv_quantize_reference(x)
    assert codes.dtype == torch.uint8 and codes.shape == x.shape and scales.shape == x.shape[:1]
    # value(code) * d in fp64 from the code's fields; the fp32 oracle equals it except where it leaves fp32's range:
    # the largest finite bf16 scales to 255, rounds to the code of 256, and 256 * 2^120 = 2^128
    deq = fp8_ref.decode(codes, fp8_ref.E4M3) * scales.double()[:, None]
    deq32 = DC.kv_dequantize_reference(codes, scales).double()
    assert torch.equal(deq32[deq.abs() < 2.0 ** 128], deq[deq.abs() < 2.0 ** 128]) and int((deq.abs() >= 2.0 ** 128).sum()) == 1
    for i, row in enumerate(x):
        amax = float(row.float().abs().max())
        e = 0 if amax == 0 else max(torch.frexp(torch.tensor(amax))[1].item() - 1 - 7, -126)
        assert float(scales[i]) == 2.0 ** e, (i, amax)
        fp8_ref.assert_exact(codes[i], row, 2.0 ** -e, fp8_ref.E4M3, f"row {i}")
        assert amax == 0 or 128 <= amax * 2.0 ** -e < 256 or e == -126
    xd = x.double()
    assert bool(((xd - deq).abs() <= torch.maximum(2.0 ** -4 * xd.abs(), 2.0 ** -10 * scales.double()[:, None])).all())
    sub = x.shape[0] - 64 - 2
    assert codes[sub, :6].tolist() == [0x77, 0x04, 0x03, 0x81, 0x00, 0x00]
    nan_row = x[-1].clone()
    nan_row[3] = float("nan")
    c, s = DC.kv_quantize_reference(torch.stack([nan_row, x[-1].clone().index_fill_(0, torch.tensor([3]), float("inf"))]))
    assert s.tolist() == [1.0, 1.0] and int(c[0, 3]) & 0x7F == 0x7F and int(c[1, 3]) == 0x7E


@pytest.mark.parametrize("over", [dict(), dict(rotary=True, kv_heads=2), dict(pre_ln=True, norm="rmsnorm", ffn="swiglu")],
                         ids=["plain", "rotary-gqa", "prenorm-swiglu"])
def test_generate_fp8_on_the_cpu(over):
    """generate(kv_cache="fp8") runs on the CPU and equals a hand loop of prefill + decode_step on an fp8 cache;
    "bf16" is the default; an unknown format and a cache of the other format raise."""
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny", **over)).eval()
    ids = torch.randint(5, 1000, (3, 12), generator=torch.Generator().manual_seed(3))
    mask = (torch.arange(12)[None, :] < torch.tensor([12, 7, 1])[:, None]).long()
    tokens, lengths = m.generate(ids, 6, attention_mask=mask, kv_cache="fp8")
    assert tokens.shape == (3, 6) and lengths.tolist() == [6, 6, 6]
    assert bool(((tokens >= 0) & (tokens < m.config.vocab_size)).all())
    state = m.prefill(ids, mask, max_len=18, kv_cache="fp8")
    cache = state.cache
    assert cache.kv_cache == "fp8" and cache.kv[0].dtype == torch.uint8 and cache.scales[0].shape == cache.kv[0].shape[:4]
    logits, hand = m.decode_step(state), []
    for t in range(6):
        hand.append(logits.argmax(-1))
        if t < 5:
            logits = m.decode_step(state, hand[-1])
    assert torch.equal(torch.stack(hand, 1), tokens)
    assert cache.pos.tolist() == [17, 12, 6]
    assert torch.equal(m.generate(ids, 6, attention_mask=mask, kv_cache="bf16")[0], m.generate(ids, 6, attention_mask=mask)[0])
    for call in (m.generate, m.generate_reference):
        with pytest.raises(ValueError):
            call(ids, 2, attention_mask=mask, kv_cache="int8")
    with pytest.raises(ValueError):
        m.prefill(ids, mask, cache=cache, max_len=18)  # an fp8 cache handed to a bf16 prefill
