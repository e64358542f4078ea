"""fp8 layer weights of the decode steps on the CPU: the quantiser, and ``weights="fp8"`` through the model's torch path
against the feature's definition, the plain model whose layer-linear weights are the dequantised ones."""
import copy

import pytest
import torch

from ml_trainer_amd.ops import decode as DC


def test_weight_quantiser():
    """Scales are powers of two, the dequantised values are a fixed point of quantise-then-dequantise, and per entry
    |dequant - bf16(w)| <= 2^-4 |bf16(w)| + 2^-9 d (half a unit of 3 mantissa bits, or the smallest subnormal of the
    scaled row); a zero row has scale 1 and zero codes."""
    g = torch.Generator().manual_seed(5)
    w = torch.randn(40, 96, generator=g) * torch.exp2(torch.randint(-20, 20, (40, 1), generator=g).float())
    w[3] = 0.0
    w[7, 11] = 3.0e4  # one huge entry: the rest of the row falls into the subnormal codes or to zero
    codes, scales = DC.weight_quantize_reference(w)
    assert codes.dtype == torch.uint8 and codes.shape == w.shape and scales.shape == (40,)
    assert torch.equal(torch.exp2(torch.log2(scales).round()), scales) and float(scales[3]) == 1.0
    assert int(codes[3].max()) == 0
    deq = DC.kv_dequantize_reference(codes, scales)
    again = DC.weight_quantize_reference(deq)
    # a row whose scaled amax rounds up to 256 (code 0x78) comes back as code 128 under 2 d; others code for code
    up = (codes & 0x7F).max(-1).values == 0x78
    assert torch.equal(DC.kv_dequantize_reference(*again), deq) and 0 < int(up.sum()) < 40
    assert torch.equal(again[0][~up], codes[~up]) and torch.equal(again[1][~up], scales[~up])
    assert torch.equal(again[1][up], 2 * scales[up])
    w16 = w.to(torch.bfloat16).double()
    assert bool(((deq.double() - w16).abs() <= 2.0 ** -4 * w16.abs() + 2.0 ** -9 * scales.double()[:, None]).all())
    assert torch.equal(DC.weight_quantize_reference(w.to(torch.bfloat16))[0], codes)  # the rounding comes first


@pytest.mark.parametrize("over,extra", [
    (dict(), dict()),
    (dict(kv_heads=1, rotary=True, pre_ln=True, ffn="swiglu"), dict()),
    (dict(), dict(kv_cache="fp8")),
    (dict(), dict(pool=True)),
], ids=["plain", "gqa-rotary-prenorm-swiglu", "fp8-cache", "paged"])
def test_fp8_weights_are_the_plain_model_on_dequantised_weights(over, extra):
    """``decode_step`` and ``extend`` under ``weights="fp8"`` return the logits, bit for bit, of a deep copy whose
    layer-linear weights are the dequantised ones (head and embeddings untouched), run plain from the same prompt."""
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny", **over)).eval()
    d = copy.deepcopy(m)
    with torch.no_grad():
        for L in d.layers:
            for lin in (L.qkv, L.out, L.ffn1, L.ffn2):
                lin.weight.copy_(DC.kv_dequantize_reference(*DC.weight_quantize_reference(lin.weight)))
    ids = torch.randint(5, 1000, (2, 9), generator=torch.Generator().manual_seed(3))
    mask = (torch.arange(9)[None, :] < torch.tensor([9, 4])[:, None]).long()
    new = torch.randint(5, 1000, (2, 4), generator=torch.Generator().manual_seed(4))
    kw = dict(extra)
    pools = [DC.PagePool(m.config.layers, 8, m.config.num_kv_heads, "cpu") for _ in range(2)] if kw.pop("pool", 0) else [None] * 2
    s8 = m.prefill(ids, mask, max_len=20, weights="fp8", pool=pools[0], **kw)
    sd = m.prefill(ids, mask, max_len=20, pool=pools[1], **kw)  # the same prompt state, the plain steps
    l8 = m.decode_step(s8, new[:, 0])
    assert torch.equal(l8, d.decode_step(sd, new[:, 0]))
    assert not torch.equal(l8, m.decode_step(m.prefill(ids, mask, max_len=20), new[:, 0]))  # (it does quantise)
    if not extra:  # extend takes the contiguous bf16 cache only
        assert torch.equal(m.extend(s8, new[:, 1:]), d.extend(sd, new[:, 1:]))
    assert torch.equal(m.decode_step(s8, new[:, 0]), d.decode_step(sd, new[:, 0]))


def test_weights_argument_is_checked():
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    m = BertLMHeadModel(bert_config("bert-tiny")).eval()
    ids = torch.randint(5, 1000, (1, 4), generator=torch.Generator().manual_seed(3))
    for call in (m.generate, m.generate_reference):
        with pytest.raises(ValueError):
            call(ids, 2, weights="int8")
    with pytest.raises(ValueError):
        m.prefill(ids, weights="int8")
    assert torch.equal(m.generate(ids, 3, weights="bf16")[0], m.generate(ids, 3)[0])
