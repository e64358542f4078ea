"""The paged key/value cache on the CPU: attn_decode_paged_reference against attn_decode_reference on the gathered
cache, the PagePool / PagedKVCache bookkeeping, and generate(pool=) / generate(past=) over pages on bert-tiny."""
import pytest
import torch

from ml_trainer_amd.ops import decode as DC

R = DC.PAGE_ROWS


def _model(kw):
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    return BertLMHeadModel(bert_config("bert-tiny", **kw)).eval()


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 1)])
def test_reference_is_the_contiguous_one_on_the_gathered_cache(H, Hkv, rope):
    from ml_trainer_amd.ops.rope import rope_table
    g = torch.Generator().manual_seed(H)
    table = rope_table(6 * R) if rope else None
    for pos in ([0, 64, 383], [1, 255, 256], [63, 65, 257]):
        tab = (torch.randperm(23, generator=g)[:18] + 1).int().view(6, 3).t().contiguous()
        pool = torch.randn(2, 24, Hkv, R, 64, generator=g)
        qkv = torch.randn(3, (H + 2 * Hkv) * 64, generator=g)
        p = torch.tensor(pos, dtype=torch.int32)
        flat, before = DC.gather_pages(pool, tab), pool.clone()
        want = DC.attn_decode_reference(qkv, flat, p, H, rope=table)
        out = DC.attn_decode_paged_reference(qkv, pool, tab, p, H, rope=table)
        assert torch.equal(out, want) and torch.equal(DC.gather_pages(pool, tab), flat)
        changed = (pool != before).any(-1).nonzero().tolist()  # [tensor, page, head, row] of every changed row
        assert sorted(changed) == sorted([t, int(tab[b, n // R]), h, n % R] for t in range(2) for b, n in enumerate(pos)
                                         for h in range(Hkv))


def test_pool_and_cache_bookkeeping():
    pool = DC.PagePool(1, 8, 2, "cpu")
    assert pool.kv[0].shape == (2, 8, 2, R, 64) and pool.kv[0].dtype == torch.float32 and pool.num_free == 7
    a = DC.PagedKVCache(pool, 2, 1)
    assert a.Smax == R and a.kv_cache == "bf16" and a.scales is None and a.scale(0) is None
    assert not bool(a.block_table.any()) and a.block_table.dtype == a.pos.dtype == torch.int32
    a.reserve(R)
    first = a.block_table.clone()
    a.reserve(1), a.reserve(R)  # idempotent
    assert torch.equal(a.block_table, first) and pool.num_free == 5
    a.reserve(R + 1)  # grows the table past max_pages
    assert a.max_pages == 2 and a.Smax == 2 * R and torch.equal(a.block_table[:, :1], first) and pool.num_free == 3
    b = DC.PagedKVCache(pool, 1, 4)
    b.reserve(3 * R)
    owned = a.block_table.flatten().tolist() + b.block_table[0, :3].tolist()
    assert sorted(owned) == list(range(1, 8)) and b.block_table[0, 3] == 0  # never page 0, never a page twice
    table = a.block_table.clone()
    with pytest.raises(RuntimeError):
        a.reserve(2 * R + 1)  # two pages asked, none free
    assert torch.equal(a.block_table, table) and pool.num_free == 0 and [len(p) for p in a.pages] == [2, 2]
    a.release(), b.release()
    assert pool.num_free == 7 and not bool(a.block_table.any()) and not bool(b.block_table.any())
    with pytest.raises(ValueError):
        pool.free([3])  # not allocated


@pytest.mark.parametrize("kw", [{}, dict(kv_heads=1, rotary=True, pre_ln=True, ffn="swiglu")], ids=["plain", "gqa-rope"])
def test_generate_over_pages(kw):
    """56 prompt columns + 8 tokens: the contiguous cache has the 64 rows of the one-page table, both references
    reduce over the same columns and agree bit for bit. Then 24 more columns: they do not fit the contiguous state of
    max_len = 64; the paged one grows a page and gives the tokens of a contiguous run with max_len = 128. That run
    feeds the turn through attn_append_reference, the paged one column by column: the same sums in another order, so
    logits agree within fp32 summation error, (128 + 64) 2^-24 per attention or linear, some 10 in sequence: 2e-4."""
    m = _model(kw)
    ids = torch.randint(5, 1000, (2, 80), generator=torch.Generator().manual_seed(3))
    mask = (torch.arange(56)[None, :] < torch.tensor([56, 9])[:, None]).long()
    pool = DC.PagePool(m.config.layers, 9, m.config.num_kv_heads, "cpu")
    want = m.generate(ids[:, :56], 8, mask, return_logits=True)
    got = m.generate(ids[:, :56], 8, mask, return_logits=True, pool=pool)
    assert all(torch.equal(g, w) for g, w in zip(got, want)) and pool.num_free == 8
    got = m.generate(ids[:, :56], 8, mask, temperature=0.7, top_k=5, seed=1, sampler="device", pool=pool)
    want = m.generate(ids[:, :56], 8, mask, temperature=0.7, top_k=5, seed=1, sampler="device")
    assert all(torch.equal(g, w) for g, w in zip(got, want)) and pool.num_free == 8
    small, big = m.prefill(ids[:, :56], mask, max_len=64), m.prefill(ids[:, :56], mask, max_len=128)
    paged = m.prefill(ids[:, :56], mask, max_len=64, pool=pool)
    turn, tmask = ids[:, 56:72], (torch.arange(16)[None, :] < torch.tensor([16, 5])[:, None]).long()
    with pytest.raises(ValueError):
        m.generate(turn, 8, tmask, past=small)
    tok, lens, logits = m.generate(turn, 8, tmask, past=paged, pool=pool, return_logits=True)
    tok_c, lens_c, logits_c = m.generate(turn, 8, tmask, past=big, return_logits=True)
    assert paged.cache.max_pages == 2 and pool.num_free == 4  # grown, and still the caller's to release
    assert torch.equal(paged.pos, big.pos) and paged.width == big.width
    assert torch.equal(tok, tok_c) and torch.equal(lens, lens_c)
    assert float((logits - logits_c).abs().max()) <= 2e-4 * float(logits_c.abs().max())
    paged.release()


def test_value_errors():
    m = _model({})
    c = m.config
    ids = torch.randint(5, 1000, (1, 4))
    pool = DC.PagePool(c.layers, 4, c.num_kv_heads, "cpu")
    for kw in (dict(kv_cache="fp8"), dict(cache=DC.KVCache.allocate(c.layers, 1, c.num_kv_heads, 4, "cpu"))):
        with pytest.raises(ValueError):
            m.prefill(ids, pool=pool, **kw)
    for bad in (DC.PagePool(c.layers + 1, 4, c.num_kv_heads, "cpu"), DC.PagePool(c.layers, 4, c.num_kv_heads + 1, "cpu"),
                DC.PagePool(c.layers, 4, c.num_kv_heads, "meta")):
        with pytest.raises(ValueError):
            m.prefill(ids, pool=bad)
    for kw in (dict(kv_cache="fp8"), dict(graph=True, sampler="device")):
        with pytest.raises(ValueError):
            m.generate(ids, 2, pool=pool, **kw)
    state = m.prefill(ids, pool=pool)
    with pytest.raises(ValueError):
        m.extend(state, ids)
    with pytest.raises(ValueError):
        m.generate(ids, 2, past=m.prefill(ids, max_len=16), pool=pool)  # a contiguous state with a pool
    with pytest.raises(ValueError):
        DC.attn_append_reference(torch.zeros(1, 6 * 64), pool.kv[0], state.pos, 1, 2, block_table=state.cache.block_table)
    state.release()
    with pytest.raises(RuntimeError):
        m.prefill(torch.randint(5, 1000, (4, 4)), pool=pool)  # four sequences, three pages
    assert pool.num_free == 3
