"""attn_decode_paged.hip on the GPU: the paged launch against C.attn_decode_split on the gathered cache bit for bit
(out, the appended row, nothing else written, no dependence on gc or on where the pages lie), against
attn_decode_paged_reference within the derived allowance, kv_fill_paged against torch indexing, the refusals, and
generate(pool=) against generate() on bert-tiny. Every pool row no sequence holds below its pos is NaN."""
import pytest
import torch

from ml_trainer_amd.ops import decode as DC
from ml_trainer_amd.ops import gqa as Q
from ml_trainer_amd.ops._ext import require_native as _C
from ml_trainer_amd.ops.rope import rope_qk_reference, rope_table
from tests.attn_decode_ref import decode_bound_terms, decode_effective
from tests.helpers import assert_guard_intact, assert_within, guarded, guarded_like, store_bound

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
NAN = float("nan")
B, MAX_PAGES, PAGES, R = 3, 6, 24, 64
# three per case, every value in some case: an empty cache, the last / first row of a page, both sides of the split
# boundary (256 keys), the last row of the table
POS = [[0, 64, 383], [1, 255, 256], [63, 65, 257]]


def _bits(x):
    return x.contiguous().view(torch.int16)


def _tables(pos, seed):
    """Two tables [B, MAX_PAGES]: page i of sequence b is entry i * B + b of a seeded permutation of 1 .. PAGES - 1
    (interleaved, not monotonic); entries past the page of row pos[b] are 0, the null page."""
    out = []
    for s in (seed, seed + 100):
        perm = (torch.randperm(PAGES - 1, generator=torch.Generator().manual_seed(s)) + 1).int()
        t = perm[:B * MAX_PAGES].view(MAX_PAGES, B).t().contiguous()
        for b, n in enumerate(pos):
            t[b, n // R + 1:] = 0
        out.append(t)
    return out


def _pool(kv, table, pos):
    """The NaN pool [2, PAGES, Hkv, 64, 64] holding rows j < pos[b] of the contiguous ``kv`` in the table's pages."""
    pool = torch.full((2, PAGES, kv.shape[2], R, 64), NAN, dtype=kv.dtype)
    for b, n in enumerate(pos):
        for j in range(n):
            pool[:, table[b, j // R], :, j % R] = kv[:, b, :, j]
    return pool


def _inputs(H, Hkv, pos, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B, Q.compact_width(H, Hkv), generator=g) * 0.5).to(BF16)
    kv = (torch.randn(2, B, Hkv, MAX_PAGES * R, 64, generator=g) * 0.5).to(BF16)
    return qkv, kv, torch.tensor(pos, dtype=torch.int32)


def _paged(dev, qkv, pool, table, pos, H, rope=None, gc=0):
    """One C.attn_decode_paged launch on guarded buffers and a NaN workspace: (out, pool after) on the CPU."""
    C = _C()
    qbuf, q = guarded_like(qkv.to(dev))
    pbuf, p2 = guarded_like(pool.to(dev).view(-1, 64))
    obuf, out = guarded(B, H * 64, BF16, dev)
    shape = C.attn_decode_split_ws(B, H, table.shape[1] * R)
    wbuf, w2 = guarded(B * H * shape[2], shape[3], torch.float32, dev)
    w2.fill_(NAN)
    C.attn_decode_paged(q, p2.view(pool.shape), table.to(dev), pos.to(dev), out, w2.view(shape), H, 0.125, rope=rope,
                        gc=gc)
    torch.cuda.synchronize()
    for buf, view in ((qbuf, q), (pbuf, p2), (obuf, out), (wbuf, w2)):
        assert_guard_intact(buf, view)
    assert torch.equal(_bits(q), _bits(qkv.to(dev))), "qkv_new changed"
    return out.cpu(), p2.view(pool.shape).cpu()


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("H,Hkv", [(2, 2), (6, 2), (4, 1)])
def test_bits_of_the_split_kernel_on_the_gathered_cache(dev, H, Hkv, rope):
    C = _C()
    pos = POS[(H + rope) % 3]
    qkv, kv, p = _inputs(H, Hkv, pos, 10 * H + Hkv)
    tab_a, tab_b = _tables(pos, H)
    table = rope_table(MAX_PAGES * R, device=dev) if rope else None
    pool = _pool(kv, tab_a, pos)
    # the contiguous launch on what the table names: NaN wherever the pool is
    flat = DC.gather_pages(pool, tab_a).to(dev)
    want = torch.empty(B, H * 64, dtype=BF16, device=dev)
    ws = torch.empty(C.attn_decode_split_ws(B, H, MAX_PAGES * R), dtype=torch.float32, device=dev)
    C.attn_decode_split(qkv.to(dev), flat, p.to(dev), want, ws, H, 0.125, rope=table)
    want, flat = want.cpu(), flat.cpu()
    assert bool(torch.isfinite(want.float()).all())
    pool_want = pool.clone()
    for b, n in enumerate(pos):  # exactly the one new row per (b, KV head), with the contiguous kernel's bits
        pool_want[:, tab_a[b, n // R], :, n % R] = flat[:, b, :, n]
    G = H // Hkv
    for gc in [0, 1] + [d for d in (2, 3, 4) if G % d == 0]:
        out, after = _paged(dev, qkv, pool, tab_a, p, H, table, gc)
        assert torch.equal(_bits(out), _bits(want)), f"out, gc={gc}"
        assert torch.equal(_bits(after), _bits(pool_want)), f"pool, gc={gc}"
    out, _ = _paged(dev, qkv, _pool(kv, tab_b, pos), tab_b, p, H, table)
    assert torch.equal(_bits(out), _bits(want)), "the same rows in other pages"


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
def test_within_the_bound_of_the_reference(dev, rope):
    """|kernel - attn_decode_paged_reference (fp32 copies)| <= the kernel's allowance + the reference's, both around
    the fp64 value O of tests/attn_decode_ref.py: store_bound(O, t_core + 2 t_merge, bf16) as the split kernel's test
    derives it, and t_core + t_merge + (Smax + 4) 2^-24 max|v| as tests/test_attn_decode_cpu.py derives the fp32
    reference's."""
    H, pos = 2, POS[1]
    qkv, kv, p = _inputs(H, H, pos, 5)
    tab, _ = _tables(pos, 9)
    table = rope_table(MAX_PAGES * R, device=dev) if rope else None
    pool = _pool(kv, tab, pos)
    out, after = _paged(dev, qkv, pool, tab, p, H, table)
    pool32 = pool.float()  # NaN and all: the reference selects stale rows out, it never multiplies them
    ref = DC.attn_decode_paged_reference(qkv, pool32, tab, p, H, 0.125, None if table is None else table.cpu())
    rot = rope_qk_reference(qkv, table.cpu(), H, pos=p) if rope else qkv
    q, k, v = decode_effective(rot, DC.gather_pages(pool, tab), pos)
    O, t_core, t_merge = decode_bound_terms(q, k, v, pos, 0.125)
    O, t_core, t_merge = (x.view(B, H * 64) for x in (O, t_core, t_merge))
    vmax = float(torch.nan_to_num(v).abs().amax())  # (over the rows that count: the stale ones are NaN)
    tol = store_bound(O, t_core + 2 * t_merge, BF16) + t_core + t_merge + (MAX_PAGES * R + 4) * 2.0 ** -24 * vmax
    r = assert_within(out, ref.double(), tol, "paged kernel against its reference")
    print(f"rope {rope}: |err| / bound {r:.3f}")
    for b, n in enumerate(pos):  # the reference appended the same row (its fp32 copy of the same bf16 bits)
        assert torch.equal(after[:, tab[b, n // R], :, n % R].float(), pool32[:, tab[b, n // R], :, n % R])


@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 1)])
@pytest.mark.parametrize("S", [1, 64, 70])
def test_kv_fill_paged(dev, S, H, Hkv):
    C, Bf, P, G = _C(), 2, 8, H // Hkv
    g = torch.Generator().manual_seed(S + H)
    qkv = torch.randn(Bf * S, 3 * H * 64, generator=g).to(BF16)
    tab = torch.tensor([[5, 2], [3, 7]], dtype=torch.int32)
    tab[:, -(-S // R):] = 0  # unowned: the null page
    want = torch.full((2, P, Hkv, R, 64), NAN, dtype=BF16)
    x, rows = qkv.view(Bf, S, 3, H, 64), torch.arange(S)
    for t in range(2):
        want[t][tab.long()[:, rows // R], :, rows % R] = x[:, :, 1 + t, ::G]
    qbuf, q = guarded_like(qkv.to(dev), ld=3 * H * 64 + 8)  # a row-strided view
    pbuf, p2 = guarded_like(torch.full((2 * P * Hkv * R, 64), NAN, dtype=BF16, device=dev))
    C.kv_fill_paged(q, p2.view(want.shape), tab.to(dev), Bf, S, H)
    torch.cuda.synchronize()
    assert_guard_intact(qbuf, q)
    assert_guard_intact(pbuf, p2)
    assert torch.equal(_bits(p2.view(want.shape).cpu()), _bits(want))


def test_refused_calls(dev):
    C, H, Hkv, P = _C(), 4, 2, 8
    z = lambda *s, dt=BF16: torch.full(s, 3.0, dtype=dt, device=dev)
    shape = C.attn_decode_split_ws(B, H, MAX_PAGES * R)
    assert C.attn_decode_paged_page_rows() == R == DC.PAGE_ROWS and list(shape) == [B, H, 2, 68]
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    tab = torch.ones(B, MAX_PAGES, dtype=torch.int32, device=dev)
    out, pool = z(B, H * 64), z(2, P, Hkv, R, 64)
    rope = torch.zeros(MAX_PAGES * R - 1, 32, 2, device=dev)
    ok = lambda: dict(qkv_new=z(B, 8 * 64), pool=pool, block_table=tab, pos=pos, out=out,
                      ws=z(*shape, dt=torch.float32), H=H, scale=0.125)
    bad = [dict(pool=z(2, P, Hkv, 32, 64)), dict(pool=z(2, P, Hkv, R, 128)[..., :64]), dict(pool=pool.float()),
           dict(pool=z(2, P, 3, R, 64), qkv_new=z(B, 10 * 64)),  # Hkv = 3 does not divide H = 4
           dict(block_table=tab.long()), dict(block_table=tab[0]), dict(block_table=tab[:2]),
           dict(block_table=tab.t().contiguous().t()), dict(block_table=tab.cpu()), dict(rope=rope),
           dict(ws=z(B, H, 1, 68, dt=torch.float32)), dict(gc=4)]
    for over in bad:
        with pytest.raises(RuntimeError):
            C.attn_decode_paged(**{**ok(), **over})
    with pytest.raises(RuntimeError):
        C.kv_fill_paged(z(B * 4, 3 * H * 64), pool, tab.long(), B, 4, H)
    with pytest.raises(RuntimeError):
        C.kv_fill_paged(z(B * 4, 3 * H * 64), z(2, P, Hkv, 32, 64), tab, B, 4, H)
    with pytest.raises(ValueError):
        DC.attn_decode(z(B, 8 * 64), pool, pos, H, kv_scale=z(2, B, Hkv, R, dt=torch.float32), block_table=tab)
    with pytest.raises(ValueError):
        DC.attn_append(z(B, 8 * 64), pool, pos, B, H, block_table=tab)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((pool == 3.0).all()), "a refused call wrote something"
    C.attn_decode_paged(**ok())


@pytest.mark.parametrize("kw", [{}, dict(kv_heads=1, rotary=True, pre_ln=True, ffn="swiglu")], ids=["plain", "gqa-rope"])
def test_generate_with_a_pool_has_the_contiguous_bits(dev, kw):
    """Prompts of 60 and 9 tokens plus 8 new ones: sequence 0 crosses a page boundary while decoding. Fewer than 256
    rows are cached, so the paged launch has one active split and with it the single kernel's bits."""
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny", **kw)).eval().to(dev)
    ids = torch.randint(5, 1000, (2, 60), generator=torch.Generator().manual_seed(3)).to(dev)
    mask = (torch.arange(60)[None, :] < torch.tensor([60, 9])[:, None]).long().to(dev)
    pool = DC.PagePool(m.config.layers, 9, m.config.num_kv_heads, dev)
    for layer in pool.kv:
        layer.fill_(NAN)
    free = pool.num_free
    tok, lens, logits = m.generate(ids, 8, mask, return_logits=True)
    tok_p, lens_p, logits_p = m.generate(ids, 8, mask, return_logits=True, pool=pool)
    assert bool(torch.isfinite(logits_p).all())
    assert torch.equal(tok_p, tok) and torch.equal(lens_p, lens) and torch.equal(logits_p, logits)
    assert pool.num_free == free
    state = m.prefill(ids, mask, pool=pool)
    for t in range(6):  # width 60 -> 66: the second page arrives with row 64
        m.decode_step(state, tok[:, t])
    assert pool.num_free == free - 4
    state.release()
    assert pool.num_free == free and not bool(state.cache.block_table.any())
