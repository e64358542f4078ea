"""attn_decode_f8.hip on the GPU: the bytes kv_fill_f8 and a step's append write against the oracle of ops/decode.py,
the attention against float64 over the dequantised cache within the derived allowance of the bf16 kernels' tests, the
bitwise invariances, the model with kv_cache="fp8", and the refused calls. Every launch runs on guarded buffers."""
import pytest
import torch

from ml_trainer_amd.ops import decode as DC
from ml_trainer_amd.ops import gqa as Q
from ml_trainer_amd.ops.rope import rope_qk_reference, rope_table
from tests.attn_decode_ref import decode_bound_terms, decode_edge_inputs
from tests.helpers import assert_guard_intact, assert_within, bf16_t_used, guarded, guarded_1d, guarded_like, store_bound
from tests.test_unpad_gpu import _close

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _C():
    from ml_trainer_amd.ops._ext import require_native
    return require_native()


def _step(dev, qkv, codes, scales, pos, H, scale, table=None, split=False, gc=0):
    """One C.attn_decode_f8 launch on guarded buffers (and a NaN workspace): (out, codes after, scales after)."""
    C = _C()
    _, B, _, Smax, _ = codes.shape
    qbuf, q = guarded_like(qkv.to(dev))
    cbuf, c2 = guarded_like(codes.to(dev).view(-1, 64))
    sbuf, s1 = guarded_1d(scales.numel(), dev)
    s1.copy_(scales.reshape(-1))
    obuf, out = guarded(B, H * 64, BF16, dev)
    bufs, ws = [(qbuf, q), (cbuf, c2), (sbuf, s1), (obuf, out)], None
    if split:
        shape = C.attn_decode_split_ws(B, H, Smax)
        wbuf, w2 = guarded(B * H * shape[2], shape[3], torch.float32, dev)
        w2.fill_(float("nan"))
        bufs.append((wbuf, w2))
        ws = w2.view(shape)
    C.attn_decode_f8(q, c2.view(codes.shape), s1.view(scales.shape), pos.to(dev), out, H, scale, rope=table, ws=ws, gc=gc)
    torch.cuda.synchronize()
    for buf, view in bufs:
        assert_guard_intact(buf, view)
    return out.cpu(), c2.view(codes.shape).cpu(), s1.view(scales.shape).cpu()


def _inputs(H, Hkv, Smax, pos, scale, seed=7):
    """decode_edge_inputs (its sentinels on every KV head's first query head), compact for Hkv < H, the cache
    quantised by the oracle; then every row j > pos[b] holds code 0x7F and a NaN scale, row pos[b] an infinite one
    over the codes of the negated lead."""
    G = H // Hkv
    qkv, kv, p = decode_edge_inputs((len(pos), H, Smax, pos, scale), seed)
    x = qkv.view(len(pos), 3, H, 64)
    qkv = torch.cat([x[:, 0].reshape(len(pos), -1), x[:, 1, ::G].reshape(len(pos), -1), x[:, 2, ::G].reshape(len(pos), -1)], 1)
    codes, scales = DC.kv_quantize_reference(kv[:, :, ::G])
    for b, n in enumerate(pos):
        codes[:, b, :, n + 1:], scales[:, b, :, n + 1:], scales[:, b, :, n] = 0x7F, float("nan"), float("inf")
    return qkv.contiguous(), codes.contiguous(), scales.contiguous(), p


def _expected(qkv, codes, scales, p, H, scale, table):
    """(O, t_core, t_merge [B, H * 64] fp64, codes after, scales after): the oracle places the new row, the fp64
    reference runs over the dequantised rows j <= pos[b] with the (rotated, bf16) queries the kernel dots."""
    B, Hkv = codes.shape[1], codes.shape[2]
    c, s = codes.clone(), scales.clone()
    DC.attn_decode_reference(qkv, c, p, H, scale, rope=table, kv_scale=s)
    wide = Q.gqa_expand_reference(qkv, H, Hkv) if Hkv != H else qkv
    if table is not None:
        wide = rope_qk_reference(wide, table, H, pos=p)
    k, v = DC.kv_dequantize_reference(c, s).double().repeat_interleave(H // Hkv, dim=2).unbind(0)
    terms = decode_bound_terms(wide.double().view(B, 3, H, 64)[:, 0], k, v, p.tolist(), scale)
    return [t.reshape(B, H * 64) for t in terms] + [c, s]


def _check(dev, H, Hkv, Smax, pos, scale, rope, split, gc, what):
    qkv, codes, scales, p = _inputs(H, Hkv, Smax, pos, scale)
    table = rope_table(Smax) if rope else None
    O, t_core, t_merge, c_want, s_want = _expected(qkv, codes, scales, p, H, scale, table)
    out, c_got, s_got = _step(dev, qkv, codes, scales, p, H, scale, None if table is None else table.to(dev), split, gc)
    t = t_core + (2 if split else 1) * (8 / 7) * t_merge
    r = assert_within(out, O, store_bound(O, t, BF16), what)
    print(f"{what}: |err| / bound {r:.3f}, bf16_t_used {bf16_t_used(out, O, t):.5f}")
    assert torch.equal(c_got, c_want) and torch.equal(s_got.view(torch.int32), s_want.view(torch.int32)), "the append"
    return out


CASES = [(1, [0], 0.125), (40, [15, 16, 17], 0.125), (130, [63, 64, 65], 0.2), (300, [255, 256, 257, 299], 0.125)]


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("H,Hkv,gc", [(2, 2, 1), (6, 2, 3), (4, 1, 4), (8, 1, 2)])
@pytest.mark.parametrize("Smax,pos,scale", CASES, ids=[f"Smax{c[0]}" for c in CASES])
def test_within_bound(dev, Smax, pos, scale, H, Hkv, gc, rope):
    """out against decode_bound_terms (fp64) over kv_dequantize_reference of the cache, within
    store_bound(O, t_core + 8/7 t_merge, bf16); the row pos[b] the step writes equals the oracle's bytes and no other
    byte of the cache changes. Stale rows hold NaN codes and NaN scales, row pos[b] an infinite scale.

    The allowance is the bf16 kernels' with their operation counts: scores are a 16-term fma chain + 2 quad levels
    (18 <= 64 additions of exact bf16 x e4m3 products, helpers._attn_eta as it stands); a state sums at most
    ceil(n / 16) + 1 <= c1 keys; the loop takes ceil(n / 256) <= steps rescales; the scales are powers of two and add
    no term. The merge has a FOURTH butterfly level (16 lane groups): I' + 1 multiplies + 4 levels + 3 wave additions
    = I' + 8 operations against the I + 7 that t_merge counts, I' <= I, so new / old <= 8 / 7 (reached at n = 0):
    t_merge is scaled by 8 / 7. The boundaries are the kernel's: 16 keys (a load), 64 (a wave), 256 (a step)."""
    _check(dev, H, Hkv, Smax, pos, scale, rope, False, gc, f"Smax {Smax} H {H}/{Hkv} gc {gc} rope {rope}")


@pytest.mark.parametrize("H,Hkv", [(2, 2), (4, 1)])
def test_split_within_bound_and_invariances(dev, H, Hkv):
    """The split form (Smax = 2048, one workgroup per 256 keys, then attn_decode_merge_kernel) against the same
    reference within t_core + 2 x 8/7 t_merge: the merge kernel's 2 Za <= steps + 7 roundings and its one more rescale
    are a second t_merge, as in tests/test_attn_decode_split_gpu.py (C = 256 here too). Then: a row's bits do not
    depend on gc, on the batch it is decoded in, or on Smax (2048 against 4096)."""
    pos, G = [0, 255, 256, 257, 2047], H // Hkv
    base = _check(dev, H, Hkv, 2048, pos, 0.125, True, True, 0, f"split H {H}/{Hkv}")
    qkv, codes, scales, p = _inputs(H, Hkv, 2048, pos, 0.125)
    table = rope_table(4096, device=dev)
    for gc in [d for d in (1, 2, 4) if G % d == 0]:
        assert torch.equal(_step(dev, qkv, codes, scales, p, H, 0.125, table, True, gc)[0].view(torch.int16), base.view(torch.int16))
    big_c = torch.full((2, 1, Hkv, 4096, 64), 0x7F, dtype=torch.uint8)
    big_s = torch.full((2, 1, Hkv, 4096), float("nan"))
    big_c[:, :, :, :2048], big_s[:, :, :, :2048] = codes[:, 3:4], scales[:, 3:4]
    alone = _step(dev, qkv[3:4], big_c, big_s, p[3:4], H, 0.125, table, True)[0]
    assert torch.equal(alone[0].view(torch.int16), base[3].view(torch.int16)), "alone, Smax 4096"


@pytest.mark.parametrize("G", [6, 8])
def test_bits_independent_of_gc(dev, G):
    qkv, codes, scales, p = _inputs(G, 1, 300, [17, 256, 299], 0.125)
    base = _step(dev, qkv, codes, scales, p, G, 0.125, gc=1)
    for gc in [0] + [d for d in (2, 3, 4, 6, 8) if G % d == 0]:
        got = _step(dev, qkv, codes, scales, p, G, 0.125, gc=gc)
        assert all(torch.equal(a.view(torch.int16 if a.dtype == BF16 else torch.uint8), b.view(torch.int16 if b.dtype == BF16 else torch.uint8))
                   for a, b in zip(got, base)), f"gc={gc}"


@pytest.mark.parametrize("Hkv", [4, 2, 1])
def test_fill_bytes(dev, Hkv):
    """kv_fill_f8 from the wide and from the compact buffer: rows 0 .. S - 1 equal the oracle byte for byte, every
    other row of the guarded cache keeps its bytes."""
    B, H, S, Smax = 3, 4, 5, 40
    g = torch.Generator().manual_seed(Hkv)
    compact = (torch.randn(B * S, Q.compact_width(H, Hkv), generator=g) * torch.exp2(torch.randint(-12, 12, (B * S, 1), generator=g).float())).to(BF16)
    wide = Q.gqa_expand_reference(compact, H, Hkv).contiguous()
    want_c, want_s = torch.full((2, B, Hkv, Smax, 64), 0x11, dtype=torch.uint8), torch.full((2, B, Hkv, Smax), 7.0)
    x = wide.view(B, S, 3, H, 64)[:, :, 1:, ::H // Hkv].permute(2, 0, 3, 1, 4)
    want_c[:, :, :, :S], want_s[:, :, :, :S] = DC.kv_quantize_reference(x)
    for qkv in (wide, compact):
        qbuf, q = guarded_like(qkv.to(dev))
        cbuf, c2 = guarded(2 * B * Hkv * Smax, 64, torch.uint8, dev)
        sbuf, s1 = guarded_1d(2 * B * Hkv * Smax, dev)
        c2.fill_(0x11), s1.fill_(7.0)
        _C().kv_fill_f8(q, c2.view(want_c.shape), s1.view(want_s.shape), B, S, H)
        torch.cuda.synchronize()
        for buf, view in ((qbuf, q), (cbuf, c2), (sbuf, s1)):
            assert_guard_intact(buf, view)
        assert torch.equal(c2.cpu().view(want_c.shape), want_c) and torch.equal(s1.cpu().view(want_s.shape), want_s)


def test_model_fp8(dev):
    """bert-tiny, rotary, kv_heads 2: decode_step logits on an fp8 cache against the CPU fp32 path of the same model
    and option (tests/test_generate_gpu.py's tolerance: 5e-2 of the reference's largest magnitude); the graph-replayed
    generation returns the eager tokens; a sequence alone gets the logits it gets in a batch of 3, bit for bit."""
    import copy
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    ref = BertLMHeadModel(bert_config("bert-tiny", rotary=True, kv_heads=2)).eval()
    m = copy.deepcopy(ref).to(dev).eval()
    ids = torch.randint(5, 1000, (3, 24), generator=torch.Generator().manual_seed(5))
    lens = torch.tensor([24, 17, 1])
    mask = (torch.arange(24)[None, :] < lens[:, None]).long()
    feed = torch.randint(5, 1000, (3, 20), generator=torch.Generator().manual_seed(6))
    sr, sg = ref.prefill(ids, mask, max_len=48, kv_cache="fp8"), m.prefill(ids.to(dev), mask.to(dev), max_len=48, kv_cache="fp8")
    cg = sg.cache  # sequence 1 alone, from the same prefilled cache (as tests/test_gqa_gpu.py takes it)
    s1 = DC.DecodeState(DC.KVCache([x[:, 1:2].clone() for x in cg.kv], cg.pos[1:2].clone(), 48,
                                   [x[:, 1:2].clone() for x in cg.scales]), sg.hidden[1:2].clone())
    assert cg.kv[0].dtype == torch.uint8 and cg.scales[0].is_cuda and cg.scales[0].shape == (2, 3, 2, 48)
    for t in range(20):
        lg = m.decode_step(sg, feed[:, t].to(dev))
        _close(lg.cpu(), ref.decode_step(sr, feed[:, t]), 5e-2)
        assert torch.equal(m.decode_step(s1, feed[1:2, t].to(dev))[0], lg[1]), f"step {t}: alone != in the batch"
    kw = dict(attention_mask=mask.to(dev), temperature=0.8, top_k=20, seed=3, sampler="device", kv_cache="fp8")
    eager = m.generate(ids.to(dev), 12, **kw)
    for _ in range(2):  # the capture, then a replay of the cached graph
        graphed = m.generate(ids.to(dev), 12, graph=True, **kw)
        assert torch.equal(graphed[0], eager[0]) and torch.equal(graphed[1], eager[1])
    assert m.decode_graph_captures == 1


def test_refused_calls(dev):
    C = _C()
    B, H, Hkv, Smax = 2, 4, 2, 300
    z = lambda *s, dt=BF16: torch.full(s, 3, dtype=dt, device=dev)
    shape = C.attn_decode_split_ws(B, H, Smax)
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    out, kv8, sc = z(B, H * 64), z(2, B, Hkv, Smax, 64, dt=torch.uint8), z(2, B, Hkv, Smax, dt=torch.float32)
    ok = lambda: dict(qkv_new=z(B, 8 * 64), kv8=kv8, kv_scale=sc, pos=pos, out=out, H=H, scale=0.125)
    bad = [dict(kv8=z(2, B, Hkv, Smax, 64)), dict(kv8=z(2, B, Hkv, Smax, 64, dt=torch.int8)),  # the code dtype
           dict(kv_scale=z(2, B, Hkv, Smax + 1, dt=torch.float32)), dict(kv_scale=z(2, B, Hkv, Smax, 1, dt=torch.float32)),
           dict(kv_scale=z(2, B, Hkv, Smax)), dict(ws=z(B, H, 1, 68, dt=torch.float32)),
           dict(ws=z(B * H * shape[2] * 68 + 1, dt=torch.float32)[1:].view(shape)),  # a misaligned workspace
           dict(kv8=z(2, B, 3, Smax, 64, dt=torch.uint8), kv_scale=z(2, B, 3, Smax, dt=torch.float32)),  # Hkv = 3, H = 4
           dict(gc=3), dict(pos=pos.long())]
    for over in bad:
        with pytest.raises((RuntimeError, TypeError, ValueError)):
            C.attn_decode_f8(**{**ok(), **over})
    with pytest.raises((RuntimeError, TypeError, ValueError)):
        C.kv_fill_f8(z(B * 5, 3 * H * 64), kv8, z(2, B, Hkv, Smax + 1, dt=torch.float32), B, 5, H)
    torch.cuda.synchronize()
    assert bool((out == 3).all()) and bool((kv8 == 3).all()) and bool((sc == 3).all()), "a refused call wrote something"
    C.attn_decode_f8(**ok())
    C.attn_decode_f8(**ok(), ws=z(*shape, dt=torch.float32))
