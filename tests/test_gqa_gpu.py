"""Grouped-query attention on the GPU: ``C.attn_decode_gqa`` bitwise against ``C.attn_decode`` on the repeated
cache and against float64 (tests/attn_decode_ref.py's derived allowance), ``C.gqa_expand`` / ``C.gqa_reduce`` bitwise
against ops/gqa.py, and bert-tiny with ``kv_heads`` at the thresholds of tests/test_clm_gpu.py (training) and
tests/test_generate_gpu.py / tests/test_preln_gpu.py (decode: TOL = 5e-2, bitwise where those are bitwise)."""
import pytest
import torch

from ml_trainer_amd.ops import gqa as Q
from tests.attn_decode_ref import decode_bound, decode_effective, nan_stale_rows
from tests.helpers import assert_guard_intact, assert_within, guarded, guarded_like, store_bound
from tests.test_clm_gpu import _batch, _grads
from tests.test_unpad_gpu import _close

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
B, SMAX, SCALE = 5, 160, 0.125
# (H, Hkv): G = 2, 3, 4, 6, 8, 12, 16, 5 and bert-base's 3. Every listed GC that divides G is forced in turn (so
# GC = 2, 3, 4, 6, 8; 6 x 2, 8 x 2, 1 x 5 chunks), next to the launcher's own choice (gc = 0)
CASES = [(4, 2), (3, 1), (4, 1), (6, 1), (8, 1), (12, 1), (16, 2), (5, 1), (12, 4)]
# every case: an empty cache, a wave boundary, a workgroup-step boundary, the last row, and one of the others
POS_FIXED, POS_OTHER = [0, 32, 128, 159], [1, 7, 8, 31, 127, 129]


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == BF16 else torch.int32)


def _decode_case(dev, H, Hkv, rope, strided, gc=0):
    """One launch of each kernel on the same problem; everything a test compares, as a dict."""
    from ml_trainer_amd.ops._ext import require_native
    from ml_trainer_amd.ops.rope import rope_table
    C, G, W = require_native(), H // Hkv, Q.compact_width(H, Hkv)
    g = torch.Generator().manual_seed(100 * H + Hkv)
    pos = POS_FIXED + [POS_OTHER[(H + Hkv) % len(POS_OTHER)]]
    pos_t = torch.tensor(pos, dtype=torch.int32, device=dev)
    compact = (torch.randn(B, W, generator=g) * 0.5).to(BF16).to(dev)
    kv0 = nan_stale_rows((torch.randn(2, B, Hkv, SMAX, 64, generator=g) * 0.5).to(BF16), pos).to(dev)
    table = rope_table(SMAX, device=dev) if rope else None
    # the MHA kernel on the G-times repeated cache and the expanded row
    wide = Q.gqa_expand_reference(compact, H, Hkv).contiguous()
    kv_rep = kv0.repeat_interleave(G, dim=2).contiguous()
    kv_rep0 = kv_rep.clone()
    want = torch.empty(B, H * 64, dtype=BF16, device=dev)
    C.attn_decode(wide, kv_rep, pos_t, want, H, SCALE, rope=table)
    # the GQA kernel, every buffer inside sentinels
    qbuf, q = guarded_like(compact, ld=W + 16 if strided else None, col_off=8 if strided else 0)
    kbuf, kflat = guarded(2 * B * Hkv * SMAX, 64, BF16, dev)
    kv = kflat.view(2, B, Hkv, SMAX, 64)
    _bits(kv).copy_(_bits(kv0))
    obuf, out = guarded(B, H * 64, BF16, dev)
    C.attn_decode_gqa(q, kv, pos_t, out, H, SCALE, rope=table, gc=gc)
    first = out.clone()
    C.attn_decode_gqa(q, kv, pos_t, out, H, SCALE, rope=table, gc=gc)  # row pos[b] now holds the same token
    torch.cuda.synchronize()
    for buf, view in ((qbuf, q), (kbuf, kflat), (obuf, out)):
        assert_guard_intact(buf, view)
    return dict(G=G, pos=pos, wide=wide, kv_rep0=kv_rep0, kv_rep=kv_rep, want=want, kv0=kv0, kv=kv, first=first, out=out)


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("H,Hkv", CASES)
def test_decode_is_bitwise_the_mha_kernel_on_the_repeated_cache(dev, H, Hkv, rope):
    gcs = [0] + [d for d in (1, 2, 3, 4, 6, 8) if (H // Hkv) % d == 0]
    for gc, strided in [(gc, bool(i % 2)) for i, gc in enumerate(gcs)] + [(gcs[-1], len(gcs) % 2 == 0)]:
        r = _decode_case(dev, H, Hkv, rope, strided, gc)
        assert bool(torch.isfinite(r["want"].float()).all())
        assert torch.equal(_bits(r["first"]), _bits(r["want"])), f"out, gc={gc} strided={strided}"
        assert torch.equal(_bits(r["out"]), _bits(r["first"])), "a second launch"
        expect = r["kv0"].clone()  # nothing but row pos[b] changes, and it takes the MHA kernel's appended row
        for b, n in enumerate(r["pos"]):
            expect[:, b, :, n] = r["kv_rep"][:, b, ::r["G"], n]
        assert torch.equal(_bits(r["kv"]), _bits(expect)), f"cache, gc={gc} strided={strided}"


@pytest.mark.parametrize("H,Hkv", [(4, 2), (12, 1), (5, 1)])
def test_decode_against_float64(dev, H, Hkv):
    r = _decode_case(dev, H, Hkv, False, False)
    q, k, v = decode_effective(r["wide"].cpu(), r["kv_rep0"].cpu(), r["pos"])
    O, t = decode_bound(q, k, v, r["pos"], SCALE)
    used = assert_within(r["out"].cpu().view(B, H, 64), O, store_bound(O, t, BF16), f"H {H} Hkv {Hkv}")
    print(f"H {H} Hkv {Hkv}: largest |err| / tolerance {used:.3f}")


@pytest.mark.parametrize("H,Hkv", [(4, 2), (3, 1), (12, 4), (12, 1)])
@pytest.mark.parametrize("rows", [1, 3, 67, 300])
def test_expand_and_reduce_equal_the_oracle(dev, rows, H, Hkv):
    from ml_trainer_amd.ops._ext import require_native
    C, G, W = require_native(), H // Hkv, Q.compact_width(H, Hkv)
    g = torch.Generator().manual_seed(rows + 1000 * H + Hkv)

    def data(cols):  # mixed signs, exponents over 2^-8 .. 2^8: fp32 sums that depend on their order
        mag = torch.exp2(torch.rand(rows, cols, generator=g) * 16 - 8) * (1 + torch.rand(rows, cols, generator=g))
        return (mag * (torch.randint(0, 2, (rows, cols), generator=g) * 2 - 1)).to(BF16).to(dev)

    cbuf, compact = guarded_like(data(W), ld=W + 16, col_off=8)
    wbuf, wide = guarded(rows, 3 * H * 64, BF16, dev)
    C.gqa_expand(compact, wide, H, Hkv)
    assert torch.equal(_bits(wide), _bits(Q.gqa_expand_reference(compact, H, Hkv)))
    d = data(3 * H * 64)
    if G > 2:
        # bf16 has 8 significant bits, so inside 2^-8 .. 2^8 every two-term fp32 sum is exact and three terms round
        # once, whatever their order: the random data alone cannot tell the orders apart at G = 3. One planted
        # group per KV head does (row 0, dim 0 of dk): s = 2^-8 + 2^-15 first, then +2^9, zeros, -2^9 last.
        # Ascending: fl(s + 512) drops the 2^-15 (a tie, to even) -> 2^-8; descending: (-512 + 512) + s = s.
        grp = d[0, H * 64:2 * H * 64].view(Hkv, G, 64)
        grp[:, :, 0] = 0.0
        grp[:, 0, 0], grp[:, 1, 0], grp[:, G - 1, 0] = 2.0 ** -8 + 2.0 ** -15, 512.0, -512.0
    dbuf, dwide = guarded_like(d, ld=3 * H * 64 + 16, col_off=8)
    rbuf, red = guarded(rows, W, BF16, dev)
    C.gqa_reduce(dwide, red, H, Hkv)
    assert torch.equal(_bits(red), _bits(Q.gqa_reduce_reference(dwide, H, Hkv)))
    if G > 2:  # (two terms commute.) The fixture tells the orders apart: a wrong order cannot pass
        assert not torch.equal(_bits(red), _bits(Q.gqa_reduce_reference(dwide, H, Hkv, reverse=True)))
    for buf, view in ((cbuf, compact), (wbuf, wide), (dbuf, dwide), (rbuf, red)):
        assert_guard_intact(buf, view)


# ------------------------------------------------------------------------------------------------ the model
MODELS = {"kv2": dict(kv_heads=2), "kv1": dict(kv_heads=1),
          "kv1-rotary-preln-rms": dict(kv_heads=1, rotary=True, pre_ln=True, norm="rmsnorm")}
S, PW, STEPS, PLENS, TOL = 80, 48, 32, [48, 33, 1], 5e-2  # tests/test_generate_gpu.py


def _model(dev, name):
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny", **MODELS[name])).to(dev)
    with torch.no_grad():
        m.mlm_bias.normal_(std=0.1)
    return m


@pytest.mark.parametrize("name", list(MODELS))
def test_training_step_matches_reference(dev, name):
    m = _model(dev, name).train()
    ids, mask, labels = _batch(dev)
    hn, ln, gn = _grads(m, m, m.lm_loss, ids, mask, labels)
    hr, lr, gr = _grads(m, m.forward_reference, m.lm_loss_reference, ids, mask, labels)
    _, la, ga = _grads(m, m.forward_torch_bf16, m.mlm_loss_torch_bf16, ids, mask, labels)
    _close(hn, hr, 5e-2)
    assert abs(float(ln) - float(lr)) <= 5e-2 * abs(float(lr))
    assert tuple(gn["layers.0.qkv.weight"].shape) == ((4 + 2 * MODELS[name]["kv_heads"]) * 64, 256)
    for n in gr:
        nr = gr[n].norm().item()
        if nr < 1e-8:
            continue
        e_nat, e_ac = (gn[n] - gr[n]).norm().item() / nr, (ga[n] - gr[n]).norm().item() / nr
        print(f"{n}: native rel err {e_nat:.4f} vs autocast {e_ac:.4f}")
        assert e_nat <= max(2.0 * e_ac, 0.02), f"{n}: native rel err {e_nat:.4f} vs autocast {e_ac:.4f}"


def _decode(m, state, feed):
    hs, ls = [state.hidden.clone()], [m.decode_step(state)]
    for t in range(feed.shape[1]):
        ls.append(m.decode_step(state, feed[:, t]))
        hs.append(state.hidden.clone())
    return torch.stack(hs), torch.stack(ls)


@pytest.mark.parametrize("name", list(MODELS))
def test_cached_decode_graph_and_batch_invariance(dev, name, monkeypatch):
    from ml_trainer_amd.ops.decode import DecodeState, KVCache
    monkeypatch.delenv("MLT_DECODE_GEMM", raising=False)
    m = _model(dev, name).eval()
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(5, 1000, (3, S), generator=g).to(dev)
    pl = torch.tensor(PLENS, device=dev)
    prompt, pmask = ids[:, :PW].clone(), (torch.arange(PW, device=dev)[None, :] < pl[:, None]).long()
    feed = torch.stack([ids[b, PLENS[b]:PLENS[b] + STEPS] for b in range(3)])
    fmask = (torch.arange(S, device=dev)[None, :] < (pl + STEPS)[:, None]).long()
    rows = torch.stack([torch.arange(3, device=dev) * S + pl - 1 + k for k in range(STEPS + 1)])
    with torch.no_grad():
        hr = m.forward_reference(ids, fmask)
        ref_logits = m.mlm_logits(hr, torch.arange(3 * S, device=dev))
        nat_logits = m.mlm_logits(m(ids, fmask), torch.arange(3 * S, device=dev))
        state = m.prefill(prompt, pmask, max_len=S)
        assert tuple(state.cache.kv[0].shape) == (2, 3, MODELS[name]["kv_heads"], S, 64)
        alone = DecodeState(KVCache([kv[:, 1:2].clone() for kv in state.cache.kv], state.cache.pos[1:2].clone(), S),
                            state.hidden[1:2].clone())
        hidden, logits = _decode(m, state, feed)
        ha, la = _decode(m, alone, feed[1:2, :8])
    # cached against the fp32 reference and against the uncached native forward (tests/test_generate_gpu.py)
    for k in range(STEPS + 1):
        _close(hidden[k], hr.view(3 * S, -1)[rows[k]], TOL)
        _close(logits[k], ref_logits[rows[k]], TOL)
    ref, nat, dec = ref_logits[rows.reshape(-1)], nat_logits[rows.reshape(-1)], logits.reshape(rows.numel(), -1)
    top = ref.topk(2, -1).values
    clear = (top[:, 0] - top[:, 1]) > 2 * TOL * float(ref.abs().max())
    assert int(clear.sum()) > 0 and torch.equal(dec.argmax(-1)[clear], nat.argmax(-1)[clear])
    # alone and in the batch of 3, from the same prefilled cache: hidden rows, logits, appended cache rows
    for k in range(9):
        assert torch.equal(_bits(ha[k, 0]), _bits(hidden[k, 1])), f"hidden, step {k}"
        assert torch.equal(_bits(la[k, 0]), _bits(logits[k, 1])), f"logits, step {k}"
    for l, kv in enumerate(alone.cache.kv):
        n = PLENS[1] + 8
        assert torch.equal(_bits(kv[:, 0, :, :n]), _bits(state.cache.kv[l][:, 1, :, :n])), f"cache, layer {l}"
    # the captured graph returns the eager loop's bits, on a replay too
    kw = dict(attention_mask=pmask, sampler="device", temperature=0.8, top_k=5, top_p=0.9, seed=21)
    eager = m.generate(prompt, STEPS, **kw)
    for _ in range(2):
        graph = m.generate(prompt, STEPS, graph=True, **kw)
        assert torch.equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1])
    assert m.decode_graph_captures == 1


def test_refusals(dev):
    from ml_trainer_amd.ops._ext import require_native
    C = require_native()
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=dev)
    pos = torch.zeros(2, dtype=torch.int32, device=dev)
    ok = lambda: dict(qkv_new=z(2, 8 * 64), kv=z(2, 2, 2, 16, 64), pos=pos, out=z(2, 4 * 64), H=4, scale=SCALE)
    C.attn_decode_gqa(**ok())
    bad = [dict(kv=z(2, 2, 3, 16, 64), qkv_new=z(2, 10 * 64)),  # 3 KV heads divide nothing
           dict(qkv_new=z(2, 12 * 64)), dict(qkv_new=z(2, 8 * 64, dt=torch.float32)), dict(out=z(2, 4 * 64, dt=torch.float32)),
           dict(qkv_new=z(2, 8 * 64 + 4)[:, 4:]), dict(pos=pos.long()), dict(gc=4)]
    for over in bad:
        with pytest.raises((RuntimeError, TypeError, ValueError)):
            C.attn_decode_gqa(**{**ok(), **over})
    for fn, a, b in ((C.gqa_expand, z(3, 8 * 64), z(3, 12 * 64)), (C.gqa_reduce, z(3, 12 * 64), z(3, 8 * 64))):
        fn(a, b, 4, 2)
        for x, y, h, hk in ((a.float(), b, 4, 2), (a, b.float(), 4, 2), (a, b, 4, 3), (a[:2], b, 4, 2),
                            (torch.cat((a, a), 1)[:, 4:4 + a.shape[1]], b, 4, 2)):
            with pytest.raises((RuntimeError, TypeError, ValueError)):
                fn(x, y, h, hk)
