"""attn_decode_split.hip on the GPU: the split + merge launches against float64 within a derived allowance, and the
three bitwise properties of the design (one split = the single kernels; no bit depends on gc, on the batch or on
Smax). Every launch runs on guarded buffers with a NaN-filled workspace. Ck = C.attn_decode_split_keys()."""
import pytest
import torch

from ml_trainer_amd.ops import gqa as Q
from tests.attn_decode_ref import _LOG2E, decode_bound_terms, decode_edge_inputs, decode_effective, nan_stale_rows
from tests.helpers import assert_guard_intact, assert_within, bf16_t_used, guarded, guarded_like, store_bound

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _C():
    from ml_trainer_amd.ops._ext import require_native
    return require_native()


def _bits(x):
    return x.contiguous().view(torch.int16)


def _split(dev, qkv, kv, pos, H, scale, rope=None, gc=0):
    """One C.attn_decode_split launch on guarded buffers and a NaN workspace: (out, kv after) on the device."""
    C = _C()
    _, B, Hkv, Smax, _ = kv.shape
    qbuf, q = guarded_like(qkv.to(dev))
    kbuf, k2 = guarded_like(kv.to(dev).view(-1, 64))
    obuf, out = guarded(B, H * 64, BF16, dev)
    shape = C.attn_decode_split_ws(B, H, Smax)
    wbuf, w2 = guarded(B * H * shape[2], shape[3], torch.float32, dev)
    w2.fill_(float("nan"))
    C.attn_decode_split(q, k2.view(kv.shape), pos.to(dev), out, w2.view(shape), H, scale, rope=rope, gc=gc)
    torch.cuda.synchronize()
    for buf, view in ((qbuf, q), (kbuf, k2), (obuf, out), (wbuf, w2)):
        assert_guard_intact(buf, view)
    assert torch.equal(_bits(q), _bits(qkv.to(dev)))
    return out.clone(), k2.view(kv.shape).clone()


def _table(dev, rope, Smax):
    from ml_trainer_amd.ops.rope import rope_table
    return rope_table(Smax, device=dev) if rope else None


def _cases():
    Ck = _C().attn_decode_split_keys()
    return {"a": (4, 2, 2 * Ck + 136, [0, Ck - 1, Ck, Ck + 1]), "b": (4, 2, 3 * Ck + 8, [2 * Ck - 1, 2 * Ck, 2 * Ck + 129, 3 * Ck + 7]),
            "c": (3, 1, Ck + 16, [Ck + 7, Ck + 8, Ck + 15])}


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("name,scale", [("a", 0.125), ("b", 0.125), ("b", 0.2), ("c", 0.125)])
def test_within_bound(dev, name, scale, rope):
    """Split + merge against decode_bound_terms (fp64) within store_bound(O, t_core + 2 t_merge, bf16); the append
    bitwise, nothing else written; NaN in the stale rows changes no bit; a second launch agrees bitwise.

    The allowance. Inside a split the arithmetic is the single kernel's over fewer keys: t_core and t_merge bound it
    as they stand (t_merge counts steps = ceil(n / 128) over the WHOLE key range, which no split exceeds). The merge
    kernel adds, per key, one more rescale a_z = exp2(M_z - M*): one e_m term of t_merge already carries
    steps + 1 >= 1 such factors. It adds at most 2 Za roundings on O and on L (Za splits, a multiply and an add
    or one fma each), and 2 Za <= steps + 7 because C >= 256 = 2 x 128 gives Za <= max(1, ceil(steps / 2)): the
    (steps + 7) 2^-24 terms of t_merge cover them. Hence one more t_merge.

    Inputs: decode_edge_inputs, plus the lead multiple of q in cache row pos - 1 of the last plain (b, h): the
    one-key tail of the last active split then carries the row. Case c has a single plain (b, h), which stays
    random (a true average across splits); its plant goes into the last sentinel (b, h), where it shares the lead
    with the new token (half the row each).

    Measured (MI355X), all eight parametrisations: |err| / bound 1.000 (the bf16 rounding itself); bf16_t_used
    0.0015 in case c without rope, below 1e-5 in the other seven."""
    B, H, Smax, pos = _cases()[name]
    qkv, kv, p = decode_edge_inputs((B, H, Smax, pos, scale), 7)
    table = _table(dev, rope, Smax)
    rot = qkv
    if rope:  # what the kernel dots and appends: q and k rotated by pos[b], rounded to bf16 (bitwise ops/rope.py)
        from ml_trainer_amd.ops.rope import rope_qk_reference
        rot = rope_qk_reference(qkv, table.cpu(), H, pos=p)
    plain = [(b, h) for b in range(B) for h in range(H) if (b + h) % 2 and pos[b] >= 1]
    b, h = plain[-1] if len(plain) > 1 else [(b, h) for b in range(B) for h in range(H) if not (b + h) % 2][-1]
    qv = rot.view(B, 3, H, 64)[b, 0, h].double()
    kv[0, b, h, pos[b] - 1] = (qv * (40.0 / (qv.pow(2).sum().item() * scale * _LOG2E))).to(BF16)
    O, t_core, t_merge = decode_bound_terms(*decode_effective(rot, kv, pos), pos, scale)
    O, t = O.view(B, H * 64), (t_core + 2 * t_merge).view(B, H * 64)

    out, kv_after = _split(dev, qkv, kv, p, H, scale, table)
    r = assert_within(out.cpu(), O, store_bound(O, t, BF16), f"case {name}")
    print(f"case {name} scale {scale} rope {rope}: |err| / bound {r:.3f}, bf16_t_used {bf16_t_used(out.cpu(), O, t):.5f}")
    x = rot.view(B, 3, H, 64).to(dev)
    for cache in (kv, nan_stale_rows(kv, pos)):
        want = cache.to(dev).clone()
        for i in range(B):
            want[0, i, :, pos[i]], want[1, i, :, pos[i]] = x[i, 1], x[i, 2]
        o2, after = _split(dev, qkv, cache, p, H, scale, table)  # (the first pass repeats the launch: determinism)
        assert bool(torch.isfinite(o2.float()).all()) and torch.equal(_bits(o2), _bits(out))
        assert torch.equal(_bits(after), _bits(want))
        assert cache is not kv or torch.equal(_bits(kv_after), _bits(want))


def _gqa_inputs(H, Hkv, Smax, pos, seed):
    g = torch.Generator().manual_seed(seed)
    compact = (torch.randn(len(pos), Q.compact_width(H, Hkv), generator=g) * 0.5).to(BF16)
    kv = nan_stale_rows((torch.randn(2, len(pos), Hkv, Smax, 64, generator=g) * 0.5).to(BF16), pos)
    return compact, kv, torch.tensor(pos, dtype=torch.int32)


@pytest.mark.parametrize("rope", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("H,Hkv", [(2, 2), (6, 2), (4, 1)])
def test_one_split_has_the_single_kernels_bits(dev, H, Hkv, rope):
    C, Ck = _C(), _C().attn_decode_split_keys()
    Smax, pos = 2 * Ck, [0, 7, 129, Ck]
    qkv, kv, p = _gqa_inputs(H, Hkv, Smax, pos, 10 * H + Hkv)
    table = _table(dev, rope, Smax)
    out, kv_after = _split(dev, qkv, kv, p, H, 0.125, table)
    want, kv_s = torch.empty_like(out), kv.to(dev)
    if Hkv == H:
        C.attn_decode(qkv.to(dev), kv_s, p.to(dev), want, H, 0.125, rope=table)
    else:
        C.attn_decode_gqa(qkv.to(dev), kv_s, p.to(dev), want, H, 0.125, rope=table)
    assert bool(torch.isfinite(want.float()).all())
    assert torch.equal(_bits(out), _bits(want)) and torch.equal(_bits(kv_after), _bits(kv_s))


@pytest.mark.parametrize("H,Hkv", [(6, 2), (8, 2)])
def test_bits_independent_of_gc_batch_and_smax(dev, H, Hkv):
    Ck, G = _C().attn_decode_split_keys(), H // Hkv
    Smax, pos = 2 * Ck + 40, [5, Ck + 33, 2 * Ck + 39]
    qkv, kv, p = _gqa_inputs(H, Hkv, Smax, pos, H)
    base, kv_base = _split(dev, qkv, kv, p, H, 0.125, gc=1)
    for gc in [0] + [d for d in (2, 3, 4, 6, 8) if G % d == 0]:
        out, kv_after = _split(dev, qkv, kv, p, H, 0.125, gc=gc)
        assert torch.equal(_bits(out), _bits(base)) and torch.equal(_bits(kv_after), _bits(kv_base)), f"gc={gc}"
    wide = Q.gqa_expand_reference(qkv, H, Hkv).contiguous()
    mha, _ = _split(dev, wide, kv.repeat_interleave(G, dim=2).contiguous(), p, H, 0.125)
    assert torch.equal(_bits(mha), _bits(base)), "the multi-head launch on the repeated cache"
    big = torch.full((2, 1, Hkv, Smax + Ck, 64), float("nan"), dtype=BF16)  # sequence 1 alone, in a longer cache
    big[:, :, :, :Smax] = kv[:, 1:2]
    alone, _ = _split(dev, qkv[1:2], big, p[1:2], H, 0.125)
    assert torch.equal(_bits(alone[0]), _bits(base[1])), "alone, Smax + Ck"


def test_refused_calls(dev):
    C, Ck = _C(), _C().attn_decode_split_keys()
    B, H, Hkv, Smax = 2, 4, 2, Ck + 8
    z = lambda *s, dt=BF16: torch.full(s, 3.0, dtype=dt, device=dev)
    shape = C.attn_decode_split_ws(B, H, Smax)
    assert list(shape) == [B, H, 2, 68]
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    out, kv = z(B, H * 64), z(2, B, Hkv, Smax, 64)
    ok = lambda: dict(qkv_new=z(B, 8 * 64), kv=kv, pos=pos, out=out, ws=z(*shape, dt=torch.float32), H=H, scale=0.125)
    bad = [dict(ws=z(B, H, 1, 68, dt=torch.float32)), dict(ws=z(*shape)), dict(ws=z(*shape, dt=torch.float64)),
           dict(ws=z(B * H * 2 * 68 + 1, dt=torch.float32)[1:].view(shape)), dict(gc=4), dict(gc=5),
           dict(pos=torch.zeros(B + 1, dtype=torch.int32, device=dev)), dict(pos=pos.long())]
    for over in bad:
        with pytest.raises((RuntimeError, TypeError, ValueError)):
            C.attn_decode_split(**{**ok(), **over})
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((kv == 3.0).all()), "a refused call wrote something"
    C.attn_decode_split(**ok())
