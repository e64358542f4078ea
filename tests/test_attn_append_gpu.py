"""C.attn_append (csrc/kernels/attn_append.hip) against the causal forward's derived bound.

The reference builds, per sequence, the full [n + T] q / k / v in fp64 (cached rows: q = 0, k / v from the cache; new
rows from qkv_new, rotated by ``rope_qk_reference`` where rope is on), calls ``attn_fwd_bound_masked`` with
``causal_valid`` and holds rows n .. n + T - 1 to ``store_bound``. Shapes: the 16-key tile, the 32-key wave step, the
128-key workgroup step and the 256-key split, each from below, at and above; pos + T == Smax; T = 1, 5, 16."""
import functools

import pytest
import torch

from tests.attn_causal_ref import attn_fwd_bound_masked, causal_valid
from tests.helpers import assert_guard_intact, assert_within, guarded, guarded_like, store_bound

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SCALE = 0.125
NAN = float("nan")

# (B, H, Hkv, Smax, pos, T, rope, split, gc)
CASES = [
    (1, 2, 2, 16, (0,), 16, False, False, 0),   # the triangle alone, pos + T == Smax
    (1, 2, 2, 8, (1,), 1, True, False, 0),
    (3, 2, 2, 64, (15, 16, 17), 1, False, False, 0),
    (3, 4, 2, 64, (15, 16, 17), 5, True, False, 0),
    (3, 6, 1, 64, (15, 16, 17), 16, False, False, 1),
    (3, 6, 1, 64, (31, 32, 33), 1, True, False, 2),
    (3, 2, 2, 64, (31, 32, 33), 5, True, False, 0),
    (3, 6, 1, 64, (31, 32, 33), 16, True, False, 3),
    (3, 4, 2, 160, (127, 128, 129), 5, False, False, 0),
    (3, 2, 2, 160, (127, 128, 144), 16, True, False, 0),  # 144 + 16 == Smax
    (3, 4, 2, 544, (255, 256, 257), 16, True, True, 0),
    (3, 4, 2, 544, (255, 256, 257), 16, True, False, 0),
    (3, 6, 1, 544, (513, 0, 539), 5, False, True, 3),     # 539 + 5 == Smax
    (3, 6, 1, 544, (513, 0, 539), 5, False, False, 0),
]


def _table(Smax, dev="cpu"):
    from ml_trainer_amd.ops.rope import rope_table
    return rope_table(Smax, device=dev)


@functools.lru_cache(maxsize=None)
def _inputs(B, H, Hkv, Smax, T, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * T + Smax)
    return (torch.randn(B * T, (H + 2 * Hkv) * 64, generator=g).to(BF16),
            torch.randn(2, B, Hkv, Smax, 64, generator=g).to(BF16))


@functools.lru_cache(maxsize=None)
def _expected(B, H, Hkv, Smax, pos, T, rope):
    """(O fp64 [B * T, H * 64], tol, new k, new v bf16 [B, T, Hkv, 64]) on the CPU."""
    from ml_trainer_amd.ops.gqa import gqa_expand_reference
    from ml_trainer_amd.ops.rope import rope_qk_reference
    qkv, kv = _inputs(B, H, Hkv, Smax, T)
    G = H // Hkv
    wide = gqa_expand_reference(qkv, H, Hkv) if G > 1 else qkv
    rows = (torch.tensor(pos)[:, None] + torch.arange(T)[None, :]).reshape(-1)
    if rope:
        wide = rope_qk_reference(wide, _table(Smax), H, pos=rows)
    x = wide.view(B, T, 3, H, 64)
    O, tol = [], []
    for b, n in enumerate(pos):
        S = n + T
        new = x[b].double().permute(1, 2, 0, 3)  # [3, H, T, 64]
        q = torch.cat((torch.zeros(H, n, 64, dtype=torch.float64), new[0]), 1)[None]
        k = torch.cat((kv[0, b, :, :n].double().repeat_interleave(G, 0), new[1]), 1)[None]
        v = torch.cat((kv[1, b, :, :n].double().repeat_interleave(G, 0), new[2]), 1)[None]
        o, t, _, _ = attn_fwd_bound_masked(q, k, v, causal_valid([S], 1, S), SCALE)
        O.append(o[0, :, n:].permute(1, 0, 2).reshape(T, H * 64))
        tol.append(t[0, :, n:].permute(1, 0, 2).reshape(T, H * 64))
    O, tol = torch.cat(O), torch.cat(tol)
    return O, store_bound(O, tol, BF16), x[:, :, 1, ::G].contiguous(), x[:, :, 2, ::G].contiguous()


def _launch(C, qv, kvd, posd, B, H, T, Smax, rope, split, gc):
    dev = qv.device
    obuf, ov = guarded(B * T, H * 64, BF16, dev)
    kw = {}
    if split:
        kw = dict(ws=torch.full(C.attn_append_ws(B, T, H, Smax), NAN, dtype=torch.float32, device=dev),
                  row_pos=torch.full((B * T,), -1, dtype=torch.int32, device=dev))
    C.attn_append(qv, kvd, posd, ov, B, H, SCALE, rope=_table(Smax, dev) if rope else None, gc=gc, **kw)
    torch.cuda.synchronize()
    assert_guard_intact(obuf, ov)
    if split:
        assert kw["row_pos"].view(B, T).tolist() == [[int(n)] * T for n in posd.tolist()]
    return ov.clone()


def _run(dev, case, qkv=None, nan=False, ld=None, check_cache=True):
    """One launch on guarded buffers: the output, after the cache / input / guard checks."""
    from ml_trainer_amd.ops._ext import require_native
    C = require_native()
    B, H, Hkv, Smax, pos, T, rope, split, gc = case
    q0, kv = _inputs(B, H, Hkv, Smax, T)
    qkv = q0 if qkv is None else qkv
    kv = kv.clone()
    for b, n in enumerate(pos):
        kv[:, b, :, n:] = NAN if nan else 3.0  # the stale rows
    kbuf, kview = guarded_like(kv.view(-1, 64).to(dev))
    kvd = kview.view(2, B, Hkv, Smax, 64)
    qbuf, qv = guarded_like(qkv.to(dev), ld=ld)
    posd = torch.tensor(pos, dtype=torch.int32, device=dev)
    out = _launch(C, qv, kvd, posd, B, H, T, Smax, rope, split, gc)
    assert_guard_intact(kbuf, kview)
    assert_guard_intact(qbuf, qv)
    assert torch.equal(qv.cpu().view(torch.int16), qkv.view(torch.int16)) and posd.tolist() == list(pos)
    if check_cache:
        _, _, nk, nv = _expected(B, H, Hkv, Smax, pos, T, rope)
        for b, n in enumerate(pos):  # rows n .. n + T - 1 are the (rotated) new k / v, everything else is untouched
            kv[0, b, :, n:n + T] = nk[b].permute(1, 0, 2)
            kv[1, b, :, n:n + T] = nv[b].permute(1, 0, 2)
        assert torch.equal(kvd.cpu().view(torch.int16), kv.view(torch.int16))
        assert torch.equal(_launch(C, qv, kvd, posd, B, H, T, Smax, rope, split, gc), out)  # a second launch: same bits
    return out.cpu()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_against_bound(dev, case):
    B, H, Hkv, Smax, pos, T, rope, split, gc = case
    O, tol, _, _ = _expected(B, H, Hkv, Smax, pos, T, rope)
    out = _run(dev, case)
    print(f"max |err| / tol {assert_within(out, O, tol, 'attn_append'):.3f}")
    assert torch.equal(_run(dev, case, nan=True).view(torch.int16), out.view(torch.int16))  # stale NaN: no bit moves


def test_gc_and_batch_change_no_bit(dev):
    base = (3, 6, 1, 160, (127, 40, 129), 5, True, False)
    outs = [_run(dev, base + (gc,), check_cache=False) for gc in (1, 2, 3)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    qkv, kv = _inputs(3, 6, 1, 160, 5)
    from ml_trainer_amd.ops._ext import require_native
    C = require_native()
    for split in (False, True):  # sequence 1 alone, in a cache of another size, against its rows in the batch of 3
        both = _run(dev, base[:7] + (split, 0), check_cache=False)
        kv1 = torch.zeros(2, 1, 1, 300, 64, dtype=BF16)
        kv1[:, :, :, :40] = kv[:, 1:2, :, :40]
        posd = torch.tensor([40], dtype=torch.int32, device=dev)
        alone = _launch(C, qkv[5:10].to(dev), kv1.to(dev), posd, 1, 6, 5, 300, True, split, 0).cpu()
        assert torch.equal(alone, both[5:10])


def test_later_tokens_change_no_earlier_row(dev):
    case = (1, 4, 2, 64, (33,), 16, True, False, 0)
    qkv, _ = _inputs(1, 4, 2, 64, 16)
    other = qkv.clone()
    other[9:] = torch.randn(7, qkv.shape[1], generator=torch.Generator().manual_seed(5)).to(BF16) * 4
    a, b = _run(dev, case, check_cache=False), _run(dev, case, qkv=other, check_cache=False)
    assert torch.equal(a[:9], b[:9]) and not torch.equal(a[9:], b[9:])


def test_row_strided_input(dev):
    case = (3, 4, 2, 64, (15, 16, 17), 5, True, False, 0)
    assert torch.equal(_run(dev, case, ld=8 * 64 + 8), _run(dev, case, check_cache=False))


def test_one_token_against_attn_decode(dev):
    from ml_trainer_amd.ops._ext import require_native
    C = require_native()
    case = (3, 2, 2, 64, (31, 32, 33), 1, False, False, 0)
    B, H, Hkv, Smax, pos, T = case[:6]
    O, tol, _, _ = _expected(B, H, Hkv, Smax, pos, T, False)
    qkv, kv = _inputs(B, H, Hkv, Smax, T)
    dec = torch.empty(B, H * 64, dtype=BF16, device=dev)
    C.attn_decode(qkv.to(dev), kv.to(dev), torch.tensor(pos, dtype=torch.int32, device=dev), dec, H, SCALE)
    assert_within(dec.cpu(), O, tol, "attn_decode")
    assert_within(_run(dev, case, check_cache=False), dec.cpu().double(), 2 * tol, "attn_append vs attn_decode")


def test_refused(dev):
    from ml_trainer_amd.ops._ext import require_native
    C = require_native()
    kv = torch.zeros(2, 1, 1, 32, 64, dtype=BF16, device=dev)
    pos = torch.zeros(1, dtype=torch.int32, device=dev)
    q = lambda T, ld=384: torch.zeros(T, ld, dtype=BF16, device=dev)[:, :384]
    out = lambda T: torch.empty(T, 256, dtype=BF16, device=dev)
    ws = torch.empty(C.attn_append_ws(1, 4, 4, 32), dtype=torch.float32, device=dev)
    assert C.attn_append_max_tokens() == 16
    for args, kw in [((q(4), kv.view(torch.uint8)[..., :64].contiguous(), pos, out(4), 1, 4, SCALE), {}),  # fp8 cache
                     ((q(17), kv, pos, out(17), 1, 4, SCALE), {}),
                     ((q(4, 388), kv, pos, out(4), 1, 4, SCALE), {}),  # row stride % 8 != 0
                     ((q(4), kv, pos, out(4), 1, 4, SCALE), dict(gc=3)),
                     ((q(4), kv, pos, out(4), 1, 4, SCALE), dict(ws=ws))]:
        with pytest.raises(RuntimeError):
            C.attn_append(*args, **kw)
