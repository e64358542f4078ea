"""attn_decode.hip on the GPU: every edge case of tests/attn_decode_ref.py on guarded buffers, held to the derived
allowance (decode_bound + helpers.store_bound); the append bitwise and nothing else written; NaN in the stale
rows; a row-strided qkv_new; determinism; agreement with the causal forward kernel; refused calls.

Measured on an MI355X: see test_kernel_within_bound's docstring."""
import pytest
import torch

from tests.attn_causal_ref import attn_fwd_bound_masked, causal_valid
from tests.attn_decode_ref import (DECODE_EDGE_CASES, decode_bound, decode_edge_inputs, decode_effective,
                                   nan_stale_rows)
from tests.helpers import (assert_guard_intact, assert_within, attn_split, bf16_t_used, guarded, guarded_like,
                           store_bound)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _case_id(c):
    return f"B{c[0]}H{c[1]}S{c[2]}"


def _bits(t):
    return t.contiguous().view(torch.int16)


def _launch(dev, case, qkv, kv, pos, ld=None):
    """One launch on guarded buffers; every guard checked. Returns (out [B, D], kv after) on the device."""
    from ml_trainer_amd.ops._ext import require_native
    C = require_native()
    B, H, Smax, _, scale = case
    qbuf, q = guarded_like(qkv.to(dev), ld=ld)
    kbuf, k2 = guarded_like(kv.to(dev).view(-1, 64))
    obuf, out = guarded(B, H * 64, BF16, dev)
    C.attn_decode(q, k2.view(2, B, H, Smax, 64), pos.to(dev), out, H, scale)
    torch.cuda.synchronize()
    assert_guard_intact(qbuf, q)
    assert_guard_intact(kbuf, k2)
    assert_guard_intact(obuf, out)
    assert torch.equal(_bits(q), _bits(qkv.to(dev)))  # the input itself is untouched
    return out.clone(), k2.view(2, B, H, Smax, 64).clone()


_REF = {}


def _reference(i):
    """(inputs, O, t) of case i, computed once on the CPU and left unchanged."""
    if i not in _REF:
        case = DECODE_EDGE_CASES[i]
        B, H, Smax, pos, scale = case
        qkv, kv, p = decode_edge_inputs(case, 100 + i)
        O, t = decode_bound(*decode_effective(qkv, kv, pos), pos, scale)
        _REF[i] = (qkv, kv, p, O.view(B, H * 64), t.view(B, H * 64))
    return _REF[i]


@pytest.mark.parametrize("i", range(len(DECODE_EDGE_CASES)), ids=[_case_id(c) for c in DECODE_EDGE_CASES])
def test_kernel_within_bound(dev, i):
    """Output within the derived allowance; rows pos[b] of the cache equal the new k / v bitwise; every other
    cache element and every guard bitwise unchanged; NaN in the stale rows changes no bit of the output; two
    launches agree bitwise.

    Measured (MI355X), all seven cases: the share of the fp32-level allowance t the bf16 output needs
    (helpers.bf16_t_used) is below 1e-4, i.e. every output is the correctly rounded bf16 of a value well inside
    t, so |err| / store_bound is 1.000 wherever that rounding moves the value at all (0.000 in the one-row cache,
    where out = v exactly). The CPU emulation uses 0.035 - 0.090 of t itself (tests/test_attn_decode_cpu.py)."""
    case = DECODE_EDGE_CASES[i]
    B, H, Smax, pos, scale = case
    qkv, kv, p, O, t = _reference(i)
    out, kv_after = _launch(dev, case, qkv, kv, p)
    r = assert_within(out.cpu(), O, store_bound(O, t, BF16), f"attn_decode {_case_id(case)}")
    print(f"attn_decode {_case_id(case)}: |err| / bound {r:.3f}, fp32-level allowance used "
          f"{bf16_t_used(out.cpu(), O, t):.4f}")
    x = qkv.view(B, 3, H, 64).to(dev)
    want = kv.to(dev).clone()
    for b in range(B):
        want[0, b, :, pos[b]] = x[b, 1]
        want[1, b, :, pos[b]] = x[b, 2]
    assert torch.equal(_bits(kv_after), _bits(want))
    # stale rows: NaN above pos[b] -- finite output, bitwise equal to the run with finite sentinels there
    kv_nan = nan_stale_rows(kv, pos)
    out_nan, kv_nan_after = _launch(dev, case, qkv, kv_nan, p)
    assert bool(torch.isfinite(out_nan.float()).all())
    assert torch.equal(_bits(out_nan), _bits(out))
    want_nan = kv_nan.to(dev).clone()
    for b in range(B):
        want_nan[0, b, :, pos[b]] = x[b, 1]
        want_nan[1, b, :, pos[b]] = x[b, 2]
    assert torch.equal(_bits(kv_nan_after), _bits(want_nan))
    # determinism
    out2, _ = _launch(dev, case, qkv, kv, p)
    assert torch.equal(_bits(out2), _bits(out))


@pytest.mark.parametrize("i", [1, 3], ids=[_case_id(DECODE_EDGE_CASES[1]), _case_id(DECODE_EDGE_CASES[3])])
def test_strided_qkv_new(dev, i):
    case = DECODE_EDGE_CASES[i]
    B, H, Smax, pos, scale = case
    qkv, kv, p, _, _ = _reference(i)
    a, ka = _launch(dev, case, qkv, kv, p)
    b, kb = _launch(dev, case, qkv, kv, p, ld=3 * H * 64 + 8)
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(ka), _bits(kb))


def test_against_the_forward_kernel(dev):
    """The cache built from a random [B * S, 3D] QKV, the last token decoded at pos = S - 1 (its cache row NaN
    before the call), against row S - 1 of C.attn_fwd(causal=True): both are bounded to the same fp64 reference,
    so they differ by at most the sum of their two allowances."""
    from ml_trainer_amd.ops._ext import require_native
    C = require_native()
    B, S, H, scale = 2, 130, 2, 0.125
    D = H * 64
    g = torch.Generator().manual_seed(5)
    qkv = (torch.randn(B * S, 3 * D, generator=g) * 0.5).to(BF16)
    q, k, v = attn_split(qkv, B, S, H)
    O, t_fwd, _, _ = attn_fwd_bound_masked(q, k, v, causal_valid(None, B, S), scale)
    Od, t_dec = decode_bound(q[:, :, S - 1], k, v, [S - 1] * B, scale)
    assert float((Od - O[:, :, S - 1]).abs().max()) <= 1e-12
    dq = qkv.to(dev)
    fwd = torch.empty(B * S, D, dtype=BF16, device=dev)
    lse = torch.empty(B * H * S, dtype=torch.float32, device=dev)
    C.attn_fwd(dq, fwd, lse, None, B, S, H, scale, causal=True)
    x = dq.view(B, S, 3, H, 64)
    kv = torch.stack((x[:, :, 1].permute(0, 2, 1, 3), x[:, :, 2].permute(0, 2, 1, 3))).contiguous()
    kv[:, :, :, S - 1] = float("nan")
    new = dq.view(B, S, 3 * D)[:, S - 1]  # a row-strided view, stride S * 3D
    out = torch.empty(B, D, dtype=BF16, device=dev)
    C.attn_decode(new, kv, torch.full((B,), S - 1, dtype=torch.int32, device=dev), out, H, scale)
    a = out.cpu().double().view(B, H, 64)
    f = fwd.cpu().double().view(B, S, H, 64)[:, S - 1]
    tol = store_bound(Od, t_dec, BF16) + store_bound(Od, t_fwd[:, :, S - 1], BF16)
    assert bool(((a - f).abs() <= tol).all())
    assert_within(out.cpu().view(B, H, 64), Od, store_bound(Od, t_dec, BF16), "attn_decode vs fp64")


def test_refused_calls(dev):
    from ml_trainer_amd.ops._ext import require_native
    C = require_native()
    B, H, Smax = 2, 2, 16
    D = H * 64
    qkv = torch.zeros(B, 3 * D, dtype=BF16, device=dev)
    kv = torch.zeros(2, B, H, Smax, 64, dtype=BF16, device=dev)
    pos = torch.zeros(B, dtype=torch.int32, device=dev)
    out = torch.full((B, D), 7.0, dtype=BF16, device=dev)
    with pytest.raises(RuntimeError):
        C.attn_decode(qkv.to(torch.float16), kv, pos, out, H, 0.125)
    with pytest.raises(RuntimeError):
        C.attn_decode(qkv, kv.float(), pos, out, H, 0.125)
    with pytest.raises(RuntimeError):
        C.attn_decode(qkv, kv, pos.long(), out, H, 0.125)
    flat = torch.zeros(B * 3 * D + 8, dtype=BF16, device=dev)
    with pytest.raises(RuntimeError, match="aligned"):
        C.attn_decode(flat[4:4 + B * 3 * D].view(B, 3 * D), kv, pos, out, H, 0.125)
    wide = torch.zeros(B, 3 * D + 4, dtype=BF16, device=dev)
    with pytest.raises(RuntimeError, match="row stride"):
        C.attn_decode(wide[:, :3 * D], kv, pos, out, H, 0.125)
    with pytest.raises(RuntimeError, match="kv"):
        C.attn_decode(qkv, torch.zeros(2, B + 1, H, Smax, 64, dtype=BF16, device=dev), pos, out, H, 0.125)
    with pytest.raises(RuntimeError, match="kv"):
        C.attn_decode(qkv, kv.view(-1), pos, out, H, 0.125)
    with pytest.raises(RuntimeError):
        C.attn_decode(qkv, kv, pos[:1], out, H, 0.125)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((kv == 0).all())  # nothing was launched
