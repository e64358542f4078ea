"""Causal flash attention (the CAUSAL instantiations of attn_fwd_lean_kernel, attn_bwd_dq_ring_kernel and
attn_bwd_dkdv_ring_kernel) on the guarded buffers of tests/test_attention_edges_gpu.py, held to the masked bounds of
tests/attn_causal_ref.py against an fp64 reference.

Definition: key j of a sequence is visible to query i of the same sequence iff j <= i and j < len_b.

The checker is the one of test_attention_edges_gpu.py (sentinel-surrounded outputs, NaN-surrounded inputs, every
element of O, LSE, delta, dQ, dK, dV within its bound, two launches bitwise equal) with `causal=True`, over all of
helpers.ATTN_EDGE_SHAPES (p = 0.1 at ATTN_EDGE_DROPOUT_S, 1 group per wave forced where S >= 128) and the packed case.
The inputs carry sentinel keys on the diagonal at rows 15 | 16, 63 | 64, 127 | 128 (attn_causal_ref.causal_edge_inputs);
tests/test_attn_causal_cpu.py shows that the bounds reject an off-by-one of the diagonal in either direction.

Where causal can break -> the case that reaches it:
  a diagonal block that is also a 1-row tail ............................ S65, S129 (1 and 2 groups)
  dK/dV key block 1 starts its ring at query block 1, block 2 at the last stage ... S192 (1 group: blocks 0, 1, 2)
  a ring slot reused after a shifted start ................................ S320 (dK/dV key block 1: stages 1 .. 4)
  a length mask and a diagonal in the same block .......................... lens 130 (S192), 257 (S320)
  forward / dQ group 0 with an all-invisible last block (2 groups) ......... S129, S192, S320 default groups
  packed sequences of 200, 1, 64, 65, 129 rows (dK/dV: 1 group) ............ test_causal_edges_packed

Each test prints `headroom <output> <dtype> <figure>` (pytest -s) as the non-causal edge test does. Measured on an
MI355X (largest figure over the padded cases / over the packed cases): O 0.52 / 0.52, LSE 0.63 / 0.73, delta 0.015 /
0.011, dQ 0.79 / 0.78, dK 0.76 / 0.85, dV 0.69 / 0.83 -- every output inside its bound. (The non-causal edge test
measured O 0.52 / 0.32, LSE 0.43 / 0.53, dQ 0.77 / 0.80, dK 0.54 / 0.42, dV 0.52 / 0.31: dK and dV use more of their
allowance under the causal mask.)"""
import pytest
import torch

import tests.test_attention_edges_gpu as E
from ml_trainer_amd.ops import dropout as D
from ml_trainer_amd.ops._ext import require_native
from tests.attn_causal_ref import attn_bwd_bound_masked, attn_fwd_bound_masked, causal_edge_inputs, causal_valid
from tests.helpers import (ATTN_EDGE_SHAPES, assert_guard_intact, assert_within, attn_heads, attn_split, bf16_t_used,
                           store_bound)

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SEED, SITE, RANK = E.SEED, E.SITE, E.RANK


class CausalCase:
    """One launch shape with the causal edge inputs: guarded inputs on the device, made once, never modified."""

    def __init__(self, dev, B, S, H, lens, scale, seed, packed=False):
        self.B, self.S, self.H, self.lens, self.scale, self.packed, self.dev = B, S, H, lens, scale, packed, dev
        if packed:
            parts = [causal_edge_inputs(1, n, H, [n], scale, seed + b) for b, n in enumerate(lens)]
            qkv, dout = torch.cat([x[0] for x in parts]), torch.cat([x[1] for x in parts])
            self.cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=dev)
            self.lens_t = None
        else:
            qkv, dout = causal_edge_inputs(B, S, H, lens, scale, seed)
            self.cu = None
            self.lens_t = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
        self.T = qkv.shape[0]
        self.qkv_buf, self.qkv = E._rows_guarded(qkv.to(dev), dev)
        self.dout_buf, self.dout = E._rows_guarded(dout.to(dev), dev)

    segments = E.Case.segments


_CASES = {}


def _case(key, dev):
    if key not in _CASES:
        if key == "packed":
            H, S, lens = E.PACKED
            _CASES[key] = CausalCase(dev, len(lens), S, H, lens, 0.125, seed=900, packed=True)
        else:
            B, S, H, lens, scale = ATTN_EDGE_SHAPES[key]
            _CASES[key] = CausalCase(dev, B, S, H, lens, scale, seed=100 + key)
    return _CASES[key]


def _run(C, cs, p, qkv=None, **kw):
    """attn_fwd + attn_bwd with causal=True (or **kw) into fresh guarded buffers; guards checked."""
    dev, B, S, H, Dm, T = cs.dev, cs.B, cs.S, cs.H, cs.H * 64, cs.T
    qkv = cs.qkv if qkv is None else qkv
    kw = kw or dict(causal=True)
    r = {}
    r["out_buf"], r["out"] = E._out_rows(T, Dm, dev)
    r["lse_buf"], r["lse"] = E._out_f32(B * H * S, dev)
    r["dqkv_buf"], r["dqkv"] = E._out_rows(T, 3 * Dm, dev)
    r["delta_buf"], r["delta"] = E._out_f32(T * H, dev)
    C.attn_fwd(qkv, r["out"], r["lse"], cs.lens_t, B, S, H, cs.scale, cu_seqlens=cs.cu, **E._drop(p), **kw)
    C.attn_bwd(qkv, r["out"], cs.dout, r["lse"], r["delta"], cs.lens_t, r["dqkv"], B, S, H, cs.scale,
               cu_seqlens=cs.cu, **E._drop(p), **kw)
    torch.cuda.synchronize()
    for name in ("out", "lse", "dqkv", "delta"):
        assert_guard_intact(r[name + "_buf"], r[name])
    assert_guard_intact(cs.dout_buf, cs.dout)
    return r


def _hold(name, what, got, exp, t, bf16):
    assert_within(got, exp, store_bound(exp, t, BF16 if bf16 else F32), f"{name} {what}")
    r = bf16_t_used(got, exp, t) if bf16 else float(((got.double() - exp).abs() / t).max())
    print(f"headroom {name} {'bf16' if bf16 else 'fp32'} {r:.4f} {what}")


def _check(cs, p, r, what):
    """Every element of O, LSE, delta, dQ, dK, dV within the masked bounds against fp64; finite results; dK / dV
    of the keys past each length equal to 0."""
    B, S, H = cs.B, cs.S, cs.H
    keep = D.attention_keep_mask(SEED, SITE, RANK, B, H, S, p, device=cs.dev) if p else None
    c = D.attention_scale(p) if p else 1.0
    lse_all = r["lse"].view(B, H, S)
    for r0, n, Bs, Ss, lens, b0 in cs.segments():
        rows = slice(r0, r0 + n)
        q, k, v = attn_split(cs.qkv[rows], Bs, Ss, H)
        do = attn_heads(cs.dout[rows], Bs, Ss, H)
        kp = None if keep is None else keep[b0:b0 + Bs, :, :Ss, :Ss]
        valid = causal_valid(lens, Bs, Ss).to(cs.dev)
        tag = what if not cs.packed else f"{what} seq {b0}"
        O, tO, L, tL = attn_fwd_bound_masked(q, k, v, valid, cs.scale, kp, c)
        out = attn_heads(r["out"][rows], Bs, Ss, H)
        lse = lse_all[b0:b0 + Bs, :, :Ss].double()
        assert torch.isfinite(out).all() and torch.isfinite(lse).all(), tag
        _hold("O", tag, out, O, tO, True)
        _hold("LSE", tag, lse, L, tL, False)
        bw = attn_bwd_bound_masked(q, k, v, do, out, lse, valid, cs.scale, kp, c)
        delta = r["delta"][r0 * H:(r0 + n) * H].view(Bs, Ss, H).permute(0, 2, 1).double()
        dq, dk, dv = attn_split(r["dqkv"][rows], Bs, Ss, H)
        assert all(torch.isfinite(x).all() for x in (delta, dq, dk, dv)), tag
        _hold("delta", tag, delta, bw["delta"], bw["t_delta"], False)
        _hold("dQ", tag, dq, bw["dq"], bw["t_dq"], True)
        _hold("dK", tag, dk, bw["dk"], bw["t_dk"], True)
        _hold("dV", tag, dv, bw["dv"], bw["t_dv"], True)
    E._assert_masked_zero(cs, r["dqkv"])


def _edge_run(C, cs, p, what):
    r = _run(C, cs, p)
    _check(cs, p, r, what)
    r2 = _run(C, cs, p)
    for name in ("out", "lse", "delta", "dqkv"):
        assert E._same_bits(r[name], r2[name]), f"{what}: {name} differs between two launches"
    return r


@pytest.mark.parametrize("si,p,grp", E.CASES,
                         ids=[f"S{ATTN_EDGE_SHAPES[si][1]}-p{p}-{grp}" for si, p, grp in E.CASES])
def test_causal_edges(dev, si, p, grp, monkeypatch):
    C = require_native()
    if grp == "1":
        for env in E.GROUP_ENVS:
            monkeypatch.setenv(env, "1")
    cs = _case(si, dev)
    _edge_run(C, cs, p, f"causal S{cs.S} lens {cs.lens} p {p} groups {grp}")


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_causal_edges_packed(dev, p):
    C = require_native()
    cs = _case("packed", dev)
    _edge_run(C, cs, p, f"causal packed S{cs.S} lens {cs.lens} p {p}")


@pytest.mark.parametrize("r0", [80, 144])
@pytest.mark.parametrize("si", [6, 7], ids=["S192", "S320"])
def test_future_rows_cannot_influence(dev, si, r0):
    """Other finite values (30 * randn) in the K and V thirds of the rows >= r0 change not one bit of out, lse,
    delta or dQ of the rows < r0.

    r0 = 80 and 144 are multiples of 16 but not of 64, so the changed keys share a 64-key block, and a 64-query
    group, with rows that must not move. They are multiples of 16 for a reason: a wave's defer-max decision (rescale
    O and l or keep the stale maximum) is one __any over its 16 queries, so the rows of one wave are coupled -- a
    later row's larger score can change how an earlier row of the same wave is rounded, within the bounds -- and
    bitwise equality holds only across wave boundaries."""
    C = require_native()
    cs = _case(si, dev)
    B, S, H, Dm = cs.B, cs.S, cs.H, cs.H * 64
    a = _run(C, cs, 0.0)
    _, qkv2 = E._rows_guarded(cs.qkv, dev)
    x = qkv2.view(B, S, 3, Dm)
    x[:, r0:, 1:] = (30 * torch.randn(B, S - r0, 2, Dm, generator=torch.Generator().manual_seed(7))).to(BF16).to(dev)
    assert not E._same_bits(qkv2, cs.qkv)
    r = _run(C, cs, 0.0, qkv=qkv2)
    assert E._same_bits(a["out"].view(B, S, Dm)[:, :r0].contiguous(), r["out"].view(B, S, Dm)[:, :r0].contiguous())
    assert E._same_bits(a["lse"].view(B, H, S)[:, :, :r0].contiguous(), r["lse"].view(B, H, S)[:, :, :r0].contiguous())
    assert E._same_bits(a["delta"].view(B, S, H)[:, :r0].contiguous(), r["delta"].view(B, S, H)[:, :r0].contiguous())
    ga, gr = a["dqkv"].view(B, S, 3, Dm), r["dqkv"].view(B, S, 3, Dm)
    assert E._same_bits(ga[:, :r0, 0].contiguous(), gr[:, :r0, 0].contiguous()), "dQ of the rows before r0 changed"
    assert not E._same_bits(ga[:, r0:, 0].contiguous(), gr[:, r0:, 0].contiguous())  # the later rows do see them
    assert torch.isfinite(r["out"].float()).all() and torch.isfinite(r["dqkv"].float()).all()


@pytest.mark.parametrize("si,p", [(1, 0.1), (5, 0.0), (6, 0.1)], ids=["S17-p0.1", "S129", "S192-p0.1"])
def test_causal_false_is_the_call_without_the_keyword(dev, si, p):
    C = require_native()
    cs = E._case(si, dev)  # (the non-causal edge inputs)
    a = E._run(C, cs, p)
    b = _run(C, cs, p, causal=False)
    for name in ("out", "lse", "delta", "dqkv"):
        assert E._same_bits(a[name], b[name]), name
    c = _run(C, cs, p, causal=True)
    assert not E._same_bits(a["out"], c["out"])


def test_causal_is_refused_where_it_has_no_kernel(dev, monkeypatch):
    C = require_native()
    cs = _case(1, dev)
    B, S, H, Dm, T = cs.B, cs.S, cs.H, cs.H * 64, cs.T
    r = _run(C, cs, 0.0)
    y8 = torch.empty(T, 3 * Dm, dtype=torch.float8_e5m2, device=dev)
    with pytest.raises(RuntimeError, match="causal"):
        C.attn_bwd(cs.qkv, r["out"], cs.dout, r["lse"], r["delta"], cs.lens_t, r["dqkv"], B, S, H, cs.scale, q8_y=y8,
                   causal=True)
    monkeypatch.setenv("MLT_ATTN_RING", "0")
    with pytest.raises(RuntimeError, match="causal"):
        C.attn_bwd(cs.qkv, r["out"], cs.dout, r["lse"], r["delta"], cs.lens_t, r["dqkv"], B, S, H, cs.scale, causal=True)
    torch.cuda.synchronize()
