"""Attention edge paths (attention.hip): launch shapes no other test reaches, on GUARDED buffers, held to
the derived per-element bounds of helpers.attn_fwd_bound / attn_bwd_bound against an fp64 reference.

Every output (out, lse, delta, dqkv) is a contiguous slice in the middle of a sentinel-filled allocation
(128 rows, or 8192 floats, on both sides): a store outside the slice changes a sentinel and fails the test.
Every input (qkv, dout, and the out / lse handed to the backward) is a slice in the middle of a NaN-filled
allocation of the same margins: an over-read lands in memory the test owns and shows as a non-finite result.
With `lens`, the last valid key of each (batch, head) carries query row 0 alone and the first masked key
would carry row 1 if it leaked (helpers.attn_edge_inputs). Per case: every element of O, LSE, delta, dQ, dK,
dV within its bound; guards intact, results finite; dK / dV of masked keys equal to 0; a second launch gives
the same bits. tests/test_attn_bound_cpu.py shows on the CPU that the bounds hold for a faithful emulation
and reject an off-by-one key mask, a misplaced tail row, a missing scale, a shifted delta, the LSE of the
dropped P and a nonzero gradient of a masked key.

Each test prints `headroom <output> <dtype> <figure>` (pytest -s): for the fp32 outputs (LSE, delta) the largest
|err| / t, for the bf16 outputs the largest fraction of the fp32-level allowance t that the stored value needs
(helpers.bf16_t_used).

Branch -> the test that reaches it (test_attention_edges[...] unless another test is named):
  S < 64: min(AB, S) rows in the prologue tile, one clamped ring stage ... S1, S17 (p 0, 0.1), S63
  1-row tail block (forward tail, PATH 2 of dK/dV, clamped last stage) ... S65 (p 0, 0.1), S129 (1 and 2 groups)
  fully masked key block (k0b >= len: the zero-fill branch) ............... S65, the batches with lens 64 and 1
  half-empty last 2-group block under FULLT (q[n] < S, key[n] < S) ........ S192 default groups (lens 130 lies in it)
  exactly kRing - 1 = 3 ring stages (the prologue issues everything) ...... S192: dK/dV 3 query stages, dQ 3 key stages
  5 ring stages (slot 0 reused by stage 4) ................................ S320: dK/dV and dQ (lens 320 and 257)
  1-group dK/dV dropout grid at S >= 128 next to a 2-group dQ grid ........ S192 p 0.1, S320 p 0.1 (default groups)
  scale != 0.125 (no power of two: fp32(scale) is rounded) ................ S129, scale 0.2
  packed path (cu_seqlens; sequences of 200, 1, 64, 65, 129 rows) ......... test_attention_edges_packed
  masked K / V rows cannot reach any result ............................... test_masked_rows_cannot_influence

Measured on an MI355X against the fp64 reference and the derived allowance (largest figure over the padded
cases / over the packed case): O 0.52 / 0.32, LSE 0.43 / 0.53, delta 0.011 / 0.009, dQ 0.77 / 0.80, dK 0.54 / 0.42,
dV 0.52 / 0.31 -- every output inside its bound, no kernel change needed. The CPU emulation reaches 0.57 - 0.78
for O (|err| / t of the fp32 value), 0.35 for the LSE with an exact and 0.91 with a stale row maximum (the
kernel's defer-max lies between), 0.84 for dQ, 0.64 for dK and dV: the GPU figures sit where the emulation's do.
O, dK and dV peak at S = 17 with 5 valid keys, where a few bf16-rounded probabilities carry a row and the
allowance is nearly all that one rounding. delta stays at 0.01: its allowance charges 64 sequential fp32
additions at full magnitude, while the kernels add a short tree of exact bf16 products."""
import pytest
import torch

from ml_trainer_amd.ops import dropout as D
from ml_trainer_amd.ops._ext import require_native
from tests.helpers import (ATTN_EDGE_DROPOUT_S, ATTN_EDGE_SHAPES, assert_guard_intact, assert_within, attn_bwd_bound,
                           attn_edge_inputs, attn_fwd_bound, attn_heads, attn_split, bf16_t_used, sentinel, store_bound)

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SEED, SITE, RANK = 0x1234_5678_9ABC, D.attention_site(1), 0
PAD_ROWS, PAD_F32 = 128, 128 * 64  # margins on both sides of every buffer (multiples of 16 bytes)
PACKED = (2, 200, [200, 1, 64, 65, 129])  # (H, S = max_seqlen, lens): SHAPES[0] of tests/test_unpad_gpu.py
GROUP_ENVS = ("MLT_ATTN_FWD_GROUPS", "MLT_ATTN_DKDV_GROUPS", "MLT_ATTN_DQ_GROUPS")

# (shape index, p, groups): p = 0.1 where S is in ATTN_EDGE_DROPOUT_S, 1 group per wave forced where S >= 128
CASES = [(si, p, grp) for si, s in enumerate(ATTN_EDGE_SHAPES)
         for p in ((0.0, 0.1) if s[1] in ATTN_EDGE_DROPOUT_S else (0.0,))
         for grp in (("default", "1") if s[1] >= 128 else ("default",))]
_HEADROOM = {}


def _drop(p):
    return dict(p=p, seed=SEED, site=SITE, rank=RANK) if p else {}


def _rows_guarded(data, dev):
    """`data` [T, C] bf16 as the middle rows of a NaN-filled allocation: (buf, view)."""
    buf = sentinel((data.shape[0] + 2 * PAD_ROWS, data.shape[1]), BF16, dev)
    view = buf[PAD_ROWS:PAD_ROWS + data.shape[0]]
    view.copy_(data)
    return buf, view


def _out_rows(T, C, dev):
    buf = sentinel((T + 2 * PAD_ROWS, C), BF16, dev)
    return buf, buf[PAD_ROWS:PAD_ROWS + T]


def _out_f32(n, dev):
    buf = sentinel((n + 2 * PAD_F32,), F32, dev)
    return buf, buf[PAD_F32:PAD_F32 + n]


class Case:
    """One launch shape: guarded inputs on the device, made once and never modified."""

    def __init__(self, dev, B, S, H, lens, scale, seed, packed=False):
        self.B, self.S, self.H, self.lens, self.scale, self.packed, self.dev = B, S, H, lens, scale, packed, dev
        if packed:  # every sequence built on its own, then stacked: T = sum(lens) rows
            parts = [attn_edge_inputs(1, n, H, [n], scale, seed + b) for b, n in enumerate(lens)]
            qkv, dout = torch.cat([x[0] for x in parts]), torch.cat([x[1] for x in parts])
            self.cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=dev)
            self.lens_t = None
        else:
            qkv, dout = attn_edge_inputs(B, S, H, lens, scale, seed)
            self.cu = None
            self.lens_t = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
        self.T = qkv.shape[0]
        self.qkv_buf, self.qkv = _rows_guarded(qkv.to(dev), dev)
        self.dout_buf, self.dout = _rows_guarded(dout.to(dev), dev)

    def segments(self):
        """(row0, rows, batches, S, lens, b0) of the pieces the reference is computed on: the whole padded batch,
        or one packed sequence at a time."""
        if not self.packed:
            return [(0, self.T, self.B, self.S, self.lens, 0)]
        r0, segs = 0, []
        for b, n in enumerate(self.lens):
            segs.append((r0, n, 1, n, None, b))
            r0 += n
        return segs


_CASES = {}


def _case(key, dev):
    if key not in _CASES:
        if key == "packed":
            H, S, lens = PACKED
            _CASES[key] = Case(dev, len(lens), S, H, lens, 0.125, seed=900, packed=True)
        else:
            B, S, H, lens, scale = ATTN_EDGE_SHAPES[key]
            _CASES[key] = Case(dev, B, S, H, lens, scale, seed=100 + key)
    return _CASES[key]


def _run(C, cs, p, qkv=None):
    """attn_fwd + attn_bwd of case `cs` into fresh guarded buffers; the backward reads the forward's out and lse
    where they lie, inside their sentinel (NaN) surrounds. Guards checked; returns the views and buffers."""
    dev, B, S, H, Dm, T = cs.dev, cs.B, cs.S, cs.H, cs.H * 64, cs.T
    qkv = cs.qkv if qkv is None else qkv
    r = {}
    r["out_buf"], r["out"] = _out_rows(T, Dm, dev)
    r["lse_buf"], r["lse"] = _out_f32(B * H * S, dev)
    r["dqkv_buf"], r["dqkv"] = _out_rows(T, 3 * Dm, dev)
    r["delta_buf"], r["delta"] = _out_f32(T * H, dev)
    C.attn_fwd(qkv, r["out"], r["lse"], cs.lens_t, B, S, H, cs.scale, cu_seqlens=cs.cu, **_drop(p))
    C.attn_bwd(qkv, r["out"], cs.dout, r["lse"], r["delta"], cs.lens_t, r["dqkv"], B, S, H, cs.scale,
               cu_seqlens=cs.cu, **_drop(p))
    torch.cuda.synchronize()
    for name in ("out", "lse", "dqkv", "delta"):
        assert_guard_intact(r[name + "_buf"], r[name])
    assert_guard_intact(cs.dout_buf, cs.dout)  # (inputs: nobody wrote around them either)
    return r


def _bits(x):
    return x.view(torch.int16 if x.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _hold(name, what, got, exp, t, bf16):
    """Every element of `got` within the store's tolerance of exp given the fp32-level allowance t; notes the
    headroom (|err| / t for an fp32 output, helpers.bf16_t_used for a bf16 one)."""
    assert_within(got, exp, store_bound(exp, t, BF16 if bf16 else F32), f"{name} {what}")
    r = bf16_t_used(got, exp, t) if bf16 else float(((got.double() - exp).abs() / t).max())
    key = (name, "bf16" if bf16 else "fp32")
    _HEADROOM[key] = max(_HEADROOM.get(key, 0.0), r)
    print(f"headroom {key[0]} {key[1]} {r:.4f} {what}")


def _check(cs, p, r, what, qkv=None):
    """Assertions 1-3 of a run `r`: the bounds at every element, finite results, zero dK / dV of masked keys."""
    B, S, H, Dm = cs.B, cs.S, cs.H, cs.H * 64
    qkv = cs.qkv if qkv is None else qkv
    keep = D.attention_keep_mask(SEED, SITE, RANK, B, H, S, p, device=cs.dev) if p else None
    c = D.attention_scale(p) if p else 1.0
    lse_all = r["lse"].view(B, H, S)
    for r0, n, Bs, Ss, lens, b0 in cs.segments():
        rows = slice(r0, r0 + n)
        q, k, v = attn_split(qkv[rows], Bs, Ss, H)
        do = attn_heads(cs.dout[rows], Bs, Ss, H)
        kp = None if keep is None else keep[b0:b0 + Bs, :, :Ss, :Ss]
        tag = what if not cs.packed else f"{what} seq {b0}"
        O, tO, L, tL = attn_fwd_bound(q, k, v, lens, cs.scale, kp, c)
        out = attn_heads(r["out"][rows], Bs, Ss, H)
        lse = lse_all[b0:b0 + Bs, :, :Ss].double()
        assert torch.isfinite(out).all() and torch.isfinite(lse).all(), tag
        _hold("O", tag, out, O, tO, True)
        _hold("LSE", tag, lse, L, tL, False)
        bw = attn_bwd_bound(q, k, v, do, out, lse, lens, cs.scale, kp, c)
        delta = r["delta"][r0 * H:(r0 + n) * H].view(Bs, Ss, H).permute(0, 2, 1).double()
        dq, dk, dv = attn_split(r["dqkv"][rows], Bs, Ss, H)
        assert all(torch.isfinite(x).all() for x in (delta, dq, dk, dv)), tag
        _hold("delta", tag, delta, bw["delta"], bw["t_delta"], False)
        _hold("dQ", tag, dq, bw["dq"], bw["t_dq"], True)
        _hold("dK", tag, dk, bw["dk"], bw["t_dk"], True)
        _hold("dV", tag, dv, bw["dv"], bw["t_dv"], True)
    _assert_masked_zero(cs, r["dqkv"])


def _assert_masked_zero(cs, dqkv):
    if cs.lens is None or cs.packed:
        return
    g = dqkv.view(cs.B, cs.S, 3, cs.H * 64)
    for b, n in enumerate(cs.lens):
        assert (g[b, n:, 1:].float() == 0).all(), f"dK / dV of the masked keys of batch {b} (rows >= {n}) must be 0"


def _edge_run(C, cs, p, what):
    r = _run(C, cs, p)
    _check(cs, p, r, what)
    r2 = _run(C, cs, p)  # no atomics, nothing stored between launches: the same bits
    for name in ("out", "lse", "delta", "dqkv"):
        assert _same_bits(r[name], r2[name]), f"{what}: {name} differs between two launches"
    return r


@pytest.mark.parametrize("si,p,grp", CASES, ids=[f"S{ATTN_EDGE_SHAPES[si][1]}-p{p}-{grp}" for si, p, grp in CASES])
def test_attention_edges(dev, si, p, grp, monkeypatch):
    C = require_native()
    if grp == "1":
        for env in GROUP_ENVS:
            monkeypatch.setenv(env, "1")
    cs = _case(si, dev)
    _edge_run(C, cs, p, f"S{cs.S} lens {cs.lens} p {p} groups {grp}")


def test_attention_edges_packed(dev):
    """The same checker on a packed batch (cu_seqlens): per sequence, the reference of its own rows."""
    from tests.test_unpad_gpu import SHAPES
    assert SHAPES[0] == PACKED
    C = require_native()
    cs = _case("packed", dev)
    _edge_run(C, cs, 0.0, f"packed S{cs.S} lens {cs.lens}")


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("si", [3, 6], ids=["S65", "S192"])
def test_masked_rows_cannot_influence(dev, si, p):
    """Other finite values (30 * randn) in the K and V thirds of the rows >= lens[b] change no bit of out, lse,
    delta, dQ (all rows) or of dK / dV of the valid keys, and dK / dV of the masked keys stay 0."""
    C = require_native()
    cs = _case(si, dev)
    B, S, H, Dm = cs.B, cs.S, cs.H, cs.H * 64
    a = _run(C, cs, p)
    _, qkv2 = _rows_guarded(cs.qkv, dev)
    g = torch.Generator().manual_seed(7)
    x = qkv2.view(B, S, 3, Dm)
    for b, n in enumerate(cs.lens):
        if n < S:
            x[b, n:, 1:] = (30 * torch.randn(S - n, 2, Dm, generator=g)).to(BF16).to(dev)
    assert not _same_bits(qkv2, cs.qkv)
    r = _run(C, cs, p, qkv=qkv2)
    for name in ("out", "lse", "delta"):
        assert _same_bits(a[name], r[name]), f"{name} changed with the masked K / V rows"
    ga, gr = a["dqkv"].view(B, S, 3, Dm), r["dqkv"].view(B, S, 3, Dm)
    assert _same_bits(ga[:, :, 0].contiguous(), gr[:, :, 0].contiguous()), "dQ changed with the masked K / V rows"
    for b, n in enumerate(cs.lens):
        assert _same_bits(ga[b, :n, 1:].contiguous(), gr[b, :n, 1:].contiguous()), f"dK / dV of batch {b}'s valid keys"
    _assert_masked_zero(cs, r["dqkv"])
    assert torch.isfinite(r["out"].float()).all() and torch.isfinite(r["dqkv"].float()).all()
