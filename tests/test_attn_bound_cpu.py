"""The derived attention bounds of tests/helpers.py (attn_fwd_bound, attn_bwd_bound) against a torch
emulation of the attention kernels, on the CPU.

The emulation does what attention.hip does at the precision it does it: fp32 products and sums, the
scores scaled by the fp32 product scale * log2 e, P = 2^(s sl2 - m) with m the row maximum (optionally
stale by `off`, as defer-max leaves it), P rounded to bf16 (pack_acc) before the row sum l and the P.V
product, O = o / l (times c under dropout), LSE2 = m + log2 l of the UNDROPPED P; in the backward P from
the saved LSE, delta = rowsum(dO O), dS = P (c M dP - delta), P o M and dS rounded to bf16 before their
products, `scale` applied to the finished dQ / dK sums, bf16 stores, the key mask by length and an optional
keep mask. It runs at every shape of tests/test_attention_edges_gpu.py (helpers.ATTN_EDGE_SHAPES).

Two conditions make the bound worth using on the GPU:
  * the emulation stays within it at every element (test_emulation_within_bounds; the largest
    |fp32 value - reference| / t per output is printed, and the stored bf16 values are held to store_bound);
  * every mutation of MUTATIONS -- each a plausible kernel defect -- violates it at every shape where the
    mutation changes anything (test_mutation_violates_a_bound).
The mutation `l_unrounded` (P normalised by a row sum of the unrounded P) is the subtlest: on random rows it
moves O by the average bf16 rounding error of a row's probabilities, about 2^-9 / sqrt(keys) of |O|, which
the allowance for the bf16 rounding of P (2^-8 of the spread of V) cannot separate, and is not meant to.
It is separated on the sentinel rows (helpers.attn_edge_inputs: the last valid key carries row 0 alone, so
t_O there is at fp32 level) once that key's probability is not a bf16 number, which a stale maximum brings
about: test_unrounded_row_sum_shows_on_sentinel_rows."""
import pytest
import torch

from ml_trainer_amd.ops import dropout as D
from tests.helpers import (ATTN_EDGE_DROPOUT_S, ATTN_EDGE_SHAPES, assert_within, attn_bwd_bound, attn_edge_inputs,
                           attn_fwd_bound, attn_heads, attn_split, store_bound)

BF16 = torch.bfloat16
SEED, SITE, RANK = 0x1234_5678_9ABC, D.attention_site(1), 0
CASES = [(si, p) for si, s in enumerate(ATTN_EDGE_SHAPES)
         for p in ((0.0, 0.1) if s[1] in ATTN_EDGE_DROPOUT_S else (0.0,))]
MUTATIONS = ["mask_plus_1", "mask_minus_1", "tail_row_from_neighbour", "dq_without_scale", "delta_from_next_row",
             "lse_of_dropped_p", "masked_dkdv_1e-3"]


def _r(x):  # the bf16 rounding of an fp32 tensor, back in fp32
    return x.to(BF16).float()


def _valid(n, S):
    return (torch.arange(S)[None, :] < n[:, None])[:, None, None, :]


def _lens_of(lens, B, S, mut):
    n = torch.full((B,), S) if lens is None else torch.tensor(lens)
    if mut == "mask_plus_1":
        n = (n + 1).clamp_max(S)
    if mut == "mask_minus_1":
        n = (n - 1).clamp_min(1)
    return n


def emulate(qkv, dout, B, S, H, lens, scale, keep=None, c=1.0, off=None, mut=None):
    """fp32 emulation of attn_fwd + attn_bwd: dict of the fp32 values before their stores (o, lse, delta, dq,
    dk, dv) and the stored bf16 tensors (o_b, dq_b, dk_b, dv_b), all [B, H, S, ...]."""
    q, k, v = (x.float() for x in attn_split(qkv, B, S, H))
    do = attn_heads(dout, B, S, H).float()
    sc = torch.tensor(scale, dtype=torch.float32)
    sl2 = sc * torch.tensor(1.4426950408889634, dtype=torch.float32)
    c = torch.tensor(c, dtype=torch.float32)
    n_true = _lens_of(lens, B, S, None)
    valid = _valid(_lens_of(lens, B, S, mut), S)
    kp = torch.ones(B, H, S, S) if keep is None else keep.float()
    # forward
    s = q @ k.transpose(-1, -2)
    sm = s.masked_fill(~valid, float("-inf"))
    m = sm.max(-1, keepdim=True).values * sl2
    if off is not None:
        m = m - off
    p = torch.exp2(sm * sl2 - m)
    pb = _r(p)
    l = (p if mut == "l_unrounded" else pb).sum(-1)
    pv = _r(pb * kp)
    o = (pv @ v) * ((1.0 / l) * (c if keep is not None else 1.0))[..., None]
    lse = m[..., 0] + torch.log2(pv.sum(-1) if mut == "lse_of_dropped_p" else l)
    if mut == "tail_row_from_neighbour":
        o[:, :, S - 1], lse[:, :, S - 1] = o[:, :, S - 2].clone(), lse[:, :, S - 2].clone()
        q = q.clone()
        q[:, :, S - 1] = q[:, :, S - 2]
    o_b = o.to(BF16)
    # backward, from the stored O and the saved LSE
    delta = (do * o_b.float()).sum(-1)
    dl = torch.roll(delta, -1, -1) if mut == "delta_from_next_row" else delta
    pr = torch.where(valid, torch.exp2((q @ k.transpose(-1, -2)) * sl2 - lse[..., None]), torch.zeros(()))
    dp = do @ v.transpose(-1, -2)
    ds = pr * ((dp - dl[..., None]) if keep is None else (kp * c * dp - dl[..., None]))
    pm, dsb = _r(pr * kp), _r(ds)
    dv = pm.transpose(-1, -2) @ do
    if keep is not None:
        dv = dv * c
    dk = (dsb.transpose(-1, -2) @ q) * sc
    dq = (dsb @ k) if mut == "dq_without_scale" else (dsb @ k) * sc
    if mut == "masked_dkdv_1e-3":
        masked = ~_valid(n_true, S)[:, 0, 0, :]  # [B, S]
        dk = torch.where(masked[:, None, :, None], torch.full_like(dk, 1e-3), dk)
        dv = torch.where(masked[:, None, :, None], torch.full_like(dv, 1e-3), dv)
    return dict(o=o, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv, o_b=o_b, dq_b=dq.to(BF16), dk_b=dk.to(BF16),
                dv_b=dv.to(BF16))


_DATA = {}


def _case(si, p):
    """Inputs, keep mask and the forward reference of a case: made once, never modified."""
    if (si, p) not in _DATA:
        B, S, H, lens, scale = ATTN_EDGE_SHAPES[si]
        qkv, dout = attn_edge_inputs(B, S, H, lens, scale, seed=100 + si)
        keep = D.attention_keep_mask(SEED, SITE, RANK, B, H, S, p) if p else None
        c = D.attention_scale(p) if p else 1.0
        q, k, v = attn_split(qkv, B, S, H)
        _DATA[si, p] = (qkv, dout, keep, c, attn_fwd_bound(q, k, v, lens, scale, keep, c))
    return _DATA[si, p]


def ratios(si, p, e):
    """Largest |value - reference| / tolerance per output of an emulation result `e`: the fp32 values against
    t, the stored bf16 values against store_bound (keys ending in _b)."""
    B, S, H, lens, scale = ATTN_EDGE_SHAPES[si]
    qkv, dout, keep, c, (O, tO, L, tL) = _case(si, p)
    q, k, v = attn_split(qkv, B, S, H)
    bw = attn_bwd_bound(q, k, v, attn_heads(dout, B, S, H), e["o_b"].double(), e["lse"].double(), lens, scale, keep, c)
    ref = dict(o=(O, tO), lse=(L, tL), delta=(bw["delta"], bw["t_delta"]), dq=(bw["dq"], bw["t_dq"]),
               dk=(bw["dk"], bw["t_dk"]), dv=(bw["dv"], bw["t_dv"]))
    out = {}
    for name, (x, t) in ref.items():
        out[name] = float(((e[name].double() - x).abs() / t).max())
        if name + "_b" in e:
            out[name + "_b"] = float(((e[name + "_b"].double() - x).abs() / store_bound(x, t, BF16)).max())
    return out, ref


def _emulate_case(si, p, **kw):
    B, S, H, lens, scale = ATTN_EDGE_SHAPES[si]
    qkv, dout, keep, c, _ = _case(si, p)
    return emulate(qkv, dout, B, S, H, lens, scale, keep, c, **kw)


@pytest.mark.parametrize("stale", [False, True])
@pytest.mark.parametrize("si,p", CASES)
def test_emulation_within_bounds(si, p, stale):
    """Every element of every output of the emulation is within its bound, with the exact row maximum and
    with one that is stale by a random 0 .. 8 per row (what defer-max may leave: p up to 2^8)."""
    B, S, H, lens, scale = ATTN_EDGE_SHAPES[si]
    off = 8.0 * torch.rand(B, H, S, 1, generator=torch.Generator().manual_seed(si)) if stale else None
    e = _emulate_case(si, p, off=off)
    r, ref = ratios(si, p, e)
    print(f"S={S} p={p} stale={stale}: " + " ".join(f"{n} {r[n]:.3f}" for n in ("o", "lse", "delta", "dq", "dk", "dv")))
    for name, (x, t) in ref.items():
        assert_within(e[name], x, t, f"emulated {name} (fp32)")
        if name + "_b" in e:
            assert_within(e[name + "_b"], x, store_bound(x, t, BF16), f"emulated {name} (bf16 store)")
    n = _lens_of(lens, B, S, None)
    masked = ~_valid(n, S)[:, 0, 0, :]
    assert (e["dk_b"].float()[masked[:, None, :, None].expand_as(e["dk"])] == 0).all()
    assert (e["dv_b"].float()[masked[:, None, :, None].expand_as(e["dv"])] == 0).all()


def _applicable(mut, S, lens, p):
    n = [S] if lens is None else lens
    return {"mask_plus_1": any(x < S for x in n),          # a masked key has to exist
            "mask_minus_1": any(x >= 2 for x in n),        # ... and a second valid one
            "tail_row_from_neighbour": S >= 2,
            "dq_without_scale": any(x >= 2 for x in n),    # with one key dS = dP - delta = 0 and dQ = 0
            "delta_from_next_row": S >= 2,
            "lse_of_dropped_p": p > 0,
            "masked_dkdv_1e-3": any(x < S for x in n)}[mut]


MUTATION_CASES = [(si, p, mut) for si, p in CASES for mut in MUTATIONS
                  if _applicable(mut, ATTN_EDGE_SHAPES[si][1], ATTN_EDGE_SHAPES[si][3], p)]


@pytest.mark.parametrize("si,p,mut", MUTATION_CASES)
def test_mutation_violates_a_bound(si, p, mut):
    """Each defect, built into the emulation, puts at least one element of one STORED output outside its
    tolerance, at every shape where the defect can change a result."""
    B, S, H, lens, scale = ATTN_EDGE_SHAPES[si]
    r, _ = ratios(si, p, _emulate_case(si, p, mut=mut))
    stored = {n: x for n, x in r.items() if n.endswith("_b") or n in ("lse", "delta")}
    print(f"S={S} p={p} {mut}: " + " ".join(f"{n} {x:.3g}" for n, x in stored.items()))
    assert max(stored.values()) > 1.0, stored


@pytest.mark.parametrize("si", [i for i, s in enumerate(ATTN_EDGE_SHAPES) if s[3] is not None])
def test_unrounded_row_sum_shows_on_sentinel_rows(si):
    """Row 0 of every (batch, head) is carried by its last valid key alone. With the maximum stale by
    log2(1 + 0.49 * 2^-7) that key's probability is 1.0038, which bf16 rounds to 1: a row sum of the unrounded P
    then scales O by 1 / 1.0038, 2^10 times the fp32-level allowance of that row, and the bf16 store moves. The
    unmutated emulation with the same stale maximum stays inside (the tied rounding of numerator and
    denominator is what t_O assumes)."""
    B, S, H, lens, scale = ATTN_EDGE_SHAPES[si]
    off = torch.full((B, H, S, 1), float(torch.log2(torch.tensor(1 + 0.49 * 2.0 ** -7, dtype=torch.float64))))
    _, _, _, _, (O, tO, _, _) = _case(si, 0.0)
    tol = store_bound(O, tO, BF16)
    good = _emulate_case(si, 0.0, off=off)
    assert_within(good["o_b"], O, tol, "emulated O, stale maximum")
    bad = _emulate_case(si, 0.0, off=off, mut="l_unrounded")
    err = (bad["o_b"].double() - O).abs()
    assert bool((err[:, :, 0] > tol[:, :, 0]).any(-1).all()), "row 0 of every (b, h) must leave its tolerance"
    print(f"S={S}: row 0 |err| / tol up to {float((err[:, :, 0] / tol[:, :, 0]).max()):.3g}")


def test_half_the_unit_roundoff_rejects_the_emulation(monkeypatch):
    """u = 2^-8 is not slack by a factor of two: with 2^-9 in its place the unmutated emulation leaves the bound of
    O, dQ and dK at S = 17, len = 5 (one round-to-nearest to 8 significant bits moves a value by up to 2^-8)."""
    import tests.helpers as helpers
    si = [s[1] for s in ATTN_EDGE_SHAPES].index(17)
    B, S, H, lens, scale = ATTN_EDGE_SHAPES[si]
    qkv, dout, _, _, _ = _case(si, 0.0)
    e = emulate(qkv, dout, B, S, H, lens, scale)
    monkeypatch.setattr(helpers, "_UB", 2.0 ** -9)
    q, k, v = attn_split(qkv, B, S, H)
    O, tO, _, _ = attn_fwd_bound(q, k, v, lens, scale)
    bw = attn_bwd_bound(q, k, v, attn_heads(dout, B, S, H), e["o_b"].double(), e["lse"].double(), lens, scale)
    assert float(((e["o"].double() - O).abs() / tO).max()) > 1.0
    assert float(((e["dq"].double() - bw["dq"]).abs() / bw["t_dq"]).max()) > 1.0
    assert float(((e["dk"].double() - bw["dk"]).abs() / bw["t_dk"]).max()) > 1.0
