"""The derived bounds of the RMSNorm kernels (tests/rms_ref.py) against a torch fp32 emulation of rms_fwd_kernel
and rms_bwd_kernel + reduce_rows, on the CPU, in the style of tests/test_rowkernel_bound_cpu.py, whose emulation
pieces (the lane order, the xor butterfly, the walk of a wave's rows, reduce_rows) are reused: the geometry is
ln_bwd_kernel's. Products the kernel fuses (fmaf) are left unfused here: the bounds have to hold for both.

Cases: widths 256 .. 1024 x rows 1 / 5 / 2053 / 4100 (the backward at rows > 2048 for D = 256 only) x eps 1e-5 and
1e-12, inputs rms_ref.rms_edge_inputs. test_rmsnorm_emulation_within_bounds prints
`headroom rmsnorm <output> <largest |err| / t>`; every figure must be <= 1. Largest figures over all cases:
  rstd 0.06   Y 0.29   dx 0.44 (plain) / 0.95 (with dres: the final add's own rounding, as LayerNorm's)
  dgamma 0.87 (accumulating, one row; 0.17 otherwise)   dxsum 0.26

MUTATIONS (defect -> the output and case that must catch it):
  centred ....................... rstd and Y on every case (the mean subtracted: LayerNorm's statistics)
  eps_after_root ................ rstd, rows >= 5 (the zero row: 1 / eps instead of 1 / sqrt(eps)); NOT visible at
                                  1 row, whose only row is 64 + N(0, 1): eps does not show next to mean(x^2) ~ 4096
  ln_formula .................... dx (the backward subtracting s1 = mean(t) as LayerNorm's does)
  stats_of_prefetched_row ....... dx, 5 x 256 (rstd of row min(row + 4 nb, rows - 1))
  stats_of_next_walked_row ...... dx, 2053 x 256 and 4100 x 256 ONLY (needs a wave that walks a second row)
  dgamma_without_last_row ....... dgamma, 2053 x 256 and 1 x 256
  dxsum_of_unrounded_dx ......... dxsum, 5 x 256"""
import pytest
import torch

from tests import helpers as H
from tests import rms_ref as R
from tests.helpers import ROWK_LN_ROWS, ROWK_LN_WIDTHS, acc_bound, store_bound
from tests.test_rowkernel_bound_cpu import _inv, _ratio, _walk_sum, _wave_sum

BF16, F32 = torch.bfloat16, torch.float32
EPS = (1e-5, 1e-12)
CASES = [(rows, D) for D in ROWK_LN_WIDTHS for rows in ROWK_LN_ROWS]
BWD_CASES = [(rows, D) for rows, D in CASES if rows <= 2048 or D == 256]


def emulate_rms_fwd(x, gamma, eps, mut=None):
    x = x.float()
    D = x.shape[1]
    eps = torch.tensor(eps, dtype=F32)
    if mut == "centred":
        x = x - (_wave_sum(x) * _inv(D))[:, None]
    ms = _wave_sum(x * x) * _inv(D)
    rs = 1.0 / (torch.sqrt(ms) + eps) if mut == "eps_after_root" else torch.rsqrt(ms + eps)
    return rs, x * rs[:, None] * gamma


def emulate_rms_bwd(dy, x, gamma, rstd, dres=None, mut=None):
    """dict(dx fp32 before its store, dx_b, dgamma, dxsum) of rms_bwd_kernel<VPL, true> + reduce_rows."""
    dy, x = dy.float(), x.float()
    rows, D = x.shape
    nb = H.ln_partial_blocks(rows)
    r = torch.arange(rows)
    if mut == "stats_of_prefetched_row":
        r = (r + 4 * nb).clamp_max(rows - 1)
    if mut == "stats_of_next_walked_row":
        r = torch.where(r + 4 * nb < rows, r + 4 * nb, r)
    rs = rstd[r][:, None]
    xh = x * rs
    t = dy * gamma
    s2 = (_wave_sum(t * xh) * _inv(D))[:, None]
    b = t - xh * s2
    if mut == "ln_formula":
        b = b - (_wave_sum(t) * _inv(D))[:, None]
    o = rs * b
    if dres is not None:
        o = o + dres.float()
    dxb = o.to(BF16)
    cg = dy * xh
    if mut == "dgamma_without_last_row":
        cg = cg.clone()
        cg[rows - 1] = 0
    cx = o if mut == "dxsum_of_unrounded_dx" else dxb.float()
    return dict(dx=o, dx_b=dxb, dgamma=_walk_sum(cg, rows, nb), dxsum=_walk_sum(cx, rows, nb))


_CASE = {}


def _case(rows, D, eps):
    if (rows, D, eps) not in _CASE:
        x, dy, dres, gamma = R.rms_edge_inputs(rows, D, seed=rows * 13 + D)
        _CASE[rows, D, eps] = dict(x=x, dy=dy, dres=dres, gamma=gamma, fwd=emulate_rms_fwd(x, gamma, eps),
                                   bound=R.rms_fwd_bound(x, gamma, eps))
    return _CASE[rows, D, eps]


def rms_ratios(rows, D, eps, fwd_mut=None, bwd_mut=None, forms=("plain", "dres", "dxsum")):
    """{output: largest |value - reference| / tolerance}; the bf16 outputs (keys ending in _b) against store_bound.
    dx with and without dres are kept apart (dx / dx_dres)."""
    c = _case(rows, D, eps)
    rs, t_rs, Y, t_Y = c["bound"]
    r, y = emulate_rms_fwd(c["x"], c["gamma"], eps, fwd_mut) if fwd_mut else c["fwd"]
    out = dict(rstd=_ratio(r, rs, t_rs), Y=_ratio(y, Y, t_Y), Y_b=_ratio(y.to(BF16), Y, store_bound(Y, t_Y, BF16)))
    if (rows, D) not in BWD_CASES:
        return out
    rstd = c["fwd"][0]  # the unmutated forward's own statistics feed the backward
    depth = H.ln_bwd_depth(rows)
    upd = lambda k, v: out.__setitem__(k, max(out.get(k, 0.0), v))
    for form in forms:
        dres = c["dres"] if form == "dres" else None
        e = emulate_rms_bwd(c["dy"], c["x"], c["gamma"], rstd, dres, bwd_mut)
        b = R.rms_bwd_bound(c["dy"], c["x"], c["gamma"], rstd, dres)
        k = "dx_dres" if form == "dres" else "dx"
        upd(k, _ratio(e["dx"], b["dx"], b["t_dx"]))
        upd(k + "_b", _ratio(e["dx_b"], b["dx"], store_bound(b["dx"], b["t_dx"], BF16)))
        if form == "dxsum":  # the accumulating forms, on a prefill of ones
            prev = torch.ones(D)
            upd("dgamma_acc", _ratio(prev + e["dgamma"], 1 + b["dgamma"], acc_bound(b["t_dgamma"], prev, b["dgamma"])))
            s, t = H.colsum_stored_bound(e["dx_b"], depth)
            upd("dxsum", _ratio(prev + e["dxsum"], 1 + s, acc_bound(t, prev, s)))
        else:
            upd("dgamma", _ratio(e["dgamma"], b["dgamma"], b["t_dgamma"]))
    return out


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("rows,D", CASES)
def test_rmsnorm_emulation_within_bounds(rows, D, eps):
    r = rms_ratios(rows, D, eps)
    for k, v in r.items():
        print(f"headroom rmsnorm {k} {v:.4f} {rows}x{D} eps {eps:g}")
    assert max(r.values()) <= 1.0, r
    if (rows, D) in BWD_CASES:
        assert set(r) >= {"dx", "dx_b", "dx_dres", "dgamma", "dgamma_acc", "dxsum"}


def test_zero_row_is_exactly_zero_and_its_rstd_is_eps_alone():
    for eps in EPS:
        c = _case(5, 256, eps)
        rs, y = c["fwd"]
        assert bool((c["x"][3] == 0).all()) and bool((y[3] == 0).all())
        e32 = torch.tensor(eps, dtype=F32).double()
        assert abs(float(rs[3]) * float(e32.sqrt()) - 1) <= R.rel_rs(256)
        assert bool((c["bound"][2][3] == 0).all())


# mutation -> (forward?, the (case, output) pairs that must catch it, the cases that must NOT see it)
MUTATIONS = {
    "centred": (True, [(c, k) for c in BWD_CASES for k in ("rstd", "Y_b")], []),
    "eps_after_root": (True, [(c, "rstd") for c in BWD_CASES if c[0] >= 5], [(1, 256), (1, 1024)]),
    "ln_formula": (False, [((5, 256), "dx_b"), ((2053, 256), "dx_b")], []),
    "stats_of_prefetched_row": (False, [((5, 256), "dx_b")], []),
    "stats_of_next_walked_row": (False, [((2053, 256), "dx_b"), ((4100, 256), "dx_b")], [(1, 256), (5, 256), (5, 1024)]),
    "dgamma_without_last_row": (False, [((2053, 256), "dgamma"), ((1, 256), "dgamma")], []),
    "dxsum_of_unrounded_dx": (False, [((5, 256), "dxsum")], []),
}


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_mutation_is_caught(mut):
    """The defect, built into the emulation, leaves the bound of the named STORED output on the named case (and is
    invisible on the cases listed as blind to it)."""
    fwd, must, blind = MUTATIONS[mut]
    stored = lambda r: {k: v for k, v in r.items() if k not in ("dx", "dx_dres", "Y")}  # fp32 values before a bf16 store
    caught, least = {}, {}
    for case in BWD_CASES:
        r = stored(rms_ratios(*case, EPS[0], fwd_mut=mut, forms=()) if fwd else rms_ratios(*case, EPS[0], bwd_mut=mut))
        hit = {k: v for k, v in r.items() if v > 1.0}
        if hit:
            caught[case] = hit
            print(f"mutation {mut} caught on {case}: " + " ".join(f"{k} {v:.3g}" for k, v in hit.items()))
    for case, output in must:
        assert case in caught and output in caught[case], (mut, case, output, caught)
        least[output] = min(least.get(output, float("inf")), caught[case][output])
    print(f"mutation {mut}: least margin over the cases that must catch it " + " ".join(f"{k} {v:.3g}" for k, v in least.items()))
    for case in blind:
        assert case not in caught, (mut, case, caught[case])
