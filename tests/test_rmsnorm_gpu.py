"""The RMSNorm kernels (rms_fwd, dropout_add_rms_fwd, rms_bwd) and the LayerNorm backward with dropout AND a
residual gradient (the form the pre-norm blocks use) on the GPU: every buffer guarded, fp64 references on the
device, every output held element by element to the derived bounds of tests/rms_ref.py (proven on the CPU by
tests/test_rmsnorm_bound_cpu.py) and, for the LayerNorm form, of tests/helpers.py.

Cases: widths 256 / 512 / 768 / 1024 x rows 1 / 5 / 2053 / 4100 x the backward forms plain, dres, dxsum (also
accumulating onto a prefill, dgamma too), drop, drop + dres. Bitwise: DX identical across all rms_bwd instantiations
on the same inputs (and across the two LayerNorm forms with dres); dropout_add_rms_fwd's Z equal to
dropout_add_ln_fwd's at p = 0.1 and at a p that keeps everything; its Y / rstd equal to rms_fwd's on that Z; DXM
equal to the torch oracle of ops/dropout.py applied to the stored DX. The zero row gives Y = 0 exactly.
Rejections: D = 128 / 384 / 1280, a short `part`, a misaligned or non-contiguous operand.

Each case prints `headroom <kernel> <output> <largest |err| / t>`.

Measured on an MI355X (largest figure per output over all cases, and the case that gives it):
  rms_fwd              rstd 0.062 (1 x 256)   Y 0.083 (2053 x 256)
  dropout_add_rms_fwd  rstd 0 (as stored)   Y 0.122 (2053 x 768, p = 0.1)
  rms_bwd              dx 0.170 (4100 x 512, plain)   dx with dres 0.201 (4100 x 256)   dgamma 0.183 (5 x 1024)
                       dgamma accumulating 0.806 (1 x 1024)   dxsum accumulating 0.929 (1 x 768)
                       dxsum of DXM 0.199 (5 x 768)
  ln_bwd, drop + dres  dx 0 (every stored value the correctly rounded reference)   dgamma 0.222   dbeta 0.037
                       dxsum 0.096 (all 5 x 768)
The two figures near 1 are one-row sums added onto a prefill: the only rounding is that addition's (the CPU
emulation reaches 0.87 there), as in tests/test_rowkernel_edges_gpu.py. All bitwise checks held on the first run."""
import pytest
import torch

from ml_trainer_amd.ops import dropout as DO
from ml_trainer_amd.ops._ext import require_native
from tests import helpers as H
from tests import rms_ref as R
from tests.helpers import (ROWK_EPS, ROWK_LN_ROWS, ROWK_LN_WIDTHS, acc_bound, assert_guard_intact, assert_within,
                           bf16_t_used, guarded, guarded_1d, guarded_like, store_bound)

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SEED, SITE, RANK, P = 0x1234567, 5, 1, 0.1
FORMS = ("plain", "dres", "dxsum", "drop", "drop_dres")


def _hold(kernel, name, what, got, exp, t):
    bf16 = got.dtype == BF16
    assert bool(torch.isfinite(got.float()).all()), f"{kernel} {name} {what}: non-finite values"
    assert_within(got, exp, store_bound(exp, t, got.dtype), f"{kernel} {name} {what}")
    r = bf16_t_used(got, exp, t) if bf16 else float(((got.double() - exp).abs() / t).max())
    print(f"headroom {kernel} {name} {r:.4f} {what}")


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == BF16 else torch.int32)


def _vec(data=None, n=None, dev=None):
    if data is not None:
        n, dev = data.numel(), data.device
    buf, view = guarded_1d(n, dev)
    if data is not None:
        view.copy_(data.reshape(-1))
    return buf, view


class Guards:
    def __init__(self):
        self.pairs = []

    def __call__(self, pair):
        self.pairs.append(pair)
        return pair[1]

    def check(self):
        for buf, view in self.pairs:
            assert_guard_intact(buf, view)


def _dxm_oracle(dx):
    return DO.apply(dx, P, SEED, SITE, RANK)


@pytest.mark.parametrize("D", ROWK_LN_WIDTHS)
@pytest.mark.parametrize("rows", ROWK_LN_ROWS)
def test_rmsnorm_edges(dev, rows, D):
    C = require_native()
    what = f"{rows}x{D}"
    G = Guards()
    x, dy, dres, gamma = (a.to(dev) for a in R.rms_edge_inputs(rows, D, seed=rows * 13 + D))
    x, dy, dres = G(guarded_like(x)), G(guarded_like(dy)), G(guarded_like(dres))
    gamma = G(_vec(gamma))
    y = G(guarded(rows, D, BF16, dev))
    rstd = G(_vec(n=rows, dev=dev))
    C.rms_fwd(x, gamma, y, rstd, ROWK_EPS)
    torch.cuda.synchronize()
    G.check()
    rs, t_rs, Y, t_Y = R.rms_fwd_bound(x, gamma, ROWK_EPS)
    _hold("rms_fwd", "rstd", what, rstd, rs, t_rs)
    _hold("rms_fwd", "Y", what, y, Y, t_Y)
    if rows >= 5:
        assert bool((x[3] == 0).all()) and bool((y[3] == 0).all()), "the zero row must give exactly 0"

    nb = C.ln_partial_blocks(rows)
    depth = H.ln_bwd_depth(rows)
    g = torch.Generator().manual_seed(rows + D)
    dx_ref = {}
    for form in FORMS:
        fw = f"{what} {form}"
        B = Guards()
        dx = B(guarded(rows, D, BF16, dev))
        want = form != "plain" and form != "dres"
        acc = form == "dxsum"
        dr = dres if form in ("dres", "drop_dres") else None
        drop = form.startswith("drop")
        part = B(_vec(n=nb * (2 if want else 1) * D, dev=dev))
        prev = [torch.randn(D, generator=g).to(dev) for _ in range(2)] if acc else [None] * 2
        dg = B(_vec(prev[0], D, dev))
        dxs = B(_vec(prev[1], D, dev)) if want else None
        dxm = B(guarded(rows, D, BF16, dev)) if drop else None
        kw = dict(dxm=dxm, p=P, seed=SEED, site=SITE, rank=RANK) if drop else {}
        C.rms_bwd(dy, x, gamma, rstd, dx, part, dg, acc, dr, dxsum=dxs, dxsum_acc=acc, **kw)
        torch.cuda.synchronize()
        B.check()
        G.check()
        b = R.rms_bwd_bound(dy, x, gamma, rstd, dr)
        _hold("rms_bwd", "dx_dres" if dr is not None else "dx", fw, dx, b["dx"], b["t_dx"])
        if acc:
            _hold("rms_bwd", "dgamma_acc", fw, dg, prev[0].double() + b["dgamma"], acc_bound(b["t_dgamma"], prev[0], b["dgamma"]))
        else:
            _hold("rms_bwd", "dgamma", fw, dg, b["dgamma"], b["t_dgamma"])
        if drop:
            assert torch.equal(_bits(dxm), _bits(_dxm_oracle(dx))), f"{fw}: DXM differs from the oracle on the stored DX"
            s, t = H.colsum_stored_bound(dxm, depth)
            _hold("rms_bwd", "dxsum_drop", fw, dxs, s, t)
        elif want:
            s, t = H.colsum_stored_bound(dx, depth)
            _hold("rms_bwd", "dxsum", fw, dxs, prev[1].double() + s, acc_bound(t, prev[1], s))
        key = dr is not None
        if key in dx_ref:
            assert torch.equal(_bits(dx), _bits(dx_ref[key])), f"{fw}: DX differs from another instantiation's"
        else:
            dx_ref[key] = dx.clone()


@pytest.mark.parametrize("p", [P, 2.0 ** -40])
@pytest.mark.parametrize("rows,D", [(5, 256), (2053, 768), (9, 1024), (4100, 512)])
def test_dropout_add_rms_fwd_bitwise(dev, rows, D, p):
    """Z is dropout_add_ln_fwd's Z bit for bit; Y / rstd are rms_fwd's on that Z bit for bit. p = 2^-40 has the
    threshold 0: everything is kept and the scale is 1 in fp32, so Z = bf16(Y0 + RES)."""
    C = require_native()
    G = Guards()
    x, y0, res, gamma = (a.to(dev) for a in R.rms_edge_inputs(rows, D, seed=rows + D))
    y0, res, gamma = G(guarded_like(y0)), G(guarded_like(res)), G(_vec(gamma))
    z, y = G(guarded(rows, D, BF16, dev)), G(guarded(rows, D, BF16, dev))
    rstd = G(_vec(n=rows, dev=dev))
    C.dropout_add_rms_fwd(y0, res, gamma, z, y, rstd, ROWK_EPS, p, SEED, SITE, RANK)
    zl, yl = torch.empty_like(z), torch.empty_like(z)
    ml, rl = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    C.dropout_add_ln_fwd(y0, res, gamma, torch.zeros(D, device=dev), zl, yl, ml, rl, ROWK_EPS, p, SEED, SITE, RANK)
    y2, r2 = torch.empty_like(z), torch.empty(rows, device=dev)
    C.rms_fwd(z.contiguous(), gamma, y2, r2, ROWK_EPS)
    torch.cuda.synchronize()
    G.check()
    assert torch.equal(_bits(z), _bits(zl))
    assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(rstd), _bits(r2))
    if p < 1e-6:
        assert torch.equal(_bits(z), _bits((y0.float() + res.float()).to(BF16)))
    else:
        kept = float((z != res).float().mean())
        assert 0.85 < kept < 0.95, kept
    rs, t_rs, Y, t_Y = R.rms_fwd_bound(z, gamma, ROWK_EPS)
    _hold("dropout_add_rms_fwd", "rstd", f"{rows}x{D} p {p:g}", rstd, rs, t_rs)
    _hold("dropout_add_rms_fwd", "Y", f"{rows}x{D} p {p:g}", y, Y, t_Y)


@pytest.mark.parametrize("D", ROWK_LN_WIDTHS)
@pytest.mark.parametrize("rows", ROWK_LN_ROWS)
def test_layernorm_bwd_dropout_with_dres(dev, rows, D):
    """ln_bwd_dropout_res (dxm AND dres; ln_bwd itself keeps rejecting the pair): DX bitwise the plain dres form's, DXM the oracle on it, dxsum / dgamma / dbeta
    within their bounds."""
    C = require_native()
    what = f"{rows}x{D} drop_dres"
    G = Guards()
    x, dy, dres, gamma, beta = (a.to(dev) for a in H.ln_edge_inputs(rows, D, seed=rows * 13 + D))
    x, dy, dres = G(guarded_like(x)), G(guarded_like(dy)), G(guarded_like(dres))
    gamma, beta = G(_vec(gamma)), G(_vec(beta))
    y = torch.empty(rows, D, dtype=BF16, device=dev)
    mean, rstd = G(_vec(n=rows, dev=dev)), G(_vec(n=rows, dev=dev))
    C.ln_fwd(x, gamma, beta, y, mean, rstd, ROWK_EPS)
    nb = C.ln_partial_blocks(rows)
    dx0 = torch.empty(rows, D, dtype=BF16, device=dev)
    C.ln_bwd(dy, x, gamma, mean, rstd, dx0, torch.empty(nb * 2 * D, device=dev), torch.empty(D, device=dev),
             torch.empty(D, device=dev), False, dres)
    dx, dxm = G(guarded(rows, D, BF16, dev)), G(guarded(rows, D, BF16, dev))
    part = G(_vec(n=nb * 3 * D, dev=dev))
    dg, db, dxs = G(_vec(n=D, dev=dev)), G(_vec(n=D, dev=dev)), G(_vec(n=D, dev=dev))
    C.ln_bwd_dropout_res(dy, x, gamma, mean, rstd, dx, part, dg, db, False, dres, dxs, False, dxm, P, SEED, SITE, RANK)
    torch.cuda.synchronize()
    G.check()
    assert torch.equal(_bits(dx), _bits(dx0)), f"{what}: DX differs from the plain dres instantiation's"
    assert torch.equal(_bits(dxm), _bits(_dxm_oracle(dx))), f"{what}: DXM differs from the oracle"
    b = H.ln_bwd_bound(dy, x, gamma, mean, rstd, dres)
    _hold("ln_bwd", "dx", what, dx, b["dx"], b["t_dx"])
    _hold("ln_bwd", "dgamma", what, dg, b["dgamma"], b["t_dgamma"])
    _hold("ln_bwd", "dbeta", what, db, b["dbeta"], b["t_dbeta"])
    s, t = H.colsum_stored_bound(dxm, H.ln_bwd_depth(rows))
    _hold("ln_bwd", "dxsum", what, dxs, s, t)


def test_rmsnorm_rejections(dev):
    C = require_native()
    z = lambda *s: torch.zeros(*s, device=dev)
    for D in (128, 384, 1280):
        x = torch.zeros(4, D, dtype=BF16, device=dev)
        gamma = torch.ones(D, device=dev)
        with pytest.raises(RuntimeError):
            C.rms_fwd(x, gamma, torch.empty_like(x), z(4), ROWK_EPS)
        with pytest.raises(RuntimeError):
            C.dropout_add_rms_fwd(x, x, gamma, torch.empty_like(x), torch.empty_like(x), z(4), ROWK_EPS, 0.1, 1, 1, 0)
        with pytest.raises(RuntimeError):
            C.rms_bwd(x, x, gamma, z(4) + 1, torch.empty_like(x), z(2 * D), gamma.clone(), False, None)
    rows, D = 9, 256  # 3 blocks
    x = torch.zeros(rows, D, dtype=BF16, device=dev)
    v, gamma = z(rows) + 1, torch.ones(D, device=dev)
    ok = lambda **kw: dict(dict(DY=x, X=x, gamma=gamma, rstd=v, DX=torch.empty_like(x), part=z(3 * 2 * D),
                                dgamma=z(D)), **kw)
    C.rms_bwd(**ok())  # the arguments the rejections below each spoil in one place
    for nseg, dxs in ((1, None), (2, z(D))):
        with pytest.raises(RuntimeError):  # a short part
            C.rms_bwd(**ok(part=z(C.ln_partial_blocks(rows) * nseg * D - 1), dxsum=dxs))
    with pytest.raises(RuntimeError):  # dxm without dxsum
        C.rms_bwd(**ok(dxm=torch.empty_like(x), p=0.1))
    mis = torch.zeros(rows * D + 8, dtype=BF16, device=dev)[1:1 + rows * D].view(rows, D)  # 2 bytes off
    nonc = torch.zeros(rows, 2 * D, dtype=BF16, device=dev)[:, :D]
    for bad in (mis, nonc):
        with pytest.raises(RuntimeError):
            C.rms_fwd(bad, gamma, torch.empty_like(x), z(rows), ROWK_EPS)
        with pytest.raises(RuntimeError):
            C.rms_fwd(x, gamma, bad, z(rows), ROWK_EPS)
        with pytest.raises(RuntimeError):
            C.rms_bwd(**ok(DY=bad))
        with pytest.raises(RuntimeError):
            C.rms_bwd(**ok(dres=bad))
        with pytest.raises(RuntimeError):
            C.dropout_add_rms_fwd(x, bad, gamma, torch.empty_like(x), torch.empty_like(x), z(rows), ROWK_EPS, 0.1, 1, 1, 0)
    with pytest.raises(RuntimeError):  # gamma misaligned for the float4 loads
        C.rms_fwd(x, torch.ones(D + 4, device=dev)[1:D + 1], torch.empty_like(x), z(rows), ROWK_EPS)
    with pytest.raises(RuntimeError):  # wrong dtype
        C.rms_fwd(x.float(), gamma, torch.empty_like(x), z(rows), ROWK_EPS)
    torch.cuda.synchronize()
