"""Edge paths of the row kernels -- LayerNorm forward / backward, the embeddings, reduce_rows (layernorm.hip),
colsum (gemm.hip) and the classifier head (head.hip) -- on GUARDED buffers, every output held element by element
to the derived bounds of tests/helpers.py against an fp64 reference computed on the device.

Every 2-D bf16 / fp32 buffer, input or output, has one sentinel row before and after it; every 1-D fp32 buffer
(mean, rstd, dgamma, dbeta, dxsum, part, out, the head's tensors) is a slice starting on a multiple of 4 floats
inside a sentinel-filled allocation with 64 floats on both sides. The sentinels are NaN patterns: a store outside
a view changes one and fails assert_guard_intact, an over-read shows as a non-finite result. (colsum's workspace
is allocated inside the binding and cannot be guarded from here; its `out` and its input are.)
tests/test_rowkernel_bound_cpu.py shows on the CPU that the bounds hold for a faithful emulation of the kernels
and that they reject a one-pass variance, eps outside the root, a pipeline slip, a lost row, column sums of the
unrounded dx, a wrong position modulus, lost type-1 tokens, a chunk carry in the head and an overwritten dW_c.

Each check prints `headroom <kernel> <output> <figure>` (pytest -s): for fp32 outputs the largest |err| / t, for
bf16 outputs the largest fraction of the fp32-level allowance t the stored value needs (helpers.bf16_t_used).

Edge -> the case that reaches it:
  LayerNorm, VPL = 1 .. 4 (D = 256, 512, 768, 1024) .................. every test_layernorm_edges case; 512 had no test
  3 idle waves in the only block ...................................... rows 1
  a 1-row tail block (the constant row in it) ......................... rows 5
  ln_bwd: 5 waves walk a second row, every other prefetch clamps ...... rows 2053 (the last row is the 1000 + N one)
  ln_bwd: 4 waves walk a third row (pipeline registers reused twice) .. rows 4100
  var = 0 (only eps under the root) ................................... the constant row: rows 0 and, at 5 rows, the last
  mean >> spread (a one-pass variance would lose rstd) ................ the 64 + N(0,1) and 1000 + N(0,16) rows
  DRES instantiation; DXS with accumulate and dxsum_acc ............... the `dres` and `dxsum` forms of every case
  DX of <VPL, false> and <VPL, true> bit-identical .................... the `plain` and `dxsum` forms of every case
  D = 128 / 384 / 1280 and a short `part` rejected .................... test_layernorm_rejections
  embeddings: 3-row tail block (forward, word kernel); idle waves in
  the position kernel's second block ................................... b3s5 (rows 15, S 5)
  S > 32, B = 2, one-row type table without token types ............... b2s33
  one token ........................................................... b1s1
  a single run covering the batch ..................................... equal
  ids -3 and V + 2 read rows 0 and V - 1; token type 2 reads row 1 .... clamp
  one-row type table with type-1 tokens (forward clamp = backward) .... type1row
  word rows no token names; position rows >= S keep their bits ........ every embedding case
  colsum: two slabs, the second 16 rows | remainder loop after one
  unrolled step | rpb = 33 (M > 8192) | one row, N = 2 strips ......... (33, 8) | (45, 520) | (8193, 16) | (1, 1024)
  colsum on a strided view between NaN padding columns ................ every colsum case
  head: L = 1 | h % 256 != 0 with one label in chunk 2 | 3 chunks |
  the backward's 1024-label limit ..................................... (1,256,1) | (3,200,65) | (2,1024,130) | (2,64,1024)
  head without b_c / db_c; accumulate onto a prefill .................. every head case, both ways
  L = 1025 rejected by the backward ................................... test_head_rejects_1025_labels

Measured on an MI355X (largest figure per output over all cases, and the case that gives it):
  ln_fwd    mean 0.067 (5 x 768)   rstd 0.166 (2053 x 256)   Y 0.068 (2053 x 1024)
  ln_bwd    dx 0.088 (4100 x 768, dres)   dgamma 0.889   dbeta 0.748   dxsum 0.650 (all three: 1 row, accumulating)
  embed     out 0 (every stored value is the correctly rounded reference)   gw 0.987 (b3s5)   gp 0.984 (b1s1)   gt 0.581 (b1s1)
  colsum    out 0.709 (1 x 1024, strided, accumulating)
  head      logits 0.076 ((2, 64, 1024))   dpre 0 (as out)   dW_c 0.880 ((2, 1024, 130), accumulating)   db_c 0.660
The figures near 1 all belong to a sum of ONE term added onto a prefill: the only rounding is that addition's, and
the allowance (u |previous| + 2 u |term|) is then nearly the rounding itself; the CPU emulation reaches the same
0.987 / 0.984 / 0.880 there. Long sums stay far inside (dgamma at 4100 rows: 0.009). The rstd figure is the record of
the rsqrtf allowance (2^-22 of helpers._RSQRT_REL): 0.17 of t_rstd at most, the emulation with a correctly rounded
root reaches 0.20 -- the allowance is not exceeded and was left as derived.

What these tests found (both fixed in layernorm.hip):
  * embed_bwd lost the type gradient of the type-1 tokens of a one-row type table (type1row: gt[0, 0] 7.223 for
    8.315, 256 of 256 elements outside the bound): the forward clamps those tokens to row 0, the backward summed
    them into the partial that is never reduced. The backward now takes every token of a one-row table as type 0.
  * DX of ln_bwd_kernel<VPL, false> and <VPL, true> differed in a few elements per million (none at 1 or 5 rows,
    some at 7 of the 8 cases of 2053 and 4100 rows), both inside the dx bound: the compiler contracted the row's
    products differently in the two instantiations. The kernel now fixes the contraction in its source."""
import pytest
import torch

from ml_trainer_amd.ops._ext import require_native
from tests import helpers as H
from tests.helpers import (ROWK_COLSUM_CASES, ROWK_EMBED_CASES, ROWK_EPS, ROWK_HEAD_CASES, ROWK_LN_ROWS,
                           ROWK_LN_WIDTHS, acc_bound, assert_guard_intact, assert_within, bf16_t_used, guarded,
                           guarded_1d, guarded_like, store_bound)

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
_HEADROOM = {}


def _hold(kernel, name, what, got, exp, t):
    """Every element of `got` within the store's tolerance of exp given the fp32-level allowance t; prints the
    headroom (|err| / t for an fp32 output, helpers.bf16_t_used for a bf16 one)."""
    bf16 = got.dtype == BF16
    assert bool(torch.isfinite(got.float()).all()), f"{kernel} {name} {what}: non-finite values"
    assert_within(got, exp, store_bound(exp, t, got.dtype), f"{kernel} {name} {what}")
    r = bf16_t_used(got, exp, t) if bf16 else float(((got.double() - exp).abs() / t).max())
    _HEADROOM[kernel, name] = max(_HEADROOM.get((kernel, name), 0.0), r)
    print(f"headroom {kernel} {name} {r:.4f} {what}")


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == BF16 else torch.int32)


def _vec(data=None, n=None, dev=None):
    """A guarded fp32 vector: (buf, view), the view holding `data` (any shape, flattened) or left as sentinels."""
    if data is not None:
        n, dev = data.numel(), data.device
    buf, view = guarded_1d(n, dev)
    if data is not None:
        view.copy_(data.reshape(-1))
    return buf, view


class Guards:
    """Collects (buf, view) pairs and checks them all."""

    def __init__(self):
        self.pairs = []

    def __call__(self, pair):
        self.pairs.append(pair)
        return pair[1]

    def check(self):
        for buf, view in self.pairs:
            assert_guard_intact(buf, view)


# ------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("D", ROWK_LN_WIDTHS)
@pytest.mark.parametrize("rows", ROWK_LN_ROWS)
def test_layernorm_edges(dev, rows, D):
    C = require_native()
    what = f"{rows}x{D}"
    G = Guards()
    x, dy, dres, gamma, beta = (a.to(dev) for a in H.ln_edge_inputs(rows, D, seed=rows * 13 + D))
    x, dy, dres = G(guarded_like(x)), G(guarded_like(dy)), G(guarded_like(dres))
    gamma, beta = G(_vec(gamma)), G(_vec(beta))
    y = G(guarded(rows, D, BF16, dev))
    mean, rstd = G(_vec(n=rows, dev=dev)), G(_vec(n=rows, dev=dev))
    C.ln_fwd(x, gamma, beta, y, mean, rstd, ROWK_EPS)
    torch.cuda.synchronize()
    G.check()
    mu, t_mu, rs, t_rs, Y, t_Y = H.ln_fwd_bound(x, gamma, beta, ROWK_EPS)
    _hold("ln_fwd", "mean", what, mean, mu, t_mu)
    _hold("ln_fwd", "rstd", what, rstd, rs, t_rs)
    _hold("ln_fwd", "Y", what, y, Y, t_Y)

    nb = C.ln_partial_blocks(rows)
    assert nb == H.ln_partial_blocks(rows)
    depth = H.ln_bwd_depth(rows)
    g = torch.Generator().manual_seed(rows + D)
    dx_plain = None
    for form in ("plain", "dres", "dxsum"):
        fw = f"{what} {form}"
        B = Guards()
        dx = B(guarded(rows, D, BF16, dev))
        acc = form == "dxsum"
        part = B(_vec(n=nb * (3 if acc else 2) * D, dev=dev))
        prev = [torch.randn(D, generator=g).to(dev) for _ in range(3)] if acc else [None] * 3
        dg, db = B(_vec(prev[0], D, dev)), B(_vec(prev[1], D, dev))
        dxs = B(_vec(prev[2], D, dev)) if acc else None
        C.ln_bwd(dy, x, gamma, mean, rstd, dx, part, dg, db, acc, dres if form == "dres" else None, dxsum=dxs, dxsum_acc=acc)
        torch.cuda.synchronize()
        B.check()
        G.check()  # (the inputs and the forward's outputs: nobody wrote around them either)
        b = H.ln_bwd_bound(dy, x, gamma, mean, rstd, dres if form == "dres" else None)
        _hold("ln_bwd", "dx", fw, dx, b["dx"], b["t_dx"])
        if acc:
            _hold("ln_bwd", "dgamma", fw, dg, prev[0].double() + b["dgamma"], acc_bound(b["t_dgamma"], prev[0], b["dgamma"]))
            _hold("ln_bwd", "dbeta", fw, db, prev[1].double() + b["dbeta"], acc_bound(b["t_dbeta"], prev[1], b["dbeta"]))
            s, t = H.colsum_stored_bound(dx, depth)  # of the kernel's own stored DX
            _hold("ln_bwd", "dxsum", fw, dxs, prev[2].double() + s, acc_bound(t, prev[2], s))
            assert torch.equal(_bits(dx), _bits(dx_plain)), f"{fw}: DX differs from the plain instantiation's"
        else:
            _hold("ln_bwd", "dgamma", fw, dg, b["dgamma"], b["t_dgamma"])
            _hold("ln_bwd", "dbeta", fw, db, b["dbeta"], b["t_dbeta"])
        if form == "plain":
            dx_plain = dx.clone()


def test_layernorm_rejections(dev):
    C = require_native()
    for D in (128, 1280, 384):
        x = torch.zeros(4, D, dtype=BF16, device=dev)
        v = torch.zeros(4, device=dev)
        gamma = torch.ones(D, device=dev)
        with pytest.raises(RuntimeError):
            C.ln_fwd(x, gamma, gamma.clone(), torch.empty_like(x), v.clone(), v.clone(), ROWK_EPS)
        with pytest.raises(RuntimeError):
            C.ln_bwd(x, x, gamma, v, v + 1, torch.empty_like(x), torch.empty(2 * D, device=dev), gamma.clone(),
                     gamma.clone(), False, None)
    rows, D = 9, 256  # 3 blocks
    x = torch.zeros(rows, D, dtype=BF16, device=dev)
    v, gamma = torch.zeros(rows, device=dev), torch.ones(D, device=dev)
    for nseg, dxs in ((2, None), (3, torch.empty(D, device=dev))):
        short = torch.empty(C.ln_partial_blocks(rows) * nseg * D - 1, device=dev)
        with pytest.raises(RuntimeError):
            C.ln_bwd(x, x, gamma, v, v + 1, torch.empty_like(x), short, gamma.clone(), gamma.clone(), False, None, dxsum=dxs)


# ------------------------------------------------------------------------------------------------ embeddings
@pytest.mark.parametrize("D", ROWK_LN_WIDTHS)
@pytest.mark.parametrize("name", [c[0] for c in ROWK_EMBED_CASES])
def test_embedding_edges(dev, name, D):
    C = require_native()
    what = f"{name} D{D}"
    c = H.embed_edge_inputs(name, D, seed=D + len(name))
    c = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    B, S, V, P, ntype, ids, tt = c["B"], c["S"], c["V"], c["P"], c["ntype"], c["ids"], c["tt"]
    n = B * S
    G = Guards()
    ww, wp, wt, dout = (G(guarded_like(c[k])) for k in ("ww", "wp", "wt", "dout"))

    def fwd():
        out = G(guarded(n, D, BF16, dev))
        C.embed_fwd(ids, tt, ww, wp, wt, out, S)
        return out

    def bwd():
        gw, gp, gt = (G(guarded_like(c[k])) for k in ("gw0", "gp0", "gt0"))
        part = G(_vec(n=S * 2 * D, dev=dev))
        # as ops/transformer.py calls it: the ids clamped to the table before the stable sort
        sid, perm = torch.sort(ids.clamp(0, V - 1), stable=True)
        C.embed_bwd(sid, perm, tt, dout, gw, gp, gt, part, S)
        return gw, gp, gt

    out, (gw, gp, gt) = fwd(), bwd()
    out2, (gw2, gp2, gt2) = fwd(), bwd()
    torch.cuda.synchronize()
    G.check()
    exp, t = H.embed_fwd_bound(ww, wp, wt, ids, tt, S)
    _hold("embed_fwd", "out", what, out, exp, t)
    b = H.embed_bwd_bound(dout, ids.clamp(0, V - 1), tt, B, S, c["gw0"], c["gp0"], c["gt0"])
    _hold("embed_bwd", "gw", what, gw, b["gw"], b["t_gw"])
    _hold("embed_bwd", "gp", what, gp, b["gp"], b["t_gp"])
    _hold("embed_bwd", "gt", what, gt, b["gt"], b["t_gt"])
    idle = ~b["touched_w"]
    assert bool(idle.any())
    assert torch.equal(_bits(gw[idle]), _bits(c["gw0"][idle])), f"{what}: a word row no token names changed"
    assert torch.equal(_bits(gp[S:]), _bits(c["gp0"][S:])), f"{what}: a position row >= S changed"
    for a, a2, nm in ((out, out2, "out"), (gw, gw2, "gw"), (gp, gp2, "gp"), (gt, gt2, "gt")):
        assert torch.equal(_bits(a), _bits(a2)), f"{what}: {nm} differs between two launches"


# ---------------------------------------------------------------------------------------------------- colsum
@pytest.mark.parametrize("M,N", ROWK_COLSUM_CASES)
def test_colsum_edges(dev, M, N):
    C = require_native()
    g = torch.Generator().manual_seed(M + N)
    X = torch.randn(M, N, generator=g).to(BF16).to(dev)
    prev = torch.randn(N, generator=g).to(dev)
    depth = H.colsum_depth(M)
    s, t = H.colsum_stored_bound(X, depth)
    xb, xv = guarded_like(X)
    sb, sv = guarded(M, N, BF16, dev, ld=N + 16, col_off=8)  # the padding columns hold NaN sentinels
    sv.copy_(X)
    assert sv.stride(0) == N + 16 and not bool(torch.isfinite(sb[1, :8].float()).any())
    for what, src, acc in (("plain", xv, False), ("accumulate", xv, True), ("strided", sv, False), ("strided acc", sv, True)):
        ob, out = _vec(prev if acc else None, N, dev)
        C.colsum(src, out, acc)
        torch.cuda.synchronize()
        assert_guard_intact(ob, out)
        assert_guard_intact(xb, xv)
        assert_guard_intact(sb, sv)
        if acc:
            _hold("colsum", "out", f"{M}x{N} {what}", out, prev.double() + s, acc_bound(t, prev, s))
        else:
            _hold("colsum", "out", f"{M}x{N} {what}", out, s, t)


# ------------------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize("B,h,L", ROWK_HEAD_CASES)
def test_head_edges(dev, B, h, L):
    C = require_native()
    c = {k: v.to(dev) for k, v in H.head_edge_inputs(B, h, L, seed=B + h + L).items()}
    assert float(c["pooled"].abs().max()) < 1.0
    G = Guards()
    pooled = G(_vec(c["pooled"])).view(B, h)
    wc = G(_vec(c["wc"])).view(L, h)
    bc, dl = G(_vec(c["bc"])), G(_vec(c["dlogits"])).view(B, L)
    for with_bias in (True, False):
        what = f"({B},{h},{L}) bias {with_bias}"
        logits = G(_vec(n=B * L, dev=dev))
        C.head_cls_fwd(pooled, wc, bc if with_bias else None, logits)
        torch.cuda.synchronize()
        G.check()
        exp, t = H.head_fwd_bound(pooled, wc, bc if with_bias else None)
        _hold("head_fwd", "logits", what, logits.view(B, L), exp, t)
        for acc in (False, True):
            fw = f"{what} acc {acc}"
            dpre = G(guarded(B, h, BF16, dev))
            dwc = G(_vec(c["dw0"] if acc else None, L * h, dev))
            dbc_b, dbc = _vec(c["db0"], L, dev)  # prefilled either way: without dbc it must stay as it is
            G((dbc_b, dbc))
            C.head_cls_bwd(dl, pooled, wc, dpre, dwc.view(L, h), dbc if with_bias else None, accumulate=acc)
            torch.cuda.synchronize()
            G.check()
            b = H.head_bwd_bound(dl, pooled, wc, c["dw0"] if acc else None, c["db0"] if acc else None)
            _hold("head_bwd", "dpre", fw, dpre, b["dpre"], b["t_dpre"])
            _hold("head_bwd", "dW_c", fw, dwc.view(L, h), b["dw"], b["t_dw"])
            if with_bias:
                _hold("head_bwd", "db_c", fw, dbc, b["db"], b["t_db"])
            else:
                assert torch.equal(_bits(dbc), _bits(c["db0"])), f"{fw}: db_c written although none was passed"


def test_head_rejects_1025_labels(dev):
    C = require_native()
    B, h, L = 2, 64, 1025
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(RuntimeError):
        C.head_cls_bwd(z(B, L), z(B, h), z(L, h), torch.zeros(B, h, dtype=BF16, device=dev), z(L, h), z(L), accumulate=False)
