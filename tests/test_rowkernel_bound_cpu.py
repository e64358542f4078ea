"""The derived bounds of the row kernels in tests/helpers.py (ln_fwd_bound, ln_bwd_bound, colsum_stored_bound,
embed_fwd_bound, embed_bwd_bound, head_fwd_bound, head_bwd_bound) against a torch fp32 emulation of the kernels,
on the CPU.

The emulation does what layernorm.hip, gemm.hip's colsum and head.hip do, in their order of operations: a lane's
E = D / 64 values summed in order, the 6-level xor butterfly of wave_sum, 1 / D as an fp32 constant, the two-pass
variance, rsqrt in fp32; in the backward a wave's rows walked in order (row, row + 4 nb, ...), the 4-wave LDS sum
(w0 + w1) + (w2 + w3), reduce_rows' lane stride over the partial rows and its butterfly, dxsum from the
bf16-rounded dx; colsum's slabs of rpb rows with every 4th row to a wave; the embedding sums in token / batch /
position order; the head's strided fma chains (an fma is emulated exactly: the product in fp64, one rounding),
the per-chunk partials and the fixed-order wave sum onto the bias. Products the compiler may or may not contract
into an fma are left unfused: the bounds have to hold for both.

Two conditions make the bounds worth using on the GPU:
  * the emulation stays within them at every element of every case of the shared case lists (helpers.ROWK_*;
    the LayerNorm backward at rows > 2048 for D = 256 only, to keep this file to seconds): test_*_emulation_within_bounds,
    which print `headroom <kernel> <output> <largest |err| / t>`;
  * every mutation of MUTATIONS -- each a plausible kernel defect -- pushes the named output outside its bound on
    the named case: test_mutation_is_caught prints every (case, output) that catches it.

What the emulation settled about the two families whose formulas had not been emulated before:
  * embeddings: the formulas hold as derived;
  * head: logits, dW_c and db_c hold as derived. dpre did not: with (L + 4) u |1 - y^2| sum_l |dl_l w_lj| the
    emulation left the bound 56-fold at (B, h, L) = (1, 256, 1) and 179-fold at (5, 768, 3), at pooled values
    near +-1 (3.4- and 2.3-fold at L = 65 and 130, not at L = 1024). The derivation had
    missed that y y is rounded BEFORE it is subtracted from 1: an absolute error of up to u y^2 in 1 - y^2,
    which does not shrink with 1 - y^2. helpers.head_bwd_bound carries the term (u y^2 sum_l |dl_l w_lj|);
    test_dpre_bound_needs_the_y2_term keeps the finding.

MUTATIONS (defect -> the output and case that must catch it):
  one_pass_variance ............ rstd, LayerNorm 5 x 256 (the 1000 + N(0, 16) row)
  eps_after_root ............... rstd, LayerNorm 5 x 256 (the constant row: 1 / eps instead of 1 / sqrt(eps))
  stats_of_prefetched_row ...... dx, LayerNorm 5 x 256 (statistics of row min(row + 4 nb, rows - 1))
  stats_of_next_walked_row ..... dx, LayerNorm 2053 x 256 and 4100 x 256 ONLY: the slip on the rows that have a
                                 successor in their wave's walk, which no case of <= 2048 rows can show
  dgamma_without_last_row ...... dgamma, LayerNorm 2053 x 256 (and 1 and 4100 rows; at 5 rows the last row is the
                                 constant one, whose xhat is 0: nothing to lose there)
  dxsum_of_unrounded_dx ........ dxsum, LayerNorm 5 x 256
  pos_mod_s_plus_1 ............. out, embedding b3s5 (position row % (S + 1))
  type1_tokens_lost ............ gt, embedding type1row (one-row table, token types holding 1s)
  head_chunk_carry ............. logits, head (3, 200, 65) (the first chunk's partials added into the second)
  dwc_overwritten .............. dW_c, head (5, 768, 3), accumulating form"""
import pytest
import torch

from tests import helpers as H
from tests.helpers import (ROWK_COLSUM_CASES, ROWK_EMBED_CASES, ROWK_EPS, ROWK_HEAD_CASES, ROWK_LN_ROWS,
                           ROWK_LN_WIDTHS, acc_bound, store_bound)

BF16, F32 = torch.bfloat16, torch.float32
LN_CASES = [(rows, D) for D in ROWK_LN_WIDTHS for rows in ROWK_LN_ROWS]
LN_BWD_CASES = [(rows, D) for rows, D in LN_CASES if rows <= 2048 or D == 256]
_LANE = torch.arange(64)


# ------------------------------------------------------------------------------------------- emulation pieces
def _lanes(a):
    """[rows, D] -> [rows, 64, E]: lane l holds columns 4 (l + 64 v) + q in the order i = 4 v + q (load_row)."""
    rows, D = a.shape
    return a.view(rows, D // 256, 64, 4).permute(0, 2, 1, 3).reshape(rows, 64, D // 64)


def _seq_sum(a, dim):
    """fp32 sum along `dim` in index order, from 0.f."""
    s = torch.zeros_like(a.select(dim, 0))
    for i in range(a.shape[dim]):
        s = s + a.select(dim, i)
    return s


def _butterfly(v, dim):
    """The xor butterfly over 64 lanes along `dim` (offsets 32 .. 1); every lane ends with the same value."""
    v = v.movedim(dim, -1)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ o]
    return v[..., 0]


def _wave_sum(a):  # [rows, D] -> [rows]
    return _butterfly(_seq_sum(_lanes(a), 2), 1)


def _inv(D):
    return torch.tensor(1.0, dtype=F32) / torch.tensor(float(D), dtype=F32)


def _reduce_rows(part):
    """reduce_rows_kernel on part [R, W]: lanes stride the rows, then the butterfly."""
    R, W = part.shape
    k = -(-R // 64)
    p = torch.zeros(k * 64, W, dtype=F32)
    p[:R] = part
    return _butterfly(_seq_sum(p.view(k, 64, W), 0), 0)


def _fma(a, b, c):
    """fp32 fma: the fp32 x fp32 product is exact in fp64."""
    return (a.double() * b.double() + c.double()).float()


# ------------------------------------------------------------------------------------------------- LayerNorm
def emulate_ln_fwd(x, gamma, beta, eps, mut=None):
    x = x.float()
    D = x.shape[1]
    eps = torch.tensor(eps, dtype=F32)
    mu = _wave_sum(x) * _inv(D)
    if mut == "one_pass_variance":
        var = _wave_sum(x * x) * _inv(D) - mu * mu
    else:
        d = x - mu[:, None]
        var = _wave_sum(d * d) * _inv(D)
    rs = 1.0 / (torch.sqrt(var) + eps) if mut == "eps_after_root" else torch.rsqrt(var + eps)
    y = (x - mu[:, None]) * rs[:, None] * gamma + beta
    return mu, rs, y


def _walk_sum(contrib, rows, nb):
    """Column sums as ln_bwd_kernel + reduce_rows form them: wave w of the 4 nb walks rows w, w + 4 nb, ...."""
    D = contrib.shape[1]
    it = -(-rows // (4 * nb))
    c = torch.zeros(it * 4 * nb, D, dtype=F32)
    c[:rows] = contrib
    w = _seq_sum(c.view(it, 4 * nb, D), 0).view(nb, 4, D)
    return _reduce_rows((w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3]))


def emulate_ln_bwd(dy, x, gamma, mean, rstd, dres=None, mut=None):
    """dict(dx fp32 before its store, dx_b, dgamma, dbeta, dxsum) of ln_bwd_kernel<VPL, true> + reduce_rows."""
    dy, x = dy.float(), x.float()
    rows, D = x.shape
    nb = H.ln_partial_blocks(rows)
    r = torch.arange(rows)
    if mut == "stats_of_prefetched_row":
        r = (r + 4 * nb).clamp_max(rows - 1)
    if mut == "stats_of_next_walked_row":
        r = torch.where(r + 4 * nb < rows, r + 4 * nb, r)
    mu, rs = mean[r][:, None], rstd[r][:, None]
    xh = (x - mu) * rs
    t = dy * gamma
    s1 = (_wave_sum(t) * _inv(D))[:, None]
    s2 = (_wave_sum(t * xh) * _inv(D))[:, None]
    o = rs * (t - s1 - xh * s2)
    if dres is not None:
        o = o + dres.float()
    dxb = o.to(BF16)
    cg = dy * xh
    if mut == "dgamma_without_last_row":
        cg = cg.clone()
        cg[rows - 1] = 0
    cx = o if mut == "dxsum_of_unrounded_dx" else dxb.float()
    return dict(dx=o, dx_b=dxb, dgamma=_walk_sum(cg, rows, nb), dbeta=_walk_sum(dy, rows, nb), dxsum=_walk_sum(cx, rows, nb))


_LN = {}


def _ln_case(rows, D):
    """Inputs, the emulated forward (the `kernel's own` mean / rstd) and the forward bound: made once."""
    if (rows, D) not in _LN:
        x, dy, dres, gamma, beta = H.ln_edge_inputs(rows, D, seed=rows * 13 + D)
        _LN[rows, D] = dict(x=x, dy=dy, dres=dres, gamma=gamma, beta=beta, fwd=emulate_ln_fwd(x, gamma, beta, ROWK_EPS),
                            bound=H.ln_fwd_bound(x, gamma, beta, ROWK_EPS))
    return _LN[rows, D]


def _ratio(out, ref, tol):
    """Largest |out - ref| / tol; inf where a value is not finite or not comparable."""
    r = (out.double() - ref).abs() / tol
    return float("inf") if not bool(torch.isfinite(r).all()) else float(r.max())


def ln_ratios(rows, D, fwd_mut=None, bwd_mut=None, forms=("plain", "dres", "dxsum")):
    """{output: largest |value - reference| / tolerance} of the emulated forward and the three backward forms;
    the bf16 outputs (keys ending in _b) against store_bound."""
    c = _ln_case(rows, D)
    mu, t_mu, rs, t_rs, Y, t_Y = c["bound"]
    m, r, y = emulate_ln_fwd(c["x"], c["gamma"], c["beta"], ROWK_EPS, fwd_mut) if fwd_mut else c["fwd"]
    out = dict(mean=_ratio(m, mu, t_mu), rstd=_ratio(r, rs, t_rs), Y=_ratio(y, Y, t_Y),
               Y_b=_ratio(y.to(BF16), Y, store_bound(Y, t_Y, BF16)))
    if (rows, D) not in LN_BWD_CASES:
        return out
    mean, rstd = c["fwd"][0], c["fwd"][1]  # the unmutated forward's statistics feed the backward
    depth = H.ln_bwd_depth(rows)
    upd = lambda k, v: out.__setitem__(k, max(out.get(k, 0.0), v))
    for form in forms:
        dres = c["dres"] if form == "dres" else None
        e = emulate_ln_bwd(c["dy"], c["x"], c["gamma"], mean, rstd, dres, bwd_mut)
        b = H.ln_bwd_bound(c["dy"], c["x"], c["gamma"], mean, rstd, dres)
        upd("dx", _ratio(e["dx"], b["dx"], b["t_dx"]))
        upd("dx_b", _ratio(e["dx_b"], b["dx"], store_bound(b["dx"], b["t_dx"], BF16)))
        if form == "dxsum":  # the accumulating forms, on a prefill of ones
            prev = torch.ones(D)
            upd("dgamma", _ratio(prev + e["dgamma"], 1 + b["dgamma"], acc_bound(b["t_dgamma"], prev, b["dgamma"])))
            upd("dbeta", _ratio(prev + e["dbeta"], 1 + b["dbeta"], acc_bound(b["t_dbeta"], prev, b["dbeta"])))
            s, t = H.colsum_stored_bound(e["dx_b"], depth)
            upd("dxsum", _ratio(prev + e["dxsum"], 1 + s, acc_bound(t, prev, s)))
        else:
            upd("dgamma", _ratio(e["dgamma"], b["dgamma"], b["t_dgamma"]))
            upd("dbeta", _ratio(e["dbeta"], b["dbeta"], b["t_dbeta"]))
    return out


def _report(kernel, what, r):
    for k, v in r.items():
        print(f"headroom {kernel} {k} {v:.4f} {what}")


@pytest.mark.parametrize("rows,D", LN_CASES)
def test_layernorm_emulation_within_bounds(rows, D):
    r = ln_ratios(rows, D)
    _report("layernorm", f"{rows}x{D}", r)
    assert max(r.values()) <= 1.0, r
    if (rows, D) in LN_BWD_CASES:
        assert set(r) >= {"dx", "dx_b", "dgamma", "dbeta", "dxsum"}


def test_first_order_range_is_checked():
    """A row whose mean error could reach half its spread is reported, not bounded."""
    x = torch.full((2, 256), 3.0e4).to(BF16)
    with pytest.raises(AssertionError, match="row 0"):
        H.ln_fwd_bound(x, torch.ones(256), torch.zeros(256), 1e-12)


# ---------------------------------------------------------------------------------------------------- colsum
def emulate_colsum(X):
    X = X.float()
    M, N = X.shape
    R, rpb = H.colsum_geometry(M)
    k = -(-rpb // 4)
    p = torch.zeros(R, k * 4, N, dtype=F32)
    for s in range(R):
        rows = X[s * rpb:min(M, (s + 1) * rpb)]
        p[s, :rows.shape[0]] = rows
    w = _seq_sum(p.view(R, k, 4, N), 1)
    return _reduce_rows((w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3]))


@pytest.mark.parametrize("M,N", ROWK_COLSUM_CASES)
def test_colsum_emulation_within_bounds(M, N):
    X = torch.randn(M, N, generator=torch.Generator().manual_seed(M + N)).to(BF16)
    s, t = H.colsum_stored_bound(X, H.colsum_depth(M))
    e = emulate_colsum(X)
    prev = torch.ones(N)
    r = dict(out=_ratio(e, s, t), out_acc=_ratio(prev + e, 1 + s, acc_bound(t, prev, s)))
    _report("colsum", f"{M}x{N}", r)
    assert max(r.values()) <= 1.0, r


def test_colsum_geometry_of_the_cases():
    assert [H.colsum_geometry(M) for M, _ in ROWK_COLSUM_CASES] == [(2, 17), (2, 23), (249, 33), (1, 1)]
    assert H.ln_bwd_depth(2053) == 2 + 2 + 8 + 6 and H.ln_bwd_depth(4100) == 3 + 2 + 8 + 6 and H.ln_bwd_depth(5) == 1 + 2 + 1 + 6


# ------------------------------------------------------------------------------------------------ embeddings
def emulate_embed(c, mut=None):
    """dict(out fp32 before its store, out_b, gw, gp, gt) of embed_fwd_kernel and the two backward kernels."""
    B, S, V, ntype = c["B"], c["S"], c["V"], c["ntype"]
    ids, tt, d = c["ids"], c["tt"], c["dout"].float()
    n, D = d.shape
    wi, pi, ti = H.embed_rows(ids, tt, S, V, ntype)
    if mut == "pos_mod_s_plus_1":
        pi = torch.arange(n) % (S + 1)
    o = (c["ww"].float()[wi] + c["wp"].float()[pi]) + c["wt"].float()[ti]
    gw, gp, gt = c["gw0"].clone(), c["gp0"].clone(), c["gt0"].clone()
    sid, perm = torch.sort(wi, stable=True)  # the backward is called with the clamped ids, as ops/transformer.py does
    i = 0
    while i < n:
        acc, j = torch.zeros(D), i
        while j < n and sid[j] == sid[i]:
            acc = acc + d[perm[j]]
            j += 1
        gw[sid[i]] = gw[sid[i]] + acc
        i = j
    part = torch.zeros(S, 2 * D)
    # the kernel's own test of a token's type; a one-row table counts every token as type 0 (as the forward reads it)
    one = torch.zeros(n, dtype=torch.bool) if tt is None or (ntype < 2 and mut != "type1_tokens_lost") else tt != 0
    for pos in range(S):
        a, t0, t1 = torch.zeros(D), torch.zeros(D), torch.zeros(D)
        for r in range(pos, n, S):
            a = a + d[r]
            t0 = t0 + (torch.zeros(D) if one[r] else d[r])
            t1 = t1 + (d[r] if one[r] else torch.zeros(D))
        gp[pos] = gp[pos] + a
        part[pos, :D], part[pos, D:] = t0, t1
    W = 2 * D if ntype >= 2 else D
    gt = gt + _reduce_rows(part[:, :W]).view(-1, D)
    return dict(out=o, out_b=o.to(BF16), gw=gw, gp=gp, gt=gt)


def embed_ratios(name, D, mut=None):
    c = H.embed_edge_inputs(name, D, seed=D + len(name))
    e = emulate_embed(c, mut)
    out, t = H.embed_fwd_bound(c["ww"], c["wp"], c["wt"], c["ids"], c["tt"], c["S"])
    b = H.embed_bwd_bound(c["dout"], c["ids"].clamp(0, c["V"] - 1), c["tt"], c["B"], c["S"], c["gw0"], c["gp0"], c["gt0"])
    # rows no token names keep their prefill bits
    assert torch.equal(e["gw"][~b["touched_w"]], c["gw0"][~b["touched_w"]]) and torch.equal(e["gp"][c["S"]:], c["gp0"][c["S"]:])
    return dict(out=_ratio(e["out"], out, t), out_b=_ratio(e["out_b"], out, store_bound(out, t, BF16)),
                gw=_ratio(e["gw"], b["gw"], b["t_gw"]), gp=_ratio(e["gp"], b["gp"], b["t_gp"]), gt=_ratio(e["gt"], b["gt"], b["t_gt"]))


EMBED_CASES = [(c[0], D) for c in ROWK_EMBED_CASES for D in ROWK_LN_WIDTHS]


@pytest.mark.parametrize("name,D", EMBED_CASES)
def test_embedding_emulation_within_bounds(name, D):
    r = embed_ratios(name, D)
    _report("embedding", f"{name} D{D}", r)
    assert max(r.values()) <= 1.0, r


def test_embedding_clamp_case_reads_the_edge_rows():
    c = H.embed_edge_inputs("clamp", 256, 1)
    wi, _, ti = H.embed_rows(c["ids"], c["tt"], c["S"], c["V"], c["ntype"])
    assert int(c["ids"].min()) == -3 and int(c["ids"].max()) == c["V"] + 2 and int(c["tt"].max()) == 2
    assert int(wi[3]) == 0 and int(wi[-1]) == c["V"] - 1 and int(ti[5]) == 1
    e = H.embed_edge_inputs("equal", 256, 1)
    assert int(e["ids"].min()) == int(e["ids"].max())
    t = H.embed_edge_inputs("type1row", 256, 1)
    assert t["ntype"] == 1 and int(t["tt"].sum()) >= 1


# ------------------------------------------------------------------------------------------------------ head
def emulate_head(c, with_bias=True, accumulate=False, mut=None, fused_tanh_grad=False):
    """dict(logits, dpre fp32 before its store, dpre_b, dw, db) of head_cls_fwd_kernel / head_cls_bwd_*_kernel."""
    x, w, dl = c["pooled"], c["wc"], c["dlogits"]
    B, h = x.shape
    L = w.shape[0]
    k = -(-h // 256)
    xp, wp = torch.zeros(B, k * 256), torch.zeros(L, k * 256)
    xp[:, :h], wp[:, :h] = x, w
    s = torch.zeros(B, L, 256)
    for i in range(k):  # thread t chains j = t, t + 256, ... (the padding adds exact zeros)
        s = _fma(xp[:, None, i * 256:(i + 1) * 256], wp[None, :, i * 256:(i + 1) * 256], s)
    red = _butterfly(s.view(B, L, 4, 64), 3)  # [B, L, 4]: red[w][l]
    if mut == "head_chunk_carry":  # the second chunk's slots still hold the first chunk's partials, added to
        red = red.clone()
        red[:, 64:128] = red[:, 64:128] + red[:, 0:min(64, L - 64)] if L > 64 else red[:, 64:128]
    logits = c["bc"].expand(B, L).clone() if with_bias else torch.zeros(B, L)
    for wv in range(4):
        logits = logits + red[:, :, wv]
    s = torch.zeros(B, h)
    for l in range(L):
        s = _fma(dl[:, l:l + 1], w[l][None, :], s)
    g = _fma(-x, x, torch.ones(())) if fused_tanh_grad else 1.0 - x * x
    dpre = s * g
    dw, db = torch.zeros(L, h), torch.zeros(L)
    for b in range(B):
        dw = _fma(dl[b][:, None], x[b][None, :], dw)
        db = db + dl[b]
    if accumulate:
        dw = dw if mut == "dwc_overwritten" else c["dw0"] + dw
        db = c["db0"] + db
    return dict(logits=logits, dpre=dpre, dpre_b=dpre.to(BF16), dw=dw, db=db)


def head_ratios(B, h, L, with_bias=True, accumulate=False, mut=None, fused=False):
    c = H.head_edge_inputs(B, h, L, seed=B + h + L)
    e = emulate_head(c, with_bias, accumulate, mut, fused)
    lo, t_lo = H.head_fwd_bound(c["pooled"], c["wc"], c["bc"] if with_bias else None)
    b = H.head_bwd_bound(c["dlogits"], c["pooled"], c["wc"], c["dw0"] if accumulate else None, c["db0"] if accumulate else None)
    return dict(logits=_ratio(e["logits"], lo, t_lo), dpre=_ratio(e["dpre"], b["dpre"], b["t_dpre"]),
                dpre_b=_ratio(e["dpre_b"], b["dpre"], store_bound(b["dpre"], b["t_dpre"], BF16)),
                dW_c=_ratio(e["dw"], b["dw"], b["t_dw"]), db_c=_ratio(e["db"], b["db"], b["t_db"]))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("B,h,L", ROWK_HEAD_CASES)
def test_head_emulation_within_bounds(B, h, L, accumulate, fused):
    """With and without the bias (tied to `accumulate` to keep the grid small), 1 - y y unfused and as one fma."""
    r = head_ratios(B, h, L, with_bias=accumulate, accumulate=accumulate, fused=fused)
    _report("head", f"({B},{h},{L}) acc {accumulate} fma {fused}", r)
    assert max(r.values()) <= 1.0, r


def test_dpre_bound_needs_the_y2_term():
    """Without the u y^2 sum_l |dl_l w_lj| term (the rounding of y y before 1 - y y) the unfused emulation leaves the
    allowance of dpre at L = 1; with the product and the subtraction contracted into one fma it does not."""
    B, h, L = ROWK_HEAD_CASES[0]
    c = H.head_edge_inputs(B, h, L, seed=B + h + L)
    x, dl, w = c["pooled"].double(), c["dlogits"].double(), c["wc"].double()
    t_old = (L + 4) * 2.0 ** -24 * (1 - x * x).abs() * (dl.abs() @ w.abs()) + 1e-30
    ref = (dl @ w) * (1 - x * x)
    assert _ratio(emulate_head(c)["dpre"], ref, t_old) > 1.0
    assert _ratio(emulate_head(c, fused_tanh_grad=True)["dpre"], ref, t_old) <= 1.0


# ------------------------------------------------------------------------------------------------- mutations
# mutation -> (family, the (case, output) pairs that must catch it, the cases that must NOT see it)
MUTATIONS = {
    "one_pass_variance": ("ln_fwd", [((5, 256), "rstd")], []),
    "eps_after_root": ("ln_fwd", [((5, 256), "rstd")], []),
    "stats_of_prefetched_row": ("ln_bwd", [((5, 256), "dx_b")], []),
    "stats_of_next_walked_row": ("ln_bwd", [((2053, 256), "dx_b"), ((4100, 256), "dx_b")], [(1, 256), (5, 256), (5, 1024)]),
    "dgamma_without_last_row": ("ln_bwd", [((2053, 256), "dgamma"), ((1, 256), "dgamma")], []),
    "dxsum_of_unrounded_dx": ("ln_bwd", [((5, 256), "dxsum")], []),
    "pos_mod_s_plus_1": ("embed", [(("b3s5", 256), "out_b")], []),
    "type1_tokens_lost": ("embed", [(("type1row", 256), "gt")], [("b3s5", 256), ("b2s33", 256)]),
    "head_chunk_carry": ("head", [((3, 200, 65), "logits")], [(5, 768, 3)]),
    "dwc_overwritten": ("head", [((5, 768, 3), "dW_c")], []),
}


def _mutated(family, case, mut):
    if family == "ln_fwd":
        return ln_ratios(*case, fwd_mut=mut, forms=())
    if family == "ln_bwd":
        return ln_ratios(*case, bwd_mut=mut)
    if family == "embed":
        return embed_ratios(*case, mut=mut)
    return head_ratios(*case, with_bias=True, accumulate=True, mut=mut)


def _family_cases(family):
    if family in ("ln_fwd", "ln_bwd"):
        return [(rows, D) for rows, D in LN_BWD_CASES if D == 256 or rows <= 5]
    return EMBED_CASES if family == "embed" else ROWK_HEAD_CASES


@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_mutation_is_caught(mut):
    """The defect, built into the emulation, leaves the bound of the named STORED output on the named case (and is
    invisible on the cases listed as blind to it: the reason the catching case exists)."""
    family, must, blind = MUTATIONS[mut]
    stored = lambda r: {k: v for k, v in r.items() if k not in ("dx", "Y", "out", "dpre")}  # fp32 values before a bf16 store
    caught = {}
    for case in _family_cases(family):
        r = stored(_mutated(family, case, mut))
        hit = {k: v for k, v in r.items() if v > 1.0}
        if hit:
            caught[case] = hit
            print(f"mutation {mut} caught on {case}: " + " ".join(f"{k} {v:.3g}" for k, v in hit.items()))
    for case, output in must:
        assert case in caught and output in caught[case], (mut, case, output, caught)
    for case in blind:
        assert case not in caught, (mut, case, caught[case])
