"""Transformer kernels (layernorm.hip, attention.hip) and autograd blocks
(ops/transformer.py) vs plain torch fp32 references of the same ops."""
import math

import pytest
import torch
import torch.nn.functional as F

from ml_trainer_amd.ops._ext import require_native

pytestmark = pytest.mark.gpu


def _bf(shape, g, scale=1.0, dev="cuda"):
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16).to(dev)


def _close(a, b, tol):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item() + 1e-6
    assert err <= tol * ref, f"max abs err {err:.4g} vs ref max {ref:.4g} (tol {tol})"


# ---------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("D", [256, 512, 768, 1024])
@pytest.mark.parametrize("rows", [1, 37, 1024])
def test_layernorm_fwd_bwd(dev, D, rows):
    C = require_native()
    g = torch.Generator().manual_seed(D + rows)
    x = _bf((rows, D), g, 2.0) + 0.5
    gamma = (torch.randn(D, generator=g) * 0.2 + 1).to(dev)
    beta = (torch.randn(D, generator=g) * 0.1).to(dev)
    y = torch.empty_like(x)
    mean = torch.empty(rows, device=dev)
    rstd = torch.empty(rows, device=dev)
    C.ln_fwd(x, gamma, beta, y, mean, rstd, 1e-5)
    xr = x.float().requires_grad_()
    gr, br = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    yr = F.layer_norm(xr, (D,), gr, br, 1e-5)
    _close(y, yr, 1e-2)
    torch.testing.assert_close(mean, xr.detach().mean(1), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(rstd, torch.rsqrt(xr.detach().double().var(1, unbiased=False) + 1e-5).float(),
                               rtol=1e-4, atol=1e-4)
    dy = _bf((rows, D), g)
    yr.backward(dy.float())
    dx = torch.empty_like(x)
    part = torch.empty(C.ln_partial_blocks(rows) * 2 * D, device=dev)
    dg = torch.empty(D, device=dev)
    db = torch.empty(D, device=dev)
    C.ln_bwd(dy, x, gamma, mean, rstd, dx, part, dg, db, False, None)
    _close(dx, xr.grad, 1.5e-2)
    _close(dg, gr.grad, 2e-3)
    _close(db, br.grad, 2e-3)
    # residual-gradient fusion + accumulate + fused column sums of dx
    dres = _bf((rows, D), g)
    dg2, db2 = dg.clone(), db.clone()
    part3 = torch.empty(C.ln_partial_blocks(rows) * 3 * D, device=dev)
    dxs = torch.ones(D, device=dev)
    C.ln_bwd(dy, x, gamma, mean, rstd, dx, part3, dg2, db2, True, dres, dxsum=dxs, dxsum_acc=True)
    _close(dx, xr.grad + dres.float(), 1.5e-2)
    _close(dg2, 2 * gr.grad, 2e-3)
    _close(db2, 2 * br.grad, 2e-3)
    torch.testing.assert_close(dxs, 1 + dx.float().sum(0), rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("M,N", [(1, 8), (37, 768), (8192, 2304), (1000, 3072), (300, 520)])
def test_colsum(dev, M, N):
    C = require_native()
    g = torch.Generator().manual_seed(M + N)
    X = _bf((M, N), g)
    out = torch.empty(N, device=dev)
    C.colsum(X, out)
    torch.testing.assert_close(out, X.float().sum(0), rtol=1e-4, atol=1e-3)
    C.colsum(X, out, accumulate=True)
    torch.testing.assert_close(out, 2 * X.float().sum(0), rtol=1e-4, atol=2e-3)
    # strided view (row stride != N)
    W = _bf((M, N + 16), g)[:, 8:N + 8]
    C.colsum(W, out)
    torch.testing.assert_close(out, W.float().sum(0), rtol=1e-4, atol=1e-3)


# ---------------------------------------------------------------- embeddings
@pytest.mark.parametrize("with_tt", [False, True])
def test_embeddings(dev, with_tt):
    C = require_native()
    g = torch.Generator().manual_seed(3)
    V, P, D, B, S = 500, 128, 256, 3, 96
    ww, wp, wt = _bf((V, D), g), _bf((P, D), g), _bf((2, D), g)
    ids = torch.randint(0, V, (B, S), generator=g).to(dev)
    ids[0, :10] = 7  # repeated ids exercise the scatter-add
    tt = torch.randint(0, 2, (B, S), generator=g).to(dev) if with_tt else None
    out = torch.empty(B * S, D, dtype=torch.bfloat16, device=dev)
    C.embed_fwd(ids.view(-1), tt.view(-1) if tt is not None else None, ww, wp, wt, out, S)
    t = tt if tt is not None else torch.zeros_like(ids)
    ref = ww.float()[ids] + wp.float()[torch.arange(S, device=dev)][None] + wt.float()[t]
    _close(out.view(B, S, D), ref, 1e-2)
    dout = _bf((B * S, D), g)
    gw, gp, gt = (torch.zeros(V, D, device=dev), torch.zeros(P, D, device=dev), torch.zeros(2, D, device=dev))
    part = torch.empty(S * 2 * D, device=dev)
    sid, perm = torch.sort(ids.view(-1), stable=True)
    gw.fill_(0.5)  # the kernels accumulate into existing gradients
    gp.fill_(0.25)
    C.embed_bwd(sid, perm, tt.view(-1) if tt is not None else None, dout, gw, gp, gt, part, S)
    gw -= 0.5
    gp -= 0.25
    # no atomics: repeated runs give the same bits
    runs = []
    for _ in range(2):
        r = (torch.zeros_like(gw), torch.zeros_like(gp), torch.zeros_like(gt))
        C.embed_bwd(sid, perm, tt.view(-1) if tt is not None else None, dout, *r, part, S)
        runs.append(r)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    d = dout.float().view(B, S, D)
    rgw = torch.zeros(V, D, device=dev).index_add_(0, ids.view(-1), d.view(-1, D))
    rgp = torch.zeros(P, D, device=dev)
    rgp[:S] = d.sum(0)
    rgt = torch.zeros(2, D, device=dev).index_add_(0, t.view(-1), d.view(-1, D))
    _close(gw, rgw, 1e-4)
    _close(gp, rgp, 1e-4)
    _close(gt, rgt, 1e-4)


# ---------------------------------------------------------------- attention
def _attn_ref(qkv, B, S, H, lens, scale):
    q, k, v = qkv.float().view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * scale
    if lens is not None:
        mask = torch.arange(S, device=qkv.device)[None, :] < lens[:, None]
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    return (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B * S, H * 64)


@pytest.mark.parametrize("B,S,H,use_lens", [(2, 64, 1, False), (2, 128, 2, False), (3, 200, 2, True),
                                            (1, 512, 4, False), (2, 256, 3, True)])
def test_attention(dev, B, S, H, use_lens):
    C = require_native()
    g = torch.Generator().manual_seed(B * 1000 + S + H)
    D = H * 64
    qkv = _bf((B * S, 3 * D), g, 1.0)
    lens = None
    if use_lens:
        lens = torch.randint(1, S + 1, (B,), generator=g).to(torch.int32)
        lens[0] = S
        lens = lens.to(dev)
    scale = 1.0 / math.sqrt(64)
    out = torch.empty(B * S, D, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(B * H * S, device=dev)
    C.attn_fwd(qkv, out, lse, lens, B, S, H, scale)
    qr = qkv.float().requires_grad_()
    ref = _attn_ref(qr, B, S, H, lens, scale)
    _close(out, ref, 2e-2)
    # base-2 log-sum-exp of the scaled scores
    q, k, _ = qkv.float().view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * scale
    if lens is not None:
        mask = torch.arange(S, device=dev)[None, :] < lens[:, None]
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    torch.testing.assert_close(lse.view(B, H, S), torch.logsumexp(s, -1) / math.log(2), rtol=1e-3, atol=1e-3)
    dout = _bf((B * S, D), g)
    ref.backward(dout.float())
    dqkv = torch.full_like(qkv, float("nan"))
    delta = torch.empty(B * S * H, device=dev)
    C.attn_bwd(qkv, out, dout, lse, delta, lens, dqkv, B, S, H, scale)
    assert torch.isfinite(dqkv.float()).all()
    gr = qr.grad.view(B * S, 3, D)
    dg = dqkv.view(B * S, 3, D)
    for j, name in enumerate("qkv"):
        err = (dg[:, j].float() - gr[:, j]).abs().max().item()
        ref_max = gr[:, j].abs().max().item() + 1e-6
        assert err <= 3e-2 * ref_max, f"d{name}: {err:.4g} vs {ref_max:.4g}"


# ---------------------------------------------------------------- blocks
def test_attention_block_and_ffn_block(dev):
    from ml_trainer_amd.ops import transformer as T
    torch.manual_seed(0)
    B, S, H = 2, 128, 4
    D, Fh = H * 64, 1024
    x = (torch.randn(B * S, D, device=dev) * 0.5).to(torch.bfloat16)
    wqkv = (torch.randn(3 * D, D, device=dev) * 0.05).requires_grad_()
    bqkv = (torch.randn(3 * D, device=dev) * 0.05).requires_grad_()
    wo = (torch.randn(D, D, device=dev) * 0.05).requires_grad_()
    bo = (torch.randn(D, device=dev) * 0.05).requires_grad_()
    xa = x.clone().requires_grad_()
    y = T.attention_block(xa, wqkv, bqkv, wo, bo, None, B, S, H)
    # fp32 reference on the bf16-rounded weights the kernels consume
    wq_r, wo_r = wqkv.detach().bfloat16().float().requires_grad_(), wo.detach().bfloat16().float().requires_grad_()
    bq_r, bo_r = bqkv.detach().clone().requires_grad_(), bo.detach().clone().requires_grad_()
    xr = x.float().requires_grad_()
    qkv = xr @ wq_r.t() + bq_r
    ctx = _attn_ref(qkv, B, S, H, None, 0.125)
    yr = ctx @ wo_r.t() + bo_r + xr
    _close(y, yr, 2e-2)
    dy = (torch.randn(B * S, D, device=dev)).to(torch.bfloat16)
    y.backward(dy)
    yr.backward(dy.float())
    _close(xa.grad, xr.grad, 3e-2)
    _close(wqkv.grad, wq_r.grad, 3e-2)
    _close(bqkv.grad, bq_r.grad, 3e-2)
    _close(wo.grad, wo_r.grad, 2e-2)
    _close(bo.grad, bo_r.grad, 1e-2)

    w1 = (torch.randn(Fh, D, device=dev) * 0.05).requires_grad_()
    b1 = (torch.randn(Fh, device=dev) * 0.05).requires_grad_()
    w2 = (torch.randn(D, Fh, device=dev) * 0.05).requires_grad_()
    b2 = (torch.randn(D, device=dev) * 0.05).requires_grad_()
    xf = x.clone().requires_grad_()
    yf = T.ffn_block(xf, w1, b1, w2, b2)
    w1r, w2r = w1.detach().bfloat16().float().requires_grad_(), w2.detach().bfloat16().float().requires_grad_()
    b1r, b2r = b1.detach().clone().requires_grad_(), b2.detach().clone().requires_grad_()
    xfr = x.float().requires_grad_()
    yfr = F.gelu(xfr @ w1r.t() + b1r) @ w2r.t() + b2r + xfr
    _close(yf, yfr, 2e-2)
    yf.backward(dy)
    yfr.backward(dy.float())
    _close(xf.grad, xfr.grad, 3e-2)
    _close(w1.grad, w1r.grad, 3e-2)
    _close(b1.grad, b1r.grad, 3e-2)
    _close(w2.grad, w2r.grad, 2e-2)
    _close(b2.grad, b2r.grad, 1e-2)


def _grads(m, fn, ids, mask, y):
    m.zero_grad(set_to_none=True)
    F.cross_entropy(fn(ids, mask).float(), y).backward()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("use_mask", [False, True])
def test_bert_tiny_matches_reference(dev, use_mask):
    """Native bf16 gradients vs the fp32 reference, error-budgeted against PyTorch's own bf16
    autocast path (same weights): the native error may not exceed 2x autocast's (+ floor)."""
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    torch.manual_seed(0)
    m = BertClassifier(bert_config("bert-tiny")).to(dev)
    ids = torch.randint(5, 1000, (2, 128), device=dev)
    mask = torch.ones(2, 128, dtype=torch.long, device=dev)
    if use_mask:
        mask[1, 100:] = 0
    y = torch.tensor([0, 1], device=dev)
    out = m(ids, mask)
    ref = m.forward_reference(ids, mask)
    _close(out, ref, 5e-2)
    gn = _grads(m, m, ids, mask, y)
    gr = _grads(m, m.forward_reference, ids, mask, y)
    ga = _grads(m, m.forward_torch_bf16, ids, mask, y)
    for n in gr:
        nr = gr[n].norm().item()
        if nr < 1e-8:
            continue
        e_nat = (gn[n] - gr[n]).norm().item() / nr
        e_ac = (ga[n] - gr[n]).norm().item() / nr
        assert e_nat <= max(2.0 * e_ac, 0.02), f"{n}: native rel err {e_nat:.4f} vs autocast {e_ac:.4f}"


def test_fused_ln_blocks_match_unfused(dev):
    from ml_trainer_amd.ops import transformer as T
    torch.manual_seed(1)
    B, S, H = 2, 128, 4
    D = H * 64
    x = (torch.randn(B * S, D, device=dev)).to(torch.bfloat16)
    ps = [(torch.randn(3 * D, D, device=dev) * 0.05), torch.randn(3 * D, device=dev) * 0.05,
          torch.randn(D, D, device=dev) * 0.05, torch.randn(D, device=dev) * 0.05,
          1 + 0.1 * torch.randn(D, device=dev), 0.1 * torch.randn(D, device=dev)]
    dy = torch.randn(B * S, D, device=dev).to(torch.bfloat16)

    def run(fused):
        xs = x.clone().requires_grad_()
        qs = [p.clone().requires_grad_() for p in ps]
        if fused:
            y = T.attention_ln_block(xs, *qs[:4], qs[4], qs[5], None, B, S, H, 1e-12)
        else:
            y = T.layer_norm(T.attention_block(xs, *qs[:4], None, B, S, H), qs[4], qs[5], 1e-12)
        y.backward(dy)
        return [y, xs.grad] + [q.grad for q in qs]

    for a, b in zip(run(True), run(False)):
        torch.testing.assert_close(a.float(), b.float(), rtol=1e-2, atol=1e-2)


def test_bert_tiny_trains(dev):
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    from ml_trainer_amd.ops.optim import FusedAdamW
    from ml_trainer_amd.utils.flat import FlatParams
    torch.manual_seed(0)
    m = BertClassifier(bert_config("bert-tiny")).to(dev)
    opt = FusedAdamW(m.parameters(), lr=3e-4, weight_decay=0.01)
    assert FlatParams.owner(m.layers[0].qkv.weight) is not None
    ids = torch.randint(5, 1000, (8, 128), device=dev)
    y = torch.randint(0, 2, (8,), device=dev)
    ids[y == 1, 5] = 3  # learnable marker
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = F.cross_entropy(m(ids), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < 0.5 * losses[0], losses


def test_direct_flat_gradients_match_returned(dev):
    """Fused backwards accumulate straight into FlatParams gradients (no AccumulateGrad); the
    result must equal the returned-gradient path, accumulate across two backwards, and notify."""
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    from ml_trainer_amd.utils.flat import FlatParams
    torch.manual_seed(0)
    m1 = BertClassifier(bert_config("bert-tiny")).to(dev)
    m2 = BertClassifier(bert_config("bert-tiny")).to(dev)
    m2.load_state_dict(m1.state_dict())
    fp = FlatParams(m2.parameters())
    seen = []
    fp.grad_ready_hooks.append(lambda p: seen.append(id(p)))
    ids = torch.randint(5, 1000, (2, 128), device=dev)
    y = torch.tensor([0, 1], device=dev)
    F.cross_entropy(m1(ids), y).backward()
    fp.zero_grad()
    for _ in range(2):
        F.cross_entropy(m2(ids), y).backward()
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        torch.testing.assert_close(p2.grad, 2 * p1.grad, rtol=1e-3, atol=1e-5, msg=n)
    direct = {id(p) for n, p in m2.named_parameters() if not n.startswith(("pooler", "classifier"))}
    assert direct <= set(seen)


@pytest.mark.parametrize("B,S,H,use_lens", [(2, 512, 3, False), (3, 200, 2, True), (2, 64, 1, False),
                                            (2, 17, 1, True), (3, 65, 1, True), (2, 192, 2, True), (2, 320, 1, False)])
def test_attention_bwd_ring_matches_register_staged(dev, B, S, H, use_lens, monkeypatch):
    """The glds ring-staged backward kernels (MLT_ATTN_RING) compute the same products in the
    same order as the register-staged ones: bit-identical dQKV, including tails and masks."""
    C = require_native()
    g = torch.Generator().manual_seed(S + H)
    D = H * 64
    qkv = _bf((B * S, 3 * D), g, 1.0)
    lens = None
    if use_lens:
        lens = torch.randint(1, S + 1, (B,), generator=g).to(torch.int32).to(dev)
    scale = 0.125
    out = torch.empty(B * S, D, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(B * H * S, device=dev)
    C.attn_fwd(qkv, out, lse, lens, B, S, H, scale)
    dout = _bf((B * S, D), g)
    res = {}
    for ring in ("0", "4"):
        monkeypatch.setenv("MLT_ATTN_RING", ring)
        for grp in ("1", "2"):
            monkeypatch.setenv("MLT_ATTN_DKDV_GROUPS", grp)
            monkeypatch.setenv("MLT_ATTN_DQ_GROUPS", grp)
            dqkv = torch.full_like(qkv, float("nan"))
            delta = torch.empty(B * S * H, device=dev)
            C.attn_bwd(qkv, out, dout, lse, delta, lens, dqkv, B, S, H, scale)
            res[ring, grp] = dqkv
    for grp in ("1", "2"):
        assert torch.equal(res["0", grp], res["4", grp])


def test_attention_bwd_rejects_unknown_ring_value(dev, monkeypatch):
    """MLT_ATTN_RING takes 4 (or unset: the ring kernels) and 0 (the register-staged oracle). Any
    other value, the retired depth 3 included, is an error raised before any launch: the
    NaN-prefilled dQKV is untouched."""
    C = require_native()
    B, S, H = 1, 64, 1
    g = torch.Generator().manual_seed(5)
    qkv = _bf((B * S, 3 * H * 64), g, 1.0)
    out = torch.empty(B * S, H * 64, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(B * H * S, device=dev)
    C.attn_fwd(qkv, out, lse, None, B, S, H, 0.125)
    dout = _bf((B * S, H * 64), g)
    dqkv = torch.full_like(qkv, float("nan"))
    delta = torch.empty(B * S * H, device=dev)
    monkeypatch.setenv("MLT_ATTN_RING", "3")
    with pytest.raises(RuntimeError, match="MLT_ATTN_RING"):
        C.attn_bwd(qkv, out, dout, lse, delta, None, dqkv, B, S, H, 0.125)
    torch.cuda.synchronize()
    assert torch.isnan(dqkv).all().item()


@pytest.mark.parametrize("B,S,H,use_lens", [(2, 512, 3, False), (3, 200, 2, True), (2, 512, 2, True)])
def test_attention_bwd_fused_bias_colsum(dev, B, S, H, use_lens, monkeypatch):
    """QKV bias gradient (column sums of dQKV) from the ring backward kernels' block partials
    (incl. fully masked key blocks and tails), and the plain fallback for the register-staged
    kernels: both match the column sums of the dQKV they wrote; set and accumulate."""
    C = require_native()
    g = torch.Generator().manual_seed(S * 3 + H)
    D = H * 64
    qkv = _bf((B * S, 3 * D), g, 1.0)
    lens = None
    if use_lens:
        lens = torch.tensor([7, S, 130][:B], dtype=torch.int32).to(dev)  # 7: most key blocks fully masked
    scale = 0.125
    out = torch.empty(B * S, D, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(B * H * S, device=dev)
    C.attn_fwd(qkv, out, lse, lens, B, S, H, scale)
    dout = _bf((B * S, D), g)
    for ring in ("0", "4"):
        monkeypatch.setenv("MLT_ATTN_RING", ring)
        for grp in ("1", "2"):
            monkeypatch.setenv("MLT_ATTN_DKDV_GROUPS", grp)
            monkeypatch.setenv("MLT_ATTN_DQ_GROUPS", grp)
            dqkv = torch.empty_like(qkv)
            delta = torch.empty(B * S * H, device=dev)
            cs = torch.full((3 * D,), 2.0, device=dev)
            C.attn_bwd(qkv, out, dout, lse, delta, lens, dqkv, B, S, H, scale, colsum_out=cs)
            ref = dqkv.float().sum(0)
            tol = 1e-2 * dqkv.float().abs().sum(0).max().item()
            torch.testing.assert_close(cs, ref, rtol=1e-2, atol=tol)
            C.attn_bwd(qkv, out, dout, lse, delta, lens, dqkv, B, S, H, scale, colsum_out=cs,
                       colsum_accumulate=True)
            torch.testing.assert_close(cs, 2 * ref, rtol=1e-2, atol=2 * tol)


@pytest.mark.parametrize("jump", [4.0, 300.0])
@pytest.mark.parametrize("use_lens", [False, True])
def test_attention_fwd_defer_max_branches(dev, jump, use_lens):
    """The forward's defer-max rescale (T13) is data dependent: one key row per head is made a
    multiple of one query row inside a LATE key block, so that query's running max jumps there --
    by ~4 (base 2: stays deferred, p up to 2^4 enters O unrescaled) or by ~50 (forces the rescale
    of O and l mid-sequence). Full-tensor fp64 reference, every query and head checked."""
    C = require_native()
    B, S, H = 2, 512, 2
    D = H * 64
    g = torch.Generator().manual_seed(11)
    qkv = (torch.randn(B * S, 3 * D, generator=g) * 0.5)
    x = qkv.view(B, S, 3, H, 64)
    qi, kj = 37, 5 * 64 + 9  # query 37 of block 0; key in block 5 of 8
    for b in range(B):
        for h in range(H):
            q = x[b, qi, 0, h]
            x[b, kj, 1, h] = q * (jump / (q.double().pow(2).sum().item() * 0.125 * 1.4426950408889634))
    qkv = qkv.to(torch.bfloat16).to(dev)
    lens = torch.tensor([S, 400], dtype=torch.int32, device=dev) if use_lens else None
    out = torch.empty(B * S, D, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(B * H * S, device=dev)
    C.attn_fwd(qkv, out, lse, lens, B, S, H, 0.125)
    q, k, v = qkv.double().view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * 0.125
    if lens is not None:
        mask = torch.arange(S, device=dev)[None, :] < lens[:, None]
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    ref = (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B * S, D)
    err = (out.double() - ref).abs().max().item()
    assert err <= 2e-2 * max(1.0, ref.abs().max().item()), err
    row = out.view(B, S, H, 64)[:, qi].double()
    assert (row - ref.view(B, S, H, 64)[:, qi]).abs().max().item() <= 2e-2
    torch.testing.assert_close(lse.view(B, H, S).double(), torch.logsumexp(s, -1) / math.log(2), rtol=1e-3,
                               atol=2e-3)


def test_classifier_head_native_matches_torch(dev):
    """Pooler GEMM (tanh epilogue) + head.hip classifier layer and backward vs fp32 torch on the
    same bf16 CLS rows (a strided row view, as in the model)."""
    from ml_trainer_amd.ops import transformer as T
    torch.manual_seed(3)
    B, S, h, L = 24, 8, 256, 3
    x = torch.randn(B * S, h, device=dev).to(torch.bfloat16)
    cls = x.view(B, S, h)[:, 0]
    wp = (torch.randn(h, h, device=dev) * 0.05).requires_grad_()
    bp = (torch.randn(h, device=dev) * 0.1).requires_grad_()
    wc = (torch.randn(L, h, device=dev) * 0.05).requires_grad_()
    bc = (torch.randn(L, device=dev) * 0.1).requires_grad_()
    y = torch.randint(0, L, (B,), device=dev)
    logits = T.classifier_head(cls, wp, bp, wc, bc)
    torch.nn.functional.cross_entropy(logits, y).backward()
    grads = [p.grad.clone() for p in (wp, bp, wc, bc)]
    cr = cls.float().clone().requires_grad_()
    wpr, bpr, wcr, bcr = [p.detach().clone().requires_grad_() for p in (wp, bp, wc, bc)]
    ref = torch.tanh(cr @ wpr.to(torch.bfloat16).float().t() + bpr) @ wcr.t() + bcr
    torch.nn.functional.cross_entropy(ref, y).backward()
    torch.testing.assert_close(logits, ref, rtol=2e-3, atol=2e-3)
    for g, r in zip(grads, (wpr.grad, bpr.grad, wcr.grad, bcr.grad)):
        torch.testing.assert_close(g, r, rtol=3e-2, atol=3e-3)


@pytest.mark.parametrize("with_aux", [False, True])
def test_dgrad_transposed_weight_matches_n_contiguous(dev, monkeypatch, with_aux):
    """Large-token dgrads use a cached k-contiguous W^T copy (MLT_DGRAD_WT, default on); the
    result must match the n-contiguous-B GEMM on the same operands, with and without the dGELU
    epilogue and the residual, and the cache must follow an optimizer update of the weight."""
    from ml_trainer_amd.ops import transformer as T
    from ml_trainer_amd.utils.flat import FlatParams
    torch.manual_seed(4)
    rows, n_out, k_in = 4096, 256, 192
    lin = torch.nn.Linear(k_in, n_out).to(dev)
    fp = FlatParams(lin.parameters())
    dy = torch.randn(rows, n_out, device=dev).to(torch.bfloat16)
    res = torch.randn(rows, k_in, device=dev).to(torch.bfloat16)
    aux = torch.randn(rows, k_in, device=dev).to(torch.bfloat16) if with_aux else None
    outs = {}
    for wt in ("1", "0"):
        monkeypatch.setenv("MLT_DGRAD_WT", wt)
        out = torch.empty(rows, k_in, dtype=torch.bfloat16, device=dev)
        outs[wt] = T.BF16.dgrad(dy, lin.weight, out, aux=aux, res=res).clone()
    torch.testing.assert_close(outs["1"].float(), outs["0"].float(), rtol=1e-2, atol=1e-2)
    # a manual edit of the fp32 masters (version bump, no optimizer generation) -> rebuilt copy
    with torch.no_grad():
        fp.data.mul_(-1.0)
    monkeypatch.setenv("MLT_DGRAD_WT", "1")
    out = torch.empty(rows, k_in, dtype=torch.bfloat16, device=dev)
    T.BF16.dgrad(dy, lin.weight, out, aux=aux, res=res)
    monkeypatch.setenv("MLT_DGRAD_WT", "0")
    ref = torch.empty(rows, k_in, dtype=torch.bfloat16, device=dev)
    T.BF16.dgrad(dy, lin.weight, ref, aux=aux, res=res)
    torch.testing.assert_close(out.float(), ref.float(), rtol=1e-2, atol=1e-2)


@pytest.mark.parametrize("R,C,off", [(768, 2304, 0), (3072, 768, 4), (100, 37, 0), (64, 64, 4), (130, 200, 0)])
def test_transpose_bf16(dev, R, C, off):
    """transpose.hip vs torch, incl. edge tiles and an only-8-byte-aligned source view."""
    C_ = require_native()
    buf = torch.randn(R * C + off, device=dev).to(torch.bfloat16)
    src = buf[off:off + R * C].view(R, C)
    dst = torch.full((C, R), float("nan"), dtype=torch.bfloat16, device=dev)
    C_.transpose_bf16(src, dst)
    assert torch.equal(dst, src.t())
