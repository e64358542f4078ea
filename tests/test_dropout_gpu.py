"""Hidden dropout on the GPU: dropout.hip and the dropout variants of the LayerNorm kernels
(layernorm.hip) against the torch Philox oracle (ops/dropout.py), bit for bit where the result is
defined exactly, and the BERT model with dropout against its torch paths with the same masks."""
import pytest
import torch
import torch.nn.functional as F

from ml_trainer_amd.ops import dropout as D
from ml_trainer_amd.ops._ext import require_native

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC_DEF  # both key words non-zero
PS = [0.1, 0.5]  # 0.5: the scale is exactly 2


def _close(a, b, tol):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item() + 1e-6
    assert err <= tol * ref, f"max abs err {err:.4g} vs ref max {ref:.4g} (tol {tol})"


def _away_from_zero(shape, g, dev):
    """bf16 with |x| in [0.5, 2): a zero output can only mean "dropped"."""
    mag = 0.5 + 1.49 * torch.rand(*shape, generator=g)
    sign = torch.where(torch.rand(*shape, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).to(torch.bfloat16).to(dev)


def _scaled(x, p):
    return (x.float() * D.scale(p)).to(torch.bfloat16)


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------- dropout.hip
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("rows,Dm", [(1, 256), (37, 768), (5, 1024)])
def test_dropout_kernel(dev, rows, Dm, p):
    C = require_native()
    g = torch.Generator().manual_seed(rows + Dm)
    x = _away_from_zero((rows, Dm), g, dev)
    out = torch.full_like(x, float("nan"))
    C.dropout(x, out, p, SEED, 3, 1)
    keep = D.keep_mask(SEED, 3, 1, rows, Dm, p, dev)
    assert torch.equal(out == 0, ~keep)
    assert torch.equal(_bits(out), _bits(torch.where(keep, _scaled(x, p), torch.zeros_like(x))))
    again = torch.empty_like(x)
    C.dropout(x, again, p, SEED, 3, 1)
    assert torch.equal(_bits(again), _bits(out))
    C.dropout(x, again, p, SEED, 4, 1)  # another site: another mask
    assert not torch.equal(again == 0, out == 0)


def test_dropout_kernel_checks(dev):
    C = require_native()
    x = torch.ones(3, 4, dtype=torch.bfloat16, device=dev)  # 12 elements
    with pytest.raises(RuntimeError):
        C.dropout(x, torch.empty_like(x), 0.1, SEED, 0, 0)
    x = torch.ones(2, 8, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError):
        C.dropout(x, torch.empty_like(x), 1.0, SEED, 0, 0)
    out = torch.empty_like(x)
    C.dropout(x, out, 0.0, SEED, 0, 0)  # p = 0 keeps everything, scale 1
    assert torch.equal(out, x)


def test_dropout_autograd(dev):
    from ml_trainer_amd.ops import transformer as T
    g = torch.Generator().manual_seed(5)
    x = _away_from_zero((37, 256), g, dev).requires_grad_()
    dy = _away_from_zero((37, 256), g, dev)
    y = T.dropout(x, 0.1, SEED, 0, 0)
    y.backward(dy)
    keep = D.keep_mask(SEED, 0, 0, 37, 256, 0.1, dev)
    assert torch.equal(_bits(y.detach()), _bits(D.apply(x.detach(), 0.1, SEED, 0, 0)))
    assert torch.equal(_bits(x.grad), _bits(torch.where(keep, _scaled(dy, 0.1), torch.zeros_like(dy))))


# ---------------------------------------------------------------- LayerNorm kernels
LN_SHAPES = [(rows, Dm) for Dm in (256, 512, 768, 1024) for rows in (1, 37, 2085)]
# 37 rows leave a partial block; 2085 rows exceed the backward's 512-block x 4-row grid, so its
# waves walk two rows and the software pipeline's clamped fetch runs


def _gamma_beta(Dm, g, dev):
    return (torch.randn(Dm, generator=g) * 0.2 + 1).to(dev), (torch.randn(Dm, generator=g) * 0.1).to(dev)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("rows,Dm", LN_SHAPES)
def test_dropout_add_ln_fwd(dev, rows, Dm, p):
    C = require_native()
    g = torch.Generator().manual_seed(rows * 7 + Dm)
    y0 = _away_from_zero((rows, Dm), g, dev)
    gamma, beta = _gamma_beta(Dm, g, dev)
    keep = D.keep_mask(SEED, 5, 2, rows, Dm, p, dev)

    def run(res):
        z, y = torch.full_like(y0, float("nan")), torch.full_like(y0, float("nan"))
        mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
        C.dropout_add_ln_fwd(y0, res, gamma, beta, z, y, mean, rstd, 1e-5, p, SEED, 5, 2)
        # Y / mean / rstd: bitwise the plain LayerNorm kernel on the kernel's own Z
        y2, mean2, rstd2 = torch.empty_like(y0), torch.empty(rows, device=dev), torch.empty(rows, device=dev)
        C.ln_fwd(z, gamma, beta, y2, mean2, rstd2, 1e-5)
        assert torch.equal(_bits(y), _bits(y2))
        assert torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
        return z

    z = run(torch.zeros_like(y0))
    assert torch.equal(z == 0, ~keep)
    assert torch.equal(_bits(z), _bits(torch.where(keep, _scaled(y0, p), torch.zeros_like(y0))))
    res = (torch.randn(rows, Dm, generator=g)).to(torch.bfloat16).to(dev)
    z = run(res)
    _close(z, torch.where(keep, y0.float() * D.scale(p), torch.zeros((), device=dev)) + res.float(), 1e-2)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("rows,Dm", LN_SHAPES)
def test_ln_bwd_dropout(dev, rows, Dm, p):
    C = require_native()
    g = torch.Generator().manual_seed(rows * 11 + Dm)
    x = (torch.randn(rows, Dm, generator=g) * 2.0).to(torch.bfloat16).to(dev) + 0.5
    gamma, beta = _gamma_beta(Dm, g, dev)
    y, mean, rstd = torch.empty_like(x), torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    C.ln_fwd(x, gamma, beta, y, mean, rstd, 1e-5)
    dy = torch.randn(rows, Dm, generator=g).to(torch.bfloat16).to(dev)
    nb = C.ln_partial_blocks(rows)
    # today's kernel on the same inputs
    dx0 = torch.empty_like(x)
    dg0, db0, dxs0 = torch.empty(Dm, device=dev), torch.empty(Dm, device=dev), torch.empty(Dm, device=dev)
    C.ln_bwd(dy, x, gamma, mean, rstd, dx0, torch.empty(nb * 3 * Dm, device=dev), dg0, db0, False, None, dxsum=dxs0)
    # fp32 torch reference of dgamma / dbeta
    xr = x.float().requires_grad_()
    gr, br = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    F.layer_norm(xr, (Dm,), gr, br, 1e-5).backward(dy.float())

    keep = D.keep_mask(SEED, 6, 0, rows, Dm, p, dev)
    dx, dxm = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    dg, db, dxs = torch.empty(Dm, device=dev), torch.empty(Dm, device=dev), torch.empty(Dm, device=dev)
    part = torch.empty(nb * 3 * Dm, device=dev)
    C.ln_bwd(dy, x, gamma, mean, rstd, dx, part, dg, db, False, None, dxsum=dxs, dxm=dxm, p=p, seed=SEED, site=6,
             rank=0)
    assert torch.equal(_bits(dx), _bits(dx0))
    _close(dg, gr.grad, 2e-3)
    _close(db, br.grad, 2e-3)
    want = torch.where(keep, _scaled(dx, p), torch.zeros_like(dx))
    assert torch.equal(_bits(dxm), _bits(want))
    torch.testing.assert_close(dxs, dxm.float().sum(0), rtol=1e-4, atol=1e-3)
    # accumulate forms: dgamma / dbeta and the column sums add to what is there
    dg2, db2, dxs2 = dg.clone(), db.clone(), torch.ones(Dm, device=dev)
    dxm2 = torch.empty_like(x)
    C.ln_bwd(dy, x, gamma, mean, rstd, dx, part, dg2, db2, True, None, dxsum=dxs2, dxsum_acc=True, dxm=dxm2, p=p,
             seed=SEED, site=6, rank=0)
    assert torch.equal(_bits(dxm2), _bits(dxm))
    _close(dg2, 2 * gr.grad, 2e-3)
    _close(db2, 2 * br.grad, 2e-3)
    torch.testing.assert_close(dxs2, 1 + dxm.float().sum(0), rtol=1e-4, atol=1e-3)


def test_ln_bwd_dropout_checks(dev):
    C = require_native()
    x = torch.randn(8, 256, device=dev).to(torch.bfloat16)
    gamma = torch.ones(256, device=dev)
    v = torch.zeros(8, device=dev)
    o = torch.empty(256, device=dev)
    part = torch.empty(C.ln_partial_blocks(8) * 3 * 256, device=dev)
    with pytest.raises(RuntimeError):  # the column sums are part of the variant
        C.ln_bwd(x, x, gamma, v, v + 1, torch.empty_like(x), part, o, o.clone(), False, None,
                 dxm=torch.empty_like(x), p=0.1, seed=1, site=0, rank=0)
    with pytest.raises(RuntimeError):  # and a residual gradient is not
        C.ln_bwd(x, x, gamma, v, v + 1, torch.empty_like(x), part, o, o.clone(), False, x, dxsum=o.clone(),
                 dxm=torch.empty_like(x), p=0.1, seed=1, site=0, rank=0)


# ---------------------------------------------------------------- model
def _grads(m, fn, ids, mask, y, **kw):
    m.zero_grad(set_to_none=True)
    F.cross_entropy(fn(ids, mask, **kw).float(), y).backward()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("use_mask", [False, True])
def test_bert_tiny_dropout_matches_reference(dev, use_mask):
    """The rule of test_bert_tiny_matches_reference with hidden dropout 0.1 and one seed given to
    all three paths (identical masks): native gradient error vs the fp32 reference at most
    max(2 x autocast's error, 0.02) per parameter."""
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    torch.manual_seed(0)
    m = BertClassifier(bert_config("bert-tiny", hidden_dropout=0.1)).to(dev)
    m.train()
    ids = torch.randint(5, 1000, (2, 128), device=dev)
    mask = torch.ones(2, 128, dtype=torch.long, device=dev)
    if use_mask:
        mask[1, 100:] = 0
    y = torch.tensor([0, 1], device=dev)
    seed = 2 ** 61 + 12345
    out = m(ids, mask, dropout_seed=seed)
    ref = m.forward_reference(ids, mask, dropout_seed=seed)
    _close(out, ref, 5e-2)
    assert not torch.equal(ref, m.forward_reference(ids, mask, dropout_seed=seed + 1))
    gn = _grads(m, m, ids, mask, y, dropout_seed=seed)
    gr = _grads(m, m.forward_reference, ids, mask, y, dropout_seed=seed)
    ga = _grads(m, m.forward_torch_bf16, ids, mask, y, dropout_seed=seed)
    bad = []
    for n in gr:
        nr = gr[n].norm().item()
        if nr < 1e-8:
            continue
        e_nat = (gn[n] - gr[n]).norm().item() / nr
        e_ac = (ga[n] - gr[n]).norm().item() / nr
        print(f"{n}: native rel err {e_nat:.4f} vs autocast {e_ac:.4f}")
        if e_nat > max(2.0 * e_ac, 0.02):
            bad.append(f"{n}: native rel err {e_nat:.4f} vs autocast {e_ac:.4f}")
    assert not bad, bad


def test_bert_tiny_dropout_determinism(dev):
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    torch.manual_seed(0)
    m0 = BertClassifier(bert_config("bert-tiny")).to(dev)
    m = BertClassifier(bert_config("bert-tiny", hidden_dropout=0.1)).to(dev)
    m.load_state_dict(m0.state_dict())
    m.train()
    ids = torch.randint(5, 1000, (2, 128), device=dev)
    y = torch.tensor([0, 1], device=dev)
    g1 = _grads(m, m, ids, None, y, dropout_seed=11)
    g2 = _grads(m, m, ids, None, y, dropout_seed=11)
    g3 = _grads(m, m, ids, None, y, dropout_seed=12)
    assert all(torch.equal(g1[n], g2[n]) for n in g1)
    assert any(not torch.equal(g1[n], g3[n]) for n in g1)
    # without a seed: drawn from the default CPU generator, reproducible under manual_seed
    torch.manual_seed(3)
    a = m(ids)
    s = m.last_dropout_seed
    torch.manual_seed(3)
    assert torch.equal(m(ids), a) and m.last_dropout_seed == s
    assert not torch.equal(m(ids), a)
    m.eval()
    m0.eval()
    with torch.no_grad():
        assert torch.equal(m(ids), m0(ids))


def _fp8_dropout_run(dev, steps):
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    torch.manual_seed(0)
    m8 = BertClassifier(bert_config("bert-tiny", fp8=True, hidden_dropout=0.1)).to(dev)
    m8.train()
    ids = torch.randint(5, 1000, (4, 128), device=dev)
    y = torch.randint(0, 2, (4,), device=dev)
    for s in range(steps):  # fresh fp8 scaling state per model: the steps replay identically
        m8.zero_grad(set_to_none=True)
        o8 = m8(ids, dropout_seed=77 + s)
        F.cross_entropy(o8, y).backward()
    return m8, ids, y, o8.detach()


def test_fp8_bert_dropout_close_to_bf16(dev):
    """Thresholds of test_fp8_bert_close_to_bf16: 0.1 on the output, 0.25 per gradient."""
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    m8, ids, y, o8 = _fp8_dropout_run(dev, 1)
    m16 = BertClassifier(bert_config("bert-tiny", hidden_dropout=0.1)).to(dev)
    m16.load_state_dict(m8.state_dict())
    m16.train()
    o16 = m16(ids, dropout_seed=77)
    rel = (o8 - o16).norm() / o16.norm()
    assert rel < 0.1, rel
    F.cross_entropy(o16, y).backward()
    for (n, p8), p16 in zip(m8.named_parameters(), m16.parameters()):
        r = (p8.grad - p16.grad).norm() / (p16.grad.norm() + 1e-12)
        assert r < 0.25, (n, float(r))


def test_dropout_flat_gradients_match_returned(dev):
    """As test_direct_flat_gradients_match_returned, under dropout: with a FusedAdamW owning the
    parameters the out-projection / FFN2 bias gradients (the DXM column sums) and every other
    gradient land in the flat buffer and equal the returned-gradient run's."""
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    from ml_trainer_amd.ops.optim import FusedAdamW
    from ml_trainer_amd.utils.flat import FlatParams
    torch.manual_seed(0)
    m1 = BertClassifier(bert_config("bert-tiny", hidden_dropout=0.1)).to(dev)
    m2 = BertClassifier(bert_config("bert-tiny", hidden_dropout=0.1)).to(dev)
    m2.load_state_dict(m1.state_dict())
    opt = FusedAdamW(m2.parameters(), lr=1e-4)
    fp = FlatParams.owner(m2.layers[0].out.bias)
    assert fp is not None and FlatParams.owner(m2.layers[0].ffn2.bias) is fp
    ids = torch.randint(5, 1000, (2, 128), device=dev)
    y = torch.tensor([0, 1], device=dev)
    F.cross_entropy(m1(ids, dropout_seed=21), y).backward()
    opt.zero_grad()
    for _ in range(2):  # accumulates across two backwards
        F.cross_entropy(m2(ids, dropout_seed=21), y).backward()
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        torch.testing.assert_close(p2.grad, 2 * p1.grad, rtol=1e-3, atol=1e-5, msg=n)
    for b in (m2.layers[0].out.bias, m2.layers[1].ffn2.bias):
        assert fp.grad_sink(b) is not None and b.grad.abs().sum().item() > 0
