"""Attention-probability dropout inside the flash attention kernels (attention.hip: forward, dQ
ring, dK/dV ring) against the torch byte-mask oracle (ops/dropout.py): exact mask probes per
kernel, numerics against an fp32 reference with the same mask, and the BERT model with attention
dropout against its torch paths."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from ml_trainer_amd.ops import dropout as D
from ml_trainer_amd.ops._ext import require_native

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC_DEF  # both key words non-zero
SITE = D.ATTENTION_SITE0 + 5
RANK = 3
SCALE = 1.0 / math.sqrt(64)

# (B, S, H, lens): one block / two groups / partial 64-blocks + the FULLT = false ring / the ring
# wraps (8 stages through 4 slots) / S % 4 != 0 (partial mask tiles; the kernels take S = 70 -- the
# numerics test below holds it to the fp32 reference -- so there is no need to fall back to 72)
PROBE_SHAPES = [(1, 64, 1, None), (2, 128, 2, None), (3, 200, 2, (200, 130, 77)), (1, 512, 2, None),
                (1, 70, 1, None)]


def _drop(p):
    return dict(p=p, seed=SEED, site=SITE, rank=RANK)


@functools.lru_cache(maxsize=None)
def _keep(B, H, S, p):
    return D.attention_keep_mask(SEED, SITE, RANK, B, H, S, p, device="cuda")


def _lens(lens, dev):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)


def _valid(B, S, lens, dev):
    """bool [B, S]: key k of batch b is inside the sequence."""
    if lens is None:
        return torch.ones(B, S, dtype=torch.bool, device=dev)
    return torch.arange(S, device=dev)[None, :] < torch.tensor(lens, device=dev)[:, None]


def _fwd(C, qkv, lens, B, S, H, **kw):
    out = torch.empty(B * S, H * 64, dtype=torch.bfloat16, device=qkv.device)
    lse = torch.empty(B * H * S, device=qkv.device)
    C.attn_fwd(qkv, out, lse, lens, B, S, H, SCALE, **kw)
    return out, lse


def _bwd(C, qkv, out, dout, lse, lens, B, S, H, **kw):
    dqkv = torch.full_like(qkv, float("nan"))
    delta = torch.empty(B * S * H, device=qkv.device)
    C.attn_bwd(qkv, out, dout, lse, delta, lens, dqkv, B, S, H, SCALE, **kw)
    return dqkv


def _one_hot_rows(S, blk, dev):
    """[S, 64]: row r = e_(r - 64 blk) inside 64-row block ``blk``, 0 elsewhere."""
    t = torch.zeros(S, 64, device=dev)
    r = torch.arange(64 * blk, min(64 * blk + 64, S), device=dev)
    t[r, r - 64 * blk] = 1.0
    return t


# ---------------------------------------------------------------- exact mask probes
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,S,H,lens", PROBE_SHAPES)
def test_fwd_mask_probe(dev, B, S, H, lens, p):
    """Q = 0 (P uniform over the valid keys), V one-hot on one 64-key block: O[q, d] != 0 iff
    element (q, 64 kb0 + d) is kept."""
    C = require_native()
    keep, valid, ln = _keep(B, H, S, p), _valid(B, S, lens, dev), _lens(lens, dev)
    g = torch.Generator().manual_seed(S)
    for kb0 in range((S + 63) // 64):
        qkv = torch.zeros(B, S, 3, H, 64, device=dev)
        qkv[:, :, 1] = torch.randn(B, S, H, 64, generator=g).to(dev)
        qkv[:, :, 2] = _one_hot_rows(S, kb0, dev)[None, :, None, :]
        out, _ = _fwd(C, qkv.view(B * S, -1).to(torch.bfloat16), ln, B, S, H, **_drop(p))
        n = min(64, S - 64 * kb0)
        got = out.view(B, S, H, 64).permute(0, 2, 1, 3)[..., :n] != 0  # [B, H, q, d]
        want = keep[:, :, :, 64 * kb0:64 * kb0 + n]
        ok = valid[:, None, None, 64 * kb0:64 * kb0 + n].expand_as(want)
        assert torch.equal(got[ok], want[ok]), f"key block {kb0}"
        assert not got[~ok].any()


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,S,H,lens", PROBE_SHAPES)
def test_dkdv_mask_probe(dev, B, S, H, lens, p):
    """Q = 0, dO one-hot on one 64-query block: dV[k, d] != 0 iff element (64 qb0 + d, k) is kept."""
    C = require_native()
    keep, valid, ln = _keep(B, H, S, p), _valid(B, S, lens, dev), _lens(lens, dev)
    g = torch.Generator().manual_seed(S + 1)
    qkv = torch.zeros(B, S, 3, H, 64, device=dev)
    qkv[:, :, 1:] = torch.randn(B, S, 2, H, 64, generator=g).to(dev)
    qkv = qkv.view(B * S, -1).to(torch.bfloat16)
    out, lse = _fwd(C, qkv, ln, B, S, H, **_drop(p))
    for qb0 in range((S + 63) // 64):
        dout = _one_hot_rows(S, qb0, dev)[None, :, None, :].expand(B, S, H, 64).reshape(B * S, -1).to(torch.bfloat16)
        dqkv = _bwd(C, qkv, out, dout, lse, ln, B, S, H, **_drop(p))
        n = min(64, S - 64 * qb0)
        got = dqkv.view(B, S, 3, H, 64)[:, :, 2].permute(0, 2, 1, 3)[..., :n] != 0  # [B, H, k, d]
        want = keep[:, :, 64 * qb0:64 * qb0 + n, :].transpose(-1, -2)  # [B, H, k, q - 64 qb0]
        ok = valid[:, None, :, None].expand_as(want)
        assert torch.equal(got[ok], want[ok]), f"query block {qb0}"
        assert not got[~ok].any()


@pytest.mark.parametrize("B,S,H,lens", PROBE_SHAPES)
def test_dq_mask_probe(dev, B, S, H, lens):
    """Q = 0, V[k] = e_0, dO[q] = e_0, K one-hot on one 64-key block, p = 0.5 (s - delta ~ 1):
    dQ[q, d] > 0 iff element (q, 64 kb0 + d) is kept -- a kept entry gives P (s - delta) > 0, a
    dropped one -P delta < 0."""
    C = require_native()
    p = 0.5
    keep, valid, ln = _keep(B, H, S, p), _valid(B, S, lens, dev), _lens(lens, dev)
    dout = torch.zeros(B * S, H, 64, device=dev)
    dout[:, :, 0] = 1.0
    dout = dout.view(B * S, -1).to(torch.bfloat16)
    for kb0 in range((S + 63) // 64):
        qkv = torch.zeros(B, S, 3, H, 64, device=dev)
        qkv[:, :, 1] = _one_hot_rows(S, kb0, dev)[None, :, None, :]
        qkv[:, :, 2, :, 0] = 1.0
        qkv = qkv.view(B * S, -1).to(torch.bfloat16)
        out, lse = _fwd(C, qkv, ln, B, S, H, **_drop(p))
        dqkv = _bwd(C, qkv, out, dout, lse, ln, B, S, H, **_drop(p))
        n = min(64, S - 64 * kb0)
        dq = dqkv.view(B, S, 3, H, 64)[:, :, 0].permute(0, 2, 1, 3)[..., :n].float()  # [B, H, q, d]
        want = keep[:, :, :, 64 * kb0:64 * kb0 + n]
        ok = valid[:, None, None, 64 * kb0:64 * kb0 + n].expand_as(want)
        assert (dq[ok] != 0).all()
        assert torch.equal(dq[ok] > 0, want[ok]), f"key block {kb0}"
        assert (dq[~ok] == 0).all()


# ---------------------------------------------------------------- numerics
def _attn_ref(qkv, B, S, H, lens, keep, p):
    q, k, v = qkv.float().view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * SCALE
    if lens is not None:
        mask = torch.arange(S, device=qkv.device)[None, :] < lens[:, None]
        s = s.masked_fill(~mask[:, None, None, :], float("-inf"))
    pr = s.softmax(-1) * keep * D.attention_scale(p)
    return (pr @ v).permute(0, 2, 1, 3).reshape(B * S, H * 64)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,S,H,use_lens", [(2, 64, 1, False), (2, 128, 2, False), (3, 200, 2, True),
                                            (1, 512, 4, False), (2, 256, 3, True), (1, 70, 1, False)])
def test_attention_dropout_numerics(dev, B, S, H, use_lens, p):
    """The scheme and tolerances of test_transformer_gpu.py::test_attention, with the oracle mask and
    scale applied in the fp32 reference: 2e-2 on O, 3e-2 on dQ / dK / dV of the reference maximum."""
    C = require_native()
    g = torch.Generator().manual_seed(B * 1000 + S + H)
    Dm = H * 64
    qkv = (torch.randn(B * S, 3 * Dm, generator=g)).to(torch.bfloat16).to(dev)
    lens = None
    if use_lens:
        lens = torch.randint(1, S + 1, (B,), generator=g).to(torch.int32)
        lens[0] = S
        lens = lens.to(dev)
    keep = D.attention_keep_mask(SEED, SITE, RANK, B, H, S, p, device=dev)
    out, lse = _fwd(C, qkv, lens, B, S, H, **_drop(p))
    out0, lse0 = _fwd(C, qkv, lens, B, S, H)
    assert torch.equal(lse, lse0)  # the LSE is the undropped softmax's, bit for bit
    qr = qkv.float().requires_grad_()
    ref = _attn_ref(qr, B, S, H, lens, keep, p)
    err = (out.float() - ref).abs().max().item()
    ref_max = ref.abs().max().item() + 1e-6
    print(f"O: max abs err {err:.4g} vs ref max {ref_max:.4g}")
    assert err <= 2e-2 * ref_max, f"O: {err:.4g} vs {ref_max:.4g}"
    dout = torch.randn(B * S, Dm, generator=g).to(torch.bfloat16).to(dev)
    ref.backward(dout.float())
    dqkv = _bwd(C, qkv, out, dout, lse, lens, B, S, H, **_drop(p))
    assert torch.isfinite(dqkv.float()).all()
    gr = qr.grad.view(B * S, 3, Dm)
    dg = dqkv.view(B * S, 3, Dm)
    errs = {}
    for j, name in enumerate("qkv"):
        errs[name] = ((dg[:, j].float() - gr[:, j]).abs().max().item(), gr[:, j].abs().max().item() + 1e-6)
        print(f"d{name}: max abs err {errs[name][0]:.4g} vs ref max {errs[name][1]:.4g}")
    for name, (e, m) in errs.items():
        assert e <= 3e-2 * m, f"d{name}: {e:.4g} vs {m:.4g}"
    # no atomics, nothing stored: a second launch gives the same bits
    out2, lse2 = _fwd(C, qkv, lens, B, S, H, **_drop(p))
    assert torch.equal(out2.view(torch.int16), out.view(torch.int16)) and torch.equal(lse2, lse)
    dqkv2 = _bwd(C, qkv, out, dout, lse, lens, B, S, H, **_drop(p))
    assert torch.equal(dqkv2.view(torch.int16), dqkv.view(torch.int16))
    # p = 0.0 through the new keywords is the positional call
    outk, lsek = _fwd(C, qkv, lens, B, S, H, p=0.0, seed=SEED, site=SITE, rank=RANK)
    assert torch.equal(outk.view(torch.int16), out0.view(torch.int16)) and torch.equal(lsek, lse0)
    d0 = _bwd(C, qkv, out0, dout, lse0, lens, B, S, H)
    dk = _bwd(C, qkv, out0, dout, lse0, lens, B, S, H, p=0.0, seed=SEED, site=SITE, rank=RANK)
    assert torch.equal(dk.view(torch.int16), d0.view(torch.int16))


def test_attention_dropout_checks(dev, monkeypatch):
    C = require_native()
    B, S, H = 1, 64, 1
    qkv = torch.randn(B * S, 3 * 64, device=dev).to(torch.bfloat16)
    with pytest.raises((ValueError, RuntimeError)):
        _fwd(C, qkv, None, B, S, H, p=1.0, seed=1, site=SITE, rank=0)
    with pytest.raises(ValueError):  # rounds to 0/256: not a silent no-op
        _fwd(C, qkv, None, B, S, H, p=0.001, seed=1, site=SITE, rank=0)
    out, lse = _fwd(C, qkv, None, B, S, H, **_drop(0.1))
    dout = torch.randn(B * S, 64, device=dev).to(torch.bfloat16)
    with pytest.raises((ValueError, RuntimeError)):
        _bwd(C, qkv, out, dout, lse, None, B, S, H, p=1.0, seed=1, site=SITE, rank=0)
    monkeypatch.setenv("MLT_ATTN_RING", "0")  # the register-staged kernels are dropout-free
    with pytest.raises(RuntimeError, match="ring"):
        _bwd(C, qkv, out, dout, lse, None, B, S, H, **_drop(0.1))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- model
def _grads(m, fn, ids, mask, y, **kw):
    m.zero_grad(set_to_none=True)
    F.cross_entropy(fn(ids, mask, **kw).float(), y).backward()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("use_mask", [False, True])
def test_bert_tiny_attention_dropout_matches_reference(dev, use_mask):
    """The rule of test_bert_tiny_dropout_matches_reference with attention dropout 0.1 next to
    hidden dropout 0.1 and one seed given to all three paths (identical masks): native gradient
    error vs the fp32 reference at most max(2 x autocast's error, 0.02) per parameter."""
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    torch.manual_seed(0)
    m = BertClassifier(bert_config("bert-tiny", attention_dropout=0.1, hidden_dropout=0.1)).to(dev)
    m.train()
    ids = torch.randint(5, 1000, (2, 128), device=dev)
    mask = torch.ones(2, 128, dtype=torch.long, device=dev)
    if use_mask:
        mask[1, 100:] = 0
    y = torch.tensor([0, 1], device=dev)
    seed = 2 ** 61 + 12345
    out = m(ids, mask, dropout_seed=seed)
    ref = m.forward_reference(ids, mask, dropout_seed=seed)
    err = (out.float() - ref).abs().max().item()
    assert err <= 5e-2 * (ref.abs().max().item() + 1e-6), err
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


def test_bert_tiny_attention_dropout_determinism(dev):
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    torch.manual_seed(0)
    m0 = BertClassifier(bert_config("bert-tiny")).to(dev)
    m = BertClassifier(bert_config("bert-tiny", attention_dropout=0.1)).to(dev)
    m.load_state_dict(m0.state_dict())
    m.train()
    ids = torch.randint(5, 1000, (2, 128), device=dev)
    y = torch.tensor([0, 1], device=dev)
    g1 = _grads(m, m, ids, None, y, dropout_seed=11)
    g2 = _grads(m, m, ids, None, y, dropout_seed=11)
    g3 = _grads(m, m, ids, None, y, dropout_seed=12)
    assert all(torch.equal(g1[n], g2[n]) for n in g1)
    assert any(not torch.equal(g1[n], g3[n]) for n in g1)
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


def test_fp8_bert_attention_dropout_close_to_bf16(dev):
    """Thresholds of test_fp8_bert_close_to_bf16: 0.1 on the output, 0.25 per gradient (the q8
    epilogue of the backward kernels together with dropout)."""
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    torch.manual_seed(0)
    m8 = BertClassifier(bert_config("bert-tiny", fp8=True, attention_dropout=0.1)).to(dev)
    m8.train()
    ids = torch.randint(5, 1000, (4, 128), device=dev)
    y = torch.randint(0, 2, (4,), device=dev)
    o8 = m8(ids, dropout_seed=77)
    F.cross_entropy(o8, y).backward()
    m16 = BertClassifier(bert_config("bert-tiny", attention_dropout=0.1)).to(dev)
    m16.load_state_dict(m8.state_dict())
    m16.train()
    o16 = m16(ids, dropout_seed=77)
    rel = (o8.detach() - o16).norm() / o16.norm()
    assert rel < 0.1, rel
    F.cross_entropy(o16, y).backward()
    for (n, p8), p16 in zip(m8.named_parameters(), m16.parameters()):
        r = (p8.grad - p16.grad).norm() / (p16.grad.norm() + 1e-12)
        assert r < 0.25, (n, float(r))


def test_attention_dropout_flat_gradients_match_returned(dev):
    """As test_dropout_flat_gradients_match_returned, with attention dropout on: gradients written
    into a FusedAdamW's flat buffer equal the returned-gradient run's, accumulated over two backwards."""
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    from ml_trainer_amd.ops.optim import FusedAdamW
    from ml_trainer_amd.utils.flat import FlatParams
    torch.manual_seed(0)
    cfg = bert_config("bert-tiny", attention_dropout=0.1, hidden_dropout=0.1)
    m1 = BertClassifier(cfg).to(dev)
    m2 = BertClassifier(cfg).to(dev)
    m2.load_state_dict(m1.state_dict())
    opt = FusedAdamW(m2.parameters(), lr=1e-4)
    fp = FlatParams.owner(m2.layers[0].qkv.bias)
    assert fp is not None and FlatParams.owner(m2.layers[0].out.bias) is fp
    ids = torch.randint(5, 1000, (2, 128), device=dev)
    y = torch.tensor([0, 1], device=dev)
    F.cross_entropy(m1(ids, dropout_seed=21), y).backward()
    opt.zero_grad()
    for _ in range(2):  # accumulates across two backwards
        F.cross_entropy(m2(ids, dropout_seed=21), y).backward()
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        torch.testing.assert_close(p2.grad, 2 * p1.grad, rtol=1e-3, atol=1e-5, msg=n)
    for b in (m2.layers[0].qkv.bias, m2.layers[1].out.bias):
        assert fp.grad_sink(b) is not None and b.grad.abs().sum().item() > 0
