"""Unpadded (packed) BERT execution on the GPU: the packed instantiations of the flash attention
kernels (cu_seqlens), the embedding kernels with explicit positions, and the model / Trainer on top."""
import math

import pytest
import torch
import torch.nn.functional as F

from ml_trainer_amd.ops import dropout as D
from ml_trainer_amd.ops._ext import require_native

pytestmark = pytest.mark.gpu

SCALE = 0.125
SEED, SITE, RANK = 0x1234_5678_9ABC, D.attention_site(1), 0

# the smallest shapes at which the packed kernels can still go wrong: (H, S = max_seqlen, lens)
SHAPES = [
    (2, 200, [200, 1, 64, 65, 129]),  # S no multiple of 64, block edges, one-token sequence, odd row offsets
    (3, 256, [256, 128, 127]),  # the 2-group path; an S that is FULLT in padded mode
    (1, 64, [64, 3]),  # the 1-group path
]


def _close(a, b, tol):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item() + 1e-6
    assert err <= tol * ref, f"max abs err {err:.4g} vs ref max {ref:.4g} (tol {tol})"


def _drop(p):
    return dict(p=p, seed=SEED, site=SITE, rank=RANK) if p else {}


def _cu(lens, dev):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=dev)


_INPUTS = {}


def _inputs(si, dev):
    """qkv [T, 3D], dout [T, D] (bf16) and cu_seqlens of shape ``si``: made once, never modified."""
    if si not in _INPUTS:
        H, S, lens = SHAPES[si]
        g = torch.Generator().manual_seed(1000 * si + S + H)
        T, Dm = sum(lens), H * 64
        qkv = torch.randn(T, 3 * Dm, generator=g).to(torch.bfloat16).to(dev)
        dout = torch.randn(T, Dm, generator=g).to(torch.bfloat16).to(dev)
        _INPUTS[si] = (qkv, dout, _cu(lens, dev))
    return _INPUTS[si]


_REFS = {}


def _reference(si, p, dev):
    """fp32 per-sequence reference of shape ``si`` at dropout ``p`` (computed once): out [T, D], the base-2
    LSE per sequence [H, len] and d(qkv) [T, 3D]; the mask is the padded run's, sliced to [:len, :len]."""
    if (si, p) not in _REFS:
        H, S, lens = SHAPES[si]
        qkv, dout, _ = _inputs(si, dev)
        keep = D.attention_keep_mask(SEED, SITE, RANK, len(lens), H, S, p, device=dev) if p else None
        qr = qkv.float().requires_grad_()
        outs, lses, r0 = [], [], 0
        for b, n in enumerate(lens):
            q, k, v = qr[r0:r0 + n].view(n, 3, H, 64).permute(1, 2, 0, 3)
            s = (q @ k.transpose(-1, -2)) * SCALE
            pr = s.softmax(-1)
            if p:
                pr = pr * keep[b, :, :n, :n] * D.attention_scale(p)
            outs.append((pr @ v).permute(1, 0, 2).reshape(n, H * 64))
            lses.append((torch.logsumexp(s, -1) / math.log(2)).detach())
            r0 += n
        out = torch.cat(outs)
        out.backward(dout.float())
        _REFS[si, p] = (out.detach(), lses, qr.grad)
    return _REFS[si, p]


def _fwd(C, qkv, cu, B, S, H, out=None, **kw):
    T = qkv.shape[0]
    out = torch.empty(T, H * 64, dtype=torch.bfloat16, device=qkv.device) if out is None else out
    lse = torch.zeros(B * H * S, device=qkv.device)
    C.attn_fwd(qkv, out, lse, None, B, S, H, SCALE, cu_seqlens=cu, **kw)
    return out, lse


def _bwd(C, qkv, out, dout, lse, cu, B, S, H, dqkv=None, **kw):
    dqkv = torch.full_like(qkv, float("nan")) if dqkv is None else dqkv
    delta = torch.empty(qkv.shape[0] * H, device=qkv.device)
    C.attn_bwd(qkv, out, dout, lse, delta, None, dqkv, B, S, H, SCALE, cu_seqlens=cu, **kw)
    return dqkv


# ---------------------------------------------------------------- packed attention numerics
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_packed_attention_numerics(dev, si, p):
    """The scheme and tolerances of test_transformer_gpu.py::test_attention (and, with dropout, of
    test_attn_dropout_gpu.py::test_attention_dropout_numerics) against the fp32 per-sequence reference:
    2e-2 on O, 1e-3 on the LSE of the valid entries, 3e-2 of the reference maximum on dQ / dK / dV."""
    C = require_native()
    H, S, lens = SHAPES[si]
    B, Dm = len(lens), H * 64
    qkv, dout, cu = _inputs(si, dev)
    ref, ref_lse, ref_g = _reference(si, p, dev)
    out, lse = _fwd(C, qkv, cu, B, S, H, **_drop(p))
    err, ref_max = (out.float() - ref).abs().max().item(), ref.abs().max().item() + 1e-6
    print(f"O: max abs err {err:.4g} vs ref max {ref_max:.4g}")
    _close(out, ref, 2e-2)
    for b, n in enumerate(lens):
        torch.testing.assert_close(lse.view(B, H, S)[b, :, :n], ref_lse[b], rtol=1e-3, atol=1e-3)
    if p:  # the LSE is the undropped softmax's, bit for bit
        assert torch.equal(lse, _fwd(C, qkv, cu, B, S, H)[1])
    dqkv = _bwd(C, qkv, out, dout, lse, cu, B, S, H, **_drop(p))
    assert torch.isfinite(dqkv.float()).all()
    gr, dg = ref_g.view(-1, 3, Dm), dqkv.view(-1, 3, Dm)
    errs = {}
    for j, name in enumerate("qkv"):
        errs[name] = ((dg[:, j].float() - gr[:, j]).abs().max().item(), gr[:, j].abs().max().item() + 1e-6)
        print(f"d{name}: max abs err {errs[name][0]:.4g} vs ref max {errs[name][1]:.4g}")
    for name, (e, m) in errs.items():
        assert e <= 3e-2 * m, f"d{name}: {e:.4g} vs {m:.4g}"
    # no atomics, nothing stored: a second launch gives the same bits
    out2, lse2 = _fwd(C, qkv, cu, B, S, H, **_drop(p))
    assert torch.equal(out2.view(torch.int16), out.view(torch.int16)) and torch.equal(lse2, lse)
    assert torch.equal(_bwd(C, qkv, out, dout, lse, cu, B, S, H, **_drop(p)).view(torch.int16), dqkv.view(torch.int16))


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_packed_attention_equals_padded_rows(dev, p):
    """A packed run and the padded run of the same sequences (lens as the key mask) multiply the same
    numbers in the same order, with the same dropout bytes: the valid rows agree bit for bit."""
    C = require_native()
    H, S, lens = SHAPES[0]
    B, Dm = len(lens), H * 64
    qkv, dout, cu = _inputs(0, dev)
    idx = torch.cat([b * S + torch.arange(n) for b, n in enumerate(lens)]).to(dev)
    pq = torch.zeros(B * S, 3 * Dm, dtype=torch.bfloat16, device=dev).index_copy_(0, idx, qkv)
    pd = torch.zeros(B * S, Dm, dtype=torch.bfloat16, device=dev).index_copy_(0, idx, dout)
    ln = torch.tensor(lens, dtype=torch.int32, device=dev)
    po = torch.empty(B * S, Dm, dtype=torch.bfloat16, device=dev)
    pl = torch.empty(B * H * S, device=dev)
    C.attn_fwd(pq, po, pl, ln, B, S, H, SCALE, **_drop(p))
    pg = torch.empty_like(pq)
    C.attn_bwd(pq, po, pd, pl, torch.empty(B * S * H, device=dev), ln, pg, B, S, H, SCALE, **_drop(p))
    out, lse = _fwd(C, qkv, cu, B, S, H, **_drop(p))
    dqkv = _bwd(C, qkv, out, dout, lse, cu, B, S, H, **_drop(p))
    assert torch.equal(out.view(torch.int16), po[idx].view(torch.int16))
    assert torch.equal(dqkv.view(torch.int16), pg[idx].view(torch.int16))


# ---------------------------------------------------------------- isolation and bounds
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_packed_attention_isolation_and_bounds(dev, p):
    """No guard lets in the rows after a sequence: with NaN in the 64 rows after the last sequence of the
    inputs every result is finite and the 64 sentinel rows after the outputs are untouched; changing one
    sequence's rows leaves every other sequence's results bitwise unchanged. The allocations cover the
    extra rows, so a wrong guard shows as a wrong value here, never as a fault."""
    C = require_native()
    H, S, lens = SHAPES[0]
    B, Dm, T, X = len(lens), H * 64, sum(lens), 64
    qkv0, dout0, cu = _inputs(0, dev)
    qkv_big = torch.full((T + X, 3 * Dm), float("nan"), dtype=torch.bfloat16, device=dev)
    dout_big = torch.full((T + X, Dm), float("nan"), dtype=torch.bfloat16, device=dev)
    qkv_big[:T] = qkv0
    dout_big[:T] = dout0
    SENT = 77.0
    out_big = torch.full((T + X, Dm), SENT, dtype=torch.bfloat16, device=dev)
    dqkv_big = torch.full((T + X, 3 * Dm), SENT, dtype=torch.bfloat16, device=dev)
    cs = torch.zeros(3 * Dm, device=dev)
    qkv, dout = qkv_big[:T], dout_big[:T]
    out, lse = _fwd(C, qkv, cu, B, S, H, out=out_big[:T], **_drop(p))
    dqkv = _bwd(C, qkv, out, dout, lse, cu, B, S, H, dqkv=dqkv_big[:T], colsum_out=cs, **_drop(p))
    assert torch.isfinite(out.float()).all() and torch.isfinite(dqkv.float()).all() and torch.isfinite(cs).all()
    for b, n in enumerate(lens):
        assert torch.isfinite(lse.view(B, H, S)[b, :, :n]).all()
    assert (out_big[T:] == SENT).all() and (dqkv_big[T:] == SENT).all()
    out_a, dqkv_a = out.clone(), dqkv.clone()
    r0, r1 = int(cu[3]), int(cu[4])  # sequence 3 (65 rows at an odd offset) gets other values
    g = torch.Generator().manual_seed(99)
    qkv[r0:r1] = (3 * torch.randn(r1 - r0, 3 * Dm, generator=g)).to(torch.bfloat16).to(dev)
    out, lse = _fwd(C, qkv, cu, B, S, H, out=out_big[:T], **_drop(p))
    dqkv = _bwd(C, qkv, out, dout, lse, cu, B, S, H, dqkv=dqkv_big[:T], **_drop(p))
    other = torch.ones(T, dtype=torch.bool, device=dev)
    other[r0:r1] = False
    assert torch.equal(out[other].view(torch.int16), out_a[other].view(torch.int16))
    assert torch.equal(dqkv[other].view(torch.int16), dqkv_a[other].view(torch.int16))
    assert not torch.equal(out[r0:r1], out_a[r0:r1])
    assert (out_big[T:] == SENT).all() and (dqkv_big[T:] == SENT).all()


# ---------------------------------------------------------------- bias gradient, rejections
@pytest.mark.parametrize("si", [0, 1])
def test_packed_attention_bias_colsum(dev, si, monkeypatch):
    """The QKV bias gradient from the packed kernels' column partials (blocks past a sequence write
    zeros): set, and accumulated twice, with the tolerances of test_attention_bwd_fused_bias_colsum."""
    C = require_native()
    H, S, lens = SHAPES[si]
    B, Dm = len(lens), H * 64
    qkv, dout, cu = _inputs(si, dev)
    out, lse = _fwd(C, qkv, cu, B, S, H)
    for grp in ("1", "2"):
        monkeypatch.setenv("MLT_ATTN_DKDV_GROUPS", grp)
        monkeypatch.setenv("MLT_ATTN_DQ_GROUPS", grp)
        cs = torch.full((3 * Dm,), 2.0, device=dev)
        dqkv = _bwd(C, qkv, out, dout, lse, cu, B, S, H, colsum_out=cs)
        ref = dqkv.float().sum(0)
        tol = 1e-2 * dqkv.float().abs().sum(0).max().item()
        torch.testing.assert_close(cs, ref, rtol=1e-2, atol=tol)
        _bwd(C, qkv, out, dout, lse, cu, B, S, H, colsum_out=cs, colsum_accumulate=True)
        torch.testing.assert_close(cs, 2 * ref, rtol=1e-2, atol=2 * tol)
        _bwd(C, qkv, out, dout, lse, cu, B, S, H, colsum_out=cs, colsum_accumulate=True)
        torch.testing.assert_close(cs, 3 * ref, rtol=1e-2, atol=3 * tol)


def test_packed_attention_rejections(dev, monkeypatch):
    C = require_native()
    H, S, lens = SHAPES[2]
    B, Dm, T = len(lens), H * 64, sum(lens)
    qkv, dout, cu = _inputs(2, dev)
    out, lse = _fwd(C, qkv, cu, B, S, H)
    dqkv = torch.full_like(qkv, float("nan"))
    delta = torch.empty(T * H, device=dev)
    monkeypatch.setenv("MLT_ATTN_RING", "0")  # the register-staged kernels take padded batches only
    with pytest.raises(RuntimeError, match="ring"):
        C.attn_bwd(qkv, out, dout, lse, delta, None, dqkv, B, S, H, SCALE, cu_seqlens=cu)
    monkeypatch.delenv("MLT_ATTN_RING")
    y8 = torch.empty(T, 3 * Dm, dtype=torch.float8_e5m2, device=dev)
    yt8 = torch.empty(3 * Dm, T, dtype=torch.float8_e5m2, device=dev)
    with pytest.raises(RuntimeError, match="q8"):
        C.attn_bwd(qkv, out, dout, lse, delta, None, dqkv, B, S, H, SCALE, q8_y=y8, q8_yt=yt8,
                   q8_scale=torch.ones(1, device=dev), q8_amax=torch.zeros(4096, device=dev), cu_seqlens=cu)
    torch.cuda.synchronize()
    assert torch.isnan(dqkv).all().item()  # nothing was launched
    # argument checks: dtype, element count, device, row counts
    with pytest.raises(RuntimeError, match="cu_seqlens"):
        C.attn_fwd(qkv, out, lse, None, B, S, H, SCALE, cu_seqlens=cu.long())
    with pytest.raises(RuntimeError, match="cu_seqlens"):
        C.attn_fwd(qkv, out, lse, None, B, S, H, SCALE, cu_seqlens=cu[:-1])
    with pytest.raises(RuntimeError, match="cu_seqlens"):
        C.attn_fwd(qkv, out, lse, None, B, S, H, SCALE, cu_seqlens=cu.cpu())
    with pytest.raises(RuntimeError, match="out"):
        C.attn_fwd(qkv, out[:-1], lse, None, B, S, H, SCALE, cu_seqlens=cu)
    big = torch.zeros(B * S + 1, 3 * Dm, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="exceed"):
        C.attn_fwd(big, torch.empty(B * S + 1, Dm, dtype=torch.bfloat16, device=dev), lse, None, B, S, H, SCALE,
                   cu_seqlens=cu)


# ---------------------------------------------------------------- packed embeddings
@pytest.mark.parametrize("with_tt", [False, True])
def test_packed_embeddings(dev, with_tt):
    """The scheme of test_transformer_gpu.py::test_embeddings on a packed batch: explicit positions in
    the forward, the per-position sum over the sequences long enough in the backward, no atomics."""
    C = require_native()
    g = torch.Generator().manual_seed(3)
    V, P, Dm, S = 500, 128, 256, 96
    lens = [96, 1, 50, 33]
    T = sum(lens)
    cu = _cu(lens, dev)
    pos = torch.cat([torch.arange(n) for n in lens]).to(torch.int32).to(dev)
    ww, wp, wt = [(torch.randn(r, Dm, generator=g)).to(torch.bfloat16).to(dev) for r in (V, P, 2)]
    ids = torch.randint(0, V, (T,), generator=g).to(dev)
    ids[:10] = 7  # repeated ids exercise the scatter-add
    tt = torch.randint(0, 2, (T,), generator=g).to(dev) if with_tt else None
    out = torch.empty(T, Dm, dtype=torch.bfloat16, device=dev)
    C.embed_fwd(ids, tt, ww, wp, wt, out, S, pos=pos)
    t = tt if tt is not None else torch.zeros_like(ids)
    _close(out, ww.float()[ids] + wp.float()[pos.long()] + wt.float()[t], 1e-2)
    dout = torch.randn(T, Dm, generator=g).to(torch.bfloat16).to(dev)
    gw, gp, gt = (torch.zeros(V, Dm, device=dev), torch.zeros(P, Dm, device=dev), torch.zeros(2, Dm, device=dev))
    part = torch.empty(S * 2 * Dm, device=dev)
    sid, perm = torch.sort(ids, stable=True)
    gw.fill_(0.5)  # the kernels accumulate into existing gradients
    gp.fill_(0.25)
    C.embed_bwd(sid, perm, tt, dout, gw, gp, gt, part, S, cu_seqlens=cu)
    gw -= 0.5
    gp -= 0.25
    runs = []
    for _ in range(2):  # no atomics: repeated runs give the same bits
        r = (torch.zeros_like(gw), torch.zeros_like(gp), torch.zeros_like(gt))
        C.embed_bwd(sid, perm, tt, dout, *r, part, S, cu_seqlens=cu)
        runs.append(r)
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    d = dout.float()
    _close(gw, torch.zeros(V, Dm, device=dev).index_add_(0, ids, d), 1e-4)
    _close(gp, torch.zeros(P, Dm, device=dev).index_add_(0, pos.long(), d), 1e-4)
    _close(gt, torch.zeros(2, Dm, device=dev).index_add_(0, t, d), 1e-4)
    assert (gp[S:] == 0).all()
    with pytest.raises(RuntimeError):  # the padded form still wants whole rows of S tokens
        C.embed_fwd(ids, tt, ww, wp, wt, out, S)
    with pytest.raises(RuntimeError):
        C.embed_fwd(ids, tt, ww, wp, wt, out, S, pos=pos[:-1])


# ---------------------------------------------------------------- model
LENS = [128, 100, 1, 37]


def _batch(dev):
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(5, 1000, (4, 128), generator=g).to(dev)
    mask = (torch.arange(128)[None, :] < torch.tensor(LENS)[:, None]).long().to(dev)
    return ids, mask, torch.tensor([0, 1, 1, 0], device=dev)


def _grads(m, fn, ids, mask, y, **kw):
    m.zero_grad(set_to_none=True)
    F.cross_entropy(fn(ids, mask, **kw).float(), y).backward()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("dropout", [False, True])
def test_bert_tiny_unpad_matches_reference(dev, dropout):
    """bert-tiny with unpad=True: logits within 5e-2 of the packed fp32 reference, every parameter
    gradient within the budget of test_bert_tiny_matches_reference (native relative error at most
    max(2 x autocast's, 0.02)); with hidden and attention dropout 0.1 at a fixed seed likewise, and two
    native runs with one seed are bitwise equal."""
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    torch.manual_seed(0)
    over = dict(hidden_dropout=0.1, attention_dropout=0.1) if dropout else {}
    m = BertClassifier(bert_config("bert-tiny", unpad=True, **over)).to(dev)
    m.train()
    ids, mask, y = _batch(dev)
    kw = dict(dropout_seed=4242) if dropout else {}
    out = m(ids, mask, **kw)
    ref = m.forward_reference(ids, mask, **kw)
    _close(out, ref, 5e-2)
    gn = _grads(m, m, ids, mask, y, **kw)
    gr = _grads(m, m.forward_reference, ids, mask, y, **kw)
    ga = _grads(m, m.forward_torch_bf16, ids, mask, y, **kw)
    for n in gr:
        nr = gr[n].norm().item()
        if nr < 1e-8:
            continue
        e_nat = (gn[n] - gr[n]).norm().item() / nr
        e_ac = (ga[n] - gr[n]).norm().item() / nr
        print(f"{n}: native rel err {e_nat:.4f} vs autocast {e_ac:.4f}")
        assert e_nat <= max(2.0 * e_ac, 0.02), f"{n}: native rel err {e_nat:.4f} vs autocast {e_ac:.4f}"
    assert torch.equal(m(ids, mask, **kw), out)
    g2 = _grads(m, m, ids, mask, y, **kw)
    assert all(torch.equal(gn[n], g2[n]) for n in gn)
    if not dropout:  # pads never reach the CLS rows: the padded native model gives the same logits
        m.config = bert_config("bert-tiny")
        _close(m(ids, mask), out, 2e-2)


def test_unpad_direct_flat_gradients_match_returned(dev):
    """test_direct_flat_gradients_match_returned in packed mode: the fused backwards accumulate straight
    into FlatParams gradients, equal to the returned-gradient path, across two backwards, and notify."""
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    from ml_trainer_amd.utils.flat import FlatParams
    torch.manual_seed(0)
    m1 = BertClassifier(bert_config("bert-tiny", unpad=True)).to(dev)
    m2 = BertClassifier(bert_config("bert-tiny", unpad=True)).to(dev)
    m2.load_state_dict(m1.state_dict())
    fp = FlatParams(m2.parameters())
    seen = []
    fp.grad_ready_hooks.append(lambda p: seen.append(id(p)))
    ids, mask, y = _batch(dev)
    F.cross_entropy(m1(ids, mask), y).backward()
    fp.zero_grad()
    for _ in range(2):
        F.cross_entropy(m2(ids, mask), y).backward()
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        torch.testing.assert_close(p2.grad, 2 * p1.grad, rtol=1e-3, atol=1e-5, msg=n)
    direct = {id(p) for n, p in m2.named_parameters() if not n.startswith(("pooler", "classifier"))}
    assert direct <= set(seen)


def test_unpad_trainer_trains_and_evaluates(dev, tmp_path):
    """bert-tiny through Trainer on variable-length data with unpad=True (lengths from pad_id): the loss
    is finite and falls, and evaluate() runs the packed path under no_grad."""
    from ml_trainer_amd.data.text import SyntheticTextClassification
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    from ml_trainer_amd.trainer import Trainer
    torch.manual_seed(0)
    m = BertClassifier(bert_config("bert-tiny", unpad=True, pad_id=0))
    tr = SyntheticTextClassification(256, seq_len=64, vocab_size=1000, seed=0, learnable=True, min_len=16)
    va = SyntheticTextClassification(64, seq_len=64, vocab_size=1000, seed=1, learnable=True, min_len=16)
    t = Trainer(m, datasets=(tr, va), epochs=6, batch_size=32, model_dir=str(tmp_path), optimizer="adamw", lr=1e-3,
                metric="accuracy", options={"progress": False})
    t.fit()
    losses = t.history["train_loss"]
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses
    ev = t.evaluate()
    assert all(math.isfinite(float(v)) for v in (ev if isinstance(ev, (tuple, list)) else [ev]) if v is not None)
