"""The masked-LM head on the GPU: vocab_ce against fp64, the selection / gather / scatter kernels
against their torch oracle, the fused chunked decoder (chunk invariance, peak memory, all-ignored
batches), BertForMaskedLM against its fp32 reference, the tied word-table gradient under FlatParams,
training and the Trainer."""
import pytest
import torch

from tests import helpers
from ml_trainer_amd.ops import mlm as M

pytestmark = pytest.mark.gpu


def _C():
    from ml_trainer_amd.ops._ext import require_native
    return require_native()


# ------------------------------------------------------------------------------------- vocab_ce
# (V, ldz): the bench vocabulary; a padded small one; an odd V in a non-256 width; no padding; one
# chunk; and one width on each side of the LDS-resident limit (wider rows are read twice).
VCE_SHAPES = [(30522, 30720), (1000, 1024), (257, 264), (512, 512), (8, 8),
              (M.VOCAB_CE_RESIDENT_COLS - 3, M.VOCAB_CE_RESIDENT_COLS),
              (M.VOCAB_CE_RESIDENT_COLS + 5, M.VOCAB_CE_RESIDENT_COLS + 8)]
_VCE = {}


def _vce_case(V, ldz, dev):
    """Six rows in a guarded buffer (a guard row above and below, padding columns pre-filled with the
    NaN sentinel) and their fp64 reference, made once per shape."""
    key = (V, ldz)
    if key not in _VCE:
        g = torch.Generator().manual_seed(V)
        z = (4 * torch.randn(6, V, generator=g)).to(torch.bfloat16)
        i1, i2 = V // 3, (2 * V) // 3 + 1      # two-way tie at the maximum: the first index wins
        z[4, i1] = z[4, i2] = 24.0
        hot = V // 2                            # one column at +80, the rest at -80
        z[5] = -80.0
        z[5, hot] = 80.0
        labels = torch.tensor([0, V - 1, -100, V, i1, (hot + 1) % V], dtype=torch.int64)
        ok = torch.tensor([True, True, False, False, True, True])
        z64 = z.double()
        lse = torch.logsumexp(z64, 1)
        soft = torch.softmax(z64, 1)
        onehot = torch.zeros_like(soft)
        onehot[ok, labels[ok]] = 1.0
        zt = z64[torch.arange(6), labels.clamp(0, V - 1)]
        okd = ok.double()
        hit = torch.tensor([float(int(z64[r].argmax()) == int(labels[r])) for r in range(6)]) * ok.float()
        assert hit[4] == 1.0 and hit[5] == 0.0
        _VCE[key] = dict(z=z, labels=labels, ok=ok, loss=(lse - zt) * okd, lse=lse * okd, hit=hit,
                         grad=(soft - onehot) * okd[:, None], soft=soft)
    c = _VCE[key]
    buf, view = helpers.guarded(6, ldz, torch.bfloat16, dev)
    view[:, :V].copy_(c["z"].to(dev))
    return c, buf, view


@pytest.mark.parametrize("V,ldz", VCE_SHAPES)
def test_vocab_ce_matches_fp64(dev, V, ldz):
    C = _C()
    assert C.vocab_ce_resident_cols() == M.VOCAB_CE_RESIDENT_COLS
    c, buf, view = _vce_case(V, ldz, dev)
    labels = c["labels"].to(dev)
    before = buf.view(torch.int16).clone()

    # without write_grad: statistics only, Z untouched bit for bit
    loss, lse, hit = M.vocab_ce(view, V, labels, write_grad=False)
    assert torch.equal(buf.view(torch.int16), before)
    for name, got, ref in (("row_loss", loss, c["loss"]), ("row_lse", lse, c["lse"])):
        got = got.double().cpu()
        tol = 1e-5 * torch.clamp(ref.abs(), min=1.0)
        print(f"vocab_ce {V}/{ldz} {name}: max |err| / tol = {float(((got - ref).abs() / tol).max()):.3g}")
        assert bool(((got - ref).abs() <= tol).all()), (name, got, ref)
    assert torch.equal(hit.cpu(), c["hit"])
    assert bool((loss[2:4] == 0).all()) and bool((lse[2:4] == 0).all()) and bool((hit[2:4] == 0).all())

    # with write_grad: the same statistics, the gradient in place
    loss2, lse2, hit2 = M.vocab_ce(view, V, labels, write_grad=True)
    assert torch.equal(loss2, loss) and torch.equal(lse2, lse) and torch.equal(hit2, hit)
    helpers.assert_guard_intact(buf, view)
    got = view.cpu()
    assert bool((got[:, V:] == 0).all())            # padding columns: exactly 0
    assert bool((got[2:4] == 0).all())              # ignored rows: exactly 0
    expected, t = c["grad"], 2e-5 * c["soft"]
    used = helpers.assert_within(got[:, :V], expected, helpers.store_bound(expected, t, torch.bfloat16),
                                 f"vocab_ce gradient V={V} ldz={ldz}")
    print(f"vocab_ce {V}/{ldz} gradient: max |err| / bound = {used:.3g}")

    # a second run from the same logits: bitwise equal
    _, buf_b, view_b = _vce_case(V, ldz, dev)
    loss3, lse3, hit3 = M.vocab_ce(view_b, V, labels, write_grad=True)
    assert torch.equal(buf_b.view(torch.int16), buf.view(torch.int16))
    assert torch.equal(loss3, loss) and torch.equal(lse3, lse) and torch.equal(hit3, hit)


# ------------------------------------------------------------------------------------- select / gather / scatter
def _select_case(dev):
    g = torch.Generator().manual_seed(0)
    B, S, P = 3, 70, 8
    labels = torch.full((B, S), -100, dtype=torch.int64)
    labels[0, torch.randperm(S, generator=g)[:13]] = torch.randint(5, 1000, (13,), generator=g)  # overflows
    labels[2, torch.tensor([0, 3, 40, 64, 69])] = torch.randint(5, 1000, (5,), generator=g)     # sequence 1: none
    lens = torch.tensor([70, 33, 66], dtype=torch.int32)
    cu = torch.zeros(4, dtype=torch.int32)
    cu[1:] = torch.cumsum(lens, 0)
    return labels.to(dev), P, lens.to(dev), cu.to(dev)


@pytest.mark.parametrize("form", ["padded", "lens", "packed"])
def test_select_gather_scatter_match_oracle(dev, form):
    labels, P, lens, cu = _select_case(dev)
    kw = {"padded": {}, "lens": {"lens": lens}, "packed": {"cu_seqlens": cu}}[form]
    row, lab, ov = M.select(labels, P, **kw)
    rrow, rlab, rov = M.select_reference(labels, P, **kw)
    assert row.dtype == torch.int32 and row.numel() == 256
    assert torch.equal(row, rrow) and torch.equal(lab, rlab) and int(ov) == int(rov) == (5 if form == "padded" else 6)
    assert bool((row[8:16] == -1).all()) and bool((row[24:] == -1).all()) and bool((lab[24:] == -100).all())
    n_rows = int(cu[-1]) if form == "packed" else 3 * 70
    x = torch.randn(n_rows, 264, device=dev).to(torch.bfloat16)
    got = M.gather_rows(x, row)
    assert torch.equal(got, M.gather_reference(x, row))
    back = M.scatter_rows(got, row, n_rows)
    assert torch.equal(back, M.scatter_reference(got, row, n_rows))
    sel = row[row >= 0].long()
    expect = torch.zeros_like(x)
    expect[sel] = x[sel]
    assert torch.equal(back, expect)  # scatter(gather(x)): exactly the selected rows, zeros elsewhere


# ------------------------------------------------------------------------------------- the fused head
def _head_inputs(dev, R, V, h=256, S=16, P=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    B = R // P
    hidden = torch.randn(B * S, h, generator=g).to(torch.bfloat16).to(dev)
    labels = torch.full((B, S), -100, dtype=torch.int64)
    for b in range(B):
        k = 1 + b % P
        labels[b, torch.randperm(S, generator=g)[:k]] = torch.randint(0, V, (k,), generator=g)
    ps = [torch.randn(h, h, generator=g) * 0.05, torch.randn(h, generator=g) * 0.05,
          1 + 0.1 * torch.randn(h, generator=g), 0.1 * torch.randn(h, generator=g),
          torch.randn(V, h, generator=g) * 0.05, torch.randn(V, generator=g) * 0.1]
    return hidden, labels.to(dev), [p.to(dev) for p in ps], P


def _leaves(hidden, ps):
    return hidden.clone().requires_grad_(), [p.clone().requires_grad_() for p in ps]


def _run_head(hidden, labels, ps, P, chunk_rows, leaves=None):
    hs, qs = leaves if leaves is not None else _leaves(hidden, ps)
    out = M.mlm_head(hs, labels, P, M.MLMParams(*qs, 1e-12), chunk_rows=chunk_rows)
    out.loss.backward()
    return out, [hs.grad] + [q.grad for q in qs]


def test_head_chunk_invariance(dev):
    hidden, labels, ps, P = _head_inputs(dev, 512, 1000)
    a, ga = _run_head(hidden, labels, ps, P, 256)
    b, gb = _run_head(hidden, labels, ps, P, 512)
    assert a.row_loss.numel() == 512 and int((a.row_loss != 0).sum()) == int((labels != -100).sum())
    assert torch.equal(a.row_loss, b.row_loss)  # per-row loss: bitwise
    assert torch.equal(a.accuracy, b.accuracy) and int(a.overflow) == 0
    for x, y, n in zip(ga, gb, ["hidden", "dense_w", "dense_b", "ln_w", "ln_b", "word_w", "out_bias"]):
        torch.testing.assert_close(x.float(), y.float(), rtol=1e-3, atol=1e-5, msg=lambda m, n=n: f"{n}: {m}")
    ref = M.mlm_head_reference(hidden, labels, P, M.MLMParams(*ps, 1e-12))
    print(f"head loss native {float(a.loss.detach()):.6f} reference {float(ref.loss):.6f}")


def test_head_peak_memory_below_full_logits(dev):
    R, V = 2048, 30522
    hidden, labels, ps, P = _head_inputs(dev, R, V)
    full_logits = R * 30720 * 2  # the [R, Vp] bf16 logits the chunked decoder never materialises
    leaves = _leaves(hidden, ps)  # (the inputs are not the head's memory)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, grads = _run_head(hidden, labels, ps, P, 256, leaves)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"head peak {peak / 2 ** 20:.1f} MiB vs full logits {full_logits / 2 ** 20:.1f} MiB")
    assert bool(torch.isfinite(out.loss))
    assert peak < full_logits, (peak, full_logits)


def test_head_all_ignored_batch(dev):
    hidden, labels, ps, P = _head_inputs(dev, 256, 1000)
    out, grads = _run_head(hidden, torch.full_like(labels, -100), ps, P, 256)
    assert float(out.loss.detach()) == 0.0 and float(out.accuracy) == 0.0
    for g in grads:
        assert g is not None and float(g.float().abs().sum()) == 0.0


# ------------------------------------------------------------------------------------- the model
def _model_batch(dev, use_mask, B=3, S=64, P=8, seed=5):
    from ml_trainer_amd.data.text import SyntheticMaskedLM
    ds = SyntheticMaskedLM(B, seq_len=S, vocab_size=1000, max_predictions=P, seed=seed,
                           **({"min_len": 24} if use_mask else {}))
    ids, labels = ds.ids.to(dev), ds.labels.to(dev)
    return ids, ((ids != 0).long() if use_mask else None), labels


def _mlm_grads(m, fwd, loss_fn, ids, mask, labels):
    m.zero_grad(set_to_none=True)
    loss = loss_fn(fwd(ids, mask), labels)
    loss.backward()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("use_mask,unpad", [(False, False), (True, False), (True, True)])
def test_bert_tiny_mlm_matches_reference(dev, use_mask, unpad):
    """Native loss within 5e-2 of the fp32 reference; for every parameter (the tied table included) the
    native gradient error is at most max(2 x the autocast baseline's, 0.02)."""
    from ml_trainer_amd.models.bert import BertForMaskedLM, bert_config
    torch.manual_seed(0)
    m = BertForMaskedLM(bert_config("bert-tiny", max_predictions=8, unpad=unpad)).to(dev)
    with torch.no_grad():
        m.mlm_bias.normal_(std=0.1)
    ids, mask, labels = _model_batch(dev, use_mask)
    ln, gn = _mlm_grads(m, m, m.mlm_loss, ids, mask, labels)
    assert int(m.last_mlm_overflow) == 0
    lr, gr = _mlm_grads(m, m.forward_reference, m.mlm_loss_reference, ids, mask, labels)
    la, ga = _mlm_grads(m, m.forward_torch_bf16, m.mlm_loss_torch_bf16, ids, mask, labels)
    print(f"mlm loss native {float(ln):.5f} reference {float(lr):.5f} autocast {float(la):.5f}")
    assert abs(float(ln) - float(lr)) <= 5e-2 * abs(float(lr))
    for n in gr:
        nr = gr[n].norm().item()
        if nr < 1e-8:
            continue
        e_nat = (gn[n] - gr[n]).norm().item() / nr
        e_ac = (ga[n] - gr[n]).norm().item() / nr
        assert e_nat <= max(2.0 * e_ac, 0.02), f"{n}: native rel err {e_nat:.4f} vs autocast {e_ac:.4f}"
    rows = (labels.view(-1) != -100).nonzero().view(-1)[:5]
    if not unpad:
        with torch.no_grad():
            lg = m.mlm_logits(m(ids, mask), rows)
            lref = m.mlm_logits(m.forward_reference(ids, mask), rows)
        assert lg.shape == (rows.numel(), 1000) and lg.dtype == torch.float32
        assert float((lg - lref).abs().max()) <= 5e-2 * float(lref.abs().max())


def test_tied_table_gradient_and_single_notification(dev):
    """Under FlatParams the word table gets the decoder's weight gradient and the embedding rows, and is
    announced once -- by the embedding backward, after both have landed."""
    from ml_trainer_amd.models.bert import BertForMaskedLM, bert_config
    from ml_trainer_amd.utils.flat import FlatParams
    torch.manual_seed(0)
    m = BertForMaskedLM(bert_config("bert-tiny", max_predictions=8)).to(dev)
    ref = BertForMaskedLM(bert_config("bert-tiny", max_predictions=8)).to(dev)
    ref.load_state_dict(m.state_dict())
    ids, mask, labels = _model_batch(dev, True)
    lr, gr = _mlm_grads(ref, ref.forward_reference, ref.mlm_loss_reference, ids, mask, labels)
    la, ga = _mlm_grads(ref, ref.forward_torch_bf16, ref.mlm_loss_torch_bf16, ids, mask, labels)
    lu, gu = _mlm_grads(ref, ref, ref.mlm_loss, ids, mask, labels)  # native, returned gradients (autograd sums)
    fp = FlatParams(m.parameters())
    table = m.word_embeddings.weight
    seen, at_hook = [], []

    def hook(p):
        seen.append(id(p))
        if p is table:
            at_hook.append(p.grad.detach().clone())

    fp.grad_ready_hooks.append(hook)
    fp.zero_grad()
    m.mlm_loss(m(ids, mask), labels).backward()
    assert seen.count(id(table)) == 1
    assert sorted(seen) == sorted(id(p) for p in m.parameters())  # every parameter exactly once
    assert torch.equal(at_hook[0], table.grad)  # nothing lands after the notification
    name = "word_embeddings.weight"
    torch.testing.assert_close(table.grad, gu[name], rtol=1e-3, atol=1e-5)
    nr = gr[name].norm().item()
    e_nat = (table.grad - gr[name]).norm().item() / nr
    e_ac = (ga[name] - gr[name]).norm().item() / nr
    print(f"tied table: native rel err {e_nat:.4f}, autocast {e_ac:.4f}")
    assert e_nat <= max(2.0 * e_ac, 0.02)
    # both contributions are there: the embedding rows (tokens that are no target's label) and the
    # decoder's dense gradient (rows of tokens that never occur in the batch)
    absent = torch.ones(1000, dtype=torch.bool, device=dev)
    absent[ids.view(-1)] = False
    assert float(table.grad[absent].abs().sum()) > 0 and float(gr[name][absent].abs().sum()) > 0


def test_bert_tiny_mlm_trains(dev):
    from ml_trainer_amd.data.text import SyntheticMaskedLM
    from ml_trainer_amd.models.bert import BertForMaskedLM, bert_config
    from ml_trainer_amd.ops.optim import FusedAdamW
    torch.manual_seed(0)
    m = BertForMaskedLM(bert_config("bert-tiny")).to(dev)
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01)
    ds = SyntheticMaskedLM(8, seq_len=128, vocab_size=1000, seed=0)
    ids, labels = ds.ids.to(dev), ds.labels.to(dev)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = m.mlm_loss(m(ids), labels)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < 0.5 * losses[0], losses


def test_trainer_mlm_criterion(dev):
    from ml_trainer_amd.data.text import SyntheticMaskedLM
    from ml_trainer_amd.models.bert import BertForMaskedLM, bert_config
    from ml_trainer_amd.trainer import Trainer
    torch.manual_seed(0)
    m = BertForMaskedLM(bert_config("bert-tiny", max_predictions=8))
    ds = SyntheticMaskedLM(8, seq_len=32, vocab_size=1000, max_predictions=8, seed=0)
    tr = Trainer(m, datasets=(ds, ds), epochs=1, batch_size=4, optimizer="adamw", lr=1e-3, criterion="mlm",
                 metric="accuracy", options={"progress": False})
    assert tr.device.type == "cuda"
    loss = tr.train_step((ds.ids[:4], ds.labels[:4]))
    assert bool(torch.isfinite(loss))
    ev_loss, ev_acc = tr.evaluate()
    assert ev_loss == ev_loss and abs(ev_loss) < float("inf") and 0.0 <= ev_acc <= 1.0
