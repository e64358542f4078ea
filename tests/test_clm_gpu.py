"""The causal language-model task on the GPU: a 2-layer, hidden 256, 4-head BertLMHeadModel (bert-tiny) at S = 80
with lens [80, 33, 1], native ``causal=True`` against the fp32 ``forward_reference``, padded and ``unpad``.

Tolerances are those of the same comparison of the non-causal model (tests/test_unpad_gpu.py
test_bert_tiny_unpad_matches_reference, tests/test_mlm_gpu.py test_bert_tiny_mlm_matches_reference): hidden states
within 5e-2 of the reference's largest magnitude (``_close``), the loss within 5e-2 relative, and for every
parameter a native gradient error of at most max(2 x the eager autocast baseline's, 0.02). The causal run needs no
looser ones."""
import pytest
import torch

from tests.test_unpad_gpu import _close

pytestmark = pytest.mark.gpu

S, LENS = 80, [80, 33, 1]


def _batch(dev):
    from ml_trainer_amd.models.bert import shift_labels
    g = torch.Generator().manual_seed(11)
    lens = torch.tensor(LENS)
    ids = torch.randint(5, 1000, (len(LENS), S), generator=g)
    mask = torch.arange(S)[None, :] < lens[:, None]
    labels = shift_labels(ids, lens)
    return ids.to(dev), mask.long().to(dev), labels.to(dev)


def _grads(m, fwd, loss_fn, ids, mask, labels, **kw):
    m.zero_grad(set_to_none=True)
    hidden = fwd(ids, mask, **kw)
    loss = loss_fn(hidden, labels)
    loss.backward()
    return hidden.detach(), loss.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("dropout", [False, True], ids=["plain", "dropout"])
@pytest.mark.parametrize("unpad", [False, True], ids=["padded", "unpad"])
def test_bert_tiny_clm_matches_reference(dev, unpad, dropout):
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    over = dict(hidden_dropout=0.1, attention_dropout=0.1) if dropout else {}
    m = BertLMHeadModel(bert_config("bert-tiny", unpad=unpad, **over)).to(dev)
    assert m.config.causal and m.config.layers == 2 and m.config.hidden == 256 and m.config.heads == 4
    m.train()
    with torch.no_grad():
        m.mlm_bias.normal_(std=0.1)
    ids, mask, labels = _batch(dev)
    targets = int((labels != -100).sum())
    assert targets == sum(n - 1 for n in LENS)
    kw = dict(dropout_seed=4242) if dropout else {}
    hn, ln, gn = _grads(m, m, m.lm_loss, ids, mask, labels, **kw)
    assert int(m.last_mlm_overflow) == 0  # one slot per position: no target is dropped
    acc = float(m.last_mlm_accuracy)
    hr, lr, gr = _grads(m, m.forward_reference, m.lm_loss_reference, ids, mask, labels, **kw)
    assert int(m.last_mlm_overflow) == 0
    _, la, ga = _grads(m, m.forward_torch_bf16, m.mlm_loss_torch_bf16, ids, mask, labels, **kw)
    rows = hr.shape[0]  # unpad: the T real tokens (the native tensor ends in inert tail rows)
    assert rows == (sum(LENS) if unpad else len(LENS) * S)
    _close(hn[:rows], hr, 5e-2)
    print(f"clm loss native {float(ln):.5f} reference {float(lr):.5f} autocast {float(la):.5f} accuracy {acc:.3f}")
    assert abs(float(ln) - float(lr)) <= 5e-2 * abs(float(lr))
    assert 0.0 <= acc <= 1.0
    for n in gr:
        nr = gr[n].norm().item()
        if nr < 1e-8:
            continue
        e_nat = (gn[n] - gr[n]).norm().item() / nr
        e_ac = (ga[n] - gr[n]).norm().item() / nr
        print(f"{n}: native rel err {e_nat:.4f} vs autocast {e_ac:.4f}")
        assert e_nat <= max(2.0 * e_ac, 0.02), f"{n}: native rel err {e_nat:.4f} vs autocast {e_ac:.4f}"


def test_native_hidden_states_ignore_the_future(dev):
    """Through the whole native model: other ids at positions >= 48 (a wave boundary of the attention kernels)
    leave the hidden states of the positions before it bitwise unchanged."""
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny")).to(dev).eval()
    ids, _, _ = _batch(dev)
    ids2 = ids.clone()
    ids2[:, 48:] = torch.randint(5, 1000, (len(LENS), S - 48), generator=torch.Generator().manual_seed(3)).to(dev)
    with torch.no_grad():
        a = m(ids).view(len(LENS), S, -1)
        b = m(ids2).view(len(LENS), S, -1)
    assert torch.equal(a[:, :48], b[:, :48])
    assert not torch.equal(a[:, 48:], b[:, 48:])


def test_trainer_clm_criterion(dev):
    from ml_trainer_amd.data.text import SyntheticCausalLM
    from ml_trainer_amd.models import build_model
    from ml_trainer_amd.trainer import Trainer
    torch.manual_seed(0)
    m = build_model("bert-tiny", task="clm", pad_id=0)
    ds = SyntheticCausalLM(8, seq_len=64, vocab_size=1000, seed=0, min_len=8, pad_id=0)
    tr = Trainer(m, datasets=(ds, ds), epochs=1, batch_size=4, optimizer="adamw", lr=1e-3, criterion="clm",
                 metric="accuracy", options={"progress": False})
    losses = [float(tr.train_step((ds.ids[:4], ds.labels[:4]))) for _ in range(6)]
    assert tr.device.type == "cuda"
    assert all(x == x for x in losses) and losses[-1] < losses[0], losses
    ev_loss, ev_acc = tr.evaluate()
    assert ev_loss == ev_loss and 0.0 <= ev_acc <= 1.0
