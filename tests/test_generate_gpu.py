"""Incremental decoding through the whole native model on the GPU: bert-tiny BertLMHeadModel, ids [3, 80], prompt
width 48 with lens [48, 33, 1], teacher-forced for 32 steps (through position 79 of sequence 0), so sequences 0
and 1 cross the 64-key boundary and sequence 2 grows from a single token.

Tolerance: the one the project already uses for native against ``forward_reference``
(tests.test_unpad_gpu._close(..., 5e-2): 5e-2 of the reference's largest magnitude, as in tests/test_clm_gpu.py).

The argmax comparisons hold wherever the reference's top-2 logit gap exceeds twice that allowance. For a randomly
initialised bert-tiny the logits of a step are about 1000 near-Gaussian values of standard deviation 0.33 under a
largest magnitude of 1.6, so the allowance is 0.08 and the top-2 gap (median 0.09) exceeds twice of it at 18 - 25 %
of the 99 positions for every ``mlm_bias`` seed tried (0 .. 3, measured on the CPU reference): a 90 % share cannot
be reached with this fixture, by any seed. ``test_argmax_against_uncached_native`` therefore asserts the equality
at every qualifying position, asserts that some qualify, prints the share, and adds a check that needs no gap and
covers every position: the token either native path picks has a reference logit within twice the allowance of the
reference's best."""
import pytest
import torch

from tests.test_unpad_gpu import _close

pytestmark = pytest.mark.gpu

S, PW, STEPS = 80, 48, 32
PLENS = [48, 33, 1]
TOL = 5e-2


class _Fixture:
    def __init__(self, dev):
        from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
        torch.manual_seed(0)
        self.m = m = BertLMHeadModel(bert_config("bert-tiny")).to(dev).eval()
        with torch.no_grad():
            m.mlm_bias.normal_(std=0.1)
        g = torch.Generator().manual_seed(11)
        self.ids = ids = torch.randint(5, 1000, (3, S), generator=g).to(dev)
        self.plens = pl = torch.tensor(PLENS, device=dev)
        self.prompt = ids[:, :PW].clone()
        self.pmask = (torch.arange(PW, device=dev)[None, :] < pl[:, None]).long()
        # teacher forcing: at step t sequence b is fed ids[b, plen_b + t]; the logits then belong to that position
        self.feed = torch.stack([ids[b, PLENS[b]:PLENS[b] + STEPS] for b in range(3)])  # [3, STEPS]
        flens = pl + STEPS
        fmask = (torch.arange(S, device=dev)[None, :] < flens[:, None]).long()
        # position of the logits after k fed tokens (k = 0: the prompt's last token), as flat rows of [3 * S]
        self.rows = torch.stack([torch.arange(3, device=dev) * S + pl - 1 + k for k in range(STEPS + 1)])
        with torch.no_grad():
            hr = m.forward_reference(ids, fmask)  # fp32 torch, uncached
            self.ref_hidden = hr.view(3 * S, -1)
            self.ref_logits = m.mlm_logits(hr, torch.arange(3 * S, device=dev))
            hn = m(ids, fmask)  # the native uncached forward
            self.nat_logits = m.mlm_logits(hn, torch.arange(3 * S, device=dev))
            self.hidden, self.logits, self.state = self.run()

    def run(self, poison=False):
        """prefill + STEPS teacher-forced decode steps: (hidden [STEPS + 1, 3, h], logits [STEPS + 1, 3, V], state)."""
        m = self.m
        state = m.prefill(self.prompt, self.pmask, max_len=S)
        if poison:
            for kv in state.cache.kv:
                for b, n in enumerate(PLENS):
                    kv[:, b, :, n:] = float("nan")
        hs, ls = [state.hidden.clone()], [m.decode_step(state)]
        for t in range(STEPS):
            ls.append(m.decode_step(state, self.feed[:, t]))
            hs.append(state.hidden.clone())
        return torch.stack(hs), torch.stack(ls), state


@pytest.fixture(scope="module")
def fx():
    return _Fixture(torch.device("cuda", 0))


def test_decode_matches_fp32_reference(fx):
    assert fx.state.pos.tolist() == [n + STEPS for n in PLENS]
    assert fx.logits.dtype == torch.float32 and fx.logits.shape == (STEPS + 1, 3, fx.m.config.vocab_size)
    for k in range(STEPS + 1):
        _close(fx.hidden[k], fx.ref_hidden[fx.rows[k]], TOL)
        _close(fx.logits[k], fx.ref_logits[fx.rows[k]], TOL)


def test_argmax_against_uncached_native(fx):
    rows = fx.rows.reshape(-1)
    ref, nat, dec = fx.ref_logits[rows], fx.nat_logits[rows], fx.logits.reshape(len(rows), -1)
    allow = TOL * float(ref.abs().max())
    top = ref.topk(2, -1).values
    clear = (top[:, 0] - top[:, 1]) > 2 * allow
    share = float(clear.float().mean())
    print(f"top-2 gap > 2 x allowance ({allow:.3f}) at {int(clear.sum())} of {len(rows)} positions ({share:.2f})")
    assert int(clear.sum()) > 0
    assert torch.equal(dec.argmax(-1)[clear], nat.argmax(-1)[clear])
    assert torch.equal(dec.argmax(-1)[clear], ref.argmax(-1)[clear])
    # every position: the picked token is one of the reference's near-best
    for got in (dec, nat):
        picked = ref.gather(1, got.argmax(-1, keepdim=True))[:, 0]
        assert bool((top[:, 0] - picked <= 2 * allow).all())


def test_stale_cache_rows_never_read(fx):
    """Every cache row >= lens[b] poisoned with NaN after prefill: all later logits bitwise equal."""
    _, logits, _ = fx.run(poison=True)
    assert bool(torch.isfinite(logits).all())
    assert torch.equal(logits, fx.logits)


def test_ragged_equals_separate(fx):
    """Sequence 1 decoded alone (B = 1), fed the tokens the batch of 3 generated greedily: its argmax is the
    batch's token wherever the batch's top-2 gap exceeds twice the allowance."""
    m = fx.m
    tok, _, logits = m.generate(fx.prompt, STEPS, attention_mask=fx.pmask, return_logits=True)
    allow = TOL * float(logits.abs().max())
    top = logits[1].topk(2, -1).values
    clear = (top[:, 0] - top[:, 1]) > 2 * allow
    state = m.prefill(fx.prompt[1:2, :PLENS[1]], max_len=S)
    alone = [m.decode_step(state)]
    for t in range(STEPS - 1):
        alone.append(m.decode_step(state, tok[1:2, t]))
    alone = torch.cat(alone)
    same = alone.argmax(-1) == tok[1]
    print(f"alone vs batch: {int(same.sum())} of {STEPS} tokens equal, {int(clear.sum())} clear, bitwise logits "
          f"{torch.equal(alone, logits[1])}")
    assert bool(same[clear].all())
    _close(alone, logits[1], TOL)


def test_generate_modes(fx):
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    m = fx.m
    a, na = m.generate(fx.prompt, 16, attention_mask=fx.pmask)
    b, nb = m.generate(fx.prompt, 16, attention_mask=fx.pmask)
    assert a.shape == (3, 16) and torch.equal(a, b) and torch.equal(na, nb) and not m.training
    kw = dict(attention_mask=fx.pmask, temperature=1.0, top_k=5, seed=7, return_logits=True)
    s1, _, lg = m.generate(fx.prompt, 16, **kw)
    s2, _, _ = m.generate(fx.prompt, 16, **kw)
    assert torch.equal(s1, s2)
    assert bool((lg.topk(5, -1).indices == s1[..., None]).any(-1).all())
    torch.manual_seed(0)
    d = BertLMHeadModel(bert_config("bert-tiny", hidden_dropout=0.1)).to(fx.ids.device)
    d.train()
    t1, _ = d.generate(fx.prompt, 16, attention_mask=fx.pmask)
    assert d.training
    d.eval()
    t2, _ = d.generate(fx.prompt, 16, attention_mask=fx.pmask)
    assert torch.equal(t1, t2)


def test_generate_after_training(dev):
    """Weights living in the flat buffer's bf16 shadow: the setup of test_clm_gpu.test_trainer_clm_criterion."""
    from ml_trainer_amd.data.text import SyntheticCausalLM
    from ml_trainer_amd.models import build_model
    from ml_trainer_amd.trainer import Trainer
    torch.manual_seed(0)
    m = build_model("bert-tiny", task="clm", pad_id=0)
    ds = SyntheticCausalLM(8, seq_len=64, vocab_size=1000, seed=0, min_len=8, pad_id=0)
    tr = Trainer(m, datasets=(ds, ds), epochs=1, batch_size=4, optimizer="adamw", lr=1e-3, criterion="clm",
                 metric="accuracy", options={"progress": False})
    for _ in range(6):
        tr.train_step((ds.ids[:4], ds.labels[:4]))
    model = tr.model
    while not hasattr(model, "generate") and hasattr(model, "module"):
        model = model.module
    was = model.training
    tok, n = model.generate(ds.ids[:4, :8].to(tr.device), 8)
    assert model.training == was
    assert tok.shape == (4, 8) and bool(((tok >= 0) & (tok < 1000)).all()) and n.tolist() == [8, 8, 8, 8]
