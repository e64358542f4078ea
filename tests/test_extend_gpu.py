"""``BertLMHeadModel.extend`` and ``generate(past=)`` through the native model: bert-tiny, ids [3, 80], ``prefill`` on
prompts of width 48 with lens [48, 33, 1], then ``extend`` with T = 20 (two pieces) and counts [20, 7, 13], held against
the uncached fp32 ``forward_reference`` of the full sequences with the project's ``_close(..., 5e-2)``."""
import pytest
import torch

from tests.test_unpad_gpu import _close

pytestmark = pytest.mark.gpu

S, PW, T = 80, 48, 20
PLENS, COUNTS = [48, 33, 1], [20, 7, 13]
TOL = 5e-2


class _Fixture:
    def __init__(self, dev, kw):
        from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
        torch.manual_seed(0)
        self.m = m = BertLMHeadModel(bert_config("bert-tiny", **kw)).to(dev).eval()
        with torch.no_grad():
            m.mlm_bias.normal_(std=0.1)
        self.ids = ids = torch.randint(5, 1000, (3, S), generator=torch.Generator().manual_seed(11)).to(dev)
        self.pl = pl = torch.tensor(PLENS, device=dev)
        self.prompt = ids[:, :PW].clone()
        self.pmask = (torch.arange(PW, device=dev)[None, :] < pl[:, None]).long()
        self.new = torch.stack([ids[b, PLENS[b]:PLENS[b] + T] for b in range(3)])
        fmask = (torch.arange(S, device=dev)[None, :] < (pl + T + 1)[:, None]).long()
        with torch.no_grad():
            hr = m.forward_reference(ids, fmask)
            self.ref_hidden = hr.view(3 * S, -1)
            self.ref_logits = m.mlm_logits(hr, torch.arange(3 * S, device=dev))
        self.base = torch.arange(3, device=dev) * S + pl  # flat row of every sequence's first new token


@pytest.fixture(scope="module", params=[{}, dict(kv_heads=1, rotary=True, pre_ln=True, ffn="swiglu")],
                ids=["plain", "gqa-rope-preln-swiglu"])
def fx(request):
    return _Fixture(torch.device("cuda", 0), request.param)


def test_extend_matches_fp32_reference(fx):
    m, dev = fx.m, fx.ids.device
    state = m.prefill(fx.prompt, fx.pmask, max_len=S)
    counts = torch.tensor(COUNTS, dtype=torch.int32, device=dev)
    logits = m.extend(state, fx.new, counts=counts)
    assert logits.dtype == torch.float32 and logits.shape == (3, T, m.config.vocab_size)
    assert state.pos.tolist() == [n + c for n, c in zip(PLENS, COUNTS)]
    rows = fx.base[:, None] + torch.arange(T, device=dev)[None, :]
    _close(logits, fx.ref_logits[rows.reshape(-1)].view(3, T, -1), TOL)
    _close(state.hidden, fx.ref_hidden[fx.base + counts.long() - 1], TOL)
    # the next token of every sequence: rows past counts[b] were written but are stale, and must not be seen
    nxt = fx.ids[torch.arange(3, device=dev), fx.pl + counts.long()]
    _close(m.decode_step(state, nxt), fx.ref_logits[fx.base + counts.long()], TOL)
    zero = m.extend(state, fx.new[:, :3], counts=torch.zeros(3, dtype=torch.int32, device=dev))
    assert zero.shape[1] == 3 and state.pos.tolist() == [n + c + 1 for n, c in zip(PLENS, COUNTS)]


def test_generate_from_past(fx):
    """A second turn of ragged width through ``generate(past=)``: every picked token is one of the near-best of the
    fp32 reference of the concatenated sequence (the check of test_generate_gpu.test_argmax_against_uncached_native)."""
    m, dev = fx.m, fx.ids.device
    tl, N = [8, 3, 5], 6
    turn = fx.new[:, :8]
    tmask = (torch.arange(8, device=dev)[None, :] < torch.tensor(tl, device=dev)[:, None]).long()
    state = m.prefill(fx.prompt, fx.pmask, max_len=S)
    tok, lengths = m.generate(turn, N, attention_mask=tmask, past=state)
    assert tok.shape == (3, N) and state.pos.tolist() == [p + t + N - 1 for p, t in zip(PLENS, tl)]
    full = fx.ids.clone()
    for b in range(3):
        full[b, PLENS[b] + tl[b]:PLENS[b] + tl[b] + N] = tok[b]
    flens = torch.tensor([p + t + N for p, t in zip(PLENS, tl)], device=dev)
    with torch.no_grad():
        hr = m.forward_reference(full, (torch.arange(S, device=dev)[None, :] < flens[:, None]).long())
        rows = (torch.arange(3, device=dev) * S + flens - N - 1)[:, None] + torch.arange(N, device=dev)[None, :]
        ref = m.mlm_logits(hr, rows.reshape(-1))
    allow = TOL * float(ref.abs().max())
    picked = ref.gather(1, tok.reshape(-1, 1))[:, 0]
    assert bool((ref.max(-1).values - picked <= 2 * allow).all())
    with pytest.raises(ValueError):
        m.generate(turn, N, attention_mask=tmask, past=state, graph=True, sampler="device")
