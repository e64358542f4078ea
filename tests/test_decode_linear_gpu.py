"""Decode steps over ``ops.decode.linear_small`` through the whole native model on the GPU: bert-tiny (hidden 256,
intermediate 1024, padded vocabulary 1024), ids [3, 56], prompt width 48 with lens [48, 33, 1], teacher-forced for 8
steps, as the fixture of tests/test_generate_gpu.py with fewer steps.

Tolerance against ``forward_reference``: the one that file uses (``_close(..., 5e-2)``), with either setting of
``MLT_DECODE_GEMM``.

Batch invariance: with the skinny kernel every kernel of a decode step works row by row (``embed_fwd``, ``ln_fwd``,
``gemm_skinny``) or per (sequence, head) (``attn_decode``), so the logits of a sequence do not depend on the batch it
is decoded in. The prompt runs through ``prefill`` ONCE, as the batch of 3 (the padded forward's GEMMs pick their
kernel by the row count; they are not part of a decode step); sequence 1's cache rows, position and last hidden row
are then copied into a state of its own (B = 1), and both states are fed the same tokens. The B = 1 logits equal
row 1 of the batch's bit for bit at every step, the prompt's included: no top-2-gap condition, no position left out."""
import pytest
import torch

from tests.test_unpad_gpu import _close

pytestmark = pytest.mark.gpu

STEPS, PW = 8, 48
S = PW + STEPS
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
        pl = torch.tensor(PLENS, device=dev)
        self.prompt = ids[:, :PW].clone()
        self.pmask = (torch.arange(PW, device=dev)[None, :] < pl[:, None]).long()
        self.feed = torch.stack([ids[b, PLENS[b]:PLENS[b] + STEPS] for b in range(3)])  # [3, STEPS]
        fmask = (torch.arange(S, device=dev)[None, :] < (pl + STEPS)[:, None]).long()
        self.rows = torch.stack([torch.arange(3, device=dev) * S + pl - 1 + k for k in range(STEPS + 1)])
        with torch.no_grad():  # the fp32 reference, once for every test of the module
            hr = m.forward_reference(ids, fmask)
            self.ref_hidden = hr.view(3 * S, -1)
            self.ref_logits = m.mlm_logits(hr, torch.arange(3 * S, device=dev))

    def decode(self, state, feed):
        """(hidden [STEPS + 1, B, h], logits [STEPS + 1, B, V]) of `state` fed `feed` [B, STEPS]."""
        m = self.m
        hs, ls = [state.hidden.clone()], [m.decode_step(state)]
        for t in range(STEPS):
            ls.append(m.decode_step(state, feed[:, t]))
            hs.append(state.hidden.clone())
        return torch.stack(hs), torch.stack(ls)


@pytest.fixture(scope="module")
def fx():
    return _Fixture(torch.device("cuda", 0))


@pytest.mark.parametrize("setting", ["1", "0"])
def test_decode_matches_fp32_reference(fx, monkeypatch, setting):
    from ml_trainer_amd.ops import decode as DC
    monkeypatch.setenv("MLT_DECODE_GEMM", setting)
    assert DC.decode_linear_path(3, 256, 256) == ("skinny" if setting == "1" else "gemm")
    state = fx.m.prefill(fx.prompt, fx.pmask, max_len=S)
    hidden, logits = fx.decode(state, fx.feed)
    assert state.pos.tolist() == [n + STEPS for n in PLENS]
    assert logits.dtype == torch.float32 and logits.shape == (STEPS + 1, 3, fx.m.config.vocab_size)
    for k in range(STEPS + 1):
        _close(hidden[k], fx.ref_hidden[fx.rows[k]], TOL)
        _close(logits[k], fx.ref_logits[fx.rows[k]], TOL)


def test_alone_equals_its_row_of_the_batch_bitwise(fx, monkeypatch):
    from ml_trainer_amd.ops.decode import DecodeState, KVCache
    monkeypatch.delenv("MLT_DECODE_GEMM", raising=False)
    m = fx.m
    batch = m.prefill(fx.prompt, fx.pmask, max_len=S)
    alone = DecodeState(KVCache([kv[:, 1:2].clone() for kv in batch.cache.kv], batch.cache.pos[1:2].clone(), S),
                        batch.hidden[1:2].clone())
    hb, lb = fx.decode(batch, fx.feed)
    ha, la = fx.decode(alone, fx.feed[1:2])
    assert alone.pos.tolist() == [PLENS[1] + STEPS]
    assert bool(torch.isfinite(la).all())
    for k in range(STEPS + 1):
        assert torch.equal(ha[k, 0].view(torch.int16), hb[k, 1].view(torch.int16)), f"hidden, step {k}"
        assert torch.equal(la[k, 0].view(torch.int32), lb[k, 1].view(torch.int32)), f"logits, step {k}"
    for l in range(len(batch.cache.kv)):  # and the rows the steps appended to the cache
        assert torch.equal(alone.cache.kv[l][:, 0].view(torch.int16), batch.cache.kv[l][:, 1].view(torch.int16))
