"""Incremental decoding on the CPU: the derived bound of the decode attention kernel against a torch emulation
of it (and against three plausible defects), the torch reference of the kernel, the cached model against the
uncached one, generate() and the command line."""
import json

import pytest
import torch

from tests.attn_causal_ref import attn_fwd_bound_masked, causal_valid
from tests.attn_decode_ref import (DECODE_EDGE_CASES, decode_bound, decode_bound_terms, decode_edge_inputs,
                                   decode_effective, emulate_attn_decode)
from tests.test_attn_causal_cpu import _cli

MUTATIONS = ("drop_new_key", "plus_1", "stale_new_key")
S, LENS = 80, [80, 33, 1]


def _case_id(c):
    return f"B{c[0]}H{c[1]}S{c[2]}"


def _ratio(out, O, t):
    """Largest |out - O| / t; inf when any element is not finite."""
    err = (out.double() - O).abs() / t
    return float("inf") if not bool(torch.isfinite(err).all()) else float(err.max())


@pytest.fixture(scope="module")
def edge():
    """Per case: inputs, the fp64 reference and the allowance, computed once."""
    out = {}
    for i, case in enumerate(DECODE_EDGE_CASES):
        B, H, Smax, pos, scale = case
        qkv, kv, p = decode_edge_inputs(case, 100 + i)
        q, k, v = decode_effective(qkv, kv, pos)
        O, t = decode_bound(q, k, v, pos, scale)
        out[case[:3]] = (qkv, kv, p, O.view(B, H * 64), t.view(B, H * 64))
    return out


@pytest.mark.parametrize("case", DECODE_EDGE_CASES, ids=_case_id)
def test_emulation_within_bound(edge, case):
    B, H, Smax, pos, scale = case
    qkv, kv, p, O, t = edge[case[:3]]
    r = _ratio(emulate_attn_decode(qkv, kv, p, H, scale), O, t)
    print(f"decode emulation {_case_id(case)}: max |err| / allowance = {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("mut", MUTATIONS)
def test_mutations_break_the_bound(edge, mut):
    """A loose bound would hide these: each defect must leave the allowance on at least one case."""
    worst = 0.0
    for case in DECODE_EDGE_CASES:
        B, H, Smax, pos, scale = case
        qkv, kv, p, O, t = edge[case[:3]]
        worst = max(worst, _ratio(emulate_attn_decode(qkv, kv, p, H, scale, mut=mut), O, t))
    print(f"{mut}: max |err| / allowance = {worst:.3g}")
    assert worst > 1.0


@pytest.mark.parametrize("case", DECODE_EDGE_CASES, ids=_case_id)
def test_bound_no_looser_than_the_forward(case):
    """Without its merge terms the allowance of query pos[b] does not exceed the causal forward's t_O for the
    same row and keys (attn_fwd_bound_masked at S = pos[b] + 1, last row). Both are fp64 evaluations of their
    formulas, compared with 1e-9 relative slack for the evaluation order."""
    B, H, Smax, pos, scale = case
    qkv, kv, _ = decode_edge_inputs(case, 7)
    q, k, v = decode_effective(qkv, kv, pos)
    _, t_core, t_merge = decode_bound_terms(q, k, v, pos, scale)
    assert bool((t_merge > 0).all())
    for b in range(B):
        n = pos[b] + 1
        qf = torch.zeros(1, H, n, 64, dtype=torch.float64)
        qf[0, :, n - 1] = q[b]
        _, t_fwd, _, _ = attn_fwd_bound_masked(qf, k[b:b + 1, :, :n], v[b:b + 1, :, :n], causal_valid(None, 1, n),
                                               scale)
        assert bool((t_core[b] <= t_fwd[0, :, n - 1] * (1 + 1e-9)).all()), (b, n)


def test_reference_matches_fp64_and_full_forward():
    """attn_decode_reference: within fp32 rounding of the fp64 reference, appends bitwise, and equal to row pos of
    the model's own full causal attention on the same QKV (BertLayer.forward_reference's formulas)."""
    from ml_trainer_amd.ops.decode import attn_decode_reference
    for i, case in enumerate(DECODE_EDGE_CASES):
        B, H, Smax, pos, scale = case
        qkv, kv, p = decode_edge_inputs(case, 40 + i)
        q, k, v = decode_effective(qkv, kv, pos)
        O, t = decode_bound(q, k, v, pos, scale)
        cache = kv.float()
        out = attn_decode_reference(qkv, cache, p, H, scale)
        # fp32 rounding of the plain softmax: the kernel's allowance (the same fp32 score, exponent and sums) plus
        # the probabilities' own division and the Smax-term fp32 P.V accumulation, (Smax + 4) 2^-24 max|v|
        tol = t.view(B, H * 64) + (Smax + 4) * 2.0 ** -24 * float(v.abs().amax())
        assert bool(((out.double() - O.view(B, H * 64)).abs() <= tol).all())
        x = qkv.float().view(B, 3, H, 64)
        for b in range(B):
            assert torch.equal(cache[0, b, :, pos[b]], x[b, 1]) and torch.equal(cache[1, b, :, pos[b]], x[b, 2])
            rest = torch.ones(Smax, dtype=torch.bool)
            rest[pos[b]] = False
            assert torch.equal(cache[:, b][:, :, rest], kv.float()[:, b][:, :, rest])
            # the full causal forward over the pos[b] + 1 rows, fp32 as in BertLayer.forward_reference
            n = pos[b] + 1
            kf, vf = k[b, :, :n].float(), v[b, :, :n].float()
            qf = torch.zeros(H, n, 64)
            qf[:, n - 1] = x[b, 0]
            s = (qf @ kf.transpose(-1, -2)) * scale
            s = s.masked_fill(~torch.ones(n, n, dtype=torch.bool).tril(), float("-inf"))
            full = (s.softmax(-1) @ vf)[:, n - 1].reshape(H * 64)
            assert bool(((out[b] - full).abs().double() <= 2 * tol[b]).all())  # two fp32 evaluations


def test_reference_ignores_nan_in_stale_rows():
    from ml_trainer_amd.ops.decode import attn_decode_reference
    from tests.attn_decode_ref import nan_stale_rows
    case = DECODE_EDGE_CASES[2]
    B, H, Smax, pos, scale = case
    qkv, kv, p = decode_edge_inputs(case, 5)
    a = attn_decode_reference(qkv, kv.float(), p, H, scale)
    b = attn_decode_reference(qkv, nan_stale_rows(kv, pos).float(), p, H, scale)
    assert bool(torch.isfinite(b).all()) and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def model():
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny")).eval()
    with torch.no_grad():
        m.mlm_bias.normal_(std=0.1)
    return m


def _ids():
    g = torch.Generator().manual_seed(11)
    return torch.randint(5, 1000, (len(LENS), S), generator=g)


def test_cached_model_equals_uncached(model):
    """Teacher-forced: prefill on 1 token, then decode_step over every further real position; logits within 2e-5
    (relative to the row's largest magnitude) of the uncached forward_reference, identical argmax, at all 114
    positions."""
    ids = _ids()
    lens = torch.tensor(LENS)
    mask = (torch.arange(S)[None, :] < lens[:, None]).long()
    with torch.no_grad():
        hidden = model.forward_reference(ids, mask)
        ref = model.mlm_logits(hidden, torch.arange(len(LENS) * S)).view(len(LENS), S, -1)
    worst, checked = 0.0, 0
    state = model.prefill(ids[:, :1], max_len=S)
    assert state.pos.tolist() == [1, 1, 1]
    logits = model.decode_step(state)
    for s in range(S):
        if s > 0:
            logits = model.decode_step(state, ids[:, s])
            assert state.pos.tolist() == [s + 1] * 3
        for b, n in enumerate(LENS):
            if s < n:
                r = ref[b, s]
                worst = max(worst, float((logits[b] - r).abs().max() / r.abs().max()))
                assert int(logits[b].argmax()) == int(r.argmax()), (b, s)
                checked += 1
    print(f"cached vs uncached logits: worst relative error {worst:.3g} over {checked} positions")
    assert checked == sum(LENS) == 114
    assert worst <= 2e-5


def _prompt():
    ids = _ids()[:, :16].clone()
    lens = torch.tensor([16, 9, 1])
    mask = (torch.arange(16)[None, :] < lens[:, None]).long()
    return ids, mask


def test_greedy_generate_equals_reference(model):
    ids, mask = _prompt()
    tok, n = model.generate(ids, 24, attention_mask=mask)
    ref, nr = model.generate_reference(ids, 24, attention_mask=mask)
    assert tok.shape == (3, 24) and tok.dtype == torch.int64
    assert torch.equal(tok, ref) and torch.equal(n, nr) and n.tolist() == [24, 24, 24]
    tok2, _ = model.generate(ids, 24, attention_mask=mask)
    assert torch.equal(tok, tok2)


def test_sampling_is_seeded_and_top_k(model):
    ids, mask = _prompt()
    kw = dict(attention_mask=mask, temperature=1.0, top_k=5, seed=7, return_logits=True)
    tok, _, logits = model.generate(ids, 24, **kw)
    tok2, _, _ = model.generate(ids, 24, **kw)
    assert torch.equal(tok, tok2)
    assert logits.shape == (3, 24, model.config.vocab_size)
    top = logits.topk(5, dim=-1).indices
    assert bool((top == tok[..., None]).any(-1).all())
    greedy, _ = model.generate(ids, 24, attention_mask=mask)
    assert not torch.equal(tok, greedy)


def test_eos_pads_the_rest(model):
    from dataclasses import replace
    ids, mask = _prompt()
    greedy, _ = model.generate(ids, 24, attention_mask=mask)
    eos = int(greedy[0, 2])
    cfg = model.config
    try:
        model.config = replace(cfg, pad_id=3)
        tok, n = model.generate(ids, 24, attention_mask=mask, eos_id=eos)
    finally:
        model.config = cfg
    for b in range(3):  # up to and including its first EOS a sequence is the greedy one, then the pad id
        hit = (greedy[b] == eos).nonzero()
        if hit.numel() == 0:
            assert torch.equal(tok[b], greedy[b]) and int(n[b]) == 24
        else:
            e = int(hit[0])
            assert torch.equal(tok[b, :e + 1], greedy[b, :e + 1]) and int(n[b]) == e + 1
            assert bool((tok[b, e + 1:] == 3).all())
    assert int(n[0]) <= 3 and bool((tok[0, 3:] == 3).all())
    tok_np, _ = model.generate(ids, 24, attention_mask=mask, eos_id=eos)  # no pad id: eos fills
    assert bool((tok_np[0, 3:] == eos).all())


def test_generate_errors(model):
    from ml_trainer_amd.models.bert import BertForMaskedLM, bert_config
    ids, mask = _prompt()
    with pytest.raises(ValueError, match="max_position"):
        model.generate(ids, model.config.max_position - 16 + 1)
    with pytest.raises(ValueError, match="max_new_tokens"):
        model.generate(ids, 0)
    with pytest.raises(ValueError, match="temperature"):
        model.generate(ids, 4, temperature=-1.0)
    with pytest.raises(ValueError, match="top_k"):
        model.generate(ids, 4, temperature=1.0, top_k=0)
    assert not hasattr(BertForMaskedLM(bert_config("bert-tiny")), "generate")
    model.generate(ids, model.config.max_position - 16)  # the largest that fits


def test_generate_leaves_the_mode_alone():
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny", hidden_dropout=0.1))
    ids, mask = _prompt()
    m.train()
    a, _ = m.generate(ids, 6, attention_mask=mask)
    assert m.training
    m.eval()
    b, _ = m.generate(ids, 6, attention_mask=mask)
    assert not m.training and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the CLI
def test_cli_generate(tmp_path):
    r = _cli(tmp_path, "--model", "bert-tiny", "--task", "clm", "--generate", "4", "--prompt_len", "4")
    assert r.returncode == 0, r.stderr[-2000:]
    with open(tmp_path / "mo" / "generated.json") as f:
        g = json.load(f)
    assert 1 <= len(g["tokens"]) <= 8 and len(g["tokens"]) == len(g["prompts"])
    assert all(len(row) == 4 for row in g["tokens"]) and all(1 <= len(p) <= 4 for p in g["prompts"])
    assert 0.0 <= g["continuation_accuracy"] <= 1.0


def test_cli_generate_error_cases(tmp_path):
    r = _cli(tmp_path, "--model", "bert-tiny", "--generate", "4")
    assert r.returncode != 0 and "--generate applies to --task clm" in r.stderr
    r = _cli(tmp_path, "--model", "bert-tiny", "--task", "clm", "--generate", "30", "--prompt_len", "4")
    assert r.returncode != 0 and "--prompt_len + --generate" in r.stderr
    r = _cli(tmp_path, "--model", "bert-tiny", "--task", "clm", "--temperature", "0.5")
    assert r.returncode != 0 and "--temperature / --top_k apply to --generate" in r.stderr
