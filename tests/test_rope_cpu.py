"""Rotary position embeddings on the CPU: the oracle of ``ops/rope.py`` against a float64 rotation, its identities,
four plausible defects the fixture must tell apart, the state dict and command-line arguments of a rotary model,
and the cached decode path against the uncached ``forward_reference``.

The bound. For a bf16 pair (a, b), the float64 table entry (c64, s64) and the float64 result y64 = a c64 - b s64
(and a s64 + b c64 for the second component), the oracle's stored bf16 value y obeys

    |y - y64| <= 2^-8 |y64| + 2^-22 (|a| + |b|).

Derivation, with u = 2^-24 the unit roundoff of fp32 and |c64|, |s64| <= 1:
  * table: c = c64 (1 + d1), s = s64 (1 + d2), |d| <= u (each entry is rounded once from float64);
  * two products: fl(a c) = a c (1 + e1), fl(b s) = b s (1 + e2), |e| <= u (a bf16 times an fp32 value needs up to 32
    significant bits, so the products do round);
  * one sum: y32 = (fl(a c) - fl(b s)) (1 + e3), |e3| <= u;
  so |y32 - y64| <= ((1 + u)^3 - 1) (|a c64| + |b s64|) <= t with t = 3 u (1 + 2 u) (|a| + |b|);
  * the bf16 store: bf16 keeps 8 significant bits, so |y - y32| <= 2^-8 |y32| <= 2^-8 (|y64| + t).
Together |y - y64| <= 2^-8 |y64| + (1 + 2^-8) t, and (1 + 2^-8) 3 (1 + 2 u) 2^-24 < 4 * 2^-24 = 2^-22: the fp32 term
has a quarter to spare. The largest ratio the test prints is 0.996, set by the bf16 store of values just above a
power of two, where the 2^-8 is attained.

sign = -1 after sign = +1: the first pass leaves x' = R x + e1 with |e1| <= bound(x) per component, the second
x'' = R^-1 x' + e2 with |e2| <= bound(x') (the same bound at the rotated values). R^-1 turns e1 into a vector whose
components are at most |e1_a| + |e1_b| (|c|, |s| <= 1), and R^-1 R is the identity up to the table's own rounding
(|c^2 + s^2 - 1| <= 4 u, on both components: 8 u (|a| + |b|)). Hence
    |x'' - x| <= (bound_a(x) + bound_b(x)) + bound(x') + 2^-21 (|a| + |b|): "the same bound applied twice".
"""
import pytest
import torch

from tests.test_attn_causal_cpu import _cli

BF16 = torch.bfloat16
P = 4096
H = 4


def _fixture():
    """x bf16 [rows, 3 * H * 64] with q | k | v, positions int64 [rows] up to P - 1 (0 and P - 1 included), the fp32
    table and the float64 table."""
    from ml_trainer_amd.ops import rope as R
    g = torch.Generator().manual_seed(0)
    rows = 1667  # x 2 x 4 heads x 64 dims = 853,504 rotated elements, plus the magnitudes below
    x = torch.randn(rows, 3 * H * 64, generator=g)
    x[:200] *= torch.exp2(torch.randint(-30, 31, (200, 1), generator=g).float())
    pos = torch.randint(0, P, (rows,), generator=g)
    pos[0], pos[1], pos[2], pos[3] = 0, P - 1, 1, 1
    return x.to(BF16), pos, R.rope_table(P), R.rope_table64(P)


@pytest.fixture(scope="module")
def fx():
    return _fixture()


def _rot64(x, t64, pos, sign=1, half_split=False):
    """float64 rotation of the [rows, n * 64] columns ``x`` at ``pos`` with the float64 table (``half_split``: pair
    i is dims (i, i + 32), the other common layout)."""
    rows = x.shape[0]
    v = x.double().view(rows, -1, 64)
    cs = t64[pos][:, None]
    c, s = cs[..., 0], cs[..., 1] * sign
    if half_split:
        a, b = v[..., :32], v[..., 32:]
        return torch.cat((a * c - b * s, a * s + b * c), -1).reshape(rows, -1)
    a, b = v[..., 0::2], v[..., 1::2]
    return torch.stack((a * c - b * s, a * s + b * c), -1).reshape(rows, -1)


def bound(x, y64):
    """2^-8 |y64| + 2^-22 (|a| + |b|) per element; ``x`` the (bf16) inputs whose pairs are (a, b)."""
    v = x.double().view(x.shape[0], -1, 2).abs().sum(-1, keepdim=True).expand(-1, -1, 2).reshape(x.shape)
    return 2.0 ** -8 * y64.abs() + 2.0 ** -22 * v


def _worst(y, y64, tol):
    return float(((y.double() - y64).abs() / tol.clamp_min(1e-300)).max())


def test_oracle_within_the_derived_bound(fx):
    from ml_trainer_amd.ops import rope as R
    x, pos, table, t64 = fx
    D = H * 64
    assert table.dtype == torch.float32 and tuple(table.shape) == (P, 32, 2)
    assert torch.equal(table, t64.float())  # each entry rounded once from float64
    assert R.rope_table(P) is table  # cached: one tensor per (P, base, device)
    for sign in (1, -1):
        y = R.rope_qk_reference(x, table, H, pos=pos, sign=sign)
        assert y.dtype == BF16
        y64 = _rot64(x[:, :2 * D], t64, pos, sign)
        r = _worst(y[:, :2 * D], y64, bound(x[:, :2 * D], y64))
        print(f"sign {sign:+d}: max |y - y64| / bound = {r:.3f} over {y64.numel()} elements")
        assert r <= 1.0
        assert torch.equal(y[:, 2 * D:].view(torch.int16), x[:, 2 * D:].view(torch.int16))  # v untouched


def test_position_zero_and_implicit_positions(fx):
    from ml_trainer_amd.ops import rope as R
    x, pos, table, _ = fx
    zero = torch.zeros_like(pos)
    assert torch.equal(R.rope_qk_reference(x, table, H, pos=zero), x)
    assert torch.equal(R.rope_qk_reference(x, table, H, S=1), x)  # row % 1 == 0
    rows = x.shape[0]
    for S in (5, 80):
        want = R.rope_qk_reference(x, table, H, pos=torch.arange(rows) % S)
        assert torch.equal(R.rope_qk_reference(x, table, H, S=S), want)
    # explicit positions are clamped into the table, as the kernels clamp them
    far = pos.clone()
    far[:4] = torch.tensor([-5, P, P + 100, -1])
    assert torch.equal(R.rope_qk_reference(x, table, H, pos=far), R.rope_qk_reference(x, table, H, pos=far.clamp(0, P - 1)))
    with pytest.raises(ValueError):
        R.rope_qk_reference(x, table, H, S=P + 1)


def test_inverse_after_forward_within_the_bound_applied_twice(fx):
    from ml_trainer_amd.ops import rope as R
    x, pos, table, t64 = fx
    D = H * 64
    y = R.rope_qk_reference(x, table, H, pos=pos)
    z = R.rope_qk_reference(y, table, H, pos=pos, sign=-1)
    xq, yq = x[:, :2 * D], y[:, :2 * D]
    b1 = bound(xq, _rot64(xq, t64, pos))
    b1 = b1.view(-1, 2).sum(-1, keepdim=True).expand(-1, 2).reshape(b1.shape)  # |e1_a| + |e1_b|
    b2 = bound(yq, _rot64(yq, t64, pos, -1))
    mag = xq.double().view(-1, 2).abs().sum(-1, keepdim=True).expand(-1, 2).reshape(xq.shape)
    r = _worst(z[:, :2 * D], xq.double(), b1 + b2 + 2.0 ** -21 * mag)
    print(f"inverse after forward: max |x'' - x| / allowance = {r:.3f}")
    assert r <= 1.0
    assert not torch.equal(z[:, :2 * D], xq)  # two roundings: not an identity in bf16


def test_scores_depend_on_relative_position_only():
    """float64: q_i . k_j after rotation is unchanged by a common shift of all positions."""
    from ml_trainer_amd.ops import rope as R
    g = torch.Generator().manual_seed(3)
    S, shift = 64, 1000
    t64 = R.rope_table64(S + shift)
    q = torch.randn(S, 64, generator=g, dtype=torch.float64)
    k = torch.randn(S, 64, generator=g, dtype=torch.float64)
    p0 = torch.arange(S)
    s0 = _rot64(q, t64, p0) @ _rot64(k, t64, p0).T
    s1 = _rot64(q, t64, p0 + shift) @ _rot64(k, t64, p0 + shift).T
    err = float((s0 - s1).abs().max())
    print(f"scores under a shift of {shift}: max difference {err:.3g}")
    assert err <= 1e-10
    assert float((s0 - q @ k.T).abs().max()) > 0.1  # and the rotation does something


MUTANTS = ("half_split", "rotate_v", "pos_plus_1", "backward_keeps_sin")


def _mutant(name, x, table, pos, sign):
    """The oracle with one plausible defect built in."""
    from ml_trainer_amd.ops import rope as R
    D = H * 64
    if name == "half_split":
        t = table.double()
        out = x.clone()
        out[:, :2 * D] = _rot64(x[:, :2 * D], t, pos, sign, half_split=True).float().to(BF16)
        return out
    if name == "rotate_v":
        out = R.rope_qk_reference(x, table, H, pos=pos, sign=sign)
        out[:, 2 * D:] = R.rope_heads(x[:, 2 * D:], table, pos, sign)
        return out
    if name == "pos_plus_1":
        return R.rope_qk_reference(x, table, H, pos=(pos + 1).clamp(max=P - 1), sign=sign)
    if name == "backward_keeps_sin":
        return R.rope_qk_reference(x, table, H, pos=pos, sign=1)
    raise KeyError(name)


@pytest.mark.parametrize("mut", MUTANTS)
def test_mutants_leave_the_bound(fx, mut):
    """Each defect must show in the checks the kernels are held to: the q / k columns against the float64 rotation
    within the bound, the v columns bit for bit; forward and backward sign."""
    x, pos, table, t64 = fx
    D = H * 64
    caught = []
    for sign in (1, -1):
        y = _mutant(mut, x, table, pos, sign)
        y64 = _rot64(x[:, :2 * D], t64, pos, sign)
        r = _worst(y[:, :2 * D], y64, bound(x[:, :2 * D], y64))
        v_same = torch.equal(y[:, 2 * D:].view(torch.int16), x[:, 2 * D:].view(torch.int16))
        print(f"{mut} sign {sign:+d}: max |y - y64| / bound = {r:.3g}, v untouched {v_same}")
        caught.append(r > 1.0 or not v_same)
    assert caught[1] if mut == "backward_keeps_sin" else all(caught)


# ------------------------------------------------------------------------------------------------ the model
_LAYER = ["qkv.weight", "qkv.bias", "out.weight", "out.bias", "ln1.weight", "ln1.bias", "ffn1.weight", "ffn1.bias",
          "ffn2.weight", "ffn2.bias", "ln2.weight", "ln2.bias"]
# the state-dict keys of a bert-tiny BertLMHeadModel before rotary positions existed, in order
LEARNED_KEYS = (["mlm_bias", "word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight",
                 "emb_ln.weight", "emb_ln.bias"] + [f"layers.{l}.{k}" for l in range(2) for k in _LAYER] +
                ["mlm_dense.weight", "mlm_dense.bias", "mlm_ln.weight", "mlm_ln.bias"])


def test_state_dict_and_config():
    from ml_trainer_amd.models.bert import (BertClassifier, BertConfig, BertForMaskedLM, BertLMHeadModel,
                                            bert_config)
    assert BertConfig().rotary is False and BertConfig().rope_base == 10000.0
    plain = BertLMHeadModel(bert_config("bert-tiny"))
    keys = list(plain.state_dict())
    assert keys == LEARNED_KEYS and plain.rope_table is None
    rot = BertLMHeadModel(bert_config("bert-tiny", rotary=True))
    assert list(rot.state_dict()) == [k for k in keys if k != "position_embeddings.weight"]
    assert rot.position_embeddings is None and not any("position" in n for n, _ in rot.named_parameters())
    assert tuple(rot.rope_table.shape) == (rot.config.max_position, 32, 2) and rot.rope_table.dtype == torch.float32
    assert "rope_table" in dict(rot.named_buffers())
    # a learned-position checkpoint loads into a rotary model but for the one key, and back
    missing = rot.load_state_dict(plain.state_dict(), strict=False)
    assert missing.unexpected_keys == ["position_embeddings.weight"] and not missing.missing_keys
    for cls in (BertClassifier, BertForMaskedLM):
        assert "position_embeddings.weight" not in cls(bert_config("bert-tiny", rotary=True)).state_dict()
    other = BertLMHeadModel(bert_config("bert-tiny", rotary=True, rope_base=500.0))
    assert not torch.equal(other.rope_table, rot.rope_table)
    with pytest.raises(ValueError, match="rotary"):
        BertClassifier(bert_config("bert-tiny", rotary=True, fp8=True))


def test_reference_paths_agree_and_depend_on_order():
    """Rotary, padded against packed forward_reference (float64: the same function), and the eager bf16 baseline
    against forward_reference; without any position information a causal model could not tell a swap of two
    earlier tokens, with rotary positions it does."""
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny", rotary=True, pad_id=0)).double().eval()
    u = BertLMHeadModel(bert_config("bert-tiny", rotary=True, pad_id=0, unpad=True)).double().eval()
    u.load_state_dict(m.state_dict())
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(5, 1000, (3, 24), generator=g)
    lens = [24, 9, 1]
    for b, n in enumerate(lens):
        ids[b, n:] = 0
    with torch.no_grad():
        hp = m.forward_reference(ids)
        hu = u.forward_reference(ids)
        keep = (ids != 0).view(-1).nonzero().view(-1)
        assert float((hp[keep] - hu).abs().max()) <= 1e-12
        f = m.float()
        h32 = f.forward_reference(ids)
        hb = f.forward_torch_bf16(ids)
        assert float((hb.float() - h32).abs().max()) <= 5e-2 * float(h32.abs().max())
        swapped = ids.clone()
        swapped[0, 2], swapped[0, 3] = ids[0, 3], ids[0, 2]
        hs = f.forward_reference(swapped)
        assert float((hs[23] - h32[23]).abs().max()) > 1e-4  # row 23 sees both tokens, in another order


S, PW, STEPS = 80, 48, 32
PLENS = [48, 33, 1]


def test_cached_rotary_model_equals_uncached():
    """bert-tiny rotary on the CPU path: prompts of lengths [48, 33, 1], 32 teacher-forced decode steps; the logits
    of every step within 2e-5 (relative to the row's largest magnitude: the tolerance of
    tests/test_attn_decode_cpu.py for the learned-position model) of forward_reference over the full sequences."""
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny", rotary=True)).eval()
    with torch.no_grad():
        m.mlm_bias.normal_(std=0.1)
    ids = torch.randint(5, 1000, (3, S), generator=torch.Generator().manual_seed(11))
    pl = torch.tensor(PLENS)
    pmask = (torch.arange(PW)[None, :] < pl[:, None]).long()
    fmask = (torch.arange(S)[None, :] < (pl + STEPS)[:, None]).long()
    with torch.no_grad():
        ref = m.mlm_logits(m.forward_reference(ids, fmask), torch.arange(3 * S)).view(3, S, -1)
    state = m.prefill(ids[:, :PW].clone(), pmask, max_len=S)
    assert state.pos.tolist() == PLENS
    worst = 0.0
    logits = m.decode_step(state)
    for t in range(STEPS + 1):
        if t > 0:
            logits = m.decode_step(state, torch.stack([ids[b, PLENS[b] + t - 1] for b in range(3)]))
        for b, n in enumerate(PLENS):
            r = ref[b, n - 1 + t]
            worst = max(worst, float((logits[b] - r).abs().max() / r.abs().max()))
            assert int(logits[b].argmax()) == int(r.argmax()), (b, t)
    print(f"rotary cached vs uncached logits: worst relative error {worst:.3g} over {3 * (STEPS + 1)} positions")
    assert state.pos.tolist() == [n + STEPS for n in PLENS]
    assert worst <= 2e-5
    # and generate() against the uncached generate_reference, greedy
    tok, n = m.generate(ids[:, :PW].clone(), 8, attention_mask=pmask)
    rtok, rn = m.generate_reference(ids[:, :PW].clone(), 8, attention_mask=pmask)
    assert torch.equal(tok, rtok) and torch.equal(n, rn)


def test_native_blocks_reject_rotary_with_fp8():
    from ml_trainer_amd.ops import transformer as T

    class NotBf16:
        pass

    with pytest.raises(ValueError, match="rotary"):
        T._attn_fwd(None, None, None, None, None, None, 1, 1, 1, impl=NotBf16(), rope=(None, None))


# ------------------------------------------------------------------------------------------------ the CLI
def test_main_rotary_argument_errors():
    """main.py's own checks, in process (the parser and build_model_and_datasets are what the command line runs)."""
    import main

    def build(*flags):
        return main.build_model_and_datasets(main.build_parser().parse_args(["--synthetic", "--synthetic_size", "16",
                                                                             "--seq_len", "32", *flags]))

    with pytest.raises(ValueError, match="--rotary / --rope_base apply to the BERT models"):
        build("--model", "default", "--rotary")
    with pytest.raises(ValueError, match="--rotary / --rope_base apply to the BERT models"):
        build("--model", "tiny", "--rope_base", "500")
    with pytest.raises(ValueError, match="rotary=True with fp8=True"):
        build("--model", "large", "--rotary")
    with pytest.raises(ValueError, match="--rope_base applies to --rotary"):
        build("--model", "bert-tiny", "--rope_base", "500")
    with pytest.raises(ValueError, match="--rope_base must be > 0"):
        build("--model", "bert-tiny", "--rotary", "--rope_base", "0")
    for task in ("classify", "mlm", "clm"):
        model, _ = build("--model", "bert-tiny", "--rotary", "--rope_base", "500", "--task", task)
        assert model.config.rotary and model.config.rope_base == 500.0 and model.position_embeddings is None
    model, _ = build("--model", "bert-tiny")
    assert not model.config.rotary and model.position_embeddings is not None


def test_cli_rotary_clm_trains_and_generates(tmp_path):
    r = _cli(tmp_path, "--model", "bert-tiny", "--task", "clm", "--rotary", "--rope_base", "500", "--generate", "4",
             "--prompt_len", "4")
    assert r.returncode == 0, r.stderr[-2000:]
    sd = torch.load(tmp_path / "mo" / "model.pth", weights_only=True)
    assert "position_embeddings.weight" not in sd and "word_embeddings.weight" in sd
    assert not any("rope" in k for k in sd)
