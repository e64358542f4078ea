"""Rotary position embeddings on the GPU.

* ``rope_qk`` (csrc/kernels/rope.hip) against the torch oracle of ``ops/rope.py``, bit for bit, forward and backward
  sign, implicit and explicit positions, in guarded row-strided buffers whose v columns and guard hold NaN / Inf.
* ``embed_fwd`` / ``embed_bwd`` without a position table against a run that passes a table of zeros.
* The ROPE instantiation of ``attn_decode`` against ``rope_qk`` followed by the plain ``attn_decode``, bit for bit.
* The whole model: bert-tiny ``BertLMHeadModel(rotary=True)``, training (fixture and thresholds of
  tests/test_clm_gpu.py) and decoding (fixture and tolerance of tests/test_generate_gpu.py).

The QKV bias gradient. The attention backward kernels can sum dQKV over the rows themselves, but under rotary
positions that sum is taken in the rotated frame and is wrong for the q and k thirds of the bias. A throw-away run
on the CPU oracle (``forward_reference``; padded, no dropout) replaced the q and k thirds of the true bias gradient
by the column sums of dq' and dk' (the rotated frame). With the fixture of tests/test_clm_gpu.py as it is, that
vector is off by a relative 0.0141 (layers.0.qkv.bias) and 0.0152 (layers.1.qkv.bias), BELOW the threshold
max(2 x autocast's, 0.02) = 0.02 (autocast's error there: 0.0063 / 0.0066): a freshly initialised model has
near-uniform attention, and the q and k thirds carry 1.6 % of the gradient's norm. The fixture here therefore
ENLARGES the q / k bias gradient: the q and k rows of every layer's QKV weight are multiplied by ``QK_GAIN`` = 4 and
the q and k thirds of the bias are drawn from N(0, 0.08^2). The same throw-away run then gives 0.0802 and 0.0909
(the q and k thirds carry 8.6 % of the norm; autocast's error 0.0065 / 0.0072), four times the threshold:
``test_bert_tiny_rotary_clm_matches_reference`` asserts that both names were compared.
"""
import pytest
import torch

from tests import helpers as H
from tests.test_unpad_gpu import _close

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
P = 128  # table rows of the kernel tests


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


# ------------------------------------------------------------------------------------------------ rope_qk
def _qk_values(rows, cols, g):
    """bf16 [rows, cols]: sign * 2^e * (1 + m / 128) with e uniform in -60 .. 60, and every 7th element +0 or -0."""
    e = torch.randint(-60, 61, (rows, cols), generator=g).double()
    m = torch.randint(0, 128, (rows, cols), generator=g).double()
    sgn = torch.randint(0, 2, (rows, cols), generator=g).double() * 2 - 1
    x = (sgn * torch.exp2(e) * (1 + m / 128)).to(BF16)
    flat = x.view(-1)
    flat[::7] = 0.0
    flat[::14] = -0.0
    return x


def _v_values(rows, cols, g):
    """bf16 [rows, cols] of the v columns: random, with NaN and +-Inf planted (nothing may read or write them)."""
    v = torch.randn(rows, cols, generator=g).to(BF16)
    flat = v.view(-1)
    flat[::5] = float("nan")
    flat[1::11] = float("inf")
    flat[2::13] = float("-inf")
    return v


def _explicit_positions(rows, g):
    """int32 [rows]: random positions in [0, P) that include 0, P - 1 and repeats; from 8 rows on also a -1 and a
    P + 7, which every build clamps to 0 and P - 1."""
    pos = torch.randint(0, P, (rows,), generator=g, dtype=torch.int32)
    fixed = [0, P - 1, P - 1, 0, 5, 5]
    if rows >= 8:
        fixed += [-1, P + 7]
    for i, v in enumerate(fixed[:rows]):
        pos[(i * 3) % rows] = v
    if rows == 1:
        pos[0] = P - 1
    return pos


@pytest.mark.parametrize("heads", [1, 4, 12])
@pytest.mark.parametrize("rows", [1, 3, 67, 300])
def test_rope_qk_equals_the_oracle_bitwise(dev, rows, heads):
    from ml_trainer_amd.ops import rope as R
    C = R.require_native()
    D = heads * 64
    table_cpu = R.rope_table(P, 10000.0, "cpu")
    table = R.rope_table(P, 10000.0, dev)
    assert torch.equal(table.cpu(), table_cpu) and table.dtype == torch.float32 and tuple(table.shape) == (P, 32, 2)
    g = torch.Generator().manual_seed(1000 * rows + heads)
    extra = 2  # data rows past `rows` that the kernel is not given
    data = torch.cat((_qk_values(rows + extra, 2 * D, g), _v_values(rows + extra, D, g)), 1)
    ld, off = 3 * D + 24, 8  # row stride > 3D, a column offset; (ld + off) % 8 == 0 keeps the 16-byte rule
    modes = [("S1", dict(S=1)), ("S5", dict(S=5)), ("S80", dict(S=80)), ("pos", dict(pos=_explicit_positions(rows, g)))]
    for name, kw in modes:
        for sign in (1, -1):
            buf, view = H.guarded_like(data.to(dev), ld=ld, col_off=off)
            before = buf.clone()
            pos = kw.get("pos")
            C.rope_qk(view[:rows], table, heads, kw.get("S", 1), pos=None if pos is None else pos.to(dev), sign=sign)
            torch.cuda.synchronize()
            want = R.rope_qk_reference(data[:rows], table_cpu, heads, kw.get("S", 1), pos=pos, sign=sign)
            expect = before.cpu()
            expect[1:1 + rows, off:off + 2 * D] = want[:, :2 * D]
            what = f"rows {rows} H {heads} {name} sign {sign}"
            # the guard rows and columns, the v columns (NaN / Inf included) and the rows past `rows`: bit for bit
            assert torch.equal(_bits(buf.cpu()), _bits(expect)), what
            assert torch.equal(_bits(want[:, 2 * D:]), _bits(data[:rows, 2 * D:])), what  # the oracle leaves v alone too
            H.assert_guard_intact(buf, buf[1:1 + rows + extra, off:off + 3 * D])


def test_rope_qk_position_zero_returns_the_input(dev):
    from ml_trainer_amd.ops import rope as R
    C = R.require_native()
    heads, rows = 4, 67
    D = heads * 64
    g = torch.Generator().manual_seed(5)
    x = torch.cat((torch.randn(rows, 2 * D, generator=g), torch.randn(rows, D, generator=g)), 1).to(BF16).to(dev)
    table = R.rope_table(P, 10000.0, dev)
    y = x.clone()
    C.rope_qk(y, table, heads, 1)  # S = 1: every row at position 0
    assert torch.equal(_bits(y), _bits(x))
    pos = torch.randint(0, P, (rows,), generator=g, dtype=torch.int32).to(dev)
    C.rope_qk(y, table, heads, 1, pos=pos)
    assert not torch.equal(_bits(y), _bits(x))
    assert torch.equal(_bits(y[:, 2 * D:]), _bits(x[:, 2 * D:]))


def test_rope_qk_rejections(dev):
    from ml_trainer_amd.ops import rope as R
    C = R.require_native()
    table = R.rope_table(P, 10000.0, dev)
    x = torch.zeros(4, 3 * 64, dtype=BF16, device=dev)
    with pytest.raises(RuntimeError):
        C.rope_qk(x, table, 1, P + 1)  # implicit positions past the table
    with pytest.raises(RuntimeError):
        C.rope_qk(x, table, 2, 1)  # 3 * H * 64 columns expected
    with pytest.raises(RuntimeError):
        C.rope_qk(x, table, 1, 1, sign=0)
    with pytest.raises(RuntimeError):
        C.rope_qk(x, table, 1, 1, pos=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError):
        C.rope_qk(x.float(), table, 1, 1)


# ------------------------------------------------------------------------------------------------ embeddings
@pytest.mark.parametrize("D", [256, 768])
@pytest.mark.parametrize("name", [c[0] for c in H.ROWK_EMBED_CASES])
def test_embeddings_without_a_position_table(dev, name, D):
    from ml_trainer_amd.ops._ext import require_native
    C = require_native()
    c = H.embed_edge_inputs(name, D, seed=D + len(name))
    c = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
    B, S, V, ids, tt = c["B"], c["S"], c["V"], c["ids"], c["tt"]
    n = B * S
    ww, wt, dout = c["ww"], c["wt"], c["dout"]
    wp0 = torch.zeros_like(c["wp"])
    outs = []
    for wp in (wp0, None):
        buf, out = H.guarded(n, D, BF16, dev)
        C.embed_fwd(ids, tt, ww, wp, wt, out, S)
        torch.cuda.synchronize()
        H.assert_guard_intact(buf, out)
        outs.append(out)
    exp, t = H.embed_fwd_bound(ww, wp0, wt, ids, tt, S)
    for out in outs:
        H.assert_within(out, exp, H.store_bound(exp, t, BF16), f"embed_fwd {name} D{D}")
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    sid, perm = torch.sort(ids.clamp(0, V - 1), stable=True)
    res = []
    for with_table in (True, False):
        gw, gt = c["gw0"].clone(), c["gt0"].clone()
        gp = c["gp0"].clone() if with_table else None
        pbuf, part = H.guarded_1d(S * 2 * D, dev)
        C.embed_bwd(sid, perm, tt, dout, gw, gp, gt, part, S)
        torch.cuda.synchronize()
        H.assert_guard_intact(pbuf, part)
        res.append((gw, gt))
    b = H.embed_bwd_bound(dout, ids.clamp(0, V - 1), tt, B, S, c["gw0"], c["gp0"], c["gt0"])
    for gw, gt in res:
        H.assert_within(gw, b["gw"], b["t_gw"], f"embed_bwd gw {name} D{D}")
        H.assert_within(gt, b["gt"], b["t_gt"], f"embed_bwd gt {name} D{D}")
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])) and torch.equal(_bits(res[0][1]), _bits(res[1][1]))


# ------------------------------------------------------------------------------------------------ attn_decode
def test_attn_decode_rope_equals_rope_qk_then_attn_decode(dev):
    from ml_trainer_amd.ops import decode as DC
    from ml_trainer_amd.ops import rope as R
    from tests.attn_decode_ref import decode_edge_inputs, nan_stale_rows
    case = (3, 4, 80, [0, 63, 79], 0.125)
    B, heads, Smax, pos, scale = case
    qkv, kv, p = decode_edge_inputs(case, 77)
    kv = nan_stale_rows(kv, pos)
    table = R.rope_table(P, 10000.0, dev)
    qkv, p = qkv.to(dev), p.to(dev)
    kv_a, kv_b = kv.to(dev), kv.to(dev)
    out_a = DC.attn_decode(qkv, kv_a, p, heads, scale, rope=table)
    rot = R.rope_qk(qkv.clone(), table, heads, 1, pos=p)
    assert not torch.equal(_bits(rot), _bits(qkv))
    out_b = DC.attn_decode(rot, kv_b, p, heads, scale)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out_a).all())
    assert torch.equal(_bits(out_a), _bits(out_b))
    assert torch.equal(_bits(kv_a), _bits(kv_b))  # the whole cache: the appended rows and the NaN rows above them
    for b, n in enumerate(pos):  # the appended key is the rotated one, the value the plain one
        assert torch.equal(_bits(kv_a[0, b, :, n]), _bits(rot[b, heads * 64:2 * heads * 64].view(heads, 64)))
        assert torch.equal(_bits(kv_a[1, b, :, n]), _bits(qkv[b, 2 * heads * 64:].view(heads, 64)))
    with pytest.raises(RuntimeError):  # a table shorter than the cache
        DC.attn_decode(qkv, kv_a, p, heads, scale, rope=R.rope_table(Smax - 1, 10000.0, dev))


# ------------------------------------------------------------------------------------------------ training
S, LENS = 80, [80, 33, 1]
QK_GAIN = 4.0  # see the module docstring: the q / k bias gradient of the fixture, enlarged


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
def test_bert_tiny_rotary_clm_matches_reference(dev, unpad, dropout):
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    over = dict(hidden_dropout=0.1, attention_dropout=0.1) if dropout else {}
    m = BertLMHeadModel(bert_config("bert-tiny", rotary=True, unpad=unpad, **over)).to(dev)
    assert m.config.rotary and m.config.causal and m.position_embeddings is None
    assert not any("position" in k or "rope" in k for k in m.state_dict())
    assert m.rope_table.device.type == "cuda" and m.rope_table.dtype == torch.float32
    m.train()
    with torch.no_grad():
        m.mlm_bias.normal_(std=0.1)
        for L in m.layers:
            L.qkv.weight[:2 * m.config.hidden] *= QK_GAIN
            L.qkv.bias[:2 * m.config.hidden].normal_(std=0.02 * QK_GAIN)
    ids, mask, labels = _batch(dev)
    kw = dict(dropout_seed=4242) if dropout else {}
    hn, ln, gn = _grads(m, m, m.lm_loss, ids, mask, labels, **kw)
    assert int(m.last_mlm_overflow) == 0
    hr, lr, gr = _grads(m, m.forward_reference, m.lm_loss_reference, ids, mask, labels, **kw)
    _, la, ga = _grads(m, m.forward_torch_bf16, m.mlm_loss_torch_bf16, ids, mask, labels, **kw)
    rows = hr.shape[0]
    assert rows == (sum(LENS) if unpad else len(LENS) * S)
    _close(hn[:rows], hr, 5e-2)
    print(f"rotary clm loss native {float(ln):.5f} reference {float(lr):.5f} autocast {float(la):.5f}")
    assert abs(float(ln) - float(lr)) <= 5e-2 * abs(float(lr))
    checked = set()
    for n in gr:
        nr = gr[n].norm().item()
        if nr < 1e-8:
            continue
        e_nat = (gn[n] - gr[n]).norm().item() / nr
        e_ac = (ga[n] - gr[n]).norm().item() / nr
        print(f"{n}: native rel err {e_nat:.4f} vs autocast {e_ac:.4f}")
        assert e_nat <= max(2.0 * e_ac, 0.02), f"{n}: native rel err {e_nat:.4f} vs autocast {e_ac:.4f}"
        checked.add(n)
    # the bias whose fused gradient would be a sum in the rotated frame (see the module docstring)
    assert {"layers.0.qkv.bias", "layers.1.qkv.bias"} <= checked


# ------------------------------------------------------------------------------------------------ decoding
PW, STEPS = 48, 32
PLENS = [48, 33, 1]
TOL = 5e-2


class _Fixture:
    def __init__(self, dev):
        from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
        torch.manual_seed(0)
        self.m = m = BertLMHeadModel(bert_config("bert-tiny", rotary=True, max_position=128)).to(dev).eval()
        with torch.no_grad():
            m.mlm_bias.normal_(std=0.1)
        g = torch.Generator().manual_seed(11)
        self.ids = ids = torch.randint(5, 1000, (3, S), generator=g).to(dev)
        self.plens = pl = torch.tensor(PLENS, device=dev)
        self.prompt = ids[:, :PW].clone()
        self.pmask = (torch.arange(PW, device=dev)[None, :] < pl[:, None]).long()
        self.feed = torch.stack([ids[b, PLENS[b]:PLENS[b] + STEPS] for b in range(3)])  # [3, STEPS]
        fmask = (torch.arange(S, device=dev)[None, :] < (pl + STEPS)[:, None]).long()
        self.rows = torch.stack([torch.arange(3, device=dev) * S + pl - 1 + k for k in range(STEPS + 1)])
        with torch.no_grad():
            hr = m.forward_reference(ids, fmask)  # fp32 torch, uncached: once for the module
            self.ref_hidden = hr.view(3 * S, -1)
            self.ref_logits = m.mlm_logits(hr, torch.arange(3 * S, device=dev))
            hn = m(ids, fmask)
            self.nat_logits = m.mlm_logits(hn, torch.arange(3 * S, device=dev))
            self.hidden, self.logits, self.state = self.decode(self.prefill(), self.feed)

    def prefill(self, poison=False):
        state = self.m.prefill(self.prompt, self.pmask, max_len=S)
        if poison:
            for kv in state.cache.kv:
                for b, n in enumerate(PLENS):
                    kv[:, b, :, n:] = float("nan")
        return state

    def decode(self, state, feed):
        m = self.m
        hs, ls = [state.hidden.clone()], [m.decode_step(state)]
        for t in range(feed.shape[1]):
            ls.append(m.decode_step(state, feed[:, t]))
            hs.append(state.hidden.clone())
        return torch.stack(hs), torch.stack(ls), state


@pytest.fixture(scope="module")
def fx():
    return _Fixture(torch.device("cuda", 0))


def test_rotary_decode_matches_fp32_reference(fx):
    assert fx.state.pos.tolist() == [n + STEPS for n in PLENS]
    assert fx.logits.dtype == torch.float32 and fx.logits.shape == (STEPS + 1, 3, fx.m.config.vocab_size)
    for k in range(STEPS + 1):
        _close(fx.hidden[k], fx.ref_hidden[fx.rows[k]], TOL)
        _close(fx.logits[k], fx.ref_logits[fx.rows[k]], TOL)


def test_rotary_picked_token_is_near_the_reference_best(fx):
    rows = fx.rows.reshape(-1)
    ref, nat, dec = fx.ref_logits[rows], fx.nat_logits[rows], fx.logits.reshape(len(rows), -1)
    allow = TOL * float(ref.abs().max())
    best = ref.max(-1).values
    for got in (dec, nat):
        picked = ref.gather(1, got.argmax(-1, keepdim=True))[:, 0]
        assert bool((best - picked <= 2 * allow).all())


def test_rotary_stale_cache_rows_never_read(fx):
    _, logits, _ = fx.decode(fx.prefill(poison=True), fx.feed)
    assert bool(torch.isfinite(logits).all())
    assert torch.equal(logits, fx.logits)


def test_rotary_alone_equals_its_row_of_the_batch_bitwise(fx, monkeypatch):
    """As tests/test_decode_linear_gpu.py: sequence 1's cache rows, position and hidden row copied out of the
    batch's prefill into a state of its own; both fed the same tokens."""
    from ml_trainer_amd.ops.decode import DecodeState, KVCache
    monkeypatch.delenv("MLT_DECODE_GEMM", raising=False)
    batch = fx.prefill()
    alone = DecodeState(KVCache([kv[:, 1:2].clone() for kv in batch.cache.kv], batch.cache.pos[1:2].clone(), S),
                        batch.hidden[1:2].clone())
    steps = 8
    hb, lb, _ = fx.decode(batch, fx.feed[:, :steps])
    ha, la, _ = fx.decode(alone, fx.feed[1:2, :steps])
    assert alone.pos.tolist() == [PLENS[1] + steps] and bool(torch.isfinite(la).all())
    for k in range(steps + 1):
        assert torch.equal(_bits(ha[k, 0]), _bits(hb[k, 1])), f"hidden, step {k}"
        assert torch.equal(_bits(la[k, 0]), _bits(lb[k, 1])), f"logits, step {k}"
    for l in range(len(batch.cache.kv)):
        assert torch.equal(_bits(alone.cache.kv[l][:, 0]), _bits(batch.cache.kv[l][:, 1]))


def test_rotary_graph_equals_eager(fx):
    kw = dict(attention_mask=fx.pmask, sampler="device", temperature=0.8, top_k=5, top_p=0.9, seed=21)
    eager = fx.m.generate(fx.prompt, STEPS, **kw)
    graph = fx.m.generate(fx.prompt, STEPS, graph=True, **kw)
    assert torch.equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1])
    g2 = fx.m.generate(fx.prompt, STEPS, graph=True, **kw)  # a replay of the captured graph
    assert torch.equal(eager[0], g2[0])


def test_rotary_generates_past_the_prompt_width(fx):
    """max_position = 128 only sizes the table: 64 greedy tokens from the 48-token prompts (positions up to 111)
    stay within the tolerance of forward_reference over the finished sequences."""
    m, new = fx.m, 64
    assert m.config.max_position == 128
    tok, n, logits = m.generate(fx.prompt, new, attention_mask=fx.pmask, return_logits=True)
    assert tok.shape == (3, new) and n.tolist() == [new] * 3
    W = PW + new
    full = torch.zeros(3, W, dtype=fx.prompt.dtype, device=fx.prompt.device)
    full[:, :PW] = fx.prompt
    for b, pl in enumerate(PLENS):
        full[b, pl:pl + new] = tok[b]
    flens = fx.plens + new
    fmask = (torch.arange(W, device=full.device)[None, :] < flens[:, None]).long()
    with torch.no_grad():
        hr = m.forward_reference(full, fmask)
        ref = m.mlm_logits(hr, torch.arange(3 * W, device=full.device)).view(3, W, -1)
    for b, pl in enumerate(PLENS):  # logits[b, t] predicts the token at position pl + t: the row of position pl + t - 1
        _close(logits[b], ref[b, pl - 1:pl - 1 + new], TOL)
    with pytest.raises(ValueError, match="max_position"):
        m.generate(fx.prompt, 128 - PW + 1, attention_mask=fx.pmask)
