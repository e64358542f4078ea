"""The SwiGLU kernels on the GPU: ``C.swiglu_fwd`` / ``C.swiglu_bwd`` against the float64 definition on the same bf16
inputs, ``C.gemm_skinny_glu`` against the unfused pair (bit for bit) and float64, and bert-tiny with ``ffn="swiglu"``
through training, cached decoding and the graph-replayed ``generate``.

Bounds (u = 2^-24; nothing here is tuned to what the kernels return). mlt_swiglu.h evaluates
``e = v_exp_f32(g * -log2e)``, ``s = v_rcp_f32(1 + e)`` with every product and sum rounded on its own. v_exp_f32 and
v_rcp_f32 are 1-ulp instructions in the ISA manual; 2 ulp = 4u each are allowed, as tests/helpers.py allows v_exp_f32.
With gc = min(|g|, 128) (past 128 the argument error cannot move e off 0 / inf):
  e: (2 gc + 4) u relative (product and constant: 2|g| u in the exponent; the instruction);
  s: rel. error (2 gc + 4)(1 - s) u + 5u <= (2 gc + 9) u, plus 2^-126 absolute where the reciprocal, or s itself
     (g < -87), falls below the normal range and is flushed to 0;
  a = (g s) u and du = da (g s): two more products, (2 gc + 11) u |result| + (|g u| + 1) 2^-126 (du: |da g|); the
     "+ 1" is the last product itself landing below the normal range, where it may be flushed;
  1 - s: absolute (2 gc + 5)(1 - s) u + 5u; f = 1 + g (1 - s): absolute (7 gc + 7) u (1 + |g| (1 - s));
  dg = (da u)(s f): (9 gc + 19) u D + (|da u| (1 + |g|) + |s f| + 1) 2^-126 with D = |da u s| (1 + |g| (1 - s)) -- in
     terms of D, not of |dg|: f crosses zero at g = -1.278 and the factor cancels there. (|s f| 2^-126: da u flushed.)
Each result is rounded to bf16 once: ``helpers.store_bound`` (bf16's own spacing at the element, denormals included).
The inputs keep |da|, |u| within 2^+-40 so that da * u, which the definition forms first, stays inside fp32.
The bias gradient is compared with the float64 column sum of the kernel's OWN stored dH1: an fp32 sum of n = rows
terms in any order is within (n - 1) u sum|x|; the accumulate mode adds the previous value once more: n u (sum|x| +
|db0|). Observed on an MI355X (``helpers.bf16_t_used``: the share of the fp32 allowance a bf16 output needs; for db
error / bound): a 0.19, dg 0.19, du 0.19, db 0.04; the gated GEMM against float64 0.96 (docs/ARCHITECTURE.md).

Gated GEMM against float64: g, u as stored by FFN1 are within eg, eu = ``store_bound(., gemm_t32, bf16)`` (the existing
skinny test's bound); |silu'| <= 1.1 and |silu(g)| <= |g| carry them to t0 = 1.1 eg (|u| + eu) + |g| eu at the
activation, the evaluation adds (2 gc + 11) u (|a| + t0), then the one bf16 store."""
import pytest
import torch

from tests.helpers import (assert_guard_intact, assert_within, bf16_t_used, gemm_expected, gemm_t32, guarded,
                           guarded_1d, guarded_like, store_bound)
from tests.test_clm_gpu import _batch, _grads
from tests.test_preln_gpu import PLENS, PW, STEPS, TOL, S, _bits, _spread_norm_weights
from tests.test_unpad_gpu import _close

pytestmark = pytest.mark.gpu
U, TINY = 2.0 ** -24, 2.0 ** -126
G_SPECIAL = [0.0, -0.0, 1.278, -1.278, 30.0, -30.0, 89.0, -89.0, 200.0, -200.0, 2.0 ** 100, -2.0 ** 100]


def _C():
    from ml_trainer_amd.ops._ext import require_native
    return require_native()


def _inputs(rows, F, dev, seed):
    """bf16 h1 = g | u and da: g normal x 4 with the special values planted, |u|, |da| = 2^(+-40) x normal."""
    gen = torch.Generator().manual_seed(seed)
    g = 4.0 * torch.randn(rows, F, generator=gen)
    g.view(-1)[:len(G_SPECIAL)] = torch.tensor(G_SPECIAL)[:rows * F]
    wide = lambda: torch.randn(rows, F, generator=gen) * torch.exp2(torch.randint(-40, 41, (rows, F), generator=gen).float())
    u, da = wide(), wide()
    u.view(-1)[10:12] = da.view(-1)[10:12] = 2.0 ** -100  # beside g = +-2^100: a = 1 and -0, everything in range
    return torch.cat((g, u), 1).to(torch.bfloat16).to(dev), da.to(torch.bfloat16).to(dev)


def _definition64(h1, da):
    """(a, dg, du) and their allowances before the bf16 store, float64."""
    F = h1.shape[1] // 2
    g, u, d = h1[:, :F].double(), h1[:, F:].double(), da.double()
    s = 1.0 / (1.0 + torch.exp(-g))
    gc = g.abs().clamp(max=128.0)
    a, du, dg = (g * s) * u, d * (g * s), (d * u) * (s * (1.0 + g * (1.0 - s)))
    D = (d * u * s).abs() * (1.0 + g.abs() * (1.0 - s))
    sf = s * (1.0 + g.abs() * (1.0 - s))
    return ((a, (2 * gc + 11) * U * a.abs() + ((g * u).abs() + 1.0) * TINY),
            (dg, (9 * gc + 19) * U * D + ((d * u).abs() * (1.0 + g.abs()) + sf + 1.0) * TINY),
            (du, (2 * gc + 11) * U * du.abs() + ((d * g).abs() + 1.0) * TINY))


@pytest.mark.parametrize("F", [8, 520, 1024])
@pytest.mark.parametrize("rows", [1, 67, 300])
def test_streaming_kernels_against_float64(dev, rows, F):
    C = _C()
    h1, da = _inputs(rows, F, dev, rows * 7 + F)
    hbuf, h1 = guarded_like(h1, ld=2 * F + 8)  # row-strided: NaN in the stride gap
    (a64, ta), (dg64, tdg), (du64, tdu) = _definition64(h1, da)
    abuf, a = guarded(rows, F, torch.bfloat16, dev, ld=F + 8)
    C.swiglu_fwd(h1, a)
    assert_guard_intact(abuf, a)
    assert_within(a, a64, store_bound(a64, ta, torch.bfloat16), "a")
    dbuf, dh1 = guarded(rows, 2 * F, torch.bfloat16, dev, ld=2 * F + 16)
    part = torch.empty(C.swiglu_partial_blocks(rows) * 2 * F, dtype=torch.float32, device=dev)
    bbuf, db = guarded_1d(2 * F, dev)
    C.swiglu_bwd(da, h1, dh1, part, db, False)  # set: the sentinel NaN must be overwritten, not added to
    assert_guard_intact(dbuf, dh1), assert_guard_intact(bbuf, db), assert_guard_intact(hbuf, h1)
    assert bool(torch.isfinite(a.float()).all() and torch.isfinite(dh1.float()).all())
    assert_within(dh1[:, :F], dg64, store_bound(dg64, tdg, torch.bfloat16), "dg")
    assert_within(dh1[:, F:], du64, store_bound(du64, tdu, torch.bfloat16), "du")
    ra, rg, ru = (bf16_t_used(o, e, t) for o, e, t in ((a, a64, ta), (dh1[:, :F], dg64, tdg), (dh1[:, F:], du64, tdu)))
    col, mag = dh1.double().sum(0), dh1.double().abs().sum(0)
    rb = assert_within(db, col, rows * U * mag + 1e-300, "db set")
    db0 = db.clone()
    C.swiglu_bwd(da, h1, dh1, part, db, True)
    rb = max(rb, assert_within(db, col + db0.double(), rows * U * (mag + db0.double().abs()) + 1e-300, "db accumulate"))
    print(f"rows {rows} F {F}: share of the fp32 allowance used a {ra:.3f} dg {rg:.3f} du {ru:.3f}; db err / bound {rb:.3f}")


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("F,K", [(16, 32), (48, 224), (1024, 256), (2048, 768)])
@pytest.mark.parametrize("M", [1, 3, 16])
def test_gated_skinny_gemm_equals_unfused_pair(dev, M, F, K, bias):
    C = _C()
    gen = torch.Generator().manual_seed(M + F + K)
    X = torch.full((16, K), float("nan"), dtype=torch.bfloat16, device=dev)  # rows past M must not reach the output
    X[:M] = torch.randn(M, K, generator=gen).to(torch.bfloat16).to(dev)
    W = (torch.randn(2 * F, K, generator=gen) / K ** 0.5 * 2).to(torch.bfloat16).to(dev)
    b = torch.randn(2 * F, generator=gen).to(dev) if bias else None
    ybuf, y = guarded(M, F, torch.bfloat16, dev, ld=F + 8)
    C.gemm_skinny_glu(X[:M], W, y, bias=b)
    assert_guard_intact(ybuf, y)
    h1 = torch.empty(M, 2 * F, dtype=torch.bfloat16, device=dev)
    C.gemm_skinny(X[:M], W, h1, bias=b)
    ref = torch.empty(M, F, dtype=torch.bfloat16, device=dev)
    C.swiglu_fwd(h1, ref)
    assert bool(torch.isfinite(y.float()).all()) and torch.equal(_bits(y), _bits(ref))
    if (M, F, K, bias) == (3, 1024, 256, True):  # and not only equal to each other: the float64 product
        X64, W64 = X[:M].double(), W.double().T
        gu, t32 = gemm_expected(X64, W64, {"bias": b.double()}), gemm_t32(X64, W64, K, {"bias": b.double()})
        e = store_bound(gu, t32, torch.bfloat16)
        (g, eg), (u, eu) = ((gu[:, :F], e[:, :F]), (gu[:, F:], e[:, F:]))
        a64 = g * torch.sigmoid(g) * u
        t0 = 1.1 * eg * (u.abs() + eu) + g.abs() * eu
        t = t0 + (2 * g.abs().clamp(max=128.0) + 11) * U * (a64.abs() + t0)
        assert_within(y, a64, store_bound(a64, t, torch.bfloat16), "gated skinny vs float64")
        print(f"gated skinny vs float64: share of the allowance used {bf16_t_used(y, a64, t):.3f}")
    with pytest.raises(RuntimeError, match="gate and up rows"):
        C.gemm_skinny_glu(X[:M], W[:F], y, bias=None)


# ------------------------------------------------------------------------------------------------ the model
CONFIGS = {"post_ln": dict(), "pre_rms_rope_gqa": dict(pre_ln=True, norm="rmsnorm", rotary=True, kv_heads=2)}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_bert_tiny_swiglu_training_matches_reference(dev, name):
    """The fixture and thresholds of tests/test_preln_gpu.py (hidden 5e-2, loss 5e-2 relative, every gradient within
    max(2 x the eager autocast baseline's error, 0.02)), unchanged."""
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny", ffn="swiglu", **CONFIGS[name])).to(dev).train()
    with torch.no_grad():
        m.mlm_bias.normal_(std=0.1)
    _spread_norm_weights(m)
    ids, mask, labels = _batch(dev)
    hn, ln, gn = _grads(m, m, m.lm_loss, ids, mask, labels)
    hr, lr, gr = _grads(m, m.forward_reference, m.lm_loss_reference, ids, mask, labels)
    _, la, ga = _grads(m, m.forward_torch_bf16, m.mlm_loss_torch_bf16, ids, mask, labels)
    _close(hn, hr, 5e-2)
    assert abs(float(ln) - float(lr)) <= 5e-2 * abs(float(lr))
    checked = set()
    for n in gr:
        nr = gr[n].norm().item()
        if nr >= 1e-8:
            e_nat, e_ac = (gn[n] - gr[n]).norm().item() / nr, (ga[n] - gr[n]).norm().item() / nr
            assert e_nat <= max(2.0 * e_ac, 0.02), f"{n}: native rel err {e_nat:.4f} vs autocast {e_ac:.4f}"
            checked.add(n)
    assert {"layers.0.ffn1.bias", "layers.1.ffn1.weight", "layers.1.ffn2.weight"} <= checked


@pytest.mark.parametrize("name", list(CONFIGS))
def test_bert_tiny_swiglu_decode(dev, name, monkeypatch):
    """The decode fixture of tests/test_generate_gpu.py as tests/test_preln_gpu.py mirrors it: cached logits against
    the uncached fp32 forward (TOL), MLT_DECODE_GLU 0 and 1 bit for bit over 8 steps, the replayed graph's tokens."""
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    monkeypatch.delenv("MLT_DECODE_GLU", raising=False)
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny", ffn="swiglu", **CONFIGS[name])).to(dev).eval()
    with torch.no_grad():
        m.mlm_bias.normal_(std=0.1)
    _spread_norm_weights(m)
    ids = torch.randint(5, 1000, (3, S), generator=torch.Generator().manual_seed(11)).to(dev)
    pl = torch.tensor(PLENS, device=dev)
    prompt, pmask = ids[:, :PW].clone(), (torch.arange(PW, device=dev)[None, :] < pl[:, None]).long()
    feed = torch.stack([ids[b, PLENS[b]:PLENS[b] + STEPS] for b in range(3)])
    fmask = (torch.arange(S, device=dev)[None, :] < (pl + STEPS)[:, None]).long()

    def decode(steps):
        state = m.prefill(prompt, pmask, max_len=S)
        return torch.stack([m.decode_step(state)] + [m.decode_step(state, feed[:, t]) for t in range(steps)])

    with torch.no_grad():
        ref = m.mlm_logits(m.forward_reference(ids, fmask), torch.arange(3 * S, device=dev))
    logits = decode(STEPS)
    for k in range(STEPS + 1):
        _close(logits[k], ref[torch.arange(3, device=dev) * S + pl - 1 + k], TOL)
    monkeypatch.setenv("MLT_DECODE_GLU", "0")
    unfused = decode(8)
    monkeypatch.delenv("MLT_DECODE_GLU")
    assert torch.equal(_bits(unfused), _bits(logits[:9]))
    kw = dict(attention_mask=pmask, sampler="device", temperature=0.8, top_k=5, top_p=0.9, seed=21)
    eager, graph = m.generate(prompt, STEPS, **kw), m.generate(prompt, STEPS, graph=True, **kw)
    again = m.generate(prompt, STEPS, graph=True, **kw)  # a replay of the captured graph
    assert torch.equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1]) and torch.equal(eager[0], again[0])
    assert m.decode_graph_captures == 1
