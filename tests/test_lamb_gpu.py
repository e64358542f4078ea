"""The per-tensor optimizer kernels (csrc/kernels/optim.hip: lamb_stage1 / lamb_finalize / lamb_stage2 and
flat_optim_seg) on the GPU.

The case. With C = _C.optim_chunk_elems(), eight tensors in one FlatParams:

    size      scale   note                          covers
    1         1       excluded                      the alignment gap, a one-float4 tensor
    15        1       gradient identically zero     r = 1 / wd from the decay term alone
    16        0.02
    17        1       excluded
    C         0.02                                  an exact chunk boundary
    C + 4     100                                   a chunk straddle
    3C + 20   1                                     the multi-chunk sum
    5         0       weights all zero              the zero-norm branch (step 1)

Weights randn * scale, gradients as test_optim_gpu.make_inputs makes them, six steps,
lr 0.01, betas (0.9, 0.999), eps 1e-6, weight decay 0.01.

Numerics (test_lamb_matches_loop_reference): R = tests/lamb_ref.lamb_loop in float64, T = the same loop
in fp32, K = the kernels; test_optim_gpu's budget max|K - R| <= 4 max|T - R| + 1e-7 max|R|, applied per
tensor (a global maximum would hide every small tensor behind the x100 one). Measured max|K - R| /
max|T - R| on an MI355X ("-" = both errors are 0):

    tensor (size)     p       m       v
    0 (1)             1.00    0.32    1.00
    1 (15)            1.00    -       -
    2 (16)            1.00    0.58    0.91
    3 (17)            1.00    1.06    1.57
    4 (C)             0.80    1.06    0.88
    5 (C + 4)         1.00    1.00    1.00
    6 (3C + 20)       1.00    0.89    1.12
    7 (5)             0.40    0.54    1.00

and 0.98 - 3.04 over the 33 tensors of bert-tiny after one step against the CPU path
(test_one_lamb_step_on_device_matches_the_cpu_path; the 3.04 is the two-element classifier bias, where
max|T - R| is 5.7e-11). The trust ratios agree with the float64 loop to the six digits printed.

Norms (test_norms_match_float64_sums): the kernel's sums of squares against float64 sums, relative bound
(d + 2) * 2^-24. d counts the additions on the longest path a term takes. For C = 4096 a chunk is 1024
float4s over 256 threads: 16 serial fused multiply-adds per thread, 6 levels of the wave tree, 4 adds of
the block's wave sums; then the finalize block: ceil(chunks / 256) = 1 serial add per thread for the
tensors here, 6 wave levels, 4 wave sums. d = 16 + 6 + 4 + 1 + 6 + 4 = 37, bound 39 * 2^-24 = 2.3e-6.
The float64 sums are formed from the fp32 state the kernel started the step from (u in float64 from
that state), so the rounding of u itself also has to fit in the bound. Measured worst relative error
over the six steps: 1.2e-7 for the sum of w^2, 2.9e-7 for the sum of u^2.
"""
import functools
import math

import pytest
import torch

from ml_trainer_amd.ops._ext import require_native
from ml_trainer_amd.ops.optim import FusedLAMB, SegmentTable, clip_grad_norm_flat
from ml_trainer_amd.utils.flat import FlatParams
from tests.lamb_ref import lamb_loop
from tests.test_optim_gpu import bits16, budget_ratio, flat_optim, make_inputs

pytestmark = pytest.mark.gpu

HP = dict(lr=0.01, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)
STEPS = 6
EXCLUDED = (0, 3)
ZERO_GRAD = 1
NORM_D = 37  # see the docstring; holds for the chunk size asserted in case()


@functools.lru_cache(maxsize=None)
def case():
    """(sizes, weights, grads[step][tensor], R, T): computed once, shared by the tests, never modified."""
    C = int(require_native().optim_chunk_elems())
    assert C == 4096, "NORM_D was counted for 4096-element chunks: count it again"
    sizes = [1, 15, 16, 17, C, C + 4, 3 * C + 20, 5]
    scales = [1.0, 1.0, 0.02, 1.0, 0.02, 100.0, 1.0, 0.0]
    weights, per_tensor = [], []
    for i, (n, s) in enumerate(zip(sizes, scales)):
        p0, gs = make_inputs(n, STEPS, 4000 + i)
        weights.append(p0 * s)
        per_tensor.append([torch.zeros(n) for _ in gs] if i == ZERO_GRAD else gs)
    grads = [[per_tensor[i][t] for i in range(len(sizes))] for t in range(STEPS)]
    R = lamb_loop(weights, grads, HP, set(EXCLUDED), torch.float64)
    T = lamb_loop(weights, grads, HP, set(EXCLUDED), torch.float32)
    return sizes, weights, grads, R, T


class Run:
    """One flat buffer of the case on the device with its segment table, state and shadow."""

    def __init__(self, dev, weights, excluded=EXCLUDED, wd=HP["weight_decay"], adapt=True, shadow=False):
        self.params = [torch.nn.Parameter(w.clone().to(dev)) for w in weights]
        self.fp = FlatParams(self.params)
        self.seg = SegmentTable(self.fp, wd, [self.params[i] for i in excluded], adapt)
        self.m, self.v = torch.zeros_like(self.fp.data), torch.zeros_like(self.fp.data)
        self.shadow = self.fp.refresh_shadow() if shadow else None

    def set_grads(self, grads):
        for g, (o, n) in zip(grads, self.seg.segments):
            self.fp.grad[o:o + n].copy_(g)

    def tensors(self, buf):
        return [buf[o:o + n] for o, n in self.seg.segments]

    def gap_mask(self):
        pad = torch.ones(self.fp.numel, dtype=torch.bool, device=self.fp.device)
        for o, n in self.seg.segments:
            pad[o:o + n] = False
        return pad

    def lamb(self, C, t_host=1.0, hp=HP, lr=None, grad_scale=1.0, lr_t=None, lr_index=None, step_t=None, coef=None,
             skip=None, max_blocks=0):
        d = self.seg.dev
        C.lamb_step(self.fp.data, self.fp.grad, self.m, self.v, d["chunks"], d["tseg"], d["wd"], d["adapt"],
                    d["part"], d["norms"], self.seg.last_trust, hp["lr"] if lr is None else lr, hp["betas"][0],
                    hp["betas"][1], hp["eps"], grad_scale, False, lr_t, lr_index, step_t, float(t_host),
                    self.shadow, coef, skip, max_blocks, 7)

    def adamw_seg(self, C, t_host=1.0, lr=0.01, max_blocks=0):
        d = self.seg.dev
        C.flat_optim_seg(self.fp.data, self.fp.grad, self.m, self.v, d["chunks"], d["wd"], lr, 0.9, 0.999, 1e-8, 1.0,
                         False, None, None, None, float(t_host), self.shadow, None, None, max_blocks)

    def state(self):
        out = [self.fp.data.clone(), self.m.clone(), self.v.clone(), self.seg.dev["norms"].clone(),
               self.seg.last_trust.clone()]
        if self.shadow is not None:
            out.append(self.shadow.clone())
        return out


def run_steps(C, dev, grads, steps=STEPS, **kw):
    _, weights, _, _, _ = case()
    r = Run(dev, weights)
    for t in range(steps):
        r.set_grads(grads[t])
        r.lamb(C, t_host=t + 1, **kw)
    return r


def assert_same_bits(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        if x.dtype == torch.bfloat16:
            x, y = bits16(x), bits16(y)
        assert torch.equal(x, y), f"{what}: buffer {i} differs"


# ---------------------------------------------------------------------------------------------
# 1. numerics   2. norms   3. moment bits
# ---------------------------------------------------------------------------------------------
def test_lamb_matches_loop_reference(dev):
    C = require_native()
    sizes, weights, grads, R, T = case()
    for name in ("p", "m", "v"):
        for i in range(len(sizes)):
            assert torch.isfinite(R[name][i]).all()
    assert min(R["trust"]) < 0.05 and max(R["trust"]) >= 99.0  # the case spans the ratios it was built for
    assert R["trust"][ZERO_GRAD] == pytest.approx(1.0 / HP["weight_decay"], rel=1e-9)
    assert all(R["trust"][i] == 1.0 for i in EXCLUDED)
    r = run_steps(C, dev, grads)
    K = dict(p=r.tensors(r.fp.data), m=r.tensors(r.m), v=r.tensors(r.v))
    rows = []
    for i, n in enumerate(sizes):
        rows.append([budget_ratio(f"lamb tensor {i} (n={n}) {name}", K[name][i], R[name][i], T[name][i])
                     for name in ("p", "m", "v")])
    for i, (n, row) in enumerate(zip(sizes, rows)):
        print(f"[ratios] tensor {i} n={n}: p {row[0]:.2f}  m {row[1]:.2f}  v {row[2]:.2f}")
    trust = r.seg.last_trust.double().cpu()
    print("[trust] kernel", [f"{x:.6g}" for x in trust.tolist()], "float64", [f"{x:.6g}" for x in R["trust"]])
    torch.testing.assert_close(trust, torch.tensor(R["trust"], dtype=torch.float64), rtol=1e-4, atol=0)


def _float64_sums(p, g, m, v, seg, t):
    """Sums of w^2 and u^2 per tensor in float64, from the fp32 state a step starts from."""
    b1, b2 = HP["betas"]
    p, g, m, v = (x.double().cpu() for x in (p, g, m, v))
    m = m + (1 - b1) * (g - m)
    v = b2 * v + (1 - b2) * g * g
    out = []
    for (o, n), wd in zip(seg.segments, seg.wd):
        s = slice(o, o + n)
        u = (m[s] / (1 - b1 ** t)) / (v[s].sqrt() / math.sqrt(1 - b2 ** t) + HP["eps"]) + wd * p[s]
        out.append((float((p[s] * p[s]).sum()), float((u * u).sum())))
    return out


def test_norms_match_float64_sums(dev):
    C = require_native()
    _, weights, grads, _, _ = case()
    bound = (NORM_D + 2) * 2.0 ** -24
    r = Run(dev, weights)
    worst = [0.0, 0.0]
    for t in range(1, STEPS + 1):
        r.set_grads(grads[t - 1])
        want = _float64_sums(r.fp.data, r.fp.grad, r.m, r.v, r.seg, t)
        r.lamb(C, t_host=t)
        got = r.seg.dev["norms"].double().cpu()
        for i, (w_sq, u_sq) in enumerate(want):
            for k, ref in enumerate((w_sq, u_sq)):
                if ref == 0.0:
                    assert got[i, k] == 0.0
                    continue
                rel = abs(got[i, k].item() - ref) / ref
                worst[k] = max(worst[k], rel)
                assert rel <= bound, f"step {t} tensor {i} {'wu'[k]}_sq: rel {rel:.3e} > {bound:.3e}"
            ratio = math.sqrt(w_sq / u_sq) if (i not in EXCLUDED and w_sq > 0 and u_sq > 0) else 1.0
            assert r.seg.last_trust[i].item() == pytest.approx(ratio, rel=4 * bound)
    print(f"[norms] worst relative error: w_sq {worst[0]:.3e}  u_sq {worst[1]:.3e}  bound {bound:.3e}")


def test_moments_are_bitwise_flat_optim_adam(dev):
    C = require_native()
    _, weights, grads, _, _ = case()
    r = Run(dev, weights)
    p2, m2, v2 = r.fp.data.clone(), torch.zeros_like(r.m), torch.zeros_like(r.v)
    for t in range(1, 4):
        r.set_grads(grads[t - 1])
        r.lamb(C, t_host=t, grad_scale=0.5)
        flat_optim(C, "adam", dict(lr=0.01, eps=1e-6), p2, r.fp.grad, m2, v2, t_host=t, grad_scale=0.5)
        assert torch.equal(r.m, m2) and torch.equal(r.v, v2), f"step {t}: moments differ from flat_optim adam"
    assert r.m.abs().max() > 0


# ---------------------------------------------------------------------------------------------
# 4. AdamW with exclusions
# ---------------------------------------------------------------------------------------------
def test_flat_optim_seg_is_bitwise_flat_optim_per_tensor(dev):
    C = require_native()
    sizes, weights, grads, _, _ = case()
    wd = 0.05
    r = Run(dev, weights, wd=wd, adapt=False, shadow=True)
    plain = {}
    for decay in (wd, 0.0):  # the whole buffer with one decay, as the plain launch runs it
        q = Run(dev, weights, shadow=True)
        plain[decay] = q
    for t in range(1, 4):
        r.set_grads(grads[t - 1])
        r.adamw_seg(C, t_host=t)
        for decay, q in plain.items():
            q.set_grads(grads[t - 1])
            flat_optim(C, "adamw", dict(lr=0.01, weight_decay=decay), q.fp.data, q.fp.grad, q.m, q.v, t_host=t,
                       shadow=q.shadow)
    for i in range(len(sizes)):
        q = plain[0.0 if i in EXCLUDED else wd]
        other = plain[wd if i in EXCLUDED else 0.0]
        for name, a, b in (("p", r.fp.data, q.fp.data), ("m", r.m, q.m), ("v", r.v, q.v)):
            assert torch.equal(r.tensors(a)[i], q.tensors(b)[i]), f"tensor {i} {name} differs from flat_optim"
        assert torch.equal(bits16(r.tensors(r.shadow)[i]), bits16(q.tensors(q.shadow)[i])), f"tensor {i} shadow"
        if sizes[i] > 1 and weights[i].abs().max() > 0:
            assert not torch.equal(r.tensors(r.fp.data)[i], other.tensors(other.fp.data)[i])
    assert torch.equal(bits16(r.shadow), bits16(r.fp.data.bfloat16()))
    gaps = r.gap_mask()
    assert gaps.any() and all((b[gaps] == 0).all() for b in (r.fp.data, r.m, r.v))
    # a lower block cap: the same bits
    r2 = Run(dev, weights, wd=wd, adapt=False, shadow=True)
    for t in range(1, 4):
        r2.set_grads(grads[t - 1])
        r2.adamw_seg(C, t_host=t, max_blocks=2)
    assert_same_bits([r.fp.data, r.m, r.v, r.shadow], [r2.fp.data, r2.m, r2.v, r2.shadow], "max_blocks=2")


# ---------------------------------------------------------------------------------------------
# 5. determinism and isolation
# ---------------------------------------------------------------------------------------------
def test_lamb_is_deterministic_grid_independent_and_isolated(dev):
    C = require_native()
    sizes, _, grads, _, _ = case()
    steps = 3
    first = run_steps(C, dev, grads, steps)
    assert_same_bits(first.state(), run_steps(C, dev, grads, steps).state(), "second run")
    for cap in (1, 3):
        assert_same_bits(first.state(), run_steps(C, dev, grads, steps, max_blocks=cap).state(), f"max_blocks={cap}")
    gaps = first.gap_mask()
    assert gaps.any() and all((b[gaps] == 0).all() for b in (first.fp.data, first.m, first.v))
    changed = 5  # the x100 tensor, between two others
    other_grads = [[g * 1.5 if i == changed else g for i, g in enumerate(gs)] for gs in grads]
    other = run_steps(C, dev, other_grads, steps)
    for i in range(len(sizes)):
        same = [torch.equal(first.tensors(a)[i], other.tensors(b)[i])
                for a, b in ((first.fp.data, other.fp.data), (first.m, other.m), (first.v, other.v))]
        assert (not any(same)) if i == changed else all(same), f"tensor {i}: {same}"


# ---------------------------------------------------------------------------------------------
# 6. device-memory arguments, shadow, skip
# ---------------------------------------------------------------------------------------------
def test_lamb_device_lr_step_coef_paths_are_bitwise_host_paths(dev):
    C = require_native()
    _, weights, grads, _, _ = case()
    table = torch.tensor([0.1, 0.05, 0.2, 0.0125, 0.075], dtype=torch.float32, device=dev)
    host, devp = Run(dev, weights, shadow=True), Run(dev, weights, shadow=True)

    def same(what):
        assert_same_bits(host.state(), devp.state(), what)
        assert torch.equal(bits16(devp.shadow), bits16(devp.fp.data.bfloat16())), f"{what}: shadow != p.bfloat16()"

    for i in range(4):  # lr table + lr_index + step from device memory; the host lr / t are decoys
        for r in (host, devp):
            r.set_grads(grads[i])
        host.lamb(C, t_host=i + 1, lr=float(table[i]))
        idx = torch.tensor([i + 1], dtype=torch.int64, device=dev)
        devp.lamb(C, t_host=99, lr=123.0, lr_t=table, lr_index=idx, step_t=idx.clone())
        same(f"step {i + 1}")
    for r in (host, devp):
        r.set_grads(grads[4])
    host.lamb(C, t_host=5, lr=float(table[0]))  # lr_t without lr_index reads element 0
    devp.lamb(C, t_host=99, lr=123.0, lr_t=table, step_t=torch.tensor([5], dtype=torch.int64, device=dev))
    same("lr_t[0]")
    for r in (host, devp):
        r.set_grads(grads[5])
    host.lamb(C, t_host=6, grad_scale=0.125)  # coef multiplies grad_scale
    devp.lamb(C, t_host=6, grad_scale=0.5, coef=torch.tensor([0.25], dtype=torch.float32, device=dev))
    same("coef")
    assert not torch.equal(host.fp.data, Run(dev, weights).fp.data)  # the steps did something


def test_skip_word_vetoes_every_write(dev):
    C = require_native()
    _, weights, grads, _, _ = case()
    r = Run(dev, weights, shadow=True)
    r.set_grads(grads[0])
    r.lamb(C, t_host=1)
    before = r.state()
    r.set_grads(grads[1])
    veto = torch.ones(1, dtype=torch.int32, device=dev)
    r.lamb(C, t_host=2, skip=veto)
    assert_same_bits(before, r.state(), "lamb under the veto")
    r.adamw_seg(C, t_host=2)  # (moves everything: the comparison below is not vacuous)
    moved = r.state()
    assert not torch.equal(moved[0], before[0])
    d = r.seg.dev
    C.flat_optim_seg(r.fp.data, r.fp.grad, r.m, r.v, d["chunks"], d["wd"], 0.01, 0.9, 0.999, 1e-8, 1.0, False, None,
                     None, None, 3.0, r.shadow, None, veto, 0)
    assert_same_bits(moved, r.state(), "flat_optim_seg under the veto")
    veto.zero_()
    r.lamb(C, t_host=3, skip=veto)  # a clear word lets the step through
    assert not torch.equal(r.fp.data, moved[0])


# ---------------------------------------------------------------------------------------------
# 7. hipGraph capture
# ---------------------------------------------------------------------------------------------
def test_lamb_steps_captured_in_a_graph_equal_eager_steps(dev):
    C = require_native()
    _, weights, grads, _, _ = case()
    table = torch.tensor([0.02, 0.01, 0.005], dtype=torch.float32, device=dev)
    eager = Run(dev, weights, shadow=True)
    for t in range(3):
        eager.set_grads(grads[t])
        eager.lamb(C, t_host=t + 1, lr=float(table[t]))

    r = Run(dev, weights, shadow=True)
    start = [r.fp.data.clone(), r.shadow.clone()]
    staged = []
    for t in range(3):
        r.set_grads(grads[t])
        staged.append(r.fp.grad.clone())
    step_t = torch.zeros(1, dtype=torch.int64, device=dev)

    def three_steps():
        for t in range(3):
            step_t.add_(1)
            r.fp.grad.copy_(staged[t])
            r.lamb(C, t_host=99, lr=123.0, lr_t=table, lr_index=step_t, step_t=step_t)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        three_steps()  # warm-up outside the capture (module load), then rewind
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        three_steps()
    for _ in range(2):  # replay twice from the same start: the graph carries no state of its own
        r.fp.data.copy_(start[0])
        r.shadow.copy_(start[1])
        r.m.zero_()
        r.v.zero_()
        step_t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert step_t.item() == 3
        assert_same_bits(eager.state(), r.state(), "graph replay")


# ---------------------------------------------------------------------------------------------
# 8. end to end
# ---------------------------------------------------------------------------------------------
def test_trainer_bert_tiny_lamb_trains_and_evaluates(dev, tmp_path):
    from ml_trainer_amd.data.text import SyntheticTextClassification
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    from ml_trainer_amd.trainer import Trainer
    torch.manual_seed(0)
    m = BertClassifier(bert_config("bert-tiny"))
    tr = SyntheticTextClassification(256, seq_len=64, vocab_size=1000, seed=0, learnable=True)
    va = SyntheticTextClassification(64, seq_len=64, vocab_size=1000, seed=1, learnable=True)
    t = Trainer(m, datasets=(tr, va), epochs=6, batch_size=32, model_dir=str(tmp_path), optimizer="lamb", lr=1e-3,
                weight_decay=0.01, metric="accuracy",
                options={"progress": False, "no_decay_1d": True, "grad_clip": 1.0})
    assert isinstance(t.optimizer, FusedLAMB) and t.optimizer.flats[0] is t.flat and t.flat.device.type == "cuda"
    t.fit()
    losses = t.history["train_loss"]
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses
    ev = t.evaluate()
    assert all(math.isfinite(float(v)) for v in (ev if isinstance(ev, (tuple, list)) else [ev]) if v is not None)
    trust = t.optimizer.last_trust()
    assert torch.isfinite(trust).all()
    for p, r in zip(t.flat.params, trust.tolist()):
        assert (r == 1.0) if p.ndim <= 1 else (r > 0.0)


def test_one_lamb_step_on_device_matches_the_cpu_path(dev):
    """Equal weights and equal (clipped) gradients into FusedLAMB on the device and on the CPU: per
    tensor within the budget of test 1, R = the float64 loop, T = the CPU path, K = the kernels."""
    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    from ml_trainer_amd.ops.optim import build_optimizer
    torch.manual_seed(0)
    cfg = bert_config("bert-tiny")
    mg = BertClassifier(cfg).to(dev)
    mc = BertClassifier(cfg)
    mc.load_state_dict({k: v.cpu() for k, v in mg.state_dict().items()})
    kw = dict(lr=1e-3, weight_decay=0.01, no_decay_1d=True)
    og, oc = build_optimizer("lamb", mg.parameters(), **kw), build_optimizer("lamb", mc.parameters(), **kw)
    ids = torch.randint(5, cfg.vocab_size, (8, 32), generator=torch.Generator().manual_seed(1))
    y = torch.randint(0, cfg.num_labels, (8,), generator=torch.Generator().manual_seed(2))
    og.zero_grad()
    torch.nn.functional.cross_entropy(mg(ids.to(dev)), y.to(dev)).backward()
    fg, fc = og.flats[0], oc.flats[0]
    clip_grad_norm_flat(fg, 1.0)
    oc.zero_grad()
    assert fg.offsets == fc.offsets and fg.numel == fc.numel
    fc.grad.copy_(fg.grad.cpu())
    weights = [p.detach().cpu().clone() for p in fg.params]
    grads = [fg.grad[o:o + p.numel()].view_as(p).cpu().clone() for p, o in zip(fg.params, fg.offsets)]
    og.step()
    oc.step()
    excluded = {i for i, p in enumerate(fg.params) if p.ndim <= 1}
    R = lamb_loop(weights, [grads], dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01), excluded,
                  torch.float64)
    worst = 0.0
    for i, (pg, pc) in enumerate(zip(fg.params, fc.params)):
        worst = max(worst, budget_ratio(f"bert-tiny tensor {i} {tuple(pg.shape)}", pg, R["p"][i], pc))
    print(f"[e2e] worst per-tensor ratio {worst:.2f}")
    torch.testing.assert_close(og.last_trust().cpu(), oc.last_trust(), rtol=1e-4, atol=0)
