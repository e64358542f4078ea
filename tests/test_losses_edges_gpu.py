"""Edge paths of the loss and metric kernels (losses.hip) -- fused softmax-cross-entropy with its backward and its
fused accuracy output, accuracy, the L1 / MSE / NLL criteria and mcrmse -- on GUARDED buffers, every output held to
the derived bounds of tests/helpers.py against an fp64 reference computed on the CPU once per case.

Every 2-D buffer the kernels read or write (logits, dl, the scaled gradient, log-probabilities, predictions) has one
sentinel row before and after it; every 1-D fp32 buffer (acc, loss, correct, stats, g, d, col, out) is a slice inside
a sentinel-filled allocation with 64 floats on both sides; the partials scratch of the regression reductions is
filled with the sentinel, so that a finalize that reads past its nb partials returns NaN and a partial kernel that
writes past them is seen. The sentinels are NaN patterns. tests/test_loss_bound_cpu.py shows on the CPU that the
bounds hold for a faithful emulation of the kernels and reject the defects listed there.

Each check prints `headroom <kernel> <output> <figure>` (pytest -s): for fp32 outputs the largest |err| / t, for
bf16 outputs the largest fraction of the fp32-level allowance t the stored value needs (helpers.bf16_t_used).

Edge -> the case that reaches it:
  ce: loss 0 and gradient 0 ........................................... (1, 1)
  a second block with one row and three idle waves ..................... (5, 10)
  exactly one chunk | a one-lane tail chunk | 65 chunks ............... (3, 64) | (3, 65) | (2, 4099)
  the maximum rising in every chunk | only in the first ............... rows 0 and 1 of (12, 130) and (12, 1000)
  a one-hot softmax with the target beside it (loss 160) .............. row 2
  ties at the maximum across chunks and inside one .................... rows 3, 4, 10 (the fused accuracy output)
  a wholly -inf first chunk | a wholly -inf second chunk .............. rows 5 | 6, label_smoothing = 0 only (with
                                                                        smoothing the loss is +inf in torch too: the
                                                                        rows are ordinary ones there)
  target C - 1 | -100 | C (out of range: ignored) ..................... rows 7 | 8 | 9
  an in-range ignore_index ............................................ test_ce_in_range_ignore_index
  non-contiguous logits, int32 targets through the module ............. test_ce_module_strided_int32
  accuracy: one row | a tail block | 250 blocks; C = 1, tail chunks ... LOSS_ACC_B x LOSS_ACC_C
  planted ties with the target first / second / neither; -100 ......... every accuracy case with C >= 2
  pointwise: the block cap and a second grid stride ................... n = 2^20 + 5
  a second trip in the finalize block ................................. n = 300001 (293 blocks)
  stale partials of a larger run ....................................... test_pointwise_module (n = 1 after 2^20 + 5)
  the target's gradient, bf16 predictions ............................. test_pointwise_module
  NLL: in-range ignore_index, out-of-range target, nothing counting ... LOSS_NLL_CASES x LOSS_NLL_IGNORE, test_nll_all_ignored
  mcrmse: C above the finalize block's 256 threads | sqrt(0) .......... (3, 300) | the zero-column form of every case

Measured on an MI355X (largest figure per output over all cases, and the case that gives it):
  ce        loss 0.137 ((3, 64) bf16, ls 0.1)   dl 0.610 ((5, 10) fp32, ls 0.1)   grad 0.518 ((12, 1000) fp32, ls 0.1,
            grad_out -0.5)   grad stored as bf16 0.056 ((12, 1000), ls 0)   correct 0.133 ((1000, 1))
            the -inf cases (ls 0): loss 0.077 / 0.086, dl 0.400 / 0.402 at (12, 130) / (12, 1000) fp32
  accuracy  out 0.133 ((1000, 1): 250 blocks each adding 4 / 1000)
  l1        loss 0.087 (n 1025, bf16 predictions)   g exact   grad 0.284 (n 300001)   target's grad 0.008
  mse       loss 0.021 (n 1)   g 1.000 (n 2^20 + 5)   grad 0.776 (n 300001)   target's grad 0.583 (n 2^20 + 5)
  nll       loss 0.044 ((513, 7), ignore_index 1)   gradient bitwise equal in every case
  mcrmse    col 0.183, out 0.059 (both (3, 300))
Where the figures are above 0.5 they press on single roundings, not on the exponential or the logarithm: ce dl 0.610
and grad 0.518 sit at classes whose probability is below 5e-5, where g = p - ls / C is the rounded constant ls / C
and its subtraction (the u (ls / C + |g|) terms; p rel_p is 12 % of t there and 0.002 % at the other); mse g 1.000 is
the one rounding of d = p - t against its allowance u |2 d|, which is that rounding's own worst case; mse grad 0.776
and the target's gradient 0.583 (its exact negation, through the module) are the three roundings d = p - t,
grad_out / n and g sc against their allowance 3 u |grad|: all three terms of it, none to spare. The CPU emulation (correctly rounded exp and log) reaches the same largest figures
for the cross-entropy outputs (0.137 / 0.610 / 0.518). The __expf / __logf allowances (_EXP2_REL, _EXPF_ARG_REL,
_LOGF_ABS) remain unmeasured as such; the largest figures that depend on them are ce loss 0.137 and ce dl 0.402 at
ls = 0, which is their record.

What these tests found (fixed in losses.hip): a row whose first 64 logits are -inf, or any row with a -inf logit at
label_smoothing = 0, gave a NaN loss (ce loss (12,130) float32 ls 0.0: non-finite values [nan]): the online rescale
took exp(-inf - -inf), and the smoothing term multiplied 0 by (lse + inf). ce_fwd_kernel now takes the rescale factor
as 1 where the maximum does not move and a -inf lane's term as 0, and leaves the smoothing term out at ls = 0.
"""
import pytest
import torch

from ml_trainer_amd.ops._ext import require_native
from tests import helpers as H
from tests.helpers import (LOSS_ACC_B, LOSS_ACC_C, LOSS_CE_GRAD_OUT, LOSS_CE_SHAPES, LOSS_CE_SMOOTHING,
                           LOSS_MCRMSE_CASES, LOSS_NLL_CASES, LOSS_NLL_IGNORE, LOSS_POINTWISE_N, assert_guard_intact,
                           assert_within, bf16_t_used, guarded, guarded_1d, guarded_like, sentinel, store_bound)

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


def _hold(kernel, name, what, got, exp, t):
    """Every element of `got` (brought to the CPU) within the store's tolerance of exp given the fp32-level
    allowance t; prints the headroom (|err| / t for an fp32 output, helpers.bf16_t_used for a bf16 one)."""
    got = got.detach().cpu()
    exp, t = torch.as_tensor(exp, dtype=torch.float64), torch.as_tensor(t, dtype=torch.float64)
    exp, t = exp.expand(got.shape), t.expand(got.shape)
    assert bool(torch.isfinite(got.float()).all()), f"{kernel} {name} {what}: non-finite values {got.flatten()[:4].tolist()}"
    assert_within(got, exp, store_bound(exp, t, got.dtype), f"{kernel} {name} {what}")
    r = bf16_t_used(got, exp, t) if got.dtype == BF16 else float(((got.double() - exp).abs() / t).max())
    print(f"headroom {kernel} {name} {r:.4f} {what}")


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == BF16 else torch.int32)


def _vec(data=None, n=None, dev=None):
    """A guarded fp32 vector: (buf, view), the view holding `data` (flattened) or left as sentinels."""
    if data is not None:
        n, dev = data.numel(), data.device
    buf, view = guarded_1d(n, dev)
    if data is not None:
        view.copy_(data.reshape(-1))
    return buf, view


class Guards:
    """Collects (buf, view) pairs and checks them all."""

    def __init__(self):
        self.pairs = []

    def __call__(self, pair):
        self.pairs.append(pair)
        return pair[1]

    def check(self):
        torch.cuda.synchronize()
        for buf, view in self.pairs:
            assert_guard_intact(buf, view)


def _partials(dev):
    return sentinel((require_native().loss_partials_needed(),), F32, dev)


# --------------------------------------------------------------------------------------------- cross-entropy
_CE = {}


def _ce_case(B, C, dtype, ls, ignore_index=-100):
    """Inputs and fp64 references (one per grad_out) of a cross-entropy case, on the CPU: made once."""
    key = (B, C, dtype, ls, ignore_index)
    if key not in _CE:
        z, y = H.ce_edge_inputs(B, C, dtype, ls, ignore_index)
        _CE[key] = dict(z=z, y=y, acc=H.accuracy_expected(z, y),
                        bound={go: H.ce_bound(z, y, ignore_index, ls, go) for go in LOSS_CE_GRAD_OUT})
    return _CE[key]


def _run_ce(dev, B, C, dtype, ls, ignore_index=-100):
    Cx = require_native()
    c = _ce_case(B, C, dtype, ls, ignore_index)
    what = f"({B},{C}) {str(dtype)[6:]} ls {ls} ignore {ignore_index}"
    G = Guards()
    z = G(guarded_like(c["z"].to(dev)))
    y = c["y"].to(dev)
    zeros = lambda n: _vec(torch.zeros(n, device=dev))

    def forward():
        dl, acc, corr, loss = G(guarded(B, C, F32, dev)), G(zeros(2)), G(zeros(1)), G(_vec(n=1, dev=dev))
        Cx.ce_fwd(z, y, dl, acc, corr, loss, ignore_index, ls)
        G.check()
        return dl, acc, corr, loss

    dl, acc, corr, loss = forward()
    x, t = c["bound"][LOSS_CE_GRAD_OUT[0]]
    _hold("ce", "loss", what, loss, x["loss"], t["loss"])
    _hold("ce", "dl", what, dl, x["dl"], t["dl"])
    assert float(acc[1]) == x["n_valid"]
    assert bool((dl[~x["ok"].to(dev)] == 0).all())  # rows that do not count: exactly 0
    assert bool((dl[torch.isinf(z)] == 0).all())  # -inf classes (ls = 0 only): p = 0 exactly
    # the fused accuracy output: the explicit first-arg-max rule, and the stand-alone kernel on the same inputs
    hits, t_acc = c["acc"]
    _hold("ce", "correct", what, corr, hits, t_acc)
    alone = G(zeros(1))
    Cx.accuracy(z, y, alone)
    G.check()
    _hold("accuracy", "out", what, alone, hits, t_acc)
    assert abs(float(alone) - float(corr)) <= 2 * t_acc
    # a second run: the per-row gradient does not depend on the order of the atomics (the loss may)
    dl2, acc2, _, loss2 = forward()
    assert torch.equal(_bits(dl2), _bits(dl)) and torch.equal(acc2[1], acc[1])
    _hold("ce", "loss", what + " (second run)", loss2, x["loss"], t["loss"])

    for go in LOSS_CE_GRAD_OUT:
        x, t = c["bound"][go]
        gout = torch.tensor([go], dtype=F32, device=dev)
        outs = []
        for _ in range(2):
            out = G(guarded(B, C, dtype, dev))
            Cx.ce_bwd(dl, gout, acc, out)
            G.check()
            outs.append(out)
        _hold("ce", "grad_bf16" if dtype == BF16 else "grad", what + f" gout {go}", outs[0], x["grad"], t["grad"])
        assert bool((outs[0][~x["ok"].to(dev)] == 0).all())
        assert torch.equal(_bits(outs[0]), _bits(outs[1]))


@pytest.mark.parametrize("ls", LOSS_CE_SMOOTHING)
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,C", LOSS_CE_SHAPES)
def test_ce_edges(dev, B, C, dtype, ls):
    _run_ce(dev, B, C, dtype, ls)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,C", [(5, 10), (12, 130)])
def test_ce_in_range_ignore_index(dev, B, C, dtype):
    """ignore_index = 0: the last row's target is 0 and does not count; -100 is then just an out-of-range target."""
    c = _ce_case(B, C, dtype, 0.0, 0)
    assert int(c["y"][B - 1]) == 0 and not bool(c["bound"][LOSS_CE_GRAD_OUT[0]][0]["ok"][B - 1])
    _run_ce(dev, B, C, dtype, 0.0, 0)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ls", LOSS_CE_SMOOTHING)
def test_ce_module_strided_int32(dev, dtype, ls):
    """The special rows through CrossEntropyLoss: logits a column slice of a wider leaf, int32 targets."""
    from ml_trainer_amd.ops.losses import CrossEntropyLoss
    B, C = 12, 130
    c = _ce_case(B, C, dtype, ls)
    go = LOSS_CE_GRAD_OUT[0]
    x, t = c["bound"][go]
    base = torch.zeros(B, C + 3, dtype=dtype, device=dev)
    base[:, :C] = c["z"].to(dev)
    base.requires_grad_(True)
    z = base[:, :C]
    assert not z.is_contiguous()
    loss = CrossEntropyLoss(label_smoothing=ls)(z, c["y"].to(dev).to(torch.int32))
    (loss * go).backward()
    what = f"module ({B},{C}) {str(dtype)[6:]} ls {ls}"
    _hold("ce", "loss", what, loss.reshape(1), x["loss"], t["loss"])
    # the scaled gradient is stored in the logits' dtype, then copied into the leaf's slice unchanged
    _hold("ce", "grad_bf16" if dtype == BF16 else "grad", what, base.grad[:, :C], x["grad"], t["grad"])
    assert bool((base.grad[:, C:] == 0).all())


# -------------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", LOSS_ACC_C)
@pytest.mark.parametrize("B", LOSS_ACC_B)
def test_accuracy_edges(dev, B, C, dtype):
    from ml_trainer_amd.ops.losses import accuracy
    Cx = require_native()
    zc, yc = H.accuracy_edge_inputs(B, C, dtype)
    hits, t = H.accuracy_expected(zc, yc)
    what = f"({B},{C}) {str(dtype)[6:]}"
    G = Guards()
    z, y = G(guarded_like(zc.to(dev))), yc.to(dev)
    out = G(_vec(torch.zeros(1, device=dev)))
    Cx.accuracy(z, y, out)
    G.check()
    _hold("accuracy", "out", what, out, hits, t)
    _hold("accuracy", "out", what + " (ops.accuracy)", accuracy(z, y).reshape(1), hits, t)
    # the same rows through ce_fwd's fused output
    dl, acc, corr, loss = (G(guarded(B, C, F32, dev)), G(_vec(torch.zeros(2, device=dev))),
                           G(_vec(torch.zeros(1, device=dev))), G(_vec(n=1, dev=dev)))
    Cx.ce_fwd(z, y, dl, acc, corr, loss, -100, 0.0)
    G.check()
    _hold("ce", "correct", what, corr, hits, t)
    assert abs(float(corr) - float(out)) <= 2 * t


# ------------------------------------------------------------------------------------------ pointwise losses
_PW = {}


def _pw_case(n, mode, dtype=F32, go=3.0):
    key = (n, mode, dtype, go)
    if key not in _PW:
        p, t = H.pointwise_edge_inputs(n, dtype)
        _PW[key] = (p, t) + H.pointwise_loss_bound(p, t, mode, go)
    return _PW[key]


@pytest.mark.parametrize("mode", [0, 1], ids=["l1", "mse"])
@pytest.mark.parametrize("n", LOSS_POINTWISE_N)
def test_pointwise_edges(dev, n, mode):
    Cx = require_native()
    kernel = ("l1", "mse")[mode]
    pc, tc, x, tol = _pw_case(n, mode)
    nb = H.reg_blocks(n)
    G = Guards()
    p, t = G(_vec(pc.to(dev))), G(_vec(tc.to(dev)))
    gout = torch.tensor([3.0], dtype=F32, device=dev)
    runs = []
    for _ in range(2):
        g, d, stats, part = G(_vec(n=n, dev=dev)), G(_vec(n=n, dev=dev)), G(_vec(n=2, dev=dev)), _partials(dev)
        Cx.pointwise_loss_fwd(p, t, mode, g, part, stats)
        Cx.loss_scale_grad(g, gout, stats, d)
        G.check()
        assert_guard_intact(part, part[:nb])  # only the nb partials were written
        runs.append((g, d, stats))
    g, d, stats = runs[0]
    _hold(kernel, "loss", f"n {n}", stats[:1], x["loss"], tol["loss"])
    assert float(stats[1]) == n
    if mode == 0:
        assert torch.equal(g.cpu().double(), x["g"])  # sign(d), with sign(0) = 0
    else:
        _hold(kernel, "g", f"n {n}", g, x["g"], tol["g"])
    if n > 1:
        assert float(g[0]) == 0.0 and float(d[0]) == 0.0
    _hold(kernel, "grad", f"n {n}", d, x["grad"], tol["grad"])
    for a, b in zip(runs[0], runs[1]):  # fixed-order reductions: bitwise reproducible
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode", [0, 1], ids=["l1", "mse"])
def test_pointwise_module(dev, mode, dtype):
    """L1Loss / MSELoss on the shared partials scratch: the largest case first, then n = 1 (whose single partial sits
    beside 1023 stale ones), then a 2-D case; predictions in fp32 and bf16, the target requiring its gradient."""
    from ml_trainer_amd.ops.losses import L1Loss, MSELoss
    crit, kernel = (L1Loss(), "l1") if mode == 0 else (MSELoss(), "mse")
    for n in (LOSS_POINTWISE_N[-1], 1, 1025):
        pc, tc, x, tol = _pw_case(n, mode, dtype)
        p, t = pc.to(dev).requires_grad_(True), tc.to(dev).requires_grad_(True)
        if n == 1025:
            p, t = (a.detach().view(25, 41).requires_grad_(True) for a in (p, t))
        loss = crit(p, t)
        what = f"module n {n} {str(dtype)[6:]}"
        _hold(kernel, "loss", what, loss.reshape(1), x["loss"], tol["loss"])
        (loss * 3.0).backward()
        assert p.grad.dtype == dtype and t.grad.dtype == F32
        _hold(kernel, "grad_bf16" if dtype == BF16 else "grad", what, p.grad.reshape(-1), x["grad"], tol["grad"])
        _hold(kernel, "grad_target", what, t.grad.reshape(-1), -x["grad"], tol["grad"])
        assert torch.equal(crit(p, t), loss)


# ------------------------------------------------------------------------------------------------------- NLL
def _run_nll(dev, logp_c, y_c, ignore_index, what):
    Cx = require_native()
    B, C = logp_c.shape
    x, t = H.nll_bound(logp_c, y_c, ignore_index)
    nb = H.reg_blocks(B)
    G = Guards()
    logp, y = G(guarded_like(logp_c.to(dev))), y_c.to(dev)
    stats, part, d = G(_vec(n=2, dev=dev)), _partials(dev), G(guarded(B, C, F32, dev))
    gout = torch.tensor([0.5], dtype=F32, device=dev)
    Cx.nll_fwd(logp, y, ignore_index, part, stats)
    Cx.nll_bwd(y, C, ignore_index, gout, stats, d)
    G.check()
    assert_guard_intact(part, part[:2 * nb])
    _hold("nll", "loss", what, stats[:1], x["loss"], t)
    assert float(stats[1]) == x["n_valid"]
    assert torch.equal(d.cpu(), H.nll_grad_expected(y_c, C, ignore_index, 0.5))
    return stats


@pytest.mark.parametrize("ignore_index", LOSS_NLL_IGNORE)
@pytest.mark.parametrize("B,C", LOSS_NLL_CASES)
def test_nll_edges(dev, B, C, ignore_index):
    logp, y = H.nll_edge_inputs(B, C, ignore_index)
    if B >= 5:
        assert int(y[1]) == C and int(y[2]) == -100 and int(y[3]) == min(1, C - 1)
    _run_nll(dev, logp, y, ignore_index, f"({B},{C}) ignore {ignore_index}")


def test_nll_all_ignored(dev):
    """Nothing counts (ignore_index, -100 and an out-of-range target): loss 0 as ops/losses.py documents, gradient 0."""
    logp, _ = H.nll_edge_inputs(5, 3, 1)
    stats = _run_nll(dev, logp, torch.tensor([1, 1, -100, 3, 1]), 1, "all ignored")
    assert float(stats[0]) == 0.0 and float(stats[1]) == 0.0


# ---------------------------------------------------------------------------------------------------- mcrmse
@pytest.mark.parametrize("zero_col", [False, True], ids=["plain", "zerocol"])
@pytest.mark.parametrize("B,C", LOSS_MCRMSE_CASES)
def test_mcrmse_edges(dev, B, C, zero_col):
    from ml_trainer_amd.ops.losses import mcrmse
    Cx = require_native()
    pc, tc = H.mcrmse_edge_inputs(B, C, zero_col)
    x, tol = H.mcrmse_bound(pc, tc)
    what = f"({B},{C}) zero column {zero_col}"
    G = Guards()
    p, t = G(guarded_like(pc.to(dev))), G(guarded_like(tc.to(dev)))
    col, out = G(_vec(n=C, dev=dev)), G(_vec(n=1, dev=dev))
    Cx.mcrmse(p, t, col, out)
    G.check()
    _hold("mcrmse", "col", what, col, x["col"], tol["col"])
    _hold("mcrmse", "out", what, out, x["out"], tol["out"])
    if zero_col:
        assert float(col[0]) == 0.0  # sqrt(0) stays 0: the finite `out` above
    assert torch.equal(mcrmse(p, t).reshape(1), out)
