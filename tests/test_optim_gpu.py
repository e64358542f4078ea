"""The flat optimizer, grad-clip and bf16-cast kernels (csrc/kernels/optim.hip) on the GPU against
plain high-precision references.

Error budget of the optimizer comparisons. Three runs start from the same p0 and see the same
gradients: R = torch.optim on an fp64 CPU parameter (the reference; hyper-parameters as the Python
floats a user passes), T = the same torch.optim class on an fp32 CPU parameter (what fp32
arithmetic alone costs), K = the HIP kernel. Every compared tensor X (parameters and both state
buffers) must satisfy

    max|K - R| <= 4 * max|T - R| + 1e-7 * max|R|

4 = margin for fused multiply-adds and the device's expm1f / log1pf / sqrtf / division (a few ulp
each); the 1e-7 floor only covers tensors where T happens to be exact.

Measured max|K - R| / max|T - R| on an MI355X (test_kernel_matches_torch_optim, n = 4112, 6 steps;
"-" = no such buffer; "before" = the update rule as it was before this file existed):

    case                    p       s1      s2      s1, s2 before
    sgd_plain               1.00    -       -
    sgd_m_wd                1.01    0.95    -
    sgd_dampening           1.04    0.70    -
    sgd_nesterov_max        1.00    0.72    -
    adam_wd                 1.00    1.00    0.70    2.66, 61.02
    adam_betas_eps_max      1.00    1.00    0.79    1.36,  6.92
    adamw                   1.00    1.00    1.03    2.75, 82.30
    adagrad_decay_wd        1.00    1.00    -
    adagrad_defaults        1.00    1.00    -
    adamax_wd               1.00    1.00    1.00    2.78,  1.00
    sgd_m_wd_grad_scale     1.01    0.95    -

The "before" column is what these tests found. The kernel formed (1.f - beta2) from the fp32-rounded
beta2, and 1.f - (float)0.999 is 1.3e-5 (relative) away from 0.001: exp_avg_sq carried that error (a
hundred fp32 ulp), and so did 1 - powf(beta2, t). The two nearly cancel in the parameters, which is
why comparing parameters alone never showed it. mlt_optim.h now keeps 1 - beta, rounded once from
the host's double (make_opt_hyper), takes beta = 1.f - omb and the bias corrections as
-expm1f(t * log1pf(-omb)), and updates exp_avg as torch's lerp_ does (s1 + (1 - beta1) * (g - s1)).
The end-to-end tests (58 parameters, 6 steps) measure 0.60 - 1.00.
"""
import functools

import pytest
import torch

from ml_trainer_amd.ops._ext import require_native
from ml_trainer_amd.ops.optim import (FusedAdagrad, FusedAdam, FusedAdamax, FusedAdamW, FusedSGD,
                                      clip_grad_norm_flat)
from ml_trainer_amd.utils.flat import FlatParams

pytestmark = pytest.mark.gpu

KIND = {"sgd": 0, "adam": 1, "adamw": 2, "adagrad": 3, "adamax": 4}
TORCH_OPT = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "adamw": torch.optim.AdamW,
             "adagrad": torch.optim.Adagrad, "adamax": torch.optim.Adamax}
# torch.optim state entries that the kernel keeps in s1 / s2
STATE_KEYS = {"sgd": ("momentum_buffer", None), "adam": ("exp_avg", "exp_avg_sq"),
              "adamw": ("exp_avg", "exp_avg_sq"), "adagrad": ("sum", None), "adamax": ("exp_avg", "exp_inf")}
DEFAULT_EPS = {"sgd": 0.0, "adam": 1e-8, "adamw": 1e-8, "adagrad": 1e-10, "adamax": 1e-8}

# (id, kind, torch.optim keyword arguments)
CASES = [
    ("sgd_plain", "sgd", dict(lr=0.1)),
    ("sgd_m_wd", "sgd", dict(lr=0.1, momentum=0.9, weight_decay=0.01)),
    ("sgd_dampening", "sgd", dict(lr=0.1, momentum=0.9, dampening=0.1)),
    ("sgd_nesterov_max", "sgd", dict(lr=0.1, momentum=0.9, nesterov=True, maximize=True)),
    ("adam_wd", "adam", dict(lr=0.01, weight_decay=0.01)),
    ("adam_betas_eps_max", "adam", dict(lr=0.01, betas=(0.8, 0.99), eps=1e-6, maximize=True)),
    ("adamw", "adamw", dict(lr=0.01, weight_decay=0.05)),
    ("adagrad_decay_wd", "adagrad", dict(lr=0.05, lr_decay=0.01, weight_decay=0.01)),
    ("adagrad_defaults", "adagrad", dict(lr=0.05)),
    ("adamax_wd", "adamax", dict(lr=0.01, weight_decay=0.01)),
]
CASE_BY_ID = {c[0]: c for c in CASES}
# one fixed setting per kind (the property test in test_property_gpu.py draws from these)
CASE_OF_KIND = {"sgd": "sgd_m_wd", "adam": "adam_wd", "adamw": "adamw", "adagrad": "adagrad_decay_wd",
                "adamax": "adamax_wd"}
N_MAIN, STEPS_MAIN = 4112, 6  # 1028 float4s: four full blocks + a four-thread tail


# ---------------------------------------------------------------------------------------------
# shared helpers
# ---------------------------------------------------------------------------------------------
def flat_optim(C, kind, hp, p, g, s1, s2, t_host=1.0, grad_scale=1.0, lr=None, lr_t=None, lr_index=None,
               step_t=None, shadow=None, coef=None):
    """One C.flat_optim call with the hyper-parameters given as torch.optim keyword arguments."""
    betas = hp.get("betas", (0.9, 0.999))
    C.flat_optim(p, g, s1, s2, KIND[kind], hp["lr"] if lr is None else lr, hp.get("momentum", 0.0),
                 hp.get("dampening", 0.0), hp.get("weight_decay", 0.0), betas[0], betas[1],
                 hp.get("eps", DEFAULT_EPS[kind]), hp.get("lr_decay", 0.0), grad_scale,
                 hp.get("nesterov", False), hp.get("maximize", False), lr_t, lr_index, step_t, float(t_host),
                 shadow, coef)


def make_inputs(n, steps, seed):
    """p0 = randn; per step a fresh gradient randn * U(0.25, 2), magnitudes below 0.05 raised to 0.05
    (keeps the Adam-family denominators away from eps). CPU generator, fp32."""
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen)
    grads = []
    for _ in range(steps):
        g = torch.randn(n, generator=gen) * (0.25 + 1.75 * torch.rand(n, generator=gen))
        g = torch.where(g.abs() < 0.05, torch.copysign(torch.full_like(g, 0.05), g), g)
        grads.append(g)
    return p0, grads


def torch_run(kind, hp, p0, grads, dtype):
    """(p, s1, s2) after torch.optim stepped a `dtype` CPU parameter through `grads`."""
    p = torch.nn.Parameter(p0.to(dtype).clone())
    opt = TORCH_OPT[kind]([p], **hp)
    for g in grads:
        p.grad = g.to(dtype).clone()
        opt.step()
    k1, k2 = STATE_KEYS[kind]
    st = opt.state[p]
    return p.detach(), (st.get(k1) if k1 else None), (st.get(k2) if k2 else None)


def kernel_run(C, dev, kind, hp, p0, grads, grad_scale=1.0, grad_mul=1.0):
    p = p0.to(dev)
    s1, s2 = torch.zeros_like(p), torch.zeros_like(p)
    for t, g in enumerate(grads, 1):
        flat_optim(C, kind, hp, p, (g * grad_mul).to(dev), s1, s2, t_host=t, grad_scale=grad_scale)
    return p, s1, s2


def budget_ratio(what, K, R, T):
    """Assert max|K-R| <= 4 max|T-R| + 1e-7 max|R|; prints and returns max|K-R| / max|T-R|."""
    R = R.detach().double().cpu()
    eK = (K.detach().double().cpu() - R).abs().max().item()
    eT = (T.detach().double().cpu() - R).abs().max().item()
    bound = 4.0 * eT + 1e-7 * R.abs().max().item()
    ratio = eK / eT if eT > 0 else (0.0 if eK == 0 else float("inf"))
    print(f"[budget] {what}: max|K-R| {eK:.3e}  max|T-R| {eT:.3e}  ratio {ratio:.2f}  bound {bound:.3e}")
    assert eK <= bound, f"{what}: max|K-R| {eK:.3e} > 4 * {eT:.3e} + 1e-7 * max|R| = {bound:.3e}"
    return ratio


@functools.lru_cache(maxsize=None)
def reference(case_id, n=N_MAIN, steps=STEPS_MAIN, seed=1234):
    """(p0, grads, R, T) of a case: computed once, shared by the tests, never modified."""
    _, kind, hp = CASE_BY_ID[case_id]
    p0, grads = make_inputs(n, steps, seed)
    return p0, grads, torch_run(kind, hp, p0, grads, torch.float64), torch_run(kind, hp, p0, grads, torch.float32)


def bits16(t):
    return t.detach().contiguous().view(torch.int16)


def check_against_reference(what, K, R, T):
    for name, k, r, t in zip(("p", "s1", "s2"), K, R, T):
        if r is None:  # this kind keeps no such buffer
            continue
        budget_ratio(f"{what} {name}", k, r, t)


# ---------------------------------------------------------------------------------------------
# flat_optim_kernel vs torch.optim
# ---------------------------------------------------------------------------------------------
# the last id: sgd_m_wd once more with gradients 8x too large and grad_scale = 1/8 (powers of two: exact)
@pytest.mark.parametrize("case_id,grad_scale", [(c[0], 1.0) for c in CASES] + [("sgd_m_wd", 0.125)],
                         ids=[c[0] for c in CASES] + ["sgd_m_wd_grad_scale"])
def test_kernel_matches_torch_optim(dev, case_id, grad_scale):
    C = require_native()
    _, kind, hp = CASE_BY_ID[case_id]
    p0, grads, R, T = reference(case_id)
    K = kernel_run(C, dev, kind, hp, p0, grads, grad_scale=grad_scale, grad_mul=1.0 / grad_scale)
    check_against_reference(f"{case_id} grad_scale {grad_scale}", K, R, T)


@pytest.mark.parametrize("case_id", ["sgd_m_wd", "adamw"])
def test_device_lr_step_coef_paths_are_bitwise_host_paths(dev, case_id):
    C = require_native()
    _, kind, hp = CASE_BY_ID[case_id]
    n = 1040
    p0, grads = make_inputs(n, 7, 77)
    table = torch.tensor([0.1, 0.05, 0.2, 0.0125, 0.075], dtype=torch.float32, device=dev)
    host = [p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
    devp = [t.clone() for t in host]

    def same(what):
        for name, a, b in zip(("p", "s1", "s2"), host, devp):
            assert torch.equal(a, b), f"{case_id} {what}: {name} differs between host and device arguments"

    for i in range(5):  # lr table + lr_index + step from device memory; the host lr / t are decoys
        g = grads[i].to(dev)
        flat_optim(C, kind, hp, host[0], g, host[1], host[2], t_host=i + 1, lr=float(table[i]))
        idx = torch.tensor([i + 1], dtype=torch.int64, device=dev)
        flat_optim(C, kind, hp, devp[0], g, devp[1], devp[2], t_host=99, lr=123.0, lr_t=table, lr_index=idx,
                   step_t=idx.clone())
        same(f"step {i + 1}")
    # lr_t without lr_index reads element 0
    g = grads[5].to(dev)
    flat_optim(C, kind, hp, host[0], g, host[1], host[2], t_host=6, lr=float(table[0]))
    flat_optim(C, kind, hp, devp[0], g, devp[1], devp[2], t_host=99, lr=123.0, lr_t=table,
               step_t=torch.tensor([6], dtype=torch.int64, device=dev))
    same("lr_t[0]")
    # coef multiplies grad_scale
    g = grads[6].to(dev)
    flat_optim(C, kind, hp, host[0], g, host[1], host[2], t_host=7, grad_scale=0.125)
    flat_optim(C, kind, hp, devp[0], g, devp[1], devp[2], t_host=7, grad_scale=0.5,
               coef=torch.tensor([0.25], dtype=torch.float32, device=dev))
    same("coef")
    assert not torch.equal(host[0], p0.to(dev))  # the steps did something


@pytest.mark.parametrize("n", [2_100_260, 16, 1040])  # n4 = 2048 * 256 + 1041; the FlatParams minimum; 4 blocks + tail
def test_grid_stride_indexing_shadow_and_bounds(dev, n):
    C = require_native()
    PAD, SENT, SENT16 = 64, -1234.0, -3.5
    bufs = {k: torch.full((n + PAD,), SENT, dtype=torch.float32, device=dev) for k in ("p", "g", "s1", "s2")}
    sh_full = torch.full((n + PAD,), SENT16, dtype=torch.bfloat16, device=dev)
    p, g, s1, s2 = (bufs[k][:n] for k in ("p", "g", "s1", "s2"))
    shadow = sh_full[:n]
    i = torch.arange(n, dtype=torch.int64)
    p0 = (i % 4093).double() / 8
    g0 = ((7 * i) % 1021).double() / 4
    p.copy_(p0.float())
    g.copy_(g0.float())

    def tails_untouched(what):
        for k, b in bufs.items():
            assert torch.equal(b[n:], torch.full((PAD,), SENT, device=dev)), f"{what}: wrote past the end of {k}"
        assert torch.equal(sh_full[n:], torch.full((PAD,), SENT16, dtype=torch.bfloat16, device=dev)), \
            f"{what}: wrote past the end of the shadow"

    # plain SGD, lr 0.5: every result is exact in fp32 -> any wrong or skipped index shows
    flat_optim(C, "sgd", dict(lr=0.5), p, g, s1, s2, shadow=shadow)
    expected = (p0 - 0.5 * g0).float().to(dev)
    assert torch.equal(p, expected)
    assert torch.equal(bits16(shadow), bits16(p.to(torch.bfloat16)))
    assert torch.equal(g, g0.float().to(dev))
    for k in ("s1", "s2"):  # plain SGD keeps no state: not even the body is touched
        assert torch.equal(bufs[k], torch.full((n + PAD,), SENT, device=dev))
    tails_untouched("sgd")

    # one AdamW step (reads and writes both state buffers): tails and shadow
    s1.zero_()
    s2.zero_()
    shadow.fill_(SENT16)
    before = p.clone()
    flat_optim(C, "adamw", dict(lr=0.01, weight_decay=0.05), p, g, s1, s2, t_host=1, shadow=shadow)
    assert torch.equal(bits16(shadow), bits16(p.to(torch.bfloat16)))
    assert not torch.equal(p, before)
    tails_untouched("adamw")


# ---------------------------------------------------------------------------------------------
# cast_bf16_kernel
# ---------------------------------------------------------------------------------------------
SPECIAL_BITS = [
    0x3F808000,  # tie, rounds to even (down)
    0x3F818000,  # tie, rounds to even (up)
    0x3F808001,  # just above the tie
    0x7F7FFFFF,  # largest finite fp32 -> inf
    0x00000000, 0x80000000,  # +-0
    0x7F800000, 0xFF800000,  # +-inf
    0x00800000,  # smallest normal
    0x00400000,  # subnormal
    0x7F7F7FFF,  # just below the tie under the largest finite bf16
    0xBF808000, 0xBF818000, 0xBF808001,  # negatives of the ties
    0x00000001,  # smallest subnormal -> 0
    0x00008000,  # tie between 0 and the smallest bf16 subnormal -> 0
]


def _from_bits(bits):
    return torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)


def _cast(C, dev, x):
    y = torch.full(x.shape, -3.5, dtype=torch.bfloat16, device=dev)
    C.cast_bf16(x.to(dev), y)
    return y.cpu()


def test_cast_bf16_matches_torch_rounding(dev):
    C = require_native()
    x = _from_bits(SPECIAL_BITS)
    assert x.numel() == 16
    got, want = _cast(C, dev, x), x.to(torch.bfloat16)
    assert torch.equal(bits16(got), bits16(want)), \
        [(hex(b), hex(a & 0xFFFF), hex(w & 0xFFFF)) for b, a, w in
         zip(SPECIAL_BITS, bits16(got).tolist(), bits16(want).tolist()) if a != w]
    gen = torch.Generator().manual_seed(5)
    for n in (1040, 525_620):  # 525_620 / 4 > 512 * 256: past one stride of a capped grid
        x = torch.randn(n, generator=gen) * torch.pow(10.0, torch.rand(n, generator=gen) * 60 - 30)
        assert torch.equal(bits16(_cast(C, dev, x)), bits16(x.to(torch.bfloat16)))
    # NaN stays NaN (payload free), neighbours unaffected
    x = torch.arange(16, dtype=torch.float32) + 0.5
    x[[0, 5, 15]] = float("nan")
    x[6] = _from_bits([0x7F800001])[0]  # signalling NaN with the payload in the dropped bits
    got = _cast(C, dev, x)
    nan = x.isnan()
    assert torch.equal(got.float().isnan(), nan)
    assert torch.equal(bits16(got)[~nan], bits16(x.to(torch.bfloat16))[~nan])


def test_refresh_shadow_matches_torch_rounding(dev):
    require_native()
    gen = torch.Generator().manual_seed(6)
    ps = [torch.nn.Parameter(torch.randn(37, 5, generator=gen).to(dev)),
          torch.nn.Parameter((torch.randn(11, generator=gen) * 1e-3).to(dev))]
    fp = FlatParams(ps)
    sh = fp.refresh_shadow()
    assert sh.dtype == torch.bfloat16 and sh.numel() == fp.numel
    assert torch.equal(bits16(sh), bits16(fp.data.to(torch.bfloat16)))
    with torch.no_grad():
        ps[0].mul_(1.2345)  # an edit through a view bumps the master's version
    assert torch.equal(bits16(fp.refresh_shadow()), bits16(fp.data.to(torch.bfloat16)))
    assert torch.equal(bits16(fp.shadow_view(ps[1])), bits16(ps[1].detach().to(torch.bfloat16)))


# ---------------------------------------------------------------------------------------------
# sq_norm_kernel / clip_coef_kernel / clip_grad_norm_flat
# ---------------------------------------------------------------------------------------------
def _flat_with_grad(dev, x):
    """A device FlatParams of one x-sized parameter whose gradient is x (the align-16 padding stays 0)."""
    fp = FlatParams([torch.nn.Parameter(torch.zeros(x.numel(), device=dev))])
    fp.grad[:x.numel()].copy_(x)
    return fp


@pytest.mark.parametrize("n", [16, 1040, 525_620])  # 525_620 / 4 > 512 * 256: sq_norm grid-strides
def test_sq_norm_and_clip(dev, n):
    C = require_native()
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    xd = x.to(dev)
    # rtol: the longest chain is < 600 fp32 adds of non-negative terms (per-thread loop, six wave levels,
    # four wave sums, <= 512 block partials): <= 600 * 2^-24 = 3.6e-5
    want_sq = x.double().square().sum().item()
    for junk in (0.0, 777.0, float("nan")):  # out is overwritten, whatever it held
        out = torch.full((1,), junk, dtype=torch.float32, device=dev)
        C.sq_norm(xd, out)
        assert out.item() == pytest.approx(want_sq, rel=1e-4)

    norm = want_sq ** 0.5
    for max_norm in (0.25 * norm, 2.0 * norm):  # clipping / not clipping
        fp = _flat_with_grad(dev, xd)
        p64 = torch.nn.Parameter(torch.zeros(n, dtype=torch.float64))
        p64.grad = x.double().clone()
        want_total = torch.nn.utils.clip_grad_norm_([p64], max_norm)
        total = clip_grad_norm_flat(fp, max_norm)
        assert total.item() == pytest.approx(want_total.item(), rel=1e-4)
        if max_norm < norm:
            torch.testing.assert_close(fp.grad[:n].cpu().double(), p64.grad, rtol=1e-4, atol=0)
            assert fp.grad.double().norm().item() == pytest.approx(max_norm, rel=1e-4)
        else:
            assert torch.equal(fp.grad[:n], xd)  # bitwise unchanged
        assert (fp.grad[n:] == 0).all()


def test_sq_norm_and_clip_are_bitwise_reproducible(dev):
    require_native()
    n = 525_620
    xd = torch.randn(n, generator=torch.Generator().manual_seed(9)).to(dev)
    fp = _flat_with_grad(dev, xd)
    first = None
    for _ in range(20):
        fp.grad[:n].copy_(xd)
        total = clip_grad_norm_flat(fp, 1.0).clone()
        if first is None:
            first = (total, fp.grad.clone())
            assert not torch.equal(fp.grad[:n], xd)  # it clipped
        else:
            assert torch.equal(total, first[0]) and torch.equal(fp.grad, first[1])


# ---------------------------------------------------------------------------------------------
# Fused* optimizer classes end to end on the device
# ---------------------------------------------------------------------------------------------
E2E = {
    "sgd": (FusedSGD, dict(momentum=0.9, weight_decay=0.01)),
    "adam": (FusedAdam, dict(weight_decay=0.01)),
    "adamw": (FusedAdamW, dict(weight_decay=0.05)),
    "adagrad": (FusedAdagrad, dict(lr_decay=0.01, weight_decay=0.01)),
    "adamax": (FusedAdamax, dict(weight_decay=0.01)),
}
E2E_LRS = (0.02, 0.05)  # two param groups


def _model(device, dtype=torch.float32):
    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))
    return m.to(device=device, dtype=dtype)  # fp32 -> fp64 is exact: every run starts from the same values


def _groups(m, lrs=E2E_LRS):
    return [{"params": list(m[i].parameters()), "lr": lrs[i]} for i in range(2)]


def _inputs(steps, seed=11):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(4, 7, generator=gen) for _ in range(steps)]


def _train_step(m, opt, x):
    p = next(m.parameters())
    opt.zero_grad()
    m(x.to(device=p.device, dtype=p.dtype)).square().sum().backward()
    opt.step()


def _train(m, opt, xs, sched=None):
    for x in xs:
        _train_step(m, opt, x)
        if sched is not None:
            sched.step()
    return m


def _all_params(m):
    return torch.cat([p.detach().reshape(-1).double().cpu() for p in m.parameters()])


def _torch_e2e(kind, hp, xs, dtype, lrs=E2E_LRS, steplr=False):
    m = _model("cpu", dtype)
    opt = TORCH_OPT[kind](_groups(m, lrs), **hp)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5) if steplr else None
    return _all_params(_train(m, opt, xs, sched))


@pytest.mark.parametrize("kind", list(E2E))
def test_fused_optimizers_end_to_end_on_device(dev, kind):
    """The 58 parameters are compared as one vector: the budget's yardstick max|T-R| is a maximum
    over elements and a three-element bias alone is too small a sample for it."""
    require_native()
    cls, hp = E2E[kind]
    xs = _inputs(7)
    m = _model(dev)
    opt = cls(_groups(m), lr=E2E_LRS[0], **hp)
    assert len(opt.flats) == 2
    for fp in opt.flats:
        fp.refresh_shadow()
    m2 = opt2 = None
    for i, x in enumerate(xs[:6]):
        _train_step(m, opt, x)
        for fp in opt.flats:  # the kernel rewrote the shadow with the new weights
            assert fp._shadow_ver == fp.data._version
            assert torch.equal(bits16(fp.shadow), bits16(fp.data.to(torch.bfloat16))), f"stale shadow after step {i + 1}"
        if m2 is not None:
            _train_step(m2, opt2, x)
        if i == 2:  # resume from a checkpoint in a fresh model + optimizer
            m2 = _model(dev)
            m2.load_state_dict(m.state_dict())
            opt2 = cls(_groups(m2), lr=123.0, **hp)
            opt2.load_state_dict(opt.state_dict())
    for p, q in zip(m.parameters(), m2.parameters()):
        assert torch.equal(p, q), "resumed run diverged from the uninterrupted one"

    R = _torch_e2e(kind, hp, xs[:6], torch.float64)
    T = _torch_e2e(kind, hp, xs[:6], torch.float32)
    budget_ratio(f"e2e {kind} params", _all_params(m), R, T)

    for gi, fp in enumerate(opt.flats):
        pad = torch.ones(fp.numel, dtype=torch.bool, device=dev)
        for p, o in zip(fp.params, fp.offsets):
            pad[o:o + p.numel()] = False
        assert pad.any()
        assert (fp.data[pad] == 0).all(), "padding of the flat parameter buffer is no longer zero"
        for s in opt.state_buffers(gi):
            assert s is None or torch.isfinite(s).all()

    # an edit outside the optimizer, then a step: the stale shadow is neither given to the kernel nor served
    for fp in opt.flats:
        with torch.no_grad():
            fp.data.mul_(1.25)
    _train_step(m, opt, xs[6])

    def shadow_views_fresh():
        return all(torch.equal(bits16(fp.shadow_view(p)), bits16(p.detach().to(torch.bfloat16)))
                   for fp in opt.flats for p in fp.params)

    assert shadow_views_fresh()
    m.load_state_dict({k: v * 0.75 for k, v in m.state_dict().items()})  # an edit through the parameters
    assert shadow_views_fresh()


def test_fused_sgd_follows_steplr_on_device(dev):
    require_native()
    hp, lrs, xs = dict(momentum=0.9), (0.08, 0.04), _inputs(6, seed=12)
    m = _model(dev)
    opt = FusedSGD(_groups(m, lrs), lr=lrs[0], **hp)
    _train(m, opt, xs, torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5))
    assert opt.param_groups[1]["lr"] == pytest.approx(lrs[1] / 64)
    R = _torch_e2e("sgd", hp, xs, torch.float64, lrs, steplr=True)
    T = _torch_e2e("sgd", hp, xs, torch.float32, lrs, steplr=True)
    budget_ratio("e2e sgd StepLR params", _all_params(m), R, T)


def test_fused_cpu_and_device_branches_agree(dev):
    """FusedAdam's CPU branch (_cpu_update) and device branch (the kernel), both within the budget of
    the same fp64 torch.optim run."""
    require_native()
    cls, hp = E2E["adam"]
    xs = _inputs(6, seed=13)
    R = _torch_e2e("adam", hp, xs, torch.float64)
    T = _torch_e2e("adam", hp, xs, torch.float32)
    for device in ("cpu", dev):
        m = _model(device)
        _train(m, cls(_groups(m), lr=E2E_LRS[0], **hp), xs)
        budget_ratio(f"e2e adam branch {torch.device(device).type}", _all_params(m), R, T)
