"""GEMM edge paths (gemm.hip, gemm_tile.hip, gemm_w4.hip, transpose.hip): odd M / N, strided and
misaligned C / aux / res / bias, the tail and demoted store paths of every epilogue, and the host
predicates that demote configuration 7 -- all on GUARDED outputs.

Every output and side operand is a view inside a sentinel-filled buffer (helpers.guarded): a store
one column past N or into row M changes a sentinel and fails the test. Every input is a view inside
a NaN-filled buffer: an over-read that reaches a stored output makes it NaN. Results are held to the
derived per-element tolerance of helpers.gemm_bound against an fp64 reference, and where a kernel is
forced the planner is asked first that the case reaches it.

Each test prints `headroom <group> <dtype> <figure>` (pytest -s shows them): for fp32 outputs the largest
|err| / tolerance, for bf16 outputs the largest fraction of the fp32-level allowance that the stored
value needs (helpers.bf16_t_used; the rounding of a correct bf16 store alone reaches its tolerance).
`<group>-gelu-out` is |err| / tolerance of the GELU output against GELU of the kernel's own aux.

Branch -> the test that reaches it:
  scalar tail stores (gn + q < N), C / aux / res ......... test_cfg0_* (N = 1, 37, 131, 126), test_tile_kernels_* (197)
  misaligned-pointer branches of epilogue_store4 ......... the `odd` / `oddld` / `oddoff` placements of the same tests
  4-byte-aligned bias ..................................... every bias of those tests (bias_off = 1)
  kind = -1 demotion in epi_side, epi_store8 refused ..... test_side_operand_paths_demote_bitwise
  N % 4 != 0 veto of the external split-K reduce ......... test_split_k_external_reduce_veto_and_guarded_reduce
  external reduce into a strided C ........................ the same test, (264, 200, 320), ldc = N + 4
  cfg 7 -> ping-pong on odd ldc / ldaux / ldres / bias ... test_cfg7_and_demotion_to_pingpong, test_gemm_f8_cfg7_*
  gemm_w4_wgrad_supported accept / refuse ................. test_cfg7_weight_gradient_form
  fp8 tiles, tails, odd ldc; gemm_f8_q strided Y / Y^T ... test_gemm_f8_*

Measured on an MI355X (largest figure per group; fp32 |err| / tolerance, bf16 fraction of the allowance):
cfg 0 0.041 / 0.0025, 256-wide tiles 0.0037 / 0.0009, ping-pong 0.0044 / 0.0006, cfg 7 0.0032 / 0.0004,
fp8 0.48 / 0.30 (the 128-deep block MFMA adds its products less exactly than an fp32 chain; still inside
the K-additions allowance), colsum 0.10. GELU output against its own aux: 0.9961 = 1 / (1 + 2^-8), the
worst case of one correct bf16 rounding, which that tolerance is."""
import pytest
import torch

from ml_trainer_amd.ops._ext import require_native
from tests.helpers import (assert_guard_intact, assert_within, bf16_t_used, dgelu_t, gelu64, gelu_grad64,
                           gelu_out_bound, gemm_expected, gemm_t32, guarded, guarded_like, sentinel, store_bound,
                           tanh_t)

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
F8 = {0: torch.float8_e4m3fn, 1: torch.float8_e5m2}
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
_HEADROOM = {}


def _note(group, dtype, ratio, what=""):
    key = (group, "bf16" if dtype == BF16 else "fp32")
    _HEADROOM[key] = max(_HEADROOM.get(key, 0.0), ratio)
    print(f"headroom {key[0]} {key[1]} {ratio:.4f} {what}")


def _check(group, out, exp, t, what, stat=None):
    """out within the store's tolerance of exp, given the fp32-level allowance t; notes the headroom:
    |err| / t for fp32 outputs, the fraction of t needed for bf16 outputs (helpers.bf16_t_used) -- over
    the elements of mask `stat` when given (the assertion always covers every element). Returns the
    tolerance."""
    tol = store_bound(exp, t, out.dtype)
    assert_within(out, exp, tol, what)
    if stat is not None:
        out, exp, t = out[stat], exp[stat], t[stat]
    if out.numel():
        r = float(((out.double() - exp).abs() / t).max()) if out.dtype == F32 else bf16_t_used(out, exp, t)
        _note(group, out.dtype, r, what)
    return tol


def _r8(x):
    return (x + 7) // 8 * 8


def _mk(shape, g, dev, scale=0.5):
    return (torch.randn(*shape, generator=g) * scale).to(BF16).to(dev)


def _in(data):
    """An input operand inside a NaN surround: 16-byte aligned base, row stride a multiple of 8."""
    return guarded_like(data, ld=_r8(data.shape[1]) + 16, col_off=8)[1]


def _ld(N, kind):
    """(ld, col_off) of an [M, N] view whose base is 16-byte aligned for either element size:
    `al` rows 16-byte aligned (ld % 8 == 0, larger than N); `q4` ld % 4 == 0 but % 8 != 0 (N + 4 when
    N % 8 == 0); `odd` an odd ld (N + 13 for even N)."""
    if kind == "al":
        return _r8(N) + 8, 8
    if kind == "q4":
        ld = N + 4
        while ld % 8 != 4:
            ld += 1
        return ld, 4
    assert kind == "odd"
    ld = N + 13 + (N % 2)
    return ld, (-ld) % 8


def _side_ld(N, kind):
    """(ld, col_off) of a bf16 [M, N] side operand (aux / res): `al`, `q4`, `odd` as _ld; `oddld` an odd
    row stride and whatever base that gives; `oddoff` a 16-byte row stride on an odd element offset (the
    pointer is 2-byte aligned only)."""
    if kind == "oddld":
        return N + 11 + (N % 2), 3
    if kind == "oddoff":
        return _r8(N) + 8, 1
    return _ld(N, kind)


def _side(data, kind):
    return guarded_like(data, *_side_ld(data.shape[1], kind))


def _bias(data, off):
    """bias [N] at element `off` of a sentinel fp32 buffer: off = 1 is 4-byte aligned only, 4 is 16."""
    buf = sentinel((data.numel() + 8,), F32, data.device)
    v = buf[off:off + data.numel()]
    v.copy_(data)
    return buf, v


class Case:
    """One GEMM problem: guarded inputs, fp64 operands in the mathematical layout, epilogue data."""

    def __init__(self, dev, a_mn, b_mn, M, N, K, seed):
        # an mn-contiguous operand's M / N is rounded up to a multiple of 8, as the binding requires
        self.M, self.N, self.K = (_r8(M) if a_mn else M), (_r8(N) if b_mn else N), K
        self.a_mn, self.b_mn, self.dev = a_mn, b_mn, dev
        M, N = self.M, self.N
        g = torch.Generator().manual_seed(seed)
        self.A = _in(_mk((K, M) if a_mn else (M, K), g, dev))
        self.B = _in(_mk((K, N) if b_mn else (N, K), g, dev))
        self.A64 = self.A.double().t() if a_mn else self.A.double()
        self.B64 = self.B.double() if b_mn else self.B.double().t()
        self.bias = torch.randn(N, generator=g).to(dev)
        self.res = _mk((M, N), g, dev, 1.0)
        self.pre = _mk((M, N), g, dev, 2.0)                 # a given pre-activation for dGELU
        self.prev = torch.randn(M, N, generator=g).to(dev)  # previous C for accumulate

    def plan(self, C, cfg, splits, accumulate=False):
        return tuple(C.gemm_plan(bool(self.a_mn), bool(self.b_mn), self.M, self.N, self.K, cfg, splits, accumulate))

    def run(self, C, epi, out_dtype, group, ckind="odd", skind="oddld", cfg=-1, splits=0, bias_off=1):
        """One call of epilogue `epi` into a guarded C (and aux); asserts guards, finiteness and the
        bound; returns the written views (C, aux) for comparisons between runs and leaves the tolerance of
        C (GELU: of aux) in self.last_tol."""
        M, N, K, dev = self.M, self.N, self.K, self.dev
        cbuf, cv = guarded(M, N, out_dtype, dev, *_ld(N, ckind))
        kw, terms, guards = {"cfg": cfg, "splits": splits}, {}, [(cbuf, cv)]
        if epi in ("bias", "bra", "gelu", "tanh"):
            bbuf, kw["bias"] = _bias(self.bias, bias_off)
            guards.append((bbuf, kw["bias"]))
            terms["bias"] = self.bias.double()
        if epi in ("res", "bra"):
            rbuf, kw["res"] = _side(self.res, skind)
            guards.append((rbuf, kw["res"]))
            terms["res"] = self.res.double()
        if epi == "bra":
            kw["alpha"] = terms["alpha"] = 0.5
        if epi == "gelu":
            abuf, av = guarded(M, N, BF16, dev, *_side_ld(N, skind))  # aux is an OUTPUT here: all sentinel
            kw.update(aux=av, mode=1)
            guards.append((abuf, av))
        if epi == "dgelu":
            abuf, av = _side(self.pre, skind)
            kw.update(aux=av, mode=2)
            guards.append((abuf, av))
        if epi == "tanh":
            kw["mode"] = 3
        if epi == "acc":
            cv.copy_(self.prev)
            kw["accumulate"] = True
            terms["c_prev"] = self.prev.double()
        C.gemm(self.A, self.B, cv, bool(self.a_mn), bool(self.b_mn), **kw)
        for buf, v in guards:
            assert_guard_intact(buf, v)
        assert bool(torch.isfinite(cv).all()), f"{epi}: non-finite output"
        exp = gemm_expected(self.A64, self.B64, terms)
        t32 = gemm_t32(self.A64, self.B64, K, terms)
        what = f"{group} {epi} {out_dtype} ldc={cv.stride(0)} cfg={cfg} splits={splits}"
        stat = None
        if epi == "gelu":
            assert bool(torch.isfinite(av).all()), "gelu: non-finite aux"
            self.last_tol = _check(group, av, exp, t32, what + " aux")
            a64 = av.double()
            _note(group + "-gelu-out", out_dtype, assert_within(cv, gelu64(a64), gelu_out_bound(a64), what))
            return cv, av
        if epi == "dgelu":
            a64 = self.pre.double()
            exp, t32, group = exp * gelu_grad64(a64), dgelu_t(exp, t32, a64), group + "-dgelu"
            # headroom over the table's exact range: at |aux| >= 8 the kernels' limit entry (0 or 1) is
            # the whole allowance there (an output of exactly 0 against an expected 1e-14)
            stat = (a64.abs() >= 2.0 ** -20) & (a64.abs() < 8.0)
        elif epi == "tanh":
            exp, t32, group = torch.tanh(exp), tanh_t(t32), group + "-tanh"
        self.last_tol = _check(group, cv, exp, t32, what, stat)
        return cv, None


# epilogue, output dtypes it is checked with (GELU / tanh: bf16 outputs; accumulate needs fp32)
EPILOGUES = [("plain", (BF16, F32)), ("bra", (BF16, F32)), ("gelu", (BF16,)), ("dgelu", (BF16, F32)),
             ("acc", (F32,)), ("tanh", (BF16,))]
# C row stride with the side-operand placement it is paired with
STRIDES = [("odd", "oddld"), ("q4", "oddoff")]


# ---- a. the 128 x 128 register-staged kernel (cfg 0) ---------------------------------------------
@pytest.mark.parametrize("a_mn,b_mn", LAYOUTS)
@pytest.mark.parametrize("M,N,K", [(1, 1, 8),        # smallest legal shape
                                   (33, 37, 40),     # one partial tile, K shorter than BK, N % 4 = 1
                                   (129, 131, 72),   # four tiles, three one row / column wide, 2nd K tile partial
                                   (130, 126, 64)])  # N % 4 = 2
def test_cfg0_tails_strides_epilogues(dev, a_mn, b_mn, M, N, K):
    """Scalar tail stores (gn + q < N), the misaligned-pointer branches of epilogue_store4 (C, aux,
    res), a 4-byte-aligned bias."""
    C = require_native()
    case = Case(dev, a_mn, b_mn, M, N, K, seed=M * 7 + N * 3 + K + 2 * a_mn + b_mn)
    assert case.plan(C, 0, 0)[0] == 0
    for ckind, skind in STRIDES:
        for epi, dtypes in EPILOGUES:
            for dt in dtypes:
                case.run(C, epi, dt, "cfg0", ckind, skind, cfg=0)


# ---- b. the 256-wide DMA tile kernels and the ping-pong kernel (cfg 1-5), split-K ----------------
def _group(cfg):
    return {5: "pingpong", 7: "cfg7"}.get(cfg, "tile")


@pytest.mark.parametrize("a_mn,b_mn", LAYOUTS)
@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5])
def test_tile_kernels_tails_strides_epilogues(dev, cfg, splits, a_mn, b_mn):
    """(263, 197, 320): an interior tile where the tile fits plus both tails for every tile size,
    5 K-tiles (odd for the ping-pong kernel; 3 + 2 over two splits), in-kernel last-arriver combine."""
    C = require_native()
    case = Case(dev, a_mn, b_mn, 263, 197, 320, seed=cfg * 100 + splits * 10 + 2 * a_mn + b_mn)
    plan = case.plan(C, cfg, splits)
    # N = 197 leaves only the in-kernel combine (an n-contiguous B rounds N up to 200: either combine)
    assert plan[:2] == (cfg, splits) and (splits == 1 or case.N % 4 == 0 or plan[4] == 0), plan
    for ckind, skind in STRIDES:
        for epi, dtypes in EPILOGUES:
            for dt in dtypes:
                case.run(C, epi, dt, _group(cfg), ckind, skind, cfg=cfg, splits=splits)


@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5])
def test_split_k_external_reduce_veto_and_guarded_reduce(dev, cfg):
    """With the external combine requested, N = 197 (N % 4 != 0) vetoes it (the in-kernel last arriver
    runs); N = 200 takes it, and the reduce kernel writes a guarded C with ldc = N + 4."""
    C = require_native()
    try:
        C.set_gemm_split_mode(1)
        for a_mn, b_mn in ((0, 0), (1, 1)):
            veto = Case(dev, a_mn, b_mn, 263, 197, 320, seed=900 + cfg)
            ext = Case(dev, a_mn, b_mn, 264, 200, 320, seed=950 + cfg)
            want_veto = 0 if veto.N % 4 else 1  # (the n-contiguous B rounds 197 up to 200: no veto then)
            assert veto.plan(C, cfg, 2)[4] == want_veto and ext.plan(C, cfg, 2)[4] == 1
            assert ((a_mn, b_mn) != (0, 0) or want_veto == 0) and _ld(ext.N, "q4")[0] == ext.N + 4
            for epi, dtypes in EPILOGUES:
                for dt in dtypes:
                    veto.run(C, epi, dt, _group(cfg), "odd", "oddld", cfg=cfg, splits=2)
                    ext.run(C, epi, dt, _group(cfg), "q4", "oddoff", cfg=cfg, splits=2)
    finally:
        C.set_gemm_split_mode(-1)


# ---- c. interior-tile side-operand paths and their demotion ---------------------------------------
@pytest.mark.parametrize("cfg", [1, 5])
def test_side_operand_paths_demote_bitwise(dev, cfg):
    """(512, 512, 192): every tile is interior. Fully aligned operands take the prefetched side-operand
    pass (epi_pass_side) / the 16-byte store (epi_store8); breaking one alignment condition at a time
    demotes to epilogue_store4 (kind = -1, or st8 off). Same arithmetic, another store path: the same
    bits (fp32 accumulate: within t32), guards intact."""
    C = require_native()
    case = Case(dev, 0, 0, 512, 512, 192, seed=300 + cfg)
    assert case.plan(C, cfg, 0)[:2] == (cfg, 1)
    g = _group(cfg)
    # epilogue, dtype, [(C stride, side placement) of the broken runs]
    table = [("res", BF16, [("odd", "al"), ("al", "oddld"), ("al", "oddoff")]),
             ("res", F32, [("odd", "al"), ("al", "oddld"), ("al", "oddoff")]),
             ("dgelu", BF16, [("odd", "al"), ("al", "oddld"), ("al", "oddoff")]),
             ("acc", F32, [("odd", "al")]),
             ("gelu", BF16, [("q4", "al"), ("al", "q4"), ("al", "oddoff")]),   # the 8-wide store: ldc / ldaux % 8
             ("plain", BF16, [("q4", "al"), ("odd", "al")])]
    for epi, dt, broken in table:
        ref_c, ref_aux = case.run(C, epi, dt, g, "al", "al", cfg=cfg)
        for ckind, skind in broken:
            out_c, out_aux = case.run(C, epi, dt, g, ckind, skind, cfg=cfg)
            if epi == "acc":
                t32 = gemm_t32(case.A64, case.B64, case.K, {"c_prev": case.prev.double()})
                assert bool(((out_c.double() - ref_c.double()).abs() <= t32).all()), (epi, ckind, skind)
            else:
                assert torch.equal(out_c, ref_c), (epi, dt, ckind, skind)
            if ref_aux is not None:
                assert torch.equal(out_aux, ref_aux), (epi, ckind, skind)


# ---- d. the 4-wave kernel (cfg 7) and its host predicates -----------------------------------------
@pytest.mark.parametrize("b_mn", [0, 1])
def test_cfg7_and_demotion_to_pingpong(dev, b_mn):
    """(256, 512, 256), cfg 7 forced. Aligned guarded views (row strides multiples of 8, larger than N)
    satisfy gemm_w4_supported; an odd ldc / ldaux / ldres or a 4-byte-aligned bias must make it refuse, and
    the ping-pong kernel takes over. All runs obey the bound (so they agree within it) with guards
    intact."""
    C = require_native()
    case = Case(dev, 0, b_mn, 256, 512, 256, seed=700 + b_mn)
    assert case.plan(C, 7, 0)[:3] == (7, 1, 4)
    runs = {"plain": [("al", "al", 4), ("odd", "al", 4)],
            "bias": [("al", "al", 4), ("odd", "al", 4), ("al", "al", 1)],
            "gelu": [("al", "al", 4), ("odd", "al", 4), ("al", "oddld", 4), ("al", "al", 1)],
            "dgelu": [("al", "al", 4), ("odd", "al", 4), ("al", "oddld", 4), ("al", "oddoff", 4)],
            "res": [("al", "al", 4), ("odd", "al", 4), ("al", "oddld", 4), ("al", "oddoff", 4)]}
    for epi, variants in runs.items():
        for dt in ((BF16, F32) if epi in ("plain", "bias") else (BF16,)):
            outs = [case.run(C, epi, dt, "cfg7", ck, sk, cfg=7, bias_off=bo) for ck, sk, bo in variants]
            tol = case.last_tol  # of the output (GELU: of aux), the same for every variant
            for o, aux in outs[1:]:  # each within the bound of the fp64 value: within twice it of each other
                a, b = (aux, outs[0][1]) if epi == "gelu" else (o, outs[0][0])
                assert bool(((a.double() - b.double()).abs() <= 2 * tol).all()), (epi, dt)


def test_cfg7_weight_gradient_form(dev):
    """A [K][M], B [K][N], (256, 256, K), guarded fp32 C with and without accumulate. The planner's own
    pick at K = 1024 is cfg 7 with split-K raw partials (even K-steps >= 4 per split, accepted by
    gemm_w4_wgrad_supported) and the external reduce, which accumulates. A forced cfg 7 plans a single split
    (the bindings ignore `splits` for it): accepted at K = 1024 without accumulate, refused with
    accumulate, with an odd ldc, and at K = 960 (15 K-steps: odd) -- the 256 x 256 tile kernel runs."""
    C = require_native()
    case = Case(dev, 1, 1, 256, 256, 1024, seed=800)
    plan = case.plan(C, -1, 0)
    assert plan[0] == 7 and plan[1] > 1 and plan[2] % 2 == 0 and plan[2] >= 4 and plan[4] == 1, plan
    assert case.plan(C, -1, 0, True)[:2] == plan[:2]
    assert case.plan(C, 7, 0)[:3] == (7, 1, 16) and case.plan(C, 7, 3)[:3] == (7, 1, 16)
    for ckind in ("q4", "odd"):
        for epi in ("plain", "acc", "bias"):
            bo = 4 if ckind == "q4" else 1  # (a 4-byte-aligned bias is refused as well)
            case.run(C, epi, F32, "cfg7", ckind, cfg=-1, bias_off=bo)  # split-K partials + reduce
            case.run(C, epi, F32, "cfg7", ckind, cfg=7, bias_off=bo)   # single split: in-kernel epilogue, or refused
        case.run(C, "bias", BF16, "cfg7", ckind, cfg=7, bias_off=bo)
    odd = Case(dev, 1, 1, 256, 256, 960, seed=801)
    assert odd.plan(C, 7, 0)[:3] == (7, 1, 15)
    for epi in ("plain", "acc"):
        odd.run(C, epi, F32, "cfg7", "q4", cfg=7)


# ---- e. fp8 ---------------------------------------------------------------------------------------
def _rand_f8(shape, fmt, g, dev, scale):
    fmax = {0: 448.0, 1: 57344.0}[fmt]
    return (torch.randn(*shape, generator=g) * scale).clamp(-fmax, fmax).to(F8[fmt]).to(dev)


def _f8_in(x):
    """fp8 [rows, K] inside a 0xA5-filled byte buffer with row stride K + 16 (16-byte aligned base)."""
    return guarded_like(x, ld=x.shape[1] + 16, col_off=0)[1]


def _run_f8(C, dev, M, N, K, fmts, cfg, splits, ckinds, group, seed):
    fa, fb = fmts
    g = torch.Generator().manual_seed(seed)
    A, B = _f8_in(_rand_f8((M, K), fa, g, dev, 4.0)), _f8_in(_rand_f8((N, K), fb, g, dev, 4.0))
    assert A.stride(0) == K + 16 and B.stride(0) == K + 16
    A64, B64 = A.float().double(), B.float().double().t()
    isa, isb = torch.tensor([0.5], device=dev), torch.tensor([0.25], device=dev)
    bias = torch.randn(N, generator=g).to(dev)
    res = _mk((M, N), g, dev, 1.0)
    plan = tuple(C.gemm_f8_plan(M, N, K, cfg, splits))
    assert plan[:2] == (cfg, splits), plan
    for ckind in ckinds:
        for dt in (BF16, F32):
            for epi in ("plain", "bra"):
                cbuf, cv = guarded(M, N, dt, dev, *_ld(N, ckind))
                kw, terms = {}, {"alpha": 0.125}  # the two inverse scales folded into alpha
                if epi == "bra":
                    bbuf, kw["bias"] = _bias(bias, 1 if ckind == "odd" else 4)
                    rbuf, kw["res"] = _side(res, "oddld" if ckind == "odd" else "al")
                    kw["alpha"] = 0.5
                    terms = {"alpha": 0.0625, "bias": bias.double(), "res": res.double()}
                C.gemm_f8(A, B, cv, fa, fb, isa, isb, cfg=cfg, splits=splits, **kw)
                assert_guard_intact(cbuf, cv)
                assert bool(torch.isfinite(cv).all())
                exp, t32 = gemm_expected(A64, B64, terms), gemm_t32(A64, B64, K, terms)
                _check(group, cv, exp, t32, f"fp8 {fmts} cfg={cfg} splits={splits} {epi} {dt} {ckind}")


@pytest.mark.parametrize("fmts", [(0, 0), (1, 0), (0, 1)])
@pytest.mark.parametrize("splits", [1, 2])
@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5])
def test_gemm_f8_tails_and_odd_ldc(dev, cfg, splits, fmts):
    C = require_native()
    seed = cfg * 10 + splits + 100 * fmts[0] + 7 * fmts[1]
    _run_f8(C, dev, 263, 197, 256, fmts, cfg, splits, ("odd",), "fp8", seed)


@pytest.mark.parametrize("fmts", [(0, 0), (1, 0), (0, 1)])
def test_gemm_f8_cfg7_and_demotion(dev, fmts):
    """The 4-wave kernel's fp8 form at (256, 256, 512): aligned rows, and an odd ldc that
    gemm_w4_f8_supported must refuse (the ping-pong kernel runs)."""
    C = require_native()
    _run_f8(C, dev, 256, 256, 512, fmts, 7, 1, ("al", "odd"), "fp8", seed=70 + fmts[0] + 2 * fmts[1])


@pytest.mark.parametrize("K", [128, 512])  # 128: the ping-pong kernel's quantising epilogue; 512: the 4-wave one too
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gemm_f8_q_strided_outputs_bitwise(dev, mode, K):
    """gemm_f8_q into guarded Y / Y^T with row strides N + 16 / M + 16: the same bytes and amax as into
    contiguous tensors (whose values tests/test_fp8_fused_gpu.py checks), guards intact."""
    C = require_native()
    M = N = 256
    g = torch.Generator().manual_seed(40 + mode + K)
    fa = fo = 1 if mode == 2 else 0
    A, B = _f8_in(_rand_f8((M, K), fa, g, dev, 2.0)), _f8_in(_rand_f8((N, K), 0, g, dev, 2.0))
    isa, isb = torch.tensor([0.5], device=dev), torch.tensor([0.125], device=dev)
    scale = torch.tensor([3.0], device=dev)
    bias = torch.randn(N, generator=g).to(dev) if mode != 2 else None
    pre = _mk((M, N), g, dev, 2.0)

    def call(Y, Yt):
        amax = torch.zeros(C.FP8_AMAX_SLOTS, device=dev)
        aux = pre.clone() if mode == 2 else (torch.zeros(M, N, dtype=BF16, device=dev) if mode == 1 else None)
        cs = torch.full((N,), 7.0, device=dev) if mode == 2 else None
        C.gemm_f8_q(A, B, Y, Yt, fa, 0, isa, isb, fo, scale, amax, bias=bias, aux=aux, mode=mode, colsum_out=cs,
                    colsum_accumulate=True)
        return amax, aux, cs

    try:
        for on in (0, 1):
            C.set_gemm_w4q8(on)
            Y0 = torch.empty(M, N, dtype=torch.uint8, device=dev)
            Yt0 = torch.empty(N, M, dtype=torch.uint8, device=dev)
            ref = call(Y0, Yt0)
            ybuf, Y = guarded(M, N, torch.uint8, dev, N + 16, 0)
            tbuf, Yt = guarded(N, M, torch.uint8, dev, M + 16, 0)
            got = call(Y, Yt)
            assert_guard_intact(ybuf, Y)
            assert_guard_intact(tbuf, Yt)
            assert torch.equal(Y, Y0) and torch.equal(Yt, Yt0) and torch.equal(Yt0, Y0.t())
            assert torch.equal(got[0], ref[0]) and float(ref[0].max()) > 0
            if mode == 1:
                assert torch.equal(got[1], ref[1])
            if mode == 2:
                assert torch.equal(got[2], ref[2])
    finally:
        C.set_gemm_w4q8(-1)


# ---- f. colsum and transpose_bf16 -----------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(1, 8), (37, 520), (300, 520)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_colsum_guarded(dev, M, N, accumulate):
    """out = buf[4:4+N] of a sentinel fp32 buffer, X a strided view with NaN around it. Tolerance: an fp32
    sum of M exact bf16 values in any order, (M + 4) 2^-24 sum |x| (twice that: truncation allowed)."""
    C = require_native()
    g = torch.Generator().manual_seed(M + N)
    X = _in(_mk((M, N), g, dev, 1.0))
    base = torch.randn(N, generator=g).to(dev)
    buf = sentinel((N + 8,), F32, dev)
    out = buf[4:4 + N]
    if accumulate:
        out.copy_(base)
    C.colsum(X, out, accumulate)
    assert_guard_intact(buf, out)
    x64 = X.double()
    exp = x64.sum(0) + (base.double() if accumulate else 0.0)
    tol = 2.0 * (M + 4) * 2.0 ** -24 * (x64.abs().sum(0) + (base.double().abs() if accumulate else 0.0)) + 1e-30
    _note("colsum", F32, assert_within(out, exp, tol, "colsum"))


@pytest.mark.parametrize("R,Cc", [(100, 37), (130, 200)])
@pytest.mark.parametrize("off", [64, 1])  # dst 16-byte aligned / 2-byte aligned only (element-wise stores)
def test_transpose_bf16_guarded(dev, R, Cc, off):
    C = require_native()
    g = torch.Generator().manual_seed(R + Cc)
    src = _mk((R, Cc), g, dev, 1.0)
    flat = sentinel((off + R * Cc + 64,), BF16, dev)
    dst = flat[off:off + R * Cc].view(Cc, R)
    C.transpose_bf16(src, dst)
    assert_guard_intact(flat, (0, 1, off, R * Cc))
    assert torch.equal(dst, src.t())


def test_zz_headroom_report():
    """Prints the largest |err| / tolerance seen per kernel group and output dtype by the tests above
    (run in file order); every ratio is at most 1 because every test asserted it."""
    for (group, dt), r in sorted(_HEADROOM.items()):
        print(f"headroom-max {group} {dt} {r:.4f}")
        assert r <= 1.0
