"""CPU checks of the GEMM test helpers (tests/helpers.py): the derived per-element tolerance admits a
plain fp32 reference at every shape the GPU edge tests use, rejects each of a written list of
single-element mistakes, and the guard helpers see a change anywhere outside the view."""
import pytest
import torch

from tests.helpers import (assert_guard_intact, assert_within, gemm_bound, gemm_expected, gemm_t32, guarded,
                           guarded_like, sentinel, store_bound)

# every (M, N, K) of tests/test_gemm_edges_gpu.py
SHAPES = [(1, 1, 8), (33, 37, 40), (129, 131, 72), (130, 126, 64),   # cfg 0
          (263, 197, 320), (264, 200, 320),                          # cfg 1-5, split-K
          (512, 512, 192),                                           # interior side-operand paths
          (256, 512, 256), (256, 256, 1024), (256, 256, 960),        # cfg 7 and its weight-gradient form
          (263, 197, 256), (256, 256, 512)]                          # fp8


def _operands(M, N, K, fp8=False):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    if fp8:
        a = (torch.randn(M, K, generator=g) * 2).to(torch.float8_e4m3fn).float()
        b = (torch.randn(K, N, generator=g) * 2).to(torch.float8_e5m2).float()
    else:
        a = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16).float()
        b = (torch.randn(K, N, generator=g) * 0.5).to(torch.bfloat16).float()
    return a, b, g


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_fp32_reference_stays_inside_the_bound(M, N, K, fp8):
    """A torch fp32 CPU matmul of the upcast inputs, stored as fp32 and rounded to bf16, with and
    without an epilogue: inside gemm_bound of the fp64 value at every element."""
    a, b, g = _operands(M, N, K, fp8)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).to(torch.bfloat16).float()
    c32 = a @ b
    for terms, out32 in (({}, c32),
                         ({"alpha": 0.5, "bias": bias.double(), "res": res.double()}, 0.5 * c32 + bias + res),
                         ({"c_prev": res.double()}, res + c32)):
        exp = gemm_expected(a.double(), b.double(), terms)
        r32 = assert_within(out32, exp, gemm_bound(a.double(), b.double(), K, terms, torch.float32), "fp32")
        r16 = assert_within(out32.to(torch.bfloat16), exp,
                            gemm_bound(a.double(), b.double(), K, terms, torch.bfloat16), "bf16")
        assert r32 <= 1.0 and r16 <= 1.0


def test_half_the_unit_roundoff_rejects_correct_rounding():
    """Why the bf16 store term is bf16's own spacing and not 2^-9 |expected|: bf16 has 8 significant
    bits, so a correct round-to-nearest moves a value by up to 2^-8 relative. 1 + 2^-8 + 2^-12 (exact
    in fp32, t32 ~ 1e-6) rounds to 1 + 2^-7: an error of 0.0037, inside store_bound, outside
    t32 (1 + 2^-9) + 2^-9 |expected| = 0.00196."""
    a = torch.zeros(1, 8, dtype=torch.float64)
    b = torch.zeros(8, 1, dtype=torch.float64)
    a[0, :3] = 1.0
    b[:3, 0] = torch.tensor([1.0, 2.0 ** -8, 2.0 ** -12], dtype=torch.float64)
    exp = gemm_expected(a, b)
    out = (a.float() @ b.float()).to(torch.bfloat16)
    assert float(out) == 1.0 + 2.0 ** -7
    t32 = gemm_t32(a, b, 8)
    assert_within(out, exp, gemm_bound(a, b, 8, None, torch.bfloat16), "bf16")
    assert abs(float(out) - float(exp)) > float(t32 * (1 + 2.0 ** -9) + 2.0 ** -9 * exp.abs())
    # ... and the interval form is never looser than the 2^-8 closed form
    e = torch.linspace(-4.0, 4.0, 4001, dtype=torch.float64)
    t = torch.full_like(e, 1e-5)
    assert bool((store_bound(e, t, torch.bfloat16) <= t * (1 + 2.0 ** -8) + 2.0 ** -8 * e.abs() + 1e-12).all())


# The mistakes the bound must catch, each applied to an otherwise correct result. A later loosening of
# gemm_bound that lets one through fails test_bound_has_teeth.
MUTATIONS = ["one product dropped from one element",
             "one 8-wide K chunk dropped from one row",
             "bias shifted by one column in the last 4-column group",
             "residual of row M-1 taken from row M-2",
             "last column left unwritten (sentinel NaN)"]


def _mutate(name, out, a, b, bias, res, alpha):
    M, N = out.shape
    K = a.shape[1]
    out = out.clone()
    if name == MUTATIONS[0]:
        # the element of largest magnitude (the widest bf16 spacing) loses its median-sized product
        i, j = divmod(int(out.abs().argmax()), N)
        prod = a[i] * b[:, j]
        k = int(prod.abs().argsort()[K // 2])
        out[i, j] -= alpha * prod[k]
    elif name == MUTATIONS[1]:
        i, k0 = M // 2, 8 * (K // 16)
        out[i] -= alpha * (a[i, k0:k0 + 8] @ b[k0:k0 + 8])
    elif name == MUTATIONS[2]:
        g0 = (N - 1) // 4 * 4
        cols = torch.arange(max(g0, 1), N)
        out[:, cols] += bias[cols - 1] - bias[cols]
    elif name == MUTATIONS[3]:
        out[M - 1] += res[M - 2] - res[M - 1]
    elif name == MUTATIONS[4]:
        out[:, N - 1] = sentinel((M,), torch.float32, "cpu")
    else:
        raise KeyError(name)
    return out


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(33, 37, 40), (130, 126, 64), (263, 197, 320)])
@pytest.mark.parametrize("name", MUTATIONS)
def test_bound_has_teeth(name, M, N, K, out_dtype):
    a, b, g = _operands(M, N, K)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g).to(torch.bfloat16).float()
    alpha = 0.5
    terms = {"alpha": alpha, "bias": bias.double(), "res": res.double()}
    exp = gemm_expected(a.double(), b.double(), terms)
    tol = gemm_bound(a.double(), b.double(), K, terms, out_dtype)
    good = alpha * (a @ b) + bias + res
    assert_within(good.to(out_dtype), exp, tol, "unmutated")
    bad = _mutate(name, good, a, b, bias, res, alpha)
    with pytest.raises(AssertionError, match="outside the bound"):
        assert_within(bad.to(out_dtype), exp, tol, name)


_POKES = ["row above", "row below", "column left", "column right", "last element of the buffer"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.uint8, torch.float8_e4m3fn])
def test_guard_helpers(dtype):
    rows, cols, ld, off = 5, 7, 13, 3
    buf, view = guarded(rows, cols, dtype, "cpu", ld, off)
    assert buf.shape == (rows + 2, ld) and view.shape == (rows, cols)
    assert view.data_ptr() == buf.data_ptr() + (ld + off) * buf.element_size()
    assert_guard_intact(buf, view)
    assert_guard_intact(buf, (1, rows, off, cols))
    view.view(torch.uint8 if buf.element_size() == 1 else view.dtype).zero_()  # writes inside the view are free
    assert_guard_intact(buf, view)
    where = {"row above": (0, off + 2), "row below": (rows + 1, off), "column left": (3, off - 1),
             "column right": (2, off + cols), "last element of the buffer": (rows + 1, ld - 1)}
    idt = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[buf.element_size()]
    for name in _POKES:
        r, c = where[name]
        b2, v2 = guarded(rows, cols, dtype, "cpu", ld, off)
        b2.view(idt)[r, c] ^= 1  # one flipped bit: for the float types still a NaN
        with pytest.raises(AssertionError, match=rf"\(row {r}, col {c}\)"):
            assert_guard_intact(b2, v2)


def test_guarded_input_and_1d_views():
    x = torch.arange(12, dtype=torch.float32).view(3, 4).to(torch.bfloat16)
    buf, v = guarded_like(x, ld=9, col_off=2)
    assert torch.equal(v, x) and bool(torch.isnan(buf[0].float()).all()) and bool(torch.isnan(buf[1, :2].float()).all())
    assert_guard_intact(buf, v)
    flat = sentinel((20,), torch.float32, "cpu")
    out = flat[4:12]
    out.zero_()
    assert_guard_intact(flat, out)
    flat.view(torch.int32)[12] = 0
    with pytest.raises(AssertionError, match=r"\(row 0, col 12\)"):
        assert_guard_intact(flat, out)
