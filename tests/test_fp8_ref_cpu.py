"""tests/fp8_ref.py, the zero-mismatch reference of the fp8 quantisation tests, checked on the CPU:
  * byte for byte equal to torch's CPU cast `x.clamp(-max, max).to(float8)` on all 65,280 finite bf16 patterns and
    on the boundary set (every code point, every midpoint of adjacent code points, every midpoint +- 1 fp32 ulp,
    both signs), both formats, at the scales the GPU tests use;
  * decode o encode is the identity on the finite codes, the quantiser is monotone;
  * the exact-comparison harness the GPU tests use (fp8_ref.mismatches / assert_exact) rejects four wrong
    quantisers -- round-half-away, truncation, flush-subnormals-to-zero, NaN -> -max -- on the inputs the GPU tests
    feed, and the ties / subnormals / NaNs that reject them are counted (printed with pytest -s)."""
import pytest
import torch

from tests import fp8_ref as R

F8 = {0: torch.float8_e4m3fn, 1: torch.float8_e5m2}
SCALES = R.SCALES


def _torch_cast(p, fmt):
    """torch's CPU cast of an fp32 product, saturating."""
    return p.clamp(-R.FMAX[fmt], R.FMAX[fmt]).to(F8[fmt]).view(torch.uint8)


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("scale", SCALES)
def test_reference_equals_torch_cpu_cast_on_all_finite_bf16(fmt, scale):
    x = R.all_finite_bf16()
    assert x.numel() == 65280
    got = R.quantize(x, scale, fmt)
    ref = _torch_cast(R.product(x, scale), fmt)
    assert torch.equal(got, ref), int((got != ref).sum())


@pytest.mark.parametrize("fmt", [0, 1])
def test_reference_equals_torch_cpu_cast_on_the_boundary_set(fmt):
    x = R.boundary_set(fmt)
    n = R.NFINITE[fmt]
    assert x.numel() == 2 * (n + 3 * (n - 1) + 4)
    got = R.quantize(x, 1.0, fmt)
    assert torch.equal(got, _torch_cast(x, fmt))
    c = R.census(x, 1.0, fmt)
    print(f"boundary set fmt {fmt}: {x.numel()} values, {c}")
    assert c["ties"] == 2 * (n - 1) and c["subnormal"] > 0 and c["saturated"] >= 8 and c["neg_zero"] == 1
    # a power-of-two scale with the inputs divided by it: the same products, the same bytes
    for s in (2.0 ** -3, 2.0 ** 7):
        assert torch.equal(R.quantize(x / s, s, fmt), got)


@pytest.mark.parametrize("fmt", [0, 1])
def test_decode_encode_identity_and_special_values(fmt):
    codes = torch.arange(256, dtype=torch.uint8)
    v = R.decode(codes, fmt)
    fin = torch.isfinite(v)
    assert int(fin.sum()) == 2 * R.NFINITE[fmt]
    assert torch.equal(R.quantize(v[fin].float(), 1.0, fmt), codes[fin])  # -0 -> 0x80 included
    assert torch.equal(v[fin].float(), codes[fin].view(F8[fmt]).float())  # the decoder against torch's
    assert float(v[R.NFINITE[fmt] - 1]) == R.FMAX[fmt]
    sp = torch.tensor([float("nan"), float("inf"), float("-inf"), 1e30, -1e30, 0.0, -0.0, 1e-30, -1e-30])
    q = R.quantize(sp, 1.0, fmt)
    top = R.NFINITE[fmt] - 1
    assert bool(R.is_nan_code(q[:1], fmt)) and not bool(R.is_nan_code(q[1:], fmt).any())
    assert q[1:].tolist() == [top, top | 0x80, top, top | 0x80, 0x00, 0x80, 0x00, 0x80]
    # NaN times any scale stays NaN; inf times a tiny scale still saturates (the product is formed first)
    assert bool(R.is_nan_code(R.quantize(sp[:1], 0.0, fmt), fmt))
    assert int(R.quantize(sp[1:2], 1e-30, fmt)) == top


@pytest.mark.parametrize("fmt", [0, 1])
def test_reference_is_monotone(fmt):
    g = torch.Generator().manual_seed(fmt)
    x = torch.cat([R.boundary_set(fmt), R.all_finite_bf16().float(),
                   torch.randn(20000, generator=g) * R.MIN_NORMAL[fmt], torch.randn(20000, generator=g) * 30])
    x = x.sort().values
    v = R.signed_value(R.quantize(x, 1.0, fmt), fmt)
    assert bool((v[1:] >= v[:-1]).all())


# ------------------------------------------------------------------------------------------------- mutants
def _mutant(kind):
    """A wrong quantiser with quantize()'s signature."""
    def q(x, scale, fmt):
        p = R.product(x, scale)
        a = p.double().abs().clamp(max=R.FMAX[fmt])
        pts, mid = R.code_points(fmt), R.midpoints(fmt)
        sign = ((p.view(torch.int32) >> 31) & 1) << 7
        if kind == "half_away":
            k = torch.searchsorted(mid, a, right=True)          # a tie goes up, whatever the parity
        elif kind == "truncate":
            k = torch.searchsorted(pts, a, right=True) - 1      # the largest code point <= a
        else:
            k = R.quantize_product(p, fmt).to(torch.int64) & 0x7F
        if kind == "flush_subnormal":
            k = torch.where(pts[k.clamp(max=pts.numel() - 1)] < R.MIN_NORMAL[fmt], torch.zeros_like(k), k)
        k = torch.where(torch.isnan(p), torch.full_like(k, R.NAN_CODE[fmt]), k)
        out = (k | sign).to(torch.uint8)
        if kind == "nan_to_neg_max":                            # what v_med3_f32(NaN, -max, max) gives
            out = torch.where(torch.isnan(p), torch.full_like(out, (R.NFINITE[fmt] - 1) | 0x80), out)
        return out
    return q


def gpu_test_inputs(fmt):
    """The exact-rounding inputs of tests/test_fp8_quant_edges_gpu.py as (name, x, scale) triples."""
    from tests.test_fp8_quant_edges_gpu import exact_inputs
    return exact_inputs(fmt)


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("kind,counted", [("half_away", "ties"), ("truncate", "ties"), ("flush_subnormal", "subnormal"),
                                          ("nan_to_neg_max", "nan")])
def test_exact_harness_rejects_mutant(fmt, kind, counted):
    """Over the GPU tests' own inputs: the reference passes its own harness, every mutant is reported, and the
    inputs hold ties, subnormal results and NaNs (the values that tell the mutants apart)."""
    q = _mutant(kind)
    total, hit = 0, 0
    for name, x, scale in gpu_test_inputs(fmt):
        assert not bool(R.mismatches(R.quantize(x, scale, fmt), x, scale, fmt).any())
        n = int(R.mismatches(q(x, scale, fmt), x, scale, fmt).sum())
        c = R.census(x, scale, fmt)[counted]
        print(f"mutant {kind} fmt {fmt} {name} scale {float(scale):g}: {n} mismatches, {c} {counted}")
        total, hit = total + n, hit + c
        if n:
            with pytest.raises(AssertionError):
                R.assert_exact(q(x, scale, fmt), x, scale, fmt, name)
    print(f"mutant {kind} fmt {fmt}: rejected by {total} bytes; {hit} {counted} in the inputs")
    assert hit > 0 and total > 0
    if kind in ("flush_subnormal", "nan_to_neg_max"):
        assert total == hit  # each such value is one mismatch
