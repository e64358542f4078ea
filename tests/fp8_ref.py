"""A plain reference for the fp8 quantisation path (csrc/kernels/fp8.hip, pack4_fp8 of csrc/include/mlt_fp8.h):
OCP e4m3 (fmt 0, "e4m3fn": no infinity, one NaN per sign, max 448) and e5m2 (fmt 1, IEEE-like, max 57344).

    quantize(x, scale, fmt) = fp8(clamp(fp32(x) * fp32(scale), -max, max))

with ONE fp32 product, round to nearest / ties to even onto the format's code points (subnormals included), the
sign bit kept on zeros and on values that round to zero, NaN -> the format's NaN, +-inf -> +-max. Nothing here
uses a torch fp8 cast: the 256 code points are decoded with integer arithmetic, and a value is placed among the
sorted non-negative code points by comparing it with their midpoints in fp64 (every fp32 value, every code point
and every midpoint is exact in fp64, so the comparisons are exact). tests/test_fp8_ref_cpu.py holds this file to
torch's CPU cast byte for byte and shows that assert_exact() rejects four wrong quantisers.

Works on any device; the tests compute it on the CPU from the very input bits the kernel read."""
import torch

E4M3, E5M2 = 0, 1
FMAX = {E4M3: 448.0, E5M2: 57344.0}
_EBITS = {E4M3: 4, E5M2: 5}
_BIAS = {E4M3: 7, E5M2: 15}
# number of finite non-negative codes: 0x00 .. 0x7E (0x7F is NaN) / 0x00 .. 0x7B (0x7C inf, 0x7D .. 0x7F NaN)
NFINITE = {E4M3: 0x7F, E5M2: 0x7C}
MIN_NORMAL = {E4M3: 2.0 ** -6, E5M2: 2.0 ** -14}
NAN_CODE = {E4M3: 0x7F, E5M2: 0x7F}
# scales of the exact-rounding tests: 2^100 saturates 86 % of the finite bf16 patterns (|x| > 2^-91 / 2^-84) and takes
# the largest ones to an infinite product
SCALES = (1.0, 2.0 ** -3, 0.75, 2.0 ** 100)


def decode(codes, fmt):
    """uint8 codes -> fp64 values (NaN and, for e5m2, +-inf as such), by integer arithmetic on the fields."""
    c = codes.to(torch.int64)
    mb = 7 - _EBITS[fmt]
    sign = torch.where((c >> 7) == 1, -1.0, 1.0).double()
    e = (c >> mb) & ((1 << _EBITS[fmt]) - 1)
    m = c & ((1 << mb) - 1)
    sub = (m.double() / (1 << mb)) * 2.0 ** (1 - _BIAS[fmt])
    nor = (1.0 + m.double() / (1 << mb)) * torch.exp2((e - _BIAS[fmt]).double())
    v = sign * torch.where(e == 0, sub, nor)
    mag = c & 0x7F
    if fmt == E4M3:
        v = torch.where(mag == 0x7F, torch.full_like(v, float("nan")), v)
    else:
        v = torch.where(mag == 0x7C, sign * float("inf"), v)
        v = torch.where(mag > 0x7C, torch.full_like(v, float("nan")), v)
    return v


def code_points(fmt, device="cpu"):
    """The finite non-negative code points in increasing order (fp64); index = code."""
    return decode(torch.arange(NFINITE[fmt], dtype=torch.uint8, device=device), fmt)


def midpoints(fmt, device="cpu"):
    """Midpoints of adjacent non-negative code points (fp64, exact, and exact in fp32 too)."""
    p = code_points(fmt, device)
    return 0.5 * (p[:-1] + p[1:])


def product(x, scale):
    """fp32(x) * fp32(scale): the single fp32 product the kernels form."""
    s = scale if isinstance(scale, torch.Tensor) else torch.tensor(float(scale))
    return x.float() * s.to(device=x.device, dtype=torch.float32).reshape(-1)[0]


def quantize_product(p, fmt):
    """fp32 product -> uint8 code: saturate, round to nearest even, keep the sign, NaN -> NAN_CODE | sign."""
    assert p.dtype == torch.float32
    a = p.double().abs().clamp(max=FMAX[fmt])  # (clamp keeps NaN)
    mid = midpoints(fmt, p.device)
    k = torch.searchsorted(mid, a.reshape(-1).contiguous()).reshape(a.shape)  # number of midpoints below a
    tie = a == mid[k.clamp(max=mid.numel() - 1)]  # a sits ON midpoint k: between codes k and k + 1, take the even one
    k = torch.where(tie & (k % 2 == 1), k + 1, k)
    k = torch.where(torch.isnan(p), torch.full_like(k, NAN_CODE[fmt]), k)
    sign = (p.view(torch.int32) >> 31) & 1  # the sign BIT: -0 and NaN payload signs included
    return (k | (sign << 7)).to(torch.uint8)


def quantize(x, scale, fmt):
    """x (bf16 / fp32, any shape), scale (float or 1-element tensor) -> uint8 codes of the same shape."""
    return quantize_product(product(x, scale), fmt)


def is_nan_code(codes, fmt):
    mag = codes.to(torch.int64) & 0x7F
    return mag == 0x7F if fmt == E4M3 else mag > 0x7C


def canon(codes, fmt):
    """Every NaN encoding -> NAN_CODE (which NaN a cast produces, and its sign, is not part of the contract)."""
    c = codes.view(torch.uint8) if codes.dtype != torch.uint8 else codes
    return torch.where(is_nan_code(c, fmt), torch.full_like(c, NAN_CODE[fmt]), c)


def signed_value(codes, fmt):
    """Codes as signed fp8 values in fp64 (for order comparisons); -0 and +0 compare equal. No NaN expected."""
    c = codes.view(torch.uint8) if codes.dtype != torch.uint8 else codes
    return decode(c, fmt)


def mismatches(got, x, scale, fmt):
    """Bool mask: bytes of `got` (fp8 or uint8 storage) that differ from quantize(x, scale, fmt), NaNs canonical."""
    g = got.view(torch.uint8) if got.dtype != torch.uint8 else got
    ref = quantize(x, scale, fmt).to(g.device)
    return canon(g.reshape(ref.shape), fmt) != canon(ref, fmt)


def assert_exact(got, x, scale, fmt, what=""):
    """Zero mismatching bytes; reports the count and the first one with its input, product and both codes."""
    bad = mismatches(got, x, scale, fmt)
    n = int(bad.sum())
    if n:
        i = int(bad.reshape(-1).nonzero()[0])
        g = got.view(torch.uint8) if got.dtype != torch.uint8 else got
        xv = x.reshape(-1)[i].float()
        raise AssertionError(f"{what}: {n} of {bad.numel()} bytes differ from the reference, first at flat index {i}: "
                             f"x = {float(xv):.9g} ({int(xv.view(torch.int32)) & 0xFFFFFFFF:#010x}), product "
                             f"{float(product(x.reshape(-1)[i:i + 1], scale)):.9g}, got {int(g.reshape(-1)[i]):#04x}, "
                             f"expected {int(quantize(x.reshape(-1)[i:i + 1], scale, fmt)):#04x}")


def census(x, scale, fmt):
    """What the inputs exercise: dict of counts over the products p = x * scale --
    ties (|p| exactly on a midpoint below max), subnormal (0 < |Q(p)| < min normal), to_zero (p != 0 rounding to 0),
    saturated (|p| > max, inf included), nan, neg_zero (p == -0)."""
    p = product(x, scale)
    a = p.double().abs()
    mid = midpoints(fmt, p.device)
    q = decode(quantize_product(p, fmt) & 0x7F, fmt)
    fin = ~torch.isnan(p)
    return dict(ties=int(torch.isin(a, mid).sum()),
                subnormal=int((fin & (q > 0) & (q < MIN_NORMAL[fmt])).sum()),
                to_zero=int((fin & (a > 0) & (q == 0)).sum()),
                saturated=int((a > FMAX[fmt]).sum()),
                nan=int((~fin).sum()),
                neg_zero=int(((p == 0) & ((p.view(torch.int32) >> 31) & 1).bool()).sum()))


def all_finite_bf16():
    """The 65,280 finite bf16 bit patterns (both signs, zeros and subnormals included) as a bf16 tensor."""
    b = torch.arange(1 << 16, dtype=torch.int32)
    b = b[((b >> 7) & 0xFF) != 0xFF]
    return b.to(torch.int16).view(torch.bfloat16)


def boundary_set(fmt):
    """fp32 values where a quantiser goes wrong: every finite code point, every midpoint of adjacent code points,
    every midpoint -1 and +1 fp32 ulp, max + 1 ulp and the e4m3 'would round to NaN' point max + half a step; all
    with both signs (so +0 and -0 are in it). All of them are exact in fp32."""
    pts = code_points(fmt).float()
    mid = midpoints(fmt).float()
    assert bool((pts.double() == code_points(fmt)).all()) and bool((mid.double() == midpoints(fmt)).all())
    bits = mid.view(torch.int32)
    extra = torch.tensor([FMAX[fmt]], dtype=torch.float32).view(torch.int32) + 1
    step = float(pts[-1] - pts[-2])
    over = torch.tensor([FMAX[fmt] + 0.5 * step, FMAX[fmt] + step, 2 * FMAX[fmt]], dtype=torch.float32)
    pos = torch.cat([pts, mid, (bits - 1).view(torch.float32), (bits + 1).view(torch.float32),
                     extra.view(torch.float32), over])
    return torch.cat([pos, -pos])
