"""The fp8 quantisation path -- cast_fp8, amax, both cast_transpose kernels, update_scale (fp8.hip), pack4_fp8 and
atomic_max_pos (mlt_fp8.h) and pack4_fp8 inside gemm_f8_q -- on GUARDED buffers, every stored byte compared with
the plain reference of tests/fp8_ref.py (one fp32 product, saturate, round to nearest even; built from the decoded
code points, held to torch's CPU cast by tests/test_fp8_ref_cpu.py). Zero mismatching bytes is the bound.

Buffers: every tensor a kernel touches is a slice, 64 elements in, of a 1-D allocation filled with a sentinel.
fp8 outputs: 0xA5 bytes. fp32 state (scale, inv_scale, fmax, hist, amax, column sums): the NaN pattern of
helpers.sentinel. INPUTS: a large FINITE pattern (fp32 bits of 3e38, bf16 0x7F7F) -- amax goes through fmaxf, which
drops a NaN, so a NaN read past the end would be invisible where a finite giant becomes the amax. Inside the
amax state only every 32nd float is a slot; the other 31 of each line are prefilled with 3e38 and must neither
change nor reach a slot. Slots are checked one by one: slot k = max(prefill, max over the blocks b = k mod 64 of
the block's own max |x|), with the block geometry of each kernel written out in _slot_expect_*.

Edge -> the case that reaches it:
  round to nearest even on every finite bf16 pattern, 4 scales ........ test_exact_rounding[bf16]: fp8_cast, the 64x64
                                                                        kernel at 320 x 256, the wide one at 256 x 256
  every code point, midpoint, midpoint +- 1 ulp, fp8 subnormals ....... test_exact_rounding[fp32]: fp8_cast and the
                                                                        64x64 kernel at 72 x 64 (a row tail)
  NaN -> NaN byte, +-inf -> +-max, +-0 and underflow keep the sign,
  amax = max over the non-NaN elements ................................ the `specials` inputs of test_exact_rounding
  NaN through a quantising GEMM epilogue .............................. test_gemm_f8_q_nan_row
  64x64 kernel: one partial tile | 2 x 3 tiles, both tails | column
  tail | row tail | 72 blocks (slot index wraps, max in block 71) ..... test_cast_transpose_tails at (4, 4) | (68, 132)
                                                                        | (64, 60) | (132, 64) | (576, 512)
  wide kernel: one tile | 2 x 3 tiles; column sums set / accumulated .. test_cast_transpose_wide
  cast / amax: one thread | a second block with one live thread |
  the grid-stride loop's second trip (3 items) ........................ test_cast_sizes at 8 | 8 * 257 | 8 * (2048 * 256 + 3)
  slot above the data kept, slot below raised, non-slot floats inert .. every launch (prefill of _amax_state)
  update_scale: second block and i >= n, per-tensor fmax, margin,
  history wrap at step 2^31 + 5, m == 0 and m == inf .................. test_update_scale
  shapes, dtypes, short amax, unaligned y / yt rejected ............... test_rejections

update_scale and an infinite amax, as it is today (pinned, not changed): the inf enters the history like any value and
stays for H steps; while it is in the window the window max is inf and scale / inv_scale keep their bits, H steps
later the slot is overwritten and the scale follows the data again (H = 16: written at step 0, still frozen at step
15, released at step 16 -- the three steps of the test). amax itself never holds a NaN: fmaxf drops it.

Each check that has a tolerance prints `headroom <what> <figure>` (pytest -s).

Measured on an MI355X:
  exact rounding ........ 0 mismatching bytes in every case (nothing here has a tolerance)
  wide-kernel colsum .... largest |err| / t 0.013 ((128, 128), e5m2, accumulating); 0.004 - 0.008 elsewhere
  scale / inv_scale ..... 0 ulp from RN(fmax / (m 2^margin)) and RN(1 / scale): the device's division is correctly
                          rounded, the comparison is exact and no ulp allowance was needed
  gemm_f8_q bracket ..... (tests/test_fp8_fused_gpu.py) share of bytes equal to Q(ref): 0.9991 - 0.9997 in modes 0 and 2,
                          1.0000 in mode 1, at every shape and at the saturating and subnormal scales; none outside

What these tests found:
  * The reading of v_med3_f32 in the issue was right. Before the fix in mlt_fp8.h a NaN input came out of every kernel
    as the largest NEGATIVE finite value: byte 0xFE (-448) in e4m3 and 0xFB (-57344) in e5m2, 4 of 4 NaNs in each of
    the bf16 and fp32 `specials` inputs, and through gemm_f8_q a NaN byte in A gave a row of 256 finite bytes
    (test_gemm_f8_q_nan_row). pack4_fp8 now saturates with the NaN-propagating maximum / minimum (v_maximum3_f32,
    v_minimum3_f32: one instruction more per value); +-inf still go to +-max. Measured cost on the large fp8 model:
    0.8 % of a step (405 - 407 ms against 402 - 404 ms); a compare and a select around the med3 cost 2.1 %.
  * Everything else held as it was: with the old pack4_fp8 the other 44 cases of this file passed unchanged -- rounding
    (ties, subnormals, signed zeros), the tail guards of the 64 x 64 kernel, the grid-stride second trip, slot wrap at
    72 blocks, the slot prefills, update_scale at n = 300 / margin / step 2^31 + 5, and every guard.
  * fp8_cast_transpose accepted y / yt at any byte offset while its 64 x 64 kernel stores dwords to them; the binding
    now rejects a y or yt that is not 4-byte aligned (test_rejections).
"""
import pytest
import torch

from ml_trainer_amd.ops._ext import require_native
from tests import fp8_ref as R
from tests.helpers import acc_bound, assert_guard_intact, assert_within, colsum_stored_bound, sentinel

pytestmark = pytest.mark.gpu

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
PAD = 64            # elements of sentinel on both sides of every view (64 fp32 / bf16 / bytes: 16-byte multiples)
GIANT = 3e38        # the finite giant of the input guards and of the non-slot amax floats
_GIANT_BITS = {F32: int(torch.tensor(GIANT).view(torch.int32)), BF16: 0x7F7F}
SLOTS, STRIDE = 64, 32


# ------------------------------------------------------------------------------------------------- inputs (CPU)
def _specials(dtype):
    """NaNs of both signs, +-inf, +-0, values that underflow to +-0 in both formats, values far above both maxima."""
    v = torch.tensor([float("nan"), 1.0, float("inf"), float("-inf"), 0.0, -0.0, 1e-30, -1e-30, 1e30, -1e30, 448.0,
                      -448.0, 57344.0, -57344.0, 464.0, -464.0, 2.0 ** -10, -2.0 ** -10, 2.0 ** -17, -2.0 ** -17,
                      float("nan"), 3.0, -5.0, 0.25, 480.0, -61440.0, 1.5, -1.5, 0.75, -0.75, 2.0, -2.0], dtype=F32)
    v = v.repeat(2)
    v.view(torch.int32)[0] = -0x400000  # 0xFFC00000: a negative NaN
    return v.to(dtype)


def exact_inputs(fmt):
    """(name, x, scale) of the exact-rounding tests, x 1-D on the CPU. tests/test_fp8_ref_cpu.py runs its mutants
    over this very list."""
    g = torch.Generator().manual_seed(1234 + fmt)
    out = []
    allb = R.all_finite_bf16()
    allb = allb[torch.randperm(allb.numel(), generator=g)]
    for s in R.SCALES:
        out.append(("bf16_all", allb, s))
    out.append(("bf16_specials", _specials(BF16), 1.0))
    b = R.boundary_set(fmt)
    sub = torch.randn(3072, generator=g) * R.MIN_NORMAL[fmt]
    for s in (1.0, 2.0 ** -3, 2.0 ** 7):  # power-of-two scales: x = value / s is exact, the product is the value
        x = torch.cat([b / s, sub / s])
        assert bool(((x * s) == torch.cat([b, sub])).all())
        out.append(("f32_boundary", x, s))
    out.append(("f32_boundary", torch.cat([b, sub / 0.75]), 0.75))
    out.append(("f32_specials", _specials(F32), 1.0))
    return out


def _pad_to(x, n, fill=0.5):
    return torch.cat([x, torch.full((n - x.numel(),), fill, dtype=x.dtype)])


# ------------------------------------------------------------------------------------------------- guarded buffers
class Guards:
    """1-D sentinel-filled allocations with the tensor PAD elements in; check() holds every surround bit for bit."""

    def __init__(self, dev):
        self.dev, self.items = dev, []

    def out(self, shape, dtype=U8):
        n = 1
        for s in shape:
            n *= s
        buf = sentinel((n + 2 * PAD,), dtype, self.dev)
        self.items.append((buf, n, None))
        return buf[PAD:PAD + n].view(*shape)

    def inp(self, data):
        """`data` (CPU, bf16 / fp32) copied bit for bit between finite giants."""
        n, fill = data.numel(), _GIANT_BITS[data.dtype]
        buf = sentinel((n + 2 * PAD,), data.dtype, self.dev, fill)
        view = buf[PAD:PAD + n].view(*data.shape)
        idt = torch.int16 if data.dtype == BF16 else torch.int32
        view.view(idt).copy_(data.contiguous().view(idt))
        self.items.append((buf, n, fill))
        return view

    def f32(self, data=None, n=None):
        """An fp32 state vector between NaN sentinels, holding `data` or left as sentinels."""
        n = data.numel() if data is not None else n
        buf = sentinel((n + 2 * PAD,), F32, self.dev)
        self.items.append((buf, n, None))
        view = buf[PAD:PAD + n]
        if data is not None:
            view.copy_(data.reshape(-1))
        return view

    def check(self):
        torch.cuda.synchronize()
        for buf, n, fill in self.items:
            assert_guard_intact(buf, (0, 1, PAD, n), fill)


def _amax_state(G, prefill=None, n=1):
    """amax state of n tensors: non-slot floats 3e38, slots 0 or `prefill` ({slot: value})."""
    a = torch.full((n * SLOTS * STRIDE,), GIANT)
    a[::STRIDE] = 0.0
    for k, v in (prefill or {}).items():
        a[k * STRIDE] = v
    return G.f32(a)


def _check_amax(amax, expect_slots, what):
    """Non-slot floats untouched, every slot equal to its expected value (fp32, exact)."""
    a = amax.cpu()
    non = torch.ones(a.numel(), dtype=torch.bool)
    non[::STRIDE] = False
    assert bool((a[non] == GIANT).all()), f"{what}: {int((a[non] != GIANT).sum())} non-slot amax floats changed"
    got = a[::STRIDE]
    if not torch.equal(got, expect_slots):
        k = int((got != expect_slots).nonzero()[0])
        raise AssertionError(f"{what}: amax slot {k} holds {float(got[k]):.9g}, expected {float(expect_slots[k]):.9g} "
                             f"({int((got != expect_slots).sum())} slots differ)")


def _absmax_nonan(x):
    a = x.float().abs()
    return torch.where(torch.isnan(a), torch.zeros_like(a), a)


def _fold_slots(block_max, prefill=None):
    """Per-block maxima (in block-id order) -> the 64 slot values on top of a prefill."""
    s = torch.zeros(SLOTS)
    for k, v in (prefill or {}).items():
        s[k] = v
    nb = block_max.numel()
    padded = torch.cat([block_max, torch.zeros((-nb) % SLOTS)]).view(-1, SLOTS).max(0).values
    return torch.maximum(s, padded)


def _slot_expect_1d(x, prefill=None):
    """cast_fp8 / amax: items of 8 elements, item i belongs to block (i / 256) mod grid, grid = min(ceil(n8 / 256), 2048)."""
    item = _absmax_nonan(x).view(-1, 8).max(1).values
    n8 = item.numel()
    grid = min(-(-n8 // 256), 2048)
    chunk = torch.cat([item, torch.zeros((-n8) % 256)]).view(-1, 256).max(1).values  # 256 consecutive items
    blk = torch.cat([chunk, torch.zeros((-chunk.numel()) % grid)]).view(-1, grid).max(0).values
    return _fold_slots(blk, prefill)


def _slot_expect_2d(x, tile, prefill=None):
    """cast_transpose: tile x tile blocks, block id = bx + by * gridDim.x."""
    a = _absmax_nonan(x)
    R_, C_ = a.shape
    gy, gx = -(-R_ // tile), -(-C_ // tile)
    p = torch.zeros(gy * tile, gx * tile)
    p[:R_, :C_] = a
    blk = p.view(gy, tile, gx, tile).amax((1, 3)).reshape(-1)
    return _fold_slots(blk, prefill)


PREFILL = {3: 1e30, 7: 1e-3, 0: 2.0 ** -140}  # above any data: kept | below: raised | an fp32 subnormal: raised


def _dscale(s, dev):
    return torch.tensor([s], dtype=F32, device=dev)


def _run_cast(C, dev, x, scale, fmt, what):
    """fp8_cast + fp8_amax of a 1-D CPU tensor on guarded buffers: exact bytes, exact slots, guards."""
    G = Guards(dev)
    xd, y = G.inp(x), G.out((x.numel(),))
    am, am2 = _amax_state(G, PREFILL), _amax_state(G, PREFILL)
    C.fp8_cast(xd, y, _dscale(scale, dev), am, fmt)
    C.fp8_amax(xd, am2)
    y2 = G.out((x.numel(),))
    C.fp8_cast(xd, y2, _dscale(scale, dev), None, fmt)  # the amax-less form writes the same bytes
    G.check()
    R.assert_exact(y.cpu(), x, scale, fmt, f"fp8_cast {what}")
    assert torch.equal(y, y2)
    exp = _slot_expect_1d(x, PREFILL)
    _check_amax(am, exp, f"fp8_cast {what}")
    _check_amax(am2, exp, f"fp8_amax {what}")


def _run_ct(C, dev, x, scale, fmt, what, tile, colsum=None):
    """fp8_cast_transpose of a 2-D CPU tensor on guarded buffers; returns (y bytes on the CPU, colsum view or None).
    tile: 64 or 128, the kernel the shape must select (the slot geometry tells them apart). colsum: None, "set"
    or "acc"."""
    G = Guards(dev)
    R_, C_ = x.shape
    xd, y, yt = G.inp(x), G.out((R_, C_)), G.out((C_, R_))
    am = _amax_state(G, PREFILL)
    kw, base = {}, None
    if colsum:
        base = torch.randn(C_, generator=torch.Generator().manual_seed(C_)) * 8
        kw = dict(colsum_out=G.f32(base if colsum == "acc" else None, C_), colsum_accumulate=colsum == "acc")
    C.fp8_cast_transpose(xd, y, yt, _dscale(scale, dev), am, fmt, **kw)
    G.check()
    yc = y.cpu()
    R.assert_exact(yc, x, scale, fmt, f"cast_transpose {what}")
    assert torch.equal(yt.cpu(), yc.t().contiguous()), f"cast_transpose {what}: yt is not the byte transpose of y"
    _check_amax(am, _slot_expect_2d(x, tile, PREFILL), f"cast_transpose {what}")
    return yc, (kw.get("colsum_out"), base)


# ------------------------------------------------------------------------------------------------- exact rounding
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("src", [BF16, F32], ids=["bf16", "fp32"])
def test_exact_rounding(dev, fmt, src):
    C = require_native()
    ran = 0
    for name, x, scale in exact_inputs(fmt):
        if x.dtype != src:
            continue
        c = R.census(x, scale, fmt)
        print(f"inputs fmt {fmt} {name} scale {scale:g}: {x.numel()} values, {c}")
        what = f"fmt {fmt} {name} scale {scale:g}"
        if name.endswith("specials"):
            assert c["nan"] == 4 and c["neg_zero"] >= 2 and c["saturated"] >= 8 and c["to_zero"] >= 4
            _run_cast(C, dev, x, scale, fmt, what)
            yc, _ = _run_ct(C, dev, x.view(4, 16), scale, fmt, what, 64)
            assert int(R.is_nan_code(yc, fmt).sum()) == 4  # (assert_exact compared them; spelled out once more)
            top = R.NFINITE[fmt] - 1
            assert yc.view(-1)[2:6].tolist() == [top, top | 0x80, 0x00, 0x80]  # +-inf -> +-max, +-0 keep the sign
        elif src == BF16:
            assert c["subnormal"] > 0 and (c["ties"] > 0 or scale > 1) and (c["saturated"] > 30000 or scale <= 1)
            _run_cast(C, dev, _pad_to(x, 65536), scale, fmt, what)
            _run_ct(C, dev, _pad_to(x, 320 * 256).view(320, 256), scale, fmt, what + " 64x64", 64)
            _run_ct(C, dev, _pad_to(x, 256 * 256).view(256, 256), scale, fmt, what + " wide", 128)
        else:
            pow2 = scale != 0.75  # the boundary set reaches the kernel's product exactly: every midpoint is a tie
            assert c["ties"] >= (2 * (R.NFINITE[fmt] - 1) if pow2 else 1) and c["subnormal"] > 100 and c["to_zero"] > 100
            _run_cast(C, dev, _pad_to(x, 72 * 64), scale, fmt, what)
            _run_ct(C, dev, _pad_to(x, 72 * 64).view(72, 64), scale, fmt, what, 64)
        ran += 1
    assert ran == 5


def test_gemm_f8_q_nan_row(dev):
    """One NaN byte in row i of A: row i of Y and column i of Y^T are NaN bytes, every other byte is the byte of the
    run without it (mode 0, (256, 256, 128): the ping-pong kernel's quantising epilogue)."""
    C = require_native()
    M, N, K, i = 256, 256, 128, 77
    g = torch.Generator().manual_seed(5)
    A = (torch.randn(M, K, generator=g) * 2).to(torch.float8_e4m3fn).view(U8)
    B = (torch.randn(N, K, generator=g) * 2).to(torch.float8_e4m3fn).view(U8).to(dev)
    one = torch.ones(1, device=dev)
    outs = []
    for nan in (False, True):
        a = A.clone()
        if nan:
            a[i, 5] = 0x7F
        G = Guards(dev)
        Y, Yt = G.out((M, N)), G.out((N, M))
        am = _amax_state(G)
        C.gemm_f8_q(a.to(dev), B, Y, Yt, 0, 0, one, one, 0, _dscale(0.25, dev), am)
        G.check()
        assert torch.equal(Yt, Y.t())
        outs.append((Y.cpu(), am.cpu()[::STRIDE].max()))
    (y0, a0), (y1, a1) = outs
    assert not bool(R.is_nan_code(y0, 0).any())
    assert bool(R.is_nan_code(y1[i], 0).all()), f"{int((~R.is_nan_code(y1[i], 0)).sum())} of {N} bytes of row {i} are finite"
    keep = torch.arange(M) != i
    assert torch.equal(y1[keep], y0[keep])
    assert bool(torch.isfinite(a1)) and float(a1) <= float(a0)  # NaN does not enter the scale state


# ------------------------------------------------------------------------------------------------- tails, geometry
def _geometry_data(shape, dtype, seed):
    """randn * 3 with the unique maximum 100 at the last element (the last block) and -90 at [0, 1]."""
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 3
    x.view(-1)[-1] = 100.0
    x.view(-1)[1] = -90.0
    return x.to(dtype)


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("src", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", [(4, 4), (68, 132), (64, 60), (132, 64), (576, 512)])
def test_cast_transpose_tails(dev, shape, src, fmt):
    C = require_native()
    x = _geometry_data(shape, src, shape[0] + shape[1] + fmt)  # (576 % 128 != 0: the wide kernel refuses it for bf16 too)
    _run_ct(C, dev, x, 0.75, fmt, f"{shape} {src} fmt {fmt}", 64)
    last = -(-shape[0] // 64) * -(-shape[1] // 64) - 1  # the block that holds the maximum: 71 -> slot 7 at (576, 512)
    assert float(_slot_expect_2d(x, 64)[last % 64]) == 100.0


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("colsum", [None, "set", "acc"])
@pytest.mark.parametrize("shape", [(128, 128), (256, 384)])
def test_cast_transpose_wide(dev, shape, colsum, fmt):
    """The 128 x 128 kernel; its column sums (the bias gradient) against fp64: 8 additions per thread, 16 over the
    row groups of a tile, then reduce_rows over the R / 128 tile rows (ceil(. / 64) + 6), on top of the previous
    value when accumulating (helpers.acc_bound)."""
    C = require_native()
    x = _geometry_data(shape, BF16, shape[1] + fmt)
    what = f"wide {shape} fmt {fmt} colsum {colsum}"
    yc, (cs, base) = _run_ct(C, dev, x, 0.75, fmt, what, 128, colsum)
    if colsum:
        depth = 8 + 16 + -(-(shape[0] // 128) // 64) + 6
        s, t = colsum_stored_bound(x, depth)
        if colsum == "acc":
            t, s = acc_bound(t, base, s), s + base.double()
        r = assert_within(cs.cpu(), s, t, what)
        print(f"headroom cast_transpose_wide colsum {r:.4f} {what}")


@pytest.mark.parametrize("src", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", [8, 8 * 257, 8 * (2048 * 256 + 3)])
def test_cast_sizes(dev, n, src):
    """The unique maximum in the last 8 elements, the largest negative value in the first 8."""
    C = require_native()
    x = _geometry_data((n,), src, n % 1000)
    for fmt in (0, 1):
        _run_cast(C, dev, x, 0.75, fmt, f"n {n} {src} fmt {fmt}")
    exp = _slot_expect_1d(x)
    n8 = n // 8
    last_block = ((n8 - 1) // 256) % min(-(-n8 // 256), 2048)
    assert float(exp[last_block % 64]) == 100.0 and float(exp.max()) == 100.0


# ------------------------------------------------------------------------------------------------- update_scale
def _ulps(a, b):
    """Largest distance in fp32 units in the last place between two positive finite fp32 tensors."""
    return int((a.view(torch.int32).long() - b.view(torch.int32).long()).abs().max())


@pytest.mark.parametrize("margin", [-1, 0, 2])
@pytest.mark.parametrize("Hn", [1, 16])
def test_update_scale(dev, Hn, margin):
    """n = 300 tensors (a second block whose last 212 threads are past n), fmax 448 / 57344 mixed, steps 0, 15, 16,
    2^31 + 5 against a history kept here. scale = RN(fmax / (m 2^margin)) and inv_scale = RN(1 / scale) exactly: HIP's
    fp32 division without fast-math is correctly rounded. Tensors 0 .. 9 record nothing at all (window max 0),
    tensors 10 .. 19 record inf at step 0 (frozen while it is in the window): both keep their prefilled bits."""
    C = require_native()
    n, extra = 300, 3
    g = torch.Generator().manual_seed(Hn * 10 + margin + 5)
    G = Guards(dev)
    fmax_c = torch.where(torch.rand(n, generator=g) < 0.5, 448.0, 57344.0)
    scale0, inv0 = torch.rand(n, generator=g) + 0.5, torch.rand(n, generator=g) + 0.5
    hist = G.f32(torch.zeros((n + extra) * Hn)).view(n + extra, Hn)
    hist[n:] = 123.0
    scale, inv, fmax = G.f32(scale0), G.f32(inv0), G.f32(fmax_c)
    amax = G.f32(torch.zeros(n * SLOTS * STRIDE)).view(n, SLOTS * STRIDE)
    h_ref = torch.zeros(n, Hn)
    s_ref, i_ref = scale0.clone(), inv0.clone()
    worst = (0, 0)
    for step in (0, 15, 16, 2 ** 31 + 5):
        a = torch.full((n, SLOTS, STRIDE), GIANT)
        a[:, :, 0] = torch.rand(n, SLOTS, generator=g) * torch.exp2(torch.randint(-20, 20, (n, 1), generator=g).float())
        a[:10, :, 0] = 0.0
        if step == 0:
            a[10:20, 5, 0] = float("inf")
        if step == 15:
            a[20:30, :, 0] = 0.0  # a step without any amax: the history still moves
        amax.copy_(a.view(n, -1))
        C.fp8_update_scale(hist[:n + extra], amax, scale, inv, fmax, step, margin)
        G.check()
        h_ref[:, step % Hn] = a[:, :, 0].amax(1)
        m = h_ref.amax(1)
        upd = (m > 0) & torch.isfinite(m)
        sc = fmax_c / (m * 2.0 ** margin)  # fp32 throughout: one product (exact: a power of two), one division
        s_ref = torch.where(upd, sc, s_ref)
        i_ref = torch.where(upd, 1.0 / sc, i_ref)
        # frozen: the 10 silent tensors always; the inf ones while the inf is in the window (H = 16: steps 0 and 15;
        # H = 1: step 0); at H = 1 the 10 tensors that record nothing at step 15 as well
        assert int((~upd).sum()) == (20 if step < 16 else 10)
        got_a = amax.cpu().view(n, SLOTS, STRIDE)
        assert bool((got_a[:, :, 0] == 0).all()), "slots not reset"
        assert bool((got_a[:, :, 1:] == GIANT).all()), "non-slot amax floats changed"
        hc = hist.cpu()
        assert torch.equal(hc[:n], h_ref) and bool((hc[n:] == 123.0).all()), f"history differs at step {step}"
        sg, ig = scale.cpu(), inv.cpu()
        assert torch.equal(sg[~upd].view(torch.int32), s_ref[~upd].view(torch.int32))  # frozen: bit for bit
        assert torch.equal(ig[~upd].view(torch.int32), i_ref[~upd].view(torch.int32))
        worst = (max(worst[0], _ulps(sg, s_ref)), max(worst[1], _ulps(ig, i_ref)))
        assert torch.equal(sg, s_ref) and torch.equal(ig, i_ref), f"step {step}: scale / inv_scale {worst} ulp off"
    print(f"headroom update_scale ulp distance scale {worst[0]} inv_scale {worst[1]} (H {Hn} margin {margin})")


# ------------------------------------------------------------------------------------------------- rejections
def test_rejections(dev):
    C = require_native()
    one = torch.ones(1, device=dev)
    amax = torch.zeros(C.FP8_AMAX_SLOTS, device=dev)
    short = torch.zeros(C.FP8_AMAX_SLOTS - 1, device=dev)
    u8 = lambda *s: torch.zeros(*s, dtype=U8, device=dev)
    x12 = torch.zeros(12, dtype=BF16, device=dev)
    x16 = torch.zeros(16, dtype=BF16, device=dev)
    bad = [
        lambda: C.fp8_cast(x12, u8(12), one, amax, 0),                                   # numel % 8
        lambda: C.fp8_amax(x12, amax),
        lambda: C.fp8_cast(x16, u8(16), one, short, 0),                                  # a short amax
        lambda: C.fp8_amax(x16, short),
        lambda: C.fp8_cast_transpose(torch.zeros(8, 8, device=dev), u8(8, 8), u8(8, 8), one, short, 0),
        lambda: C.fp8_cast_transpose(torch.zeros(6, 8, device=dev), u8(6, 8), u8(8, 6), one, amax, 0),   # R % 4
        lambda: C.fp8_cast_transpose(torch.zeros(8, 6, device=dev), u8(8, 6), u8(6, 8), one, amax, 0),   # C % 4
        lambda: C.fp8_cast_transpose(torch.zeros(6, 8, dtype=BF16, device=dev), u8(6, 8), u8(8, 6), one, amax, 0),
        lambda: C.fp8_cast_transpose(torch.zeros(128, 128, device=dev), u8(128, 128), u8(128, 128), one, amax, 1,
                                     colsum_out=torch.zeros(128, device=dev)),           # colsum with an fp32 input
    ]
    for k in (1, 2, 3):                                                                  # y / yt at an odd byte offset
        for which in (0, 1):
            for dt in (F32, BF16):
                def f(k=k, which=which, dt=dt):
                    w = torch.zeros(8, 8, dtype=dt, device=dev)
                    ys = [u8(64 + 4)[0:64].view(8, 8), u8(64 + 4)[k:k + 64].view(8, 8)]
                    C.fp8_cast_transpose(w, ys[which == 0], ys[which == 1], one, amax, 0)
                bad.append(f)
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError):
            f()
            torch.cuda.synchronize()
            pytest.fail(f"call {i} was accepted")
    # the aligned forms of the same calls are accepted
    C.fp8_cast_transpose(torch.zeros(8, 8, device=dev), u8(64 + 4)[4:68].view(8, 8), u8(8, 8), one, amax, 0)
    C.fp8_cast(x16, u8(16), one, amax, 0)
    torch.cuda.synchronize()
