import os
import socket

import torch


_PORTS_USED = set()


def free_port() -> int:
    """A rendezvous port for spawned ranks: drawn below the kernel's ephemeral range (32768+), so an
    outgoing connection cannot take it between this check and the rank's bind (which the OS-picked
    port 0 allowed: EADDRINUSE flakes), never handed out twice in one test process."""
    import random
    rng = random.Random()
    for _ in range(200):
        p = rng.randrange(20000, 32000)
        if p in _PORTS_USED:
            continue
        s = socket.socket()
        try:
            s.bind(("127.0.0.1", p))
        except OSError:
            continue
        finally:
            s.close()
        _PORTS_USED.add(p)
        return p
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class TensorCifar(torch.utils.data.Dataset):
    """Pre-tensorised CIFAR-shaped dataset (no transform RNG): [N,3,32,32] float + int labels."""

    def __init__(self, n, seed=0, learnable=True):
        g = torch.Generator().manual_seed(seed)
        self.targets = torch.randint(0, 10, (n,), generator=g)
        x = torch.randn(n, 3, 32, 32, generator=g) * 0.5
        if learnable:
            x = x + self.targets.view(n, 1, 1, 1).float() * 0.2
        self.x = x
        self.classes = [str(i) for i in range(10)]

    def __len__(self):
        return len(self.targets)

    def __getitem__(self, i):
        return self.x[i], int(self.targets[i])


def dist_env(rank, world, port):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})


# ---------------------------------------------------------------------------------------------
# Guarded buffers and the derived GEMM tolerance (tests/test_gemm_bound_cpu.py checks these on
# the CPU; tests/test_gemm_edges_gpu.py and tests/test_gemm_gpu.py use them on the GPU)
# ---------------------------------------------------------------------------------------------
# sentinel bit patterns: a NaN for the float types (any read of it that reaches an output shows),
# 0xA5 bytes for fp8 / uint8 storage (0xA5 is a finite value in both fp8 formats: -0.3125 / -1.25)
_SENTINEL = {torch.float32: (torch.int32, 0x7FC0A5A5), torch.bfloat16: (torch.int16, 0x7FA5),
             torch.uint8: (torch.uint8, 0xA5), torch.float8_e4m3fn: (torch.uint8, 0xA5),
             torch.float8_e5m2: (torch.uint8, 0xA5)}


def sentinel(shape, dtype, dev, fill=None):
    """A tensor of `shape` whose every element holds the sentinel bit pattern of `dtype`."""
    idt, pat = _SENTINEL[dtype]
    buf = torch.empty(*shape, dtype=dtype, device=dev)
    buf.view(idt).fill_(pat if fill is None else fill)
    return buf


def guarded(rows, cols, dtype, dev, ld=None, col_off=0, fill=None):
    """(buf, view): buf is [rows + 2, ld] filled with the sentinel pattern, view = buf[1:1+rows,
    col_off:col_off+cols]. The view's base sits (ld + col_off) elements into the allocation: the caller
    picks ld and col_off so that it meets the bindings' 16-byte rule ((ld + col_off) % 8 == 0 for
    bf16, % 4 for fp32, % 16 for fp8) while the row stride -- and so every later row's alignment --
    is whatever the case wants."""
    ld = cols if ld is None else ld
    assert col_off >= 0 and col_off + cols <= ld
    buf = sentinel((rows + 2, ld), dtype, dev, fill)
    return buf, buf[1:1 + rows, col_off:col_off + cols]


def guarded_like(data, ld=None, col_off=0):
    """`data` [rows, cols] copied into a guarded view (an input surrounded by sentinels)."""
    buf, view = guarded(data.shape[0], data.shape[1], data.dtype, data.device, ld, col_off)
    idt = _SENTINEL[data.dtype][0]
    view.view(idt).copy_(data.view(idt))  # the bits, whatever the dtype (fp8 has no copy kernel of its own)
    return buf, view


def assert_guard_intact(buf, view_spec, fill=None):
    """Everything of `buf` outside the view still holds the sentinel, compared bit for bit (through an
    integer dtype of the same width: NaN != NaN). view_spec is the view itself (a slice of buf) or
    (row0, rows, col0, cols); a 1-D buf counts as one row. Reports the first offending (row, col)."""
    idt, pat = _SENTINEL[buf.dtype]
    pat = pat if fill is None else fill
    b2 = buf if buf.dim() == 2 else buf.view(1, -1)
    if isinstance(view_spec, torch.Tensor):
        v = view_spec
        off = v.storage_offset() - buf.storage_offset()
        ld = b2.stride(0)
        assert off >= 0 and v.stride(-1) == 1 and (v.dim() == 1 or v.stride(0) == ld)
        row0, col0 = (off // ld, off % ld) if b2.shape[0] > 1 else (0, off)
        rows, cols = (v.shape[0], v.shape[1]) if v.dim() == 2 else (1, v.shape[0])
    else:
        row0, rows, col0, cols = view_spec
    assert row0 + rows <= b2.shape[0] and col0 + cols <= b2.shape[1]
    bad = b2.view(idt) != pat
    bad[row0:row0 + rows, col0:col0 + cols] = False
    if bool(bad.any()):
        r, c = (int(i) for i in bad.nonzero()[0])
        got = int(b2.view(idt)[r, c])
        raise AssertionError(f"guard overwritten at (row {r}, col {c}) of a {tuple(b2.shape)} buffer whose view is "
                             f"rows {row0}..{row0 + rows - 1}, cols {col0}..{col0 + cols - 1}: "
                             f"bits {got & 0xFFFFFFFF:#x}, sentinel {pat:#x} ({int(bad.sum())} elements differ)")


_U32 = 2.0 ** -24        # unit roundoff of fp32
_TANHF_ABS = 2.0 ** -20  # allowance for tanhf itself (see tanh_bound)


def gemm_expected(A64, B64, terms=None):
    """fp64 value of alpha * A.B + bias + res + c_prev. A64 [M,K], B64 [K,N] (the mathematical
    layout), terms: dict with any of alpha (float), bias [N], res [M,N], c_prev [M,N] (fp64)."""
    t = terms or {}
    e = float(t.get("alpha", 1.0)) * (A64 @ B64)
    for k in ("bias", "res", "c_prev"):
        if t.get(k) is not None:
            e = e + t[k]
    return e


def gemm_t32(A64, B64, K, terms=None):
    """Bound on |computed fp32 value - fp64 value| of one GEMM output element before its store.

    bf16 / fp8 inputs have products that are exact in fp32 (and in the fp64 reference), so the only
    errors are the at most K additions of the accumulation, each at most 2u of the running sum
    (u = 2^-24; the 2 allows a matrix core that truncates instead of rounding), and a handful of
    epilogue operations (alpha, bias, residual, previous C) -- 4 more. The running sums are bounded by
    the sum of the magnitudes, hence
        t32 = 2 (K + 4) 2^-24 (|alpha| (|A|.|B|) + |bias| + |res| + |c_prev|) + 1e-30."""
    t = terms or {}
    mag = abs(float(t.get("alpha", 1.0))) * (A64.abs() @ B64.abs())
    for k in ("bias", "res", "c_prev"):
        if t.get(k) is not None:
            mag = mag + t[k].abs()
    return 2.0 * (K + 4) * _U32 * mag + 1e-30


def _bf16_rn(x64):
    """x (fp64) -> nearest fp32 -> nearest bf16, back as fp64; monotone, like the kernels' final
    f32 -> bf16 round-to-nearest-even."""
    return x64.float().to(torch.bfloat16).double()


def store_bound(expected, t, out_dtype):
    """Tolerance on |stored - expected| when the kernel's fp32 value c obeys |c - expected| <= t.

    fp32 store: t. bf16 store: the kernel writes RN(c), rounding is monotone, so the stored value
    lies in [RN(expected - t), RN(expected + t)]; the tolerance is the farther end of that interval.
    No constant enters: the rounding term is bf16's own spacing at the element. (It is at most
    t (1 + 2^-8) + 2^-8 |expected| -- bf16 keeps 8 significant bits, so ONE round-to-nearest moves a
    value by up to 2^-8 relative; a 2^-9 constant would reject every value correctly rounded from
    the lower half of a binade, see test_gemm_bound_cpu.test_half_the_unit_roundoff_rejects_correct_rounding.)"""
    if out_dtype == torch.float32:
        return t
    assert out_dtype == torch.bfloat16
    ends = torch.maximum((_bf16_rn(expected + t) - expected).abs(), (_bf16_rn(expected - t) - expected).abs())
    return torch.maximum(ends, t)  # (never below t: an exactly representable expected value keeps a nonzero tolerance)


def gemm_bound(A64, B64, K, terms, out_dtype):
    """Per-element tolerance of a plain / bias / residual / accumulate GEMM output against
    gemm_expected(): derived (gemm_t32 + the store's rounding), not tuned."""
    return store_bound(gemm_expected(A64, B64, terms), gemm_t32(A64, B64, K, terms), out_dtype)


def _phi(x64):  # standard normal CDF, no cancellation in the negative tail
    return 0.5 * torch.special.erfc(-x64 / 2.0 ** 0.5)


def gelu64(x64):
    return x64 * _phi(x64)


def gelu_grad64(x64):
    return _phi(x64) + x64 * torch.exp(-0.5 * x64 * x64) / (2.0 * torch.pi) ** 0.5


def gelu_out_bound(aux64):
    """GELU epilogue (mode 1): tolerance of `out` against fp64 GELU at the kernel's OWN saved
    pre-activation aux (bf16 points). The kernels multiply x by a table entry that is Phi(x) rounded to
    fp32 and round the product to bf16: within 2^-8 |gelu| (+ 1e-30). Outside the table's exact range
    (2^-20 <= |x| < 8, csrc/include/mlt_gelu_table.inc) the entry is the limit value 0.5 / 0 / 1,
    whose exact distance from Phi(x) is added: at most 5e-15 in the output for |x| >= 8."""
    g = gelu64(aux64)
    a = aux64.abs()
    lim = torch.where(a < 2.0 ** -20, torch.full_like(a, 0.5), (aux64 > 0).double())
    sat = torch.where((a < 2.0 ** -20) | (a >= 8.0), a * (_phi(aux64) - lim).abs(), torch.zeros_like(a))
    return 2.0 ** -8 * g.abs() + sat + 1e-30


def dgelu_t(pre_expected, t32, aux64):
    """dGELU epilogue (mode 2): out = pre * gelu'(aux), aux a given bf16 tensor; bound on the fp32 value
    before the store. The fp32 error of pre scales by |gelu'(aux)|; the table entry is gelu'(x) rounded
    to fp32 (2^-24 relative; outside 2^-20 <= |x| < 8 the limit value 0.5 / 0 / 1, exact distance
    added) and the product rounds once more in fp32 (inside t32's four spare operations)."""
    gp = gelu_grad64(aux64)
    a = aux64.abs()
    lim = torch.where(a < 2.0 ** -20, torch.full_like(a, 0.5), (aux64 > 0).double())
    tab = torch.where((a < 2.0 ** -20) | (a >= 8.0), (gp - lim).abs(), _U32 * gp.abs())
    return t32 * gp.abs() + (pre_expected.abs() + t32) * tab


def dgelu_bound(pre_expected, t32, aux64, out_dtype):
    """Tolerance of a dGELU output against pre_expected * gelu'(aux): dgelu_t plus the store's rounding."""
    return store_bound(pre_expected * gelu_grad64(aux64), dgelu_t(pre_expected, t32, aux64), out_dtype)


def tanh_t(t32):
    """tanh epilogue (mode 3): tanh is 1-Lipschitz, so the pre-activation's t32 carries over, plus an
    absolute 2^-20 for tanhf itself. tanhf's error has not been measured on this device; 2^-20 is 2^11
    times below bf16's rounding step near 1, so the allowance cannot hide a wrong element."""
    return t32 + _TANHF_ABS


def tanh_bound(pre_expected, t32, out_dtype=torch.bfloat16):
    """Tolerance of a tanh output (bf16 outputs are what the tests check): tanh_t plus the store's rounding."""
    return store_bound(torch.tanh(pre_expected), tanh_t(t32), out_dtype)


def bf16_t_used(out, expected, t, iters=14):
    """How much of the fp32-level allowance t a bf16 output needs: the smallest s in [0, 1] with
    RN(expected - s t) <= out <= RN(expected + s t), largest over the elements (bisection, 2^-iters
    resolution). |err| / store_bound says little for bf16 -- a correctly rounded value already sits at
    the end of a narrow interval -- so this is the headroom figure for bf16 outputs."""
    o = out.double()
    d = torch.sign(o - _bf16_rn(expected))
    lo, hi = torch.zeros_like(o), torch.ones_like(o)
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        reached = (_bf16_rn(expected + d * mid * t) - o) * d >= 0
        hi = torch.where(reached, mid, hi)
        lo = torch.where(reached, lo, mid)
    return float(torch.where(d == 0, torch.zeros_like(o), hi).max())


def assert_within(out, expected, tol, what=""):
    """|out - expected| <= tol at every element (a NaN fails); returns the largest |err| / tol."""
    err = (out.double() - expected).abs()
    ok = err <= tol
    if not bool(ok.all()):
        idx = tuple(int(i) for i in (~ok).nonzero()[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} elements outside the bound, first at {idx}: "
                             f"got {float(out[idx]):.9g}, expected {float(expected[idx]):.9g}, "
                             f"|err| {float(err[idx]):.3g} > tol {float(tol[idx]):.3g}")
    return float((err / tol).max())
