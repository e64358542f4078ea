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


# ---------------------------------------------------------------------------------------------
# Derived attention bounds (tests/test_attn_bound_cpu.py checks these against a torch emulation of
# the kernels on the CPU; tests/test_attention_edges_gpu.py uses them on the GPU). Everything is fp64
# from the bf16 inputs, per (batch, head): q, k, v, do, o are [B, H, S, 64], lse [B, H, S], lens a
# list of B valid key counts or None, keep a [B, H, S, S] bool mask or None, c = attention_scale(p).
# Each function returns references together with `t`, the allowance on the kernel's fp32 value before
# its store; bf16 outputs then go through store_bound.
# ---------------------------------------------------------------------------------------------
_UB = 2.0 ** -8                  # unit roundoff of bf16 as the kernels' packs use it (see store_bound on 2^-9)
_LOG2E = 1.4426950408889634
_LN2 = 0.6931471805599453
_EXP2_REL = 2.0 ** -22           # v_exp_f32: 1 ulp (2^-23) in AMD's CDNA ISA reference; the allowance is 2 ulp


def attn_sl2(scale):
    """fp32(scale * log2 e): the factor that takes q.k to a base-2 exponent."""
    return float(torch.tensor(float(scale) * _LOG2E, dtype=torch.float64).float())


def attn_split(qkv, B, S, H):
    """qkv [B * S, 3 * H * 64] -> q, k, v [B, H, S, 64] in fp64."""
    q, k, v = qkv.double().view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    return q, k, v


def attn_heads(x, B, S, H):
    """[B * S, H * 64] -> [B, H, S, 64] in fp64."""
    return x.double().view(B, S, H, 64).permute(0, 2, 1, 3)


def _attn_valid(lens, B, S, dev):
    n = torch.full((B,), S, dtype=torch.int64) if lens is None else torch.as_tensor(list(lens), dtype=torch.int64)
    return (torch.arange(S)[None, :] < n[:, None]).to(dev)[:, None, None, :]  # [B, 1, 1, S] over the keys


def _attn_eta(q, k, s2, sl2):
    """Relative error of one fp32 probability 2^(s2 - m), without any bf16 rounding:
        ln2 (64 2^-24 sl2 sum_d |q_id k_jd| + 2^-22 |s2_ij|) + 2^-22
    = the fp32 accumulation of the 64-term dot product (the bf16 x bf16 products are exact), the fma that
    scales it and the rounding of sl2 itself, carried through 2^x (d 2^x = ln2 2^x dx), and v_exp_f32."""
    return _LN2 * (64 * _U32 * sl2 * (q.abs() @ k.abs().transpose(-1, -2)) + 2.0 ** -22 * s2.abs()) + _EXP2_REL


def attn_fwd_bound(q, k, v, lens, scale, keep=None, c=1.0):
    """(O, t_O, LSE2, t_LSE) of the forward kernel (attn_fwd_lean_kernel).

    Reference: sl2 = fp32(scale log2 e); s2_ij = (q_i . k_j) sl2 for j < len, -inf otherwise; p^ = softmax
    over j (base 2); w_j = c M_ij v_j with a keep mask M (w_j = v_j without); O_i = sum_j p^_ij w_j; LSE2_i =
    the base-2 logsumexp of the UNDROPPED scores.

    Per-score relative error of the bf16 probability the kernel multiplies with,
        eps_ij = u + ln2 (64 2^-24 sl2 sum_d |q_id k_jd| + 2^-22 |s2_ij|) + 2^-22,    u = 2^-8:
      u ......... pack_acc rounds P to bf16 before it re-enters the MFMA (unit roundoff 2^-8; 2^-9 is broken by
                  the CPU emulation at S = 17, len = 5: test_half_the_unit_roundoff_rejects_the_emulation)
      64 2^-24 .. fp32 accumulation of the 64-term q.k product (_attn_eta)
      2^-22 |s2|  the fma(s, sl2, -m) and the rounding of sl2
      2^-22 ..... v_exp_f32
    The row sum l comes from the SAME bf16 P as the P.V product (the all-ones MFMA), so numerator and
    denominator err together: O' - O = sum_j p^_ij eps_ij (w_j - O_i) / (1 + sum_j p^_ij eps_ij), hence
        t_O[i,d] = sum_j p^_ij eps_ij |w_jd - O_id| / (1 - 2u)       the tied bf16 / exponent errors
                 + S 2^-24 sum_j p^_ij |w_jd|                         fp32 accumulation over the keys
                 + 2^-22 |O_id|                                       1 / l, the multiply by it (and by c)
        t_LSE[i] = sum_j p^_ij eps_ij / (ln2 (1 - 2u))                l's relative error through log2
                 + 2^-21 max(1, |LSE2_i|)                             v_log_f32 and m + log2 l
    The running max m (stale by up to 2^8 under defer-max) cancels between P and the saved m + log2 l."""
    B, H, S, _ = q.shape
    sl2 = attn_sl2(scale)
    valid = _attn_valid(lens, B, S, q.device)
    s2 = (q @ k.transpose(-1, -2)) * sl2
    s2m = s2.masked_fill(~valid, float("-inf"))
    lse2 = torch.logsumexp(s2m * _LN2, -1) / _LN2
    ph = torch.exp2(s2m - lse2[..., None])
    pe = ph * (_UB + _attn_eta(q, k, s2, sl2))
    cm = torch.ones_like(ph) if keep is None else keep.double() * c
    O = (ph * cm) @ v
    tO = S * _U32 * ((ph * cm) @ v.abs()) + 2.0 ** -22 * O.abs() + 1e-30
    for b in range(B):
        for h in range(H):
            w = cm[b, h][:, :, None] * v[b, h][None, :, :]  # [S(i), S(j), 64]
            tO[b, h] += (pe[b, h][:, :, None] * (w - O[b, h][:, None, :]).abs()).sum(1) / (1 - 2 * _UB)
    tL = pe.sum(-1) / (_LN2 * (1 - 2 * _UB)) + 2.0 ** -21 * lse2.abs().clamp_min(1.0)
    return O, tO, lse2, tL


def attn_bwd_bound(q, k, v, do, o, lse, lens, scale, keep=None, c=1.0):
    """References and allowances of the backward kernels (attn_bwd_dq_ring_kernel, attn_bwd_dkdv_ring_kernel
    and the register-staged pair) as a dict: delta, t_delta [B, H, S]; dq, t_dq, dk, t_dk, dv, t_dv [B, H, S, 64].

    attn_bwd is a function of (qkv, out, dout, lse): `o` and `lse` are the forward kernel's OWN bf16 output
    and fp32 LSE, given inputs here as they are to the kernels.
        P_ij = 2^(s2_ij - lse_i) for j < len, else 0 (not renormalised);  delta_i = sum_d dO_id O_id
        dP_ij = sum_d dO_id v_jd;   dV_j = c sum_i (P o M)_ij dO_i;   dS_ij = P_ij (c M_ij dP_ij - delta_i)
        dQ_i = scale sum_j dS_ij k_j;   dK_j = scale sum_i dS_ij q_i
    Rounding points, as attention.hip has them:
      eta_ij = _attn_eta + ln2 2^-24 |lse_i| ... fast_exp2(sv * sl2 - lse): the fp32 score, its scaling, the
                  subtraction of the given lse (relative to the larger operand), v_exp_f32
      t_delta[i] = 64 2^-24 sum_d |dO_id O_id| ... 64 exact products summed in fp32 (the dQ prologue)
      u on P o M and on dS ..................... pack_acc: both leave the accumulators as bf16 MFMA operands
      t_dV[j,d] = c sum_i (u + eta_ij)(P o M)_ij |dO_id| + (S + 4) 2^-24 c sum_i (P o M)_ij |dO_id|
                  (fp32 accumulation over the S queries, then `dv *= c` once on the finished sum)
      e_dS_ij = (u + eta_ij)|dS_ij| + P_ij (64 2^-24 c M_ij sum_d |dO_id v_jd| + 2^-23 (c M_ij |dP_ij| + |delta_i|)
                  + t_delta[i]) ... dP is an MFMA accumulation started at -delta (or 0, then one
                  fma(c M, dP, -delta) under dropout): its 64 additions, the fold-in of delta, delta's own error
      t_dQ[i,d] = scale sum_j e_dS_ij |k_jd| + (S + 4) 2^-24 scale sum_j |dS_ij k_jd|
      t_dK[j,d] = scale sum_i e_dS_ij |q_id| + (S + 4) 2^-24 scale sum_i |dS_ij q_id|
                  (`scale` multiplies the finished fp32 accumulator once, AFTER the accumulation: the S additions
                  plus the rounding of `scale` to fp32 and that multiply, inside the 4 spare operations)."""
    B, H, S, _ = q.shape
    sl2 = attn_sl2(scale)
    valid = _attn_valid(lens, B, S, q.device)
    T_ = lambda x: x.transpose(-1, -2)
    s2 = (q @ T_(k)) * sl2
    P = torch.where(valid, torch.exp2(s2 - lse[..., None]), torch.zeros_like(s2))
    ueta = _UB + _attn_eta(q, k, s2, sl2) + _LN2 * _U32 * lse.abs()[..., None]
    delta = (do * o).sum(-1)
    t_delta = 64 * _U32 * (do * o).abs().sum(-1) + 1e-30
    cm = torch.ones_like(P) if keep is None else keep.double() * c
    keepd = torch.ones_like(P) if keep is None else keep.double()
    dP = do @ T_(v)
    PM = P * keepd
    acc = (S + 4) * _U32
    dV = c * (T_(PM) @ do)
    t_dV = c * (T_(ueta * PM) @ do.abs()) + acc * c * (T_(PM) @ do.abs()) + 1e-30
    dS = P * (cm * dP - delta[..., None])
    e_dS = ueta * dS.abs() + P * (64 * _U32 * cm * (do.abs() @ T_(v.abs()))
                                  + 2.0 ** -23 * (cm * dP.abs() + delta.abs()[..., None]) + t_delta[..., None])
    dQ = scale * (dS @ k)
    t_dQ = scale * (e_dS @ k.abs()) + acc * scale * (dS.abs() @ k.abs()) + 1e-30
    dK = scale * (T_(dS) @ q)
    t_dK = scale * (T_(e_dS) @ q.abs()) + acc * scale * (T_(dS.abs()) @ q.abs()) + 1e-30
    return dict(delta=delta, t_delta=t_delta, dq=dQ, t_dq=t_dQ, dk=dK, t_dk=t_dK, dv=dV, t_dv=t_dV)


# (B, S, H, lens, scale) of the attention edge cases, padded mode, and the S at which dropout p = 0.1 runs too
ATTN_EDGE_SHAPES = [
    (2, 1, 1, None, 0.125),               # one query, one key
    (2, 17, 2, [17, 5], 0.125),           # S < 64: min(AB, S) rows already in the prologue tile
    (2, 63, 1, [63, 1], 0.125),           # one row short of a block; a one-key sequence
    (3, 65, 1, [65, 64, 1], 0.125),       # a 1-row tail block, which lens = 64 makes a fully masked key block
    (2, 127, 2, None, 0.125),             # the last S below the 2-group kernels
    (2, 129, 1, [129, 128], 0.2),         # 2-group kernels with a 1-row tail; a scale that is no power of two
    (2, 192, 2, [192, 130], 0.125),       # FULLT, the last 2-group block half empty, exactly kRing - 1 stages
    (2, 320, 1, [320, 257], 0.125),       # FULLT, 5 stages: the first reuse of a ring slot
]
ATTN_EDGE_DROPOUT_S = (17, 65, 192, 320)


def attn_edge_inputs(B, S, H, lens, scale, seed, sentinel_keys=True):
    """qkv [B * S, 3 * H * 64] and dout [B * S, H * 64] (bf16, CPU) of one edge case. With `lens`, per (b, h),
    the construction of test_attention_fwd_defer_max_branches: key len - 1 is a multiple of query 0, so that its
    base-2 score leads row 0 by about 40 (the last valid key then carries row 0 alone: t_O there is at fp32 level
    and losing the key is an error of order |v|), and where len < S key len is the same multiple of query 1 (the
    first masked key would carry row 1 if it leaked)."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * S, 3 * H * 64, generator=g) * 0.5
    dout = torch.randn(B * S, H * 64, generator=g)
    if lens is not None and sentinel_keys:
        x = qkv.view(B, S, 3, H, 64)
        for b in range(B):
            for h in range(H):
                for key, qi in ((lens[b] - 1, 0), (lens[b], 1)):
                    if key < S and qi < S:
                        qv = x[b, qi, 0, h].to(torch.bfloat16).double()
                        x[b, key, 1, h] = (qv * (40.0 / (qv.pow(2).sum().item() * scale * _LOG2E))).float()
    return qkv.to(torch.bfloat16), dout.to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------
# Derived bounds of the row kernels: LayerNorm, embeddings, reduce_rows (layernorm.hip), colsum (gemm.hip)
# and the classifier head (head.hip). tests/test_rowkernel_bound_cpu.py checks them against a torch fp32
# emulation of the kernels on the CPU; tests/test_rowkernel_edges_gpu.py uses them on the GPU. All
# references are fp64 from the bf16 / fp32 inputs, `t` is the allowance on the kernel's fp32 value before
# its store (bf16 outputs then go through store_bound), u = 2^-24. E = D / 64 is the number of values one
# lane holds: it sums them in order, then wave_sum adds 6 levels of an xor butterfly.
# ---------------------------------------------------------------------------------------------
_RSQRT_REL = 2.0 ** -22  # allowance for rsqrtf: 2 ulp. Not measured on the device; the rstd headroom that
#                          tests/test_rowkernel_edges_gpu.py prints (and records in its docstring) is its record.
ROWK_EPS = 1e-5
ROWK_LN_WIDTHS = (256, 512, 768, 1024)  # VPL = 1 .. 4
# rows: 1 = three idle waves; 5 = a 1-row tail block; 2053 = five waves walk a second row and every other
# wave's prefetch clamps to the last row; 4100 = four waves walk a third row (a pipeline register reused twice)
ROWK_LN_ROWS = (1, 5, 2053, 4100)


def _ceil_div(a, b):
    return -(-a // b)


def ln_partial_blocks(rows):
    """ln_bwd_partial_blocks of layernorm.hip: 4 rows per block, at most 512 blocks."""
    return min(_ceil_div(rows, 4), 512)


def ln_bwd_depth(rows):
    """Number of fp32 additions behind one column output of the LayerNorm backward: the wave's own rows
    (ceil(rows / (4 nb))), the 4-wave LDS sum (2 levels), reduce_rows' lane stride over the nb partial rows
    (ceil(nb / 64)) and its 6-level butterfly."""
    nb = ln_partial_blocks(rows)
    return _ceil_div(rows, 4 * nb) + 2 + _ceil_div(nb, 64) + 6


def ln_edge_inputs(rows, D, seed):
    """(x, dy, dres bf16 [rows, D]; gamma, beta fp32 [D]) on the CPU. The rows are 0.5 + 2 N(0, 1), except the
    ill-conditioned ones a correct kernel must be told apart on:
      constant row (all 3): var = 0, only eps stands under the root;
      64 + N(0, 1) and 1000 + N(0, 16) (std 4; bf16's spacing there is 4): mean >> spread, where a one-pass
      variance E[x^2] - mean^2 loses its digits.
    They are rows 0, 1 and (rows >= 3) 2, and again the last row (rows >= 5): the constant one at 5 rows, the
    1000 one at 2053 (the row every clamped prefetch reads), the 64 one at 4100. A single row is the 64 one."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g) * 2.0 + 0.5
    special = lambda k: (torch.full((D,), 3.0), 64.0 + torch.randn(D, generator=g),
                         1000.0 + 4.0 * torch.randn(D, generator=g))[k]
    if rows == 1:
        x[0] = special(1)
    else:
        for k in range(min(rows, 3)):
            x[k] = special(k)
        if rows >= 5:
            x[rows - 1] = special({5: 0, 2053: 2}.get(rows, 1))
    dy = torch.randn(rows, D, generator=g)
    dres = torch.randn(rows, D, generator=g)
    gamma = torch.randn(D, generator=g) * 0.2 + 1
    beta = torch.randn(D, generator=g) * 0.1
    bf = lambda a: a.to(torch.bfloat16)
    return bf(x), bf(dy), bf(dres), gamma, beta


def ln_fwd_bound(x, gamma, beta, eps):
    """(mean, t_mean, rstd, t_rstd, Y, t_Y) of ln_fwd_kernel (ln_fwd_row), per row: mu = mean(x),
    var = mean((x - mu)^2), rs = 1 / sqrt(var + eps) with eps as the kernel holds it (rounded to fp32),
    Y = (x - mu) rs gamma + beta.
      t_mean = (E + 8) u mean|x| ... E - 1 + 6 additions whose running sums are bounded by sum|x|, 1 / D
                  rounded once, one multiply: E + 7, one spare
      rel_rs = 0.5 (E + 12) u + 0.5 t_mean^2 / (var + eps) + 2^-22 ... the relative error of rs:
                  (E + 12) u: the second pass sums squares of d = x - mu' (u on d twice, u on d d, E + 5
                    additions of positive terms, the scaling by 1 / D, the + eps), halved by the root;
                  t_mean^2: mean((x - mu')^2) = var + (mu - mu')^2 exactly, the kernel's own mean error
                    re-entering the variance (second order: this is what a two-pass variance buys);
                  2^-22: rsqrtf (_RSQRT_REL)
      t_rstd = rs rel_rs
      t_Y[i] = |gamma_i| rs (t_mean + |x_i - mu| (rel_rs + 3u)) + u |Y_i| + 1e-30 ... mu's error moves every
                  x_i - mu by t_mean; rs's error and the three roundings of (x - mu) rs gamma scale with
                  |x_i - mu|; the final + beta rounds at the size of Y.
    The first-order expansion of the root needs t_mean^2 <= (var + eps) / 4, which is asserted per row."""
    x, g, b = x.double(), gamma.double(), beta.double()
    E = x.shape[1] // 64
    eps = float(torch.tensor(eps, dtype=torch.float32))
    mu = x.mean(1)
    xc = x - mu[:, None]
    var = (xc * xc).mean(1)
    rs = 1.0 / torch.sqrt(var + eps)
    t_mean = (E + 8) * _U32 * x.abs().mean(1) + 1e-30
    bad = t_mean ** 2 > (var + eps) / 4
    assert not bool(bad.any()), (f"row {int(bad.nonzero()[0])}: t_mean^2 = {float(t_mean[bad][0] ** 2):.3g} exceeds "
                                 f"(var + eps) / 4 = {float((var + eps)[bad][0] / 4):.3g}: outside the first-order range")
    rel = 0.5 * (E + 12) * _U32 + 0.5 * t_mean ** 2 / (var + eps) + _RSQRT_REL
    Y = xc * rs[:, None] * g + b
    t_Y = g.abs() * rs[:, None] * (t_mean[:, None] + xc.abs() * (rel[:, None] + 3 * _U32)) + _U32 * Y.abs() + 1e-30
    return mu, t_mean, rs, rs * rel, Y, t_Y


def acc_bound(t, prev, s):
    """Allowance of an accumulating form `prev + s` whose sum s has the allowance t: t + u (|prev| + |s|)."""
    return t + _U32 * (prev.double().abs() + s.abs())


def ln_bwd_bound(dy, x, gamma, mean, rstd, dres=None, depth=None):
    """dict(dx, t_dx [rows, D]; dgamma, t_dgamma, dbeta, t_dbeta [D]) of ln_bwd_kernel + reduce_rows.

    `mean` and `rstd` are the forward kernel's OWN saved fp32 values, given inputs here as they are to the
    kernel (attn_bwd_bound takes lse the same way). xh = (x - mean) rstd, t = dy gamma, s1 = mean(t),
    s2 = mean(t xh), dx = rstd (t - s1 - xh s2) + dres; dgamma = sum_rows dy xh, dbeta = sum_rows dy.
      t_s1 = (E + 9) u mean|t| ...... u on each product t, E + 5 additions, 1 / D rounded, one multiply
      t_s2 = (E + 12) u mean|t xh| .. as s1, plus the two roundings of xh and the product t xh
      t_dx[i] = rstd (t_s1 + |xh_i| t_s2 + 7u (|t_i| + |s1| + |xh_i s2|)) + u |dx_i| + 1e-30 ... the errors of
                  s1 and s2 as they enter, up to 7 roundings on the three terms of the bracket (t, xh twice,
                  xh s2, two subtractions, the multiply by rstd), and the final + dres at the size of dx
      depth = ln_bwd_depth(rows), the additions behind a column output
      t_dgamma = (depth + 3) u sum_rows |dy xh| ... the 3: the two roundings of xh and the product dy xh
      t_dbeta = depth u sum_rows |dy|
    The accumulating forms add acc_bound's u (|previous| + |sum|). dxsum is no function of these inputs alone
    (it sums the ROUNDED dx): see colsum_stored_bound."""
    dy, x, g = dy.double(), x.double(), gamma.double()
    mean, rstd = mean.double()[:, None], rstd.double()[:, None]
    rows, D = x.shape
    E = D // 64
    depth = ln_bwd_depth(rows) if depth is None else depth
    xh = (x - mean) * rstd
    t = dy * g
    s1, s2 = t.mean(1, keepdim=True), (t * xh).mean(1, keepdim=True)
    dx = rstd * (t - s1 - xh * s2)
    if dres is not None:
        dx = dx + dres.double()
    t_s1 = (E + 9) * _U32 * t.abs().mean(1, keepdim=True)
    t_s2 = (E + 12) * _U32 * (t * xh).abs().mean(1, keepdim=True)
    t_dx = rstd * (t_s1 + xh.abs() * t_s2 + 7 * _U32 * (t.abs() + s1.abs() + (xh * s2).abs())) + _U32 * dx.abs() + 1e-30
    return dict(dx=dx, t_dx=t_dx, dgamma=(dy * xh).sum(0), t_dgamma=(depth + 3) * _U32 * (dy * xh).abs().sum(0) + 1e-30,
                dbeta=dy.sum(0), t_dbeta=depth * _U32 * dy.abs().sum(0) + 1e-30)


def colsum_stored_bound(X, depth):
    """(sum, t) of a column sum over the rows of a STORED bf16 matrix (the fused dxsum of ln_bwd_kernel, which
    adds the bf16-rounded DX -- or DXM under dropout -- and colsum): the fp64 column sum of those very values,
    t = depth u sum_rows |X| + 1e-30 with `depth` the number of additions behind one output."""
    X = X.double()
    return X.sum(0), depth * _U32 * X.abs().sum(0) + 1e-30


def colsum_geometry(M):
    """(R, rpb) of colsum_geometry in gemm.hip: R row slabs of rpb rows each (the last one shorter)."""
    R = 1 if M < 32 else min(_ceil_div(M, 32), 256)
    rpb = _ceil_div(M, R)
    return _ceil_div(M, rpb), rpb


def colsum_depth(M):
    """Additions behind one colsum output: a wave's share of its slab (every 4th row: ceil(rpb / 4)), the
    4-wave LDS sum (2), reduce_rows' lane stride over the R slabs (ceil(R / 64)) and its butterfly (6)."""
    R, rpb = colsum_geometry(M)
    return _ceil_div(rpb, 4) + 2 + _ceil_div(R, 64) + 6


# (M, N): two slabs, the second of 16 rows | a remainder loop after one unrolled 16-row step | rpb = 33 |
# one row, N a multiple of the 512-column strip
ROWK_COLSUM_CASES = [(33, 8), (45, 520), (8193, 16), (1, 1024)]

# Embedding edge cases: (name, B, S, ids, ntype, tt). V = 50 word rows, 40 position rows.
#   ids: "rand" | "equal" (one run covers the batch) | "clamp" (holds -3 and V + 2: rows 0 and V - 1)
#   tt: None | "rand" (0 / 1) | "clamp" (0 / 1 / 2: the 2 reads row 1)
ROWK_EMBED_V, ROWK_EMBED_P = 50, 40
ROWK_EMBED_CASES = [
    ("b3s5", 3, 5, "rand", 2, "rand"),         # rows = 15: a 3-row tail block; S = 5: 3 idle waves in the position kernel's block 1
    ("b2s33", 2, 33, "rand", 1, None),         # S > 32, a one-row type table without token types
    ("b1s1", 1, 1, "rand", 2, "rand"),         # one token
    ("equal", 3, 5, "equal", 1, None),         # every id equal: a single run
    ("clamp", 2, 33, "clamp", 2, "clamp"),     # out-of-range ids and token types
    ("type1row", 3, 5, "rand", 1, "rand"),     # a one-row type table WITH type-1 tokens: forward and backward clamp to row 0
]


def embed_edge_inputs(name, D, seed):
    """dict of one embedding case on the CPU: ids, tt (or None) int64 [B * S]; ww [V, D], wp [P, D], wt [ntype, D],
    dout [B * S, D] bf16; gw0, gp0, gt0 fp32 prefills of the gradient tables."""
    _, B, S, ik, ntype, tk = next(c for c in ROWK_EMBED_CASES if c[0] == name)
    V, P = ROWK_EMBED_V, ROWK_EMBED_P
    g = torch.Generator().manual_seed(seed)
    n = B * S
    ids = torch.randint(0, V, (n,), generator=g)
    if ik == "equal":
        ids = torch.full((n,), 17)
    elif ik == "clamp":
        ids[3], ids[n - 1], ids[n // 2] = -3, V + 2, V + 2
    tt = None if tk is None else torch.randint(0, 2, (n,), generator=g)
    if tk is not None and n >= 2:
        tt[0], tt[n - 1] = 0, 1  # both types present
    if tk == "clamp":
        tt[5] = 2
    bf = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16)
    f = lambda *s: torch.randn(*s, generator=g)
    return dict(B=B, S=S, V=V, P=P, ntype=ntype, ids=ids, tt=tt, ww=bf(V, D), wp=bf(P, D), wt=bf(ntype, D),
                dout=bf(n, D), gw0=f(V, D), gp0=f(P, D), gt0=f(ntype, D))


def embed_rows(ids, tt, S, V, ntype):
    """The table rows the forward reads for every token: clamped word ids, positions row % S, clamped types."""
    n = ids.numel()
    ty = torch.zeros_like(ids) if tt is None else tt.clamp(0, ntype - 1)
    return ids.clamp(0, V - 1), torch.arange(n, device=ids.device) % S, ty


def embed_fwd_bound(ww, wp, wt, ids, tt, S):
    """(out, t) of embed_fwd_kernel: out = bf16((a + b) + c) with a, b, c the word, position and type rows
    (bf16, exact in fp32): two fp32 additions, t = u (|a + b| + |a + b + c|) + 1e-30."""
    wi, pi, ti = embed_rows(ids, tt, S, ww.shape[0], wt.shape[0])
    ab = ww.double()[wi] + wp.double()[pi]
    out = ab + wt.double()[ti]
    return out, _U32 * (ab.abs() + out.abs()) + 1e-30


def embed_bwd_bound(dout, ids, tt, B, S, gw0, gp0, gt0):
    """dict(gw, t_gw, gp, t_gp, gt, t_gt; touched_w [V] bool) of embed_bwd_word_kernel / embed_bwd_pos_kernel +
    reduce_rows on top of the prefills gw0, gp0, gt0. Each output is previous + a plain fp32 sum of n bf16
    gradient rows in a fixed order, then one addition onto the previous value:
        t = (n + 1) u sum|terms| + u |previous| + 1e-30
    n = the number of tokens naming a word row (its run length); B for a position row (one row per
    sequence); B + ceil(S / 64) + 6 for a type row (the B rows of a position, then reduce_rows' lane stride
    over the S positions and its butterfly). ids are the clamped ids the backward is called with; a type
    table of one row collects every token (the forward clamps their types to row 0)."""
    d = dout.double()
    V, P, ntype, D = gw0.shape[0], gp0.shape[0], gt0.shape[0], d.shape[1]
    wi, pi, ti = embed_rows(ids, tt, S, V, ntype)

    def scatter(idx, nrows, prev, n):
        z = torch.zeros(nrows, D, dtype=torch.float64, device=d.device)
        s, a = z.clone().index_add_(0, idx, d), z.clone().index_add_(0, idx, d.abs())
        return prev.double() + s, (n + 1) * _U32 * a + _U32 * prev.double().abs() + 1e-30

    cnt = torch.zeros(V, dtype=torch.float64, device=d.device).index_add_(0, wi, torch.ones_like(wi, dtype=torch.float64))
    gw, t_gw = scatter(wi, V, gw0, cnt[:, None])
    gp, t_gp = scatter(pi, P, gp0, B)
    gt, t_gt = scatter(ti, ntype, gt0, B + _ceil_div(S, 64) + 6)
    return dict(gw=gw, t_gw=t_gw, gp=gp, t_gp=t_gp, gt=gt, t_gt=t_gt, touched_w=cnt > 0)


# Classifier head (B, h, L): L = 1 | a typical small head | h no multiple of 256 and one label in the second
# 64-label chunk | three chunks | the backward's limit of 1024 staged labels
ROWK_HEAD_CASES = [(1, 256, 1), (5, 768, 3), (3, 200, 65), (2, 1024, 130), (2, 64, 1024)]


def head_edge_inputs(B, h, L, seed):
    """dict of one head case on the CPU (all fp32): pooled in (-1, 1) as tanh gives it, wc [L, h], bc [L],
    dlogits [B, L], and the prefills dw0 [L, h], db0 [L] of the accumulating form."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(pooled=torch.tanh(1.5 * r(B, h)), wc=r(L, h) * 0.1, bc=r(L) * 0.1, dlogits=r(B, L), dw0=r(L, h), db0=r(L))


def head_fwd_bound(pooled, wc, bc=None):
    """(logits, t) of head_cls_fwd_kernel: each of 256 threads chains ceil(h / 256) fmas, wave_sum adds 6
    levels, one thread adds the 4 wave partials onto the bias: ceil(h / 256) + 10 roundings on partial sums
    bounded by sum_j |x_j w_lj| (two spare), the bias entering the last ones at its own size:
        t = (ceil(h / 256) + 12) u sum_j |x_j w_lj| + u |b_l| + 1e-30."""
    x, w = pooled.double(), wc.double()
    h = x.shape[1]
    out, mag = x @ w.T, x.abs() @ w.abs().T
    t = (_ceil_div(h, 256) + 12) * _U32 * mag + 1e-30
    if bc is not None:
        out, t = out + bc.double(), t + _U32 * bc.double().abs()
    return out, t


def head_bwd_bound(dlogits, pooled, wc, dw0=None, db0=None):
    """dict(dpre, t_dpre [B, h]; dw, t_dw [L, h]; db, t_db [L]) of head_cls_bwd_x_kernel / head_cls_bwd_w_kernel.
      dpre_j = (sum_l dl_l w_lj) (1 - y_j^2), y = pooled: L chained fmas, then y y, 1 - y y and the product:
        t_dpre = u ((L + 3) |1 - y^2| + y^2) sum_l |dl_l w_lj| + 1e-30
        (the y^2 term: y y rounds by up to u y^2 BEFORE the subtraction from 1, an absolute error in 1 - y^2
        that does not shrink with it; where the compiler contracts the two into one fma the term is unused)
      dW_c[l, j] = sum_b dl_bl x_bj, db_c[l] = sum_b dl_bl: B chained operations, two spare:
        t_dw = (B + 2) u sum_b |dl x|,  t_db = (B + 2) u sum_b |dl|  (+ 1e-30)
      accumulating onto dw0 / db0 adds u |previous| (the sum's share of that addition is in the two spare)."""
    dl, x, w = dlogits.double(), pooled.double(), wc.double()
    B, L = dl.shape
    y2 = x * x
    dpre = (dl @ w) * (1 - y2)
    t_dpre = _U32 * ((L + 3) * (1 - y2).abs() + y2) * (dl.abs() @ w.abs()) + 1e-30
    dw, t_dw = dl.T @ x, (B + 2) * _U32 * (dl.abs().T @ x.abs()) + 1e-30
    db, t_db = dl.sum(0), (B + 2) * _U32 * dl.abs().sum(0) + 1e-30
    if dw0 is not None:
        dw, t_dw = dw + dw0.double(), t_dw + _U32 * dw0.double().abs()
    if db0 is not None:
        db, t_db = db + db0.double(), t_db + _U32 * db0.double().abs()
    return dict(dpre=dpre, t_dpre=t_dpre, dw=dw, t_dw=t_dw, db=db, t_db=t_db)


def guarded_1d(n, dev, pad=64):
    """(buf, view) of an fp32 vector of n elements in the middle of a sentinel-filled allocation: `pad` floats
    (a multiple of 4, so the view keeps the bindings' 16-byte alignment) on both sides."""
    assert pad % 4 == 0
    buf = sentinel((n + 2 * pad,), torch.float32, dev)
    return buf, buf[pad:pad + n]


# ---------------------------------------------------------------------------------------------
# Derived bounds of the loss and metric kernels (losses.hip): fused softmax-cross-entropy with its
# backward, accuracy, the L1 / MSE / NLL criteria and mcrmse. tests/test_loss_bound_cpu.py checks them
# against a torch fp32 emulation of the kernels on the CPU; tests/test_losses_edges_gpu.py uses them on
# the GPU. Every reference is fp64 from the actual inputs (the bf16 points for bf16 logits, the fp32
# values for fp32), `t` is the allowance on the kernel's fp32 value before its store, u = 2^-24.
# ---------------------------------------------------------------------------------------------
# __expf(x) lowers to v_exp_f32(x * log2e). Relative error allowed: _EXP2_REL + _EXPF_ARG_REL |x|: the
# 2 ulp of v_exp_f32 that attention's bounds already use, plus the rounding of the product x * log2e and of
# the fp32 constant log2e (2 u |x| in the base-e exponent), carried through the exponential.
# __logf(s) lowers to v_log_f32(s) * ln2: absolute allowance _LOGF_ABS max(1, |log s|), the v_log_f32 term
# attn_fwd_bound uses for t_LSE. NEITHER has been measured on the device: the lse-dependent headroom that
# tests/test_losses_edges_gpu.py prints (and records in its docstring) is their record.
_EXPF_ARG_REL = 2.0 ** -23
_LOGF_ABS = 2.0 ** -21
_F32_TINY = 2.0 ** -126  # below it a result may be flushed to zero

# (B, C) of the cross-entropy edge cases: loss 0 and gradient 0 | a second block with one row and three idle
# waves | exactly one chunk | a one-lane tail chunk | the special rows, 3 chunks with a 2-lane tail | the
# special rows, 16 chunks | 65 chunks
LOSS_CE_SHAPES = [(1, 1), (5, 10), (3, 64), (3, 65), (12, 130), (12, 1000), (2, 4099)]
LOSS_CE_SMOOTHING = (0.0, 0.1)
LOSS_CE_GRAD_OUT = (1.7, -0.5)
LOSS_CE_TIE = 24.0  # planted maximum: 8 sigma of the 3 N(0, 1) logits, exact in bf16
# (B, C) = (12, 130) and (12, 1000) carry the special rows (every other row is 3 N(0, 1) with a random target):
#   0  ascending ramp z_c = 0.25 c: the running maximum rises in every chunk
#   1  the same ramp reversed: the maximum is in the first chunk, every later term is rescaled by exactly 1
#   2  -80 everywhere, +80 in column C / 2, the target one column to the right (loss 160, softmax one-hot)
#   3  two-way tie at the maximum in columns 5 and 70 (two chunks), the target the FIRST tie (a hit)
#   4  the same tie, the target the SECOND tie (a miss under the first-arg-max rule)
#   5  columns 0..63 are -inf (the whole first chunk), target 100           } label_smoothing = 0 only: with
#   6  columns 64..127 are -inf (the whole second chunk), target 3          } smoothing the loss is +inf in
#      torch too, so under label_smoothing > 0 these two rows stay ordinary random rows
#   7  the target in column C - 1
#   8  target -100 (ignored)
#   9  target C: out of range, which the kernel treats as ignored (loss 0, gradient 0, not in n_valid)
#   10 two-way tie in columns 7 and 9 (one chunk), the target the first tie: with rows 3 and 4 an odd number
#      of tie rows, so that a last-arg-max kernel changes the hit COUNT (3 -> 1 and 4 -> 0 alone would swap)
#   11 ordinary; with an in-range ignore_index its target is that index
LOSS_CE_SPECIAL = ((12, 130), (12, 1000))


def ce_edge_inputs(B, C, dtype, label_smoothing=0.0, ignore_index=-100):
    """(z [B, C] `dtype`, targets int64 [B]) of one cross-entropy case on the CPU; see LOSS_CE_SPECIAL. With an
    in-range ignore_index the last row's target is that index (B > 1)."""
    g = torch.Generator().manual_seed(1000 * B + C)
    z = 3.0 * torch.randn(B, C, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    if (B, C) in LOSS_CE_SPECIAL:
        col = torch.arange(C, dtype=torch.float32)
        z[0], z[1] = 0.25 * col, 0.25 * (C - 1 - col)
        z[2] = -80.0
        z[2, C // 2] = 80.0
        y[2] = C // 2 + 1
        for r, (i1, i2, tgt) in {3: (5, 70, 5), 4: (5, 70, 70), 10: (7, 9, 7)}.items():
            z[r, i1] = z[r, i2] = LOSS_CE_TIE
            y[r] = tgt
        if label_smoothing == 0.0:
            z[5, :64] = float("-inf")
            z[6, 64:128] = float("-inf")
        y[5], y[6], y[7], y[8], y[9] = 100, 3, C - 1, -100, C
    if ignore_index >= 0 and B > 1:
        y[B - 1] = ignore_index
    return z.to(dtype), y


def _first_argmax(z):
    """Smallest index holding the row maximum, by the explicit rule (no library arg-max)."""
    C = z.shape[1]
    idx = torch.arange(C).expand_as(z)
    return torch.where(z == z.max(1, keepdim=True).values, idx, torch.full_like(idx, C)).min(1).values


def ce_bound(z, targets, ignore_index=-100, label_smoothing=0.0, grad_out=1.0):
    """(expected, t): dicts with loss (scalar), dl [B, C] (the unscaled gradient ce_fwd writes), grad [B, C] (what
    ce_bwd stores); expected also holds ok [B] (rows that count) and n_valid. Kernels: ce_fwd_kernel (one wave per
    row, n = ceil(C / 64) chunks), ce_finalize_kernel, ce_bwd_kernel.

    Reference, per row, ls = label_smoothing as fp32 holds it: lse = log sum_c exp z_c,
    loss_i = (1 - ls)(lse - z_t) + ls (lse - mean z) (the ls term absent at ls = 0, so that -inf logits keep a
    finite loss as in torch), g = softmax - (1 - ls) onehot - ls / C, exactly 0 on rows that do not count
    (target == ignore_index or outside [0, C)). Batch: n_valid, loss = sum_i loss_i / max(n_valid, 1),
    grad = g grad_out / max(n_valid, 1), grad_out as fp32 holds it.

    The sum s = sum_c exp(z_c - m). The kernel adds exp(v - nm_k) in chunk k and multiplies the running s by
    exp(m_k - nm_k) in every later chunk; the exponents of one term's factors are all <= 0 and add up to
    x_c = z_c - m. Relative error of s, the terms being positive (p_c = softmax):
        rel_s = (n + 8) u ............................ per chunk step one rescale multiply and one add, the 6
                                                       butterfly levels, two spare
              + (rises + 1) _EXP2_REL ................. one v_exp_f32 per factor; where the maximum does not rise
                                                       the factor is __expf(0) = 1 exactly (rises = the chunks
                                                       after the first whose maximum exceeds the running one)
              + 3 u sum_c p_c |x_c| ................... _EXPF_ARG_REL |x| and the rounding of every subtraction
                                                       (u |x|), summed along a term's factors
              + C 2^-126 .............................. terms flushed to zero (s >= 1)
        t_lse = rel_s + _LOGF_ABS max(1, |log s|) + u |lse| ... log's slope 1 / s, __logf, the add m + log s
    zsum: a lane chains n additions, the butterfly adds 6 levels: t_zsum = (n + 6) u sum |z|. z_t is exact.
        t_loss_i = (1 - ls)(t_lse + u |lse - z_t|) + ls (t_lse + (t_zsum + u |zsum|) / C + u |lse - mean z|)
                   + 2 u (|(1 - ls)(lse - z_t)| + |ls (lse - mean z)|) + u |loss_i|
                   (each difference, 1 - ls, zsum / C, the two products, the final add)
        t_loss = (sum_i t_loss_i + (ceil(B / 4) + 4) u sum_i |loss_i|) / n_valid + u |loss| ... the 4 rows of a
                   block in fixed order, then one atomic per block in no fixed order; the count is exact; the divide
    Gradient: p = __expf(v - lse) at the row's own lse error:
        rel_p = t_lse + _EXP2_REL + 3 u |z_c - lse|
        t_dl = p rel_p + u ((1 - ls) on + ls / C + |p - (1 - ls) on| + |g|) + 1e-30 ... 1 - ls, ls / C, the two
                   subtractions; 1e-30 takes the values below the normal range
        t_grad = t_dl |sc| + 2 u |grad| + 1e-30, sc = grad_out / n_valid ... the divide and the multiply
    A -inf logit has p = 0 and g = -ls / C exactly; its terms enter no sum above."""
    z = z.double()
    B, C = z.shape
    n = _ceil_div(C, 64)
    ls = float(torch.tensor(float(label_smoothing), dtype=torch.float32))
    go = float(torch.tensor(float(grad_out), dtype=torch.float32))
    tg = targets.to(torch.int64)
    ok = (tg != ignore_index) & (tg >= 0) & (tg < C)
    fin = torch.isfinite(z)
    m = z.max(1).values
    x = z - m[:, None]
    e = torch.exp(x)
    s = e.sum(1)
    lse = m + torch.log(s)
    a = z - lse[:, None]
    p = torch.exp(a)
    zero = torch.zeros_like(z)
    zp = torch.full((B, n * 64), float("-inf"), dtype=torch.float64)
    zp[:, :C] = z
    cm = zp.view(B, n, 64).max(2).values
    rises = (cm[:, 1:] > torch.cummax(cm, 1).values[:, :-1]).sum(1).double()
    rel_s = ((n + 8) * _U32 + (rises + 1) * _EXP2_REL + 3 * _U32 * torch.where(fin, e * x.abs(), zero).sum(1) / s
             + C * _F32_TINY)
    t_lse = rel_s + _LOGF_ABS * torch.log(s).abs().clamp_min(1.0) + _U32 * lse.abs()

    on = torch.zeros_like(z)
    on[ok, tg[ok]] = 1.0
    gfull = p - (1 - ls) * on - ls / C
    rel_p = t_lse[:, None] + _EXP2_REL + 3 * _U32 * torch.where(fin, a.abs(), zero)
    t_dl = p * rel_p + _U32 * ((1 - ls) * on + ls / C + (p - (1 - ls) * on).abs() + gfull.abs()) + 1e-30
    okc = ok[:, None]
    dl = torch.where(okc, gfull, zero)
    t_dl = torch.where(okc, t_dl, torch.full_like(z, 1e-30))
    n_valid = int(ok.sum())
    den = max(n_valid, 1)
    sc = go / den
    grad = dl * sc
    t_grad = t_dl * abs(sc) + 2 * _U32 * grad.abs() + 1e-30

    zt = z[torch.arange(B), tg.clamp(0, C - 1)]
    hard = (1 - ls) * (lse - zt)
    t_li = (1 - ls) * (t_lse + _U32 * (lse - zt).abs()) + 2 * _U32 * hard.abs()
    li = hard
    if ls != 0.0:
        zsum = z.sum(1)
        t_zsum = (n + 6) * _U32 * z.abs().sum(1)
        soft = ls * (lse - zsum / C)
        t_li = t_li + ls * (t_lse + (t_zsum + _U32 * zsum.abs()) / C + _U32 * (lse - zsum / C).abs()) + 2 * _U32 * soft.abs()
        li = li + soft
    t_li = t_li + _U32 * li.abs()
    li, t_li = li[ok], t_li[ok]
    loss = li.sum() / den
    t_loss = (t_li.sum() + (_ceil_div(B, 4) + 4) * _U32 * li.abs().sum()) / den + _U32 * loss.abs() + 1e-30
    return (dict(loss=loss, dl=dl, grad=grad, ok=ok, n_valid=n_valid, lse=lse),
            dict(loss=t_loss, dl=t_dl, grad=t_grad, lse=t_lse))


LOSS_ACC_B = (1, 5, 1000)
LOSS_ACC_C = (1, 10, 65, 130)


def accuracy_edge_inputs(B, C, dtype):
    """(z [B, C] `dtype`, targets int64 [B]) on the CPU: 3 N(0, 1) logits (in bf16, ties at the maximum occur by
    themselves in wide rows), random targets, and by the row index i (C >= 2):
      i % 16 in (0, 8)  a planted two-way tie at the maximum (columns C / 3 and C - 1), the target the first tie: a hit
      i % 16 == 4       the same tie, the target the second tie: a miss
      i % 16 == 12      the same tie, the target neither (column 1 of C >= 4, else -100): a miss
      i % 16 == 6       target -100: a miss that still counts in the denominator B
    First ties outnumber second ties at B = 1 and B = 1000 (at B = 5 they are one each: a last-arg-max kernel
    is invisible there)."""
    g = torch.Generator().manual_seed(77 * B + C)
    z = 3.0 * torch.randn(B, C, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    i = torch.arange(B)
    if C >= 2:
        i1, i2 = C // 3, C - 1
        tie = (i % 4 == 0)
        z[tie, i1] = LOSS_CE_TIE
        z[tie, i2] = LOSS_CE_TIE
        y[i % 8 == 0] = i1
        y[i % 16 == 4] = i2
        y[i % 16 == 12] = 1 if C >= 4 else -100
    y[i % 16 == 6] = -100
    return z.to(dtype), y


def accuracy_expected(z, targets):
    """(hits / B, t) of accuracy_kernel and of ce_fwd's fused `correct` output: a hit is a row whose FIRST index
    holding the row maximum equals its target (explicit rule, computed where it is called: on the CPU). Every
    block adds (its 0..4 hits) / B atomically: one rounded divide per block and ceil(B / 4) additions of a sum
    that stays <= 1, hence t = (ceil(B / 4) + 2) u."""
    B = z.shape[0]
    hits = int((_first_argmax(z.double()) == targets.to(torch.int64)).sum())
    return hits / B, (_ceil_div(B, 4) + 2) * _U32


LOSS_REG_THREADS, LOSS_REG_MAX_BLOCKS = 256, 1024
# (a block takes 1024 elements) one element | one block, a wave with an idle lane | one block, one thread on a
# second trip | two blocks | 293 blocks: a second trip in the finalize block | the first n at which the block cap
# holds (1024 blocks) and threads walk a second grid stride
LOSS_POINTWISE_N = (1, 255, 257, 1025, 300001, 2 ** 20 + 5)
LOSS_NLL_CASES = [(1, 1), (5, 3), (513, 7), (2 ** 20 + 5, 2)]
LOSS_NLL_IGNORE = (-100, 1)
# (3, 300): C above the finalize block's 256 threads; (257, 6): a second trip for one thread of every column
LOSS_MCRMSE_CASES = [(1, 1), (3, 300), (257, 6), (5000, 2)]


def reg_blocks(n):
    """reg_blocks of losses.hip: one block per 1024 elements, at least 1, at most 1024."""
    return min(max(_ceil_div(n, 4 * LOSS_REG_THREADS), 1), LOSS_REG_MAX_BLOCKS)


def reg_geometry(n):
    """(nb, depth) of the two-pass regression reductions over n terms: nb blocks; depth = the additions behind
    the result: a thread's ceil(n / (256 nb)) chained terms, the 6-level butterfly, the 4-wave fixed-order sum,
    then in the finalize block ceil(nb / 256) chained partials, butterfly and 4-wave sum again."""
    nb = reg_blocks(n)
    return nb, _ceil_div(n, LOSS_REG_THREADS * nb) + 6 + 4 + _ceil_div(nb, LOSS_REG_THREADS) + 6 + 4


def pointwise_edge_inputs(n, dtype=torch.float32):
    """(p `dtype`, t fp32) [n] on the CPU: N(0, 1); for n > 1 element 0 has p == t (sign(0) = 0, an exact zero term)."""
    g = torch.Generator().manual_seed(n)
    p, t = torch.randn(n, generator=g).to(dtype), torch.randn(n, generator=g)
    if n > 1:
        t[0] = p[0].float()
    return p, t


def pointwise_loss_bound(p, t, mode, grad_out=1.0):
    """(expected, t) dicts with loss, g (the unscaled gradient the forward writes) and grad (the prediction's
    gradient; the target's is its exact negation) of pointwise_loss_partial_kernel + loss_finalize_kernel +
    loss_scale_grad_kernel. mode 0: mean |d|, g = sign(d) with sign(0) = 0; mode 1: mean d^2, g = 2 d; d = p - t.
      t_loss = (depth + k) u sum(term) / n + u |loss| + 1e-30: depth = reg_geometry(n) additions of positive
               terms; k = 1 for L1 (the rounding of d), 3 for MSE (d enters twice, the product); the divide by n
      g: L1 exact (the rounded difference of two different floats keeps its sign); MSE u |2 d| (d's rounding)
      grad = g grad_out / n: the divide, the multiply (and d's rounding for MSE): (2 | 3) u |grad| + 1e-30."""
    d = p.double().reshape(-1) - t.double().reshape(-1)
    n = d.numel()
    go = float(torch.tensor(float(grad_out), dtype=torch.float32))
    term, g, k = (d.abs(), torch.sign(d), 1) if mode == 0 else (d * d, 2 * d, 3)
    _, depth = reg_geometry(n)
    loss = term.sum() / n
    grad = g * go / n
    return (dict(loss=loss, g=g, grad=grad),
            dict(loss=(depth + k) * _U32 * term.sum() / n + _U32 * loss.abs() + 1e-30,
                 g=(0.0 if mode == 0 else _U32) * g.abs() + 1e-30, grad=(2 if mode == 0 else 3) * _U32 * grad.abs() + 1e-30))


def nll_edge_inputs(B, C, ignore_index):
    """(logp fp32 [B, C], targets int64 [B]) on the CPU. From 5 rows on: row 1 has the out-of-range target C,
    row 2 the target -100, row 3 the target min(1, C - 1) (the in-range ignore_index of LOSS_NLL_IGNORE),
    row 4 the target C - 1."""
    g = torch.Generator().manual_seed(31 * B + C + (ignore_index & 0xFF))
    logp = torch.log_softmax(2.0 * torch.randn(B, C, generator=g), 1)
    y = torch.randint(0, C, (B,), generator=g)
    if B >= 5:
        y[1], y[2], y[3], y[4] = C, -100, min(1, C - 1), C - 1
    return logp, y


def nll_bound(logp, targets, ignore_index=-100):
    """(expected, t): expected = dict(loss, ok [B], n_valid), t the allowance of the loss, for nll_partial_kernel +
    loss_finalize_kernel: loss = sum over the rows that count of -logp[i, t_i] / max(n_valid, 1); a row counts when
    its target is not ignore_index and inside [0, C); no row counting gives 0. The terms are exact, the count is a
    sum of ones (exact): t = depth u sum |terms| / n_valid + u |loss| + 1e-30 with depth = reg_geometry(B).
    The gradient needs no allowance: exactly fp32(-grad_out / n_valid) at the target of a counting row, 0 elsewhere
    (nll_grad_expected)."""
    lp = logp.double()
    B, C = lp.shape
    tg = targets.to(torch.int64)
    ok = (tg != ignore_index) & (tg >= 0) & (tg < C)
    terms = -lp[torch.arange(B), tg.clamp(0, C - 1)][ok]
    den = max(int(ok.sum()), 1)
    loss = terms.sum() / den
    _, depth = reg_geometry(B)
    return dict(loss=loss, ok=ok, n_valid=int(ok.sum())), depth * _U32 * terms.abs().sum() / den + _U32 * loss.abs() + 1e-30


def nll_grad_expected(targets, C, ignore_index, grad_out):
    """fp32 [B, C]: fp32(-grad_out) / fp32(max(n_valid, 1)), one correctly rounded divide, at the targets of the
    rows that count; 0 elsewhere."""
    tg = targets.to(torch.int64)
    ok = (tg != ignore_index) & (tg >= 0) & (tg < C)
    v = -torch.tensor(float(grad_out), dtype=torch.float32) / torch.tensor(float(max(int(ok.sum()), 1)), dtype=torch.float32)
    out = torch.zeros(tg.numel(), C, dtype=torch.float32)
    out[ok, tg[ok]] = v
    return out


def mcrmse_edge_inputs(B, C, zero_col=False):
    """(p, t) fp32 [B, C] on the CPU; the columns' errors differ in scale (column c: (1 + c % 5) N(0, 1)), so that
    the mean of the roots is not the root of the mean; zero_col: column 0 of p equals t's (an exact zero)."""
    g = torch.Generator().manual_seed(5 * B + C)
    t = torch.randn(B, C, generator=g)
    p = t + torch.randn(B, C, generator=g) * (1.0 + (torch.arange(C) % 5).float())
    if zero_col:
        p[:, 0] = t[:, 0]
    return p, t


def mcrmse_bound(p, t):
    """(expected, t) dicts with col [C] (colwise_mse_kernel's column means) and out (mcrmse_finalize_kernel).
      col_c = sum_r d^2 / B, d = t - p: thread chains ceil(B / 256) terms, butterfly 6, 4-wave sum 4; d's rounding
              twice and the product (3), the divide (1): rel_col = (ceil(B / 256) + 14) u
      rmse_c = sqrt(col_c): half of rel_col, and u for sqrtf (correctly rounded under the build's flags: no
              fast-math, so half an ulp): t_rmse = rmse (rel_col / 2 + u); sqrt(0) = 0 exactly
      out = sum_c rmse_c / C: ceil(C / 256) + 10 additions of positive terms, the divide:
              t = (sum t_rmse + (ceil(C / 256) + 10) u sum rmse) / C + u |out| + 1e-30."""
    d = t.double() - p.double()
    B, C = d.shape
    col = (d * d).mean(0)
    rel_col = (_ceil_div(B, LOSS_REG_THREADS) + 14) * _U32
    rmse = torch.sqrt(col)
    t_rmse = rmse * (rel_col / 2 + _U32)
    out = rmse.mean()
    t_out = (t_rmse.sum() + (_ceil_div(C, LOSS_REG_THREADS) + 10) * _U32 * rmse.sum()) / C + _U32 * out.abs() + 1e-30
    return dict(col=col, out=out), dict(col=col * rel_col + 1e-30, out=t_out)
