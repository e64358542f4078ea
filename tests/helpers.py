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
