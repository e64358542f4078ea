"""Inputs and derived bounds of the RMSNorm kernels (rms_fwd, dropout_add_rms_fwd, rms_bwd of layernorm.hip), in
the style of the LayerNorm bounds of tests/helpers.py. tests/test_rmsnorm_bound_cpu.py checks them against a torch
fp32 emulation of the kernels on the CPU, tests/test_rmsnorm_gpu.py uses them on the GPU.

References are fp64 from the bf16 / fp32 inputs, `t` is the allowance on the kernel's fp32 value before its store
(bf16 outputs then go through helpers.store_bound), u = 2^-24, E = D / 64 values per lane, `eps` as the kernel
holds it (rounded to fp32). The walk of the backward (rows per wave, 4-wave LDS sum, reduce_rows) is ln_bwd_kernel's,
so helpers.ln_partial_blocks / ln_bwd_depth / colsum_stored_bound / acc_bound apply unchanged."""
import torch

from tests import helpers as H

_U = 2.0 ** -24


def rms_edge_inputs(rows, D, seed):
    """helpers.ln_edge_inputs (x, dy, dres bf16; gamma fp32; its beta is dropped) plus the rows RMSNorm has to be
    told apart on: rows >= 5: row 3 all zeros (only eps stands under the root); rows >= 2053: row 7 = 1e4 N(0, 1)
    and row 8 = 1e-6 N(0, 1) (x^2 << eps). The 64 + N and 1000 + N rows of ln_edge_inputs are the ones a centring
    kernel gets wrong."""
    x, dy, dres, gamma, _ = H.ln_edge_inputs(rows, D, seed)
    g = torch.Generator().manual_seed(seed + 1)
    x = x.clone()
    if rows >= 5:
        x[3] = 0
    if rows >= 2053:
        x[7] = (1e4 * torch.randn(D, generator=g)).to(torch.bfloat16)
        x[8] = (1e-6 * torch.randn(D, generator=g)).to(torch.bfloat16)
    return x, dy, dres, gamma


def rel_rs(D):
    """The relative error of rstd: 0.5 (E + 10) u + 2^-22. (E + 10) u covers the squares (u each), E + 5
    additions of positive terms (E - 1 in the lane, 6 in the butterfly), the 1 / D constant and the multiply by it,
    and the + eps, all relative to a sum of positive terms; halved by the root; then rsqrtf (helpers._RSQRT_REL)."""
    return 0.5 * (D // 64 + 10) * _U + H._RSQRT_REL


def rms_fwd_bound(x, gamma, eps):
    """(rstd, t_rstd [rows]; Y, t_Y [rows, D]) of rms_fwd_kernel: rstd = 1 / sqrt(mean(x^2) + eps), Y = x rstd gamma.
      t_rstd = rstd rel_rs
      t_Y = |Y| (rel_rs + 3u) + 1e-30 ... rstd's error and the two roundings of the products, one spare.
    A zero row has Y = 0 exactly (t_Y = 1e-30)."""
    x, g = x.double(), gamma.double()
    eps = float(torch.tensor(eps, dtype=torch.float32))
    rs = 1.0 / torch.sqrt((x * x).mean(1) + eps)
    rel = rel_rs(x.shape[1])
    Y = x * rs[:, None] * g
    return rs, rs * rel, Y, Y.abs() * (rel + 3 * _U) + 1e-30


def rms_bwd_bound(dy, x, gamma, rstd, dres=None, depth=None):
    """dict(dx, t_dx [rows, D]; dgamma, t_dgamma [D]) of rms_bwd_kernel + reduce_rows. `rstd` is the forward
    kernel's OWN saved fp32 value. xh = x rstd, t = dy gamma, s2 = mean(t xh), dx = rstd (t - xh s2) + dres;
    dgamma = sum_rows dy xh.
      t_s2 = (E + 11) u mean|t xh| ... the roundings of xh and t, E + 5 additions, 1 / D rounded, one multiply
                 (the products t xh enter through an fma: exact), two spare
      t_dx[i] = rstd (|xh_i| t_s2 + 5u (|t_i| + |xh_i s2|)) + u |dx_i| + 1e-30 ... s2's error as it enters, up to 5
                 roundings on the two terms of the bracket (t, xh, the fma, the multiply by rstd, one spare), the
                 final + dres (or the multiply) at the size of dx
      t_dgamma = (depth + 2) u sum_rows |dy xh| + 1e-30 ... depth = helpers.ln_bwd_depth(rows); the 2: the rounding
                 of xh and one spare (the products dy xh enter through an fma)."""
    dy, x, g = dy.double(), x.double(), gamma.double()
    rstd = rstd.double()[:, None]
    rows, D = x.shape
    E = D // 64
    depth = H.ln_bwd_depth(rows) if depth is None else depth
    xh = x * rstd
    t = dy * g
    s2 = (t * xh).mean(1, keepdim=True)
    dx = rstd * (t - xh * s2)
    if dres is not None:
        dx = dx + dres.double()
    t_s2 = (E + 11) * _U * (t * xh).abs().mean(1, keepdim=True)
    t_dx = rstd * (xh.abs() * t_s2 + 5 * _U * (t.abs() + (xh * s2).abs())) + _U * dx.abs() + 1e-30
    return dict(dx=dx, t_dx=t_dx, dgamma=(dy * xh).sum(0), t_dgamma=(depth + 2) * _U * (dy * xh).abs().sum(0) + 1e-30)
