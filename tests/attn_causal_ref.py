"""Shared pieces of the causal attention tests (tests/test_attn_causal_cpu.py, tests/test_attention_causal_gpu.py):
the visibility mask, the derived bounds of tests/helpers.py restated for an arbitrary boolean mask, the edge
inputs with sentinel keys on the diagonal, and a CPU emulation of the causal kernels.

One definition of `causal`: key j of a sequence is visible to query i of the same sequence iff j <= i and
j < len_b. Query rows at pad positions (i >= len_b) therefore see the len_b valid keys, as without `causal`.

attn_fwd_bound_masked / attn_bwd_bound_masked are helpers.attn_fwd_bound / attn_bwd_bound line for line, with
`valid` [B, 1, S, S] (or anything that broadcasts to [B, H, S, S]) in the place of the key-padding mask: the same
eps, u = 2^-8, and (S + 4) 2^-24 accumulation terms with the launch's S. The kernels accumulate over fewer keys /
queries under `causal`, so the launch-wide S is an upper bound of the accumulation length there.
test_attn_causal_cpu.py shows that with the plain key-padding mask they return tensors torch.equal to the
helpers'."""
import torch

from tests.helpers import _LN2, _U32, _UB, _attn_eta, attn_edge_inputs, attn_heads, attn_sl2, attn_split

BF16 = torch.bfloat16
_LOG2E = 1.4426950408889634
# rows i whose key i + 1 is a sentinel (see causal_edge_inputs): the 16-, 64- and 128-row boundaries
SENTINEL_ROWS = (15, 63, 127)


def _lens_tensor(lens, B, S):
    return torch.full((B,), S, dtype=torch.int64) if lens is None else torch.as_tensor(list(lens), dtype=torch.int64)


def key_valid(lens, B, S):
    """The plain key-padding mask as [B, 1, S, S]."""
    n = _lens_tensor(lens, B, S)
    return (torch.arange(S)[None, :] < n[:, None])[:, None, None, :].expand(B, 1, S, S)


def causal_valid(lens, B, S, mut=None):
    """[B, 1, S, S] bool: key j visible to query i iff j <= i and j < len_b. Mutations (plausible kernel
    defects): causal_plus_1 makes key i + 1 visible too; causal_minus_1 hides key i for i >= 1."""
    n = _lens_tensor(lens, B, S)
    i = torch.arange(S)[:, None]
    j = torch.arange(S)[None, :]
    if mut == "causal_plus_1":
        tri = j <= i + 1
    elif mut == "causal_minus_1":
        tri = j <= (i - 1).clamp_min(0)
    else:
        assert mut is None, mut
        tri = j <= i
    return ((j[None] < n[:, None, None]) & tri[None])[:, None]


def attn_fwd_bound_masked(q, k, v, valid, scale, keep=None, c=1.0):
    """helpers.attn_fwd_bound with `valid` [B, 1, S, S] instead of lens: (O, t_O, LSE2, t_LSE)."""
    B, H, S, _ = q.shape
    sl2 = attn_sl2(scale)
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


def attn_bwd_bound_masked(q, k, v, do, o, lse, valid, scale, keep=None, c=1.0):
    """helpers.attn_bwd_bound with `valid` [B, 1, S, S] instead of lens: the same dict."""
    B, H, S, _ = q.shape
    sl2 = attn_sl2(scale)
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


def causal_edge_inputs(B, S, H, lens, scale, seed):
    """helpers.attn_edge_inputs plus sentinel keys on the diagonal: for i in SENTINEL_ROWS with i + 1 < len_b,
    query i + 1 is a copy of query i and key i + 1 a multiple of it whose base-2 score leads by about 40. Row
    i + 1 is then carried by its own diagonal key (hiding it is an error of order |v|) and row i must not see
    that key (a leak would carry row i): an off-by-one of the diagonal shows at rows 15 | 16, 63 | 64 and
    127 | 128, the last / first rows of a wave, of a 64-row group and of a 128-row block."""
    qkv, dout = attn_edge_inputs(B, S, H, lens, scale, seed)
    x = qkv.float().view(B, S, 3, H, 64)
    n = _lens_tensor(lens, B, S)
    for b in range(B):
        for h in range(H):
            for i in SENTINEL_ROWS:
                if i + 1 < int(n[b]):
                    qv = x[b, i, 0, h].to(BF16).double()
                    x[b, i + 1, 0, h] = qv.float()
                    x[b, i + 1, 1, h] = (qv * (40.0 / (qv.pow(2).sum().item() * scale * _LOG2E))).float()
    return x.view(B * S, 3 * H * 64).to(BF16), dout


def _r(x):  # the bf16 rounding of an fp32 tensor, back in fp32
    return x.to(BF16).float()


def emulate_masked(qkv, dout, B, S, H, valid, scale, keep=None, c=1.0, off=None):
    """tests/test_attn_bound_cpu.py: emulate (the fp32 emulation of attn_fwd + attn_bwd at the kernels' rounding
    points) with a boolean mask `valid` [B, 1, S, S] in the place of the length mask. Masked probabilities are
    exact zeros (exp2(-inf)), in the forward and in the backward."""
    q, k, v = (x.float() for x in attn_split(qkv, B, S, H))
    do = attn_heads(dout, B, S, H).float()
    sc = torch.tensor(scale, dtype=torch.float32)
    sl2 = sc * torch.tensor(1.4426950408889634, dtype=torch.float32)
    c = torch.tensor(c, dtype=torch.float32)
    kp = torch.ones(B, H, S, S) if keep is None else keep.float()
    s = q @ k.transpose(-1, -2)
    sm = s.masked_fill(~valid, float("-inf"))
    m = sm.max(-1, keepdim=True).values * sl2
    if off is not None:
        m = m - off
    p = torch.exp2(sm * sl2 - m)
    pb = _r(p)
    l = pb.sum(-1)
    pv = _r(pb * kp)
    o = (pv @ v) * ((1.0 / l) * (c if keep is not None else 1.0))[..., None]
    lse = m[..., 0] + torch.log2(l)
    o_b = o.to(BF16)
    delta = (do * o_b.float()).sum(-1)
    pr = torch.where(valid, torch.exp2(s * sl2 - lse[..., None]), torch.zeros(()))
    dp = do @ v.transpose(-1, -2)
    ds = pr * ((dp - delta[..., None]) if keep is None else (kp * c * dp - delta[..., None]))
    pm, dsb = _r(pr * kp), _r(ds)
    dv = pm.transpose(-1, -2) @ do
    if keep is not None:
        dv = dv * c
    dk = (dsb.transpose(-1, -2) @ q) * sc
    dq = (dsb @ k) * sc
    return dict(o=o, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv, o_b=o_b, dq_b=dq.to(BF16), dk_b=dk.to(BF16),
                dv_b=dv.to(BF16))
