"""Shared pieces of the decode attention tests (tests/test_attn_decode_cpu.py, tests/test_attn_decode_gpu.py):
the fp64 reference with its derived allowance, the edge cases with sentinel keys, and a torch fp32 emulation of
attn_decode.hip in the kernel's own order (key split and merge included).

The kernel's key split (attn_decode.hip): a lane group of 8 lanes owns one key, a wave loads 4 x 8 = 32 keys per
step, the workgroup's 4 waves 128 keys per step: cached key j belongs to wave (j % 128) // 32, load (j % 32) // 8,
lane group j % 8. Each of the 32 (wave, group) pairs keeps its own online-softmax state; the new token starts the
state of wave 0 / group 0. Boundaries: 8 (group), 32 (wave), 128 (workgroup step)."""
import torch

from tests.helpers import _EXP2_REL, _LN2, _U32, _UB, _attn_eta, attn_sl2

BF16 = torch.bfloat16
_LOG2E = 1.4426950408889634
GROUPS, UNROLL, WAVES = 8, 4, 4
WAVE_KEYS = GROUPS * UNROLL      # 32
BLOCK_KEYS = WAVES * WAVE_KEYS   # 128

# (B, H, Smax, pos list, scale). pos[b] = number of cached keys = the row the new token takes.
DECODE_EDGE_CASES = [
    (2, 1, 1, [0, 0], 0.125),                  # a one-row cache
    (4, 4, 128, [0, 1, 63, 64], 0.125),        # a single key; the 64-key boundary
    (3, 2, 130, [65, 127, 129], 0.2),          # a 1-key tail; a scale that is no power of two; the last cache row
    (4, 12, 512, [0, 5, 256, 511], 0.125),     # BERT-base heads, ragged, a full cache
    (3, 1, 16, [7, 8, 9], 0.125),              # the lane-group boundary: 8 cached keys fill one load
    (3, 2, 40, [31, 32, 33], 0.125),           # the wave chunk: 32 cached keys
    (3, 1, 136, [127, 128, 129], 0.125),       # the workgroup step: 128 cached keys, then a second step
]


def decode_bound_terms(q, k, v, pos, scale):
    """(O, t_core, t_merge), all [B, H, 64] fp64. q [B, H, 64]; k, v [B, H, Smax, 64] are the keys / values the
    query sees: cache rows j < pos[b] and the new token at row pos[b] (rows above are ignored); pos a list.

    Reference: sl2 = fp32(scale log2 e); s2_j = (q . k_j) sl2 for j <= pos, p^ = softmax_j (base 2), O = sum p^_j v_j.

    Rounding points of attn_decode.hip, n = pos cached keys, I = ceil(n / 128) steps of the key loop:
      * s_j: an 8-term fp32 fma chain per lane and a 3-step butterfly (11 <= 64 additions of exact bf16 x bf16
        products), p_j = v_exp_f32(fma(s_j, sl2, -m)): helpers._attn_eta as it stands.
      * P STAYS fp32: it is multiplied with v in fp32 fmas and never packed to bf16, so the forward's u = 2^-8
        term does not appear.
      * the same fp32 p_j enters l and O, so their errors are tied as in the forward:
        O' - O = sum_j p^_j e_j (v_j - O) / (1 + sum_j p^_j e_j), with 1 - 2u a lower bound of the denominator
        (it holds while every e_j <= 2^-7, i.e. |s2| < 2^13).
      t_core = sum_j p^_j eta_j |v_jd - O_d| / (1 - 2u)       the tied exponent errors
             + c1 2^-24 sum_j p^_j |v_jd|                      the fma chain of one state: c1 = ceil(n / 8) + 1 keys
                                                               at most (invalid slots add fma(0, 0, O) = O, exact)
             + 2^-22 |O_d|                                     1 / l and the multiply by it
      which is helpers.attn_fwd_bound's t_O for this row with u dropped and the keys actually summed for S.
      t_merge, what the split adds (the forward has no counterpart):
      * every rescale multiplies l and O of a state by alpha = v_exp_f32(fl(m_old - m_new)), once per step and
        once in the merge (I + 1 times). fl(a - b) errs by 2^-24 |a - b| <= 2^-23 max_j |s2_j|, exp2 carries it
        with ln 2 and adds its own 2^-22. The factor is common to l and O of the state, so it acts as one more
        tied relative error e_m = (I + 1)(ln2 2^-23 max|s2| + 2^-22) of each p_j:
             sum_j p^_j e_m |v_jd - O_d| / (1 - 2u)
      * the roundings of those multiplies and of the merge additions on the O side, I + 1 multiplies + 3 butterfly
        steps + 3 wave additions = I + 7 operations:      (I + 7) 2^-24 sum_j p^_j |v_jd|
      * l is an fp32 sum of its own (c1 additions in a state, the same I + 7 merge operations); its terms are
        positive, so its relative error (c1 + I + 7) 2^-24 moves O by     (c1 + I + 7) 2^-24 |O_d|."""
    B, H, Smax, _ = k.shape
    sl2 = attn_sl2(scale)
    n = torch.as_tensor(list(pos), dtype=torch.int64)
    valid = (torch.arange(Smax)[None, :] <= n[:, None])[:, None, :]  # [B, 1, Smax]
    k = torch.where(valid[..., None], k, torch.zeros_like(k))
    v = torch.where(valid[..., None], v, torch.zeros_like(v))
    s2 = (k @ q[..., None])[..., 0] * sl2
    s2m = s2.masked_fill(~valid, float("-inf"))
    lse2 = torch.logsumexp(s2m * _LN2, -1) / _LN2
    ph = torch.exp2(s2m - lse2[..., None])  # [B, H, Smax]
    eta = _attn_eta(q[:, :, None, :], k, s2[:, :, None, :], sl2)[:, :, 0, :]
    O = (ph[:, :, None, :] @ v)[:, :, 0, :]
    pv = (ph[:, :, None, :] @ v.abs())[:, :, 0, :]
    dev = (v - O[:, :, None, :]).abs()  # [B, H, Smax, 64]
    steps = ((n + BLOCK_KEYS - 1) // BLOCK_KEYS).double()[:, None, None]
    c1 = ((n + GROUPS - 1) // GROUPS + 1).double()[:, None, None]
    nm = steps + 7
    s2max = s2m.masked_fill(~valid, 0.0).abs().amax(-1)[..., None]  # [B, H, 1]
    e_m = (steps + 1) * (_LN2 * 2.0 ** -23 * s2max + _EXP2_REL)
    tied = ((ph * eta)[..., None] * dev).sum(2) / (1 - 2 * _UB)
    t_core = tied + c1 * _U32 * pv + 2.0 ** -22 * O.abs() + 1e-30
    t_merge = e_m * (ph[..., None] * dev).sum(2) / (1 - 2 * _UB) + nm * _U32 * pv + (c1 + nm) * _U32 * O.abs()
    return O, t_core, t_merge


def decode_bound(q, k, v, pos, scale):
    """(O, t_O): the fp64 reference [B, H, 64] and the allowance on the kernel's fp32 value before its bf16 store
    (which then goes through helpers.store_bound). t_O = t_core + t_merge of decode_bound_terms."""
    O, t_core, t_merge = decode_bound_terms(q, k, v, pos, scale)
    return O, t_core + t_merge


def decode_split(qkv_new, B, H):
    """qkv_new [B, 3 * H * 64] -> q, k, v [B, H, 64] in fp64."""
    q, k, v = qkv_new.double().view(B, 3, H, 64).unbind(1)
    return q, k, v


def decode_effective(qkv_new, kv, pos):
    """q [B, H, 64] and the keys / values the query must see, [B, H, Smax, 64] fp64: the cache with the new token
    at row pos[b]. Rows above pos[b] keep the cache's (stale) content; decode_bound ignores them."""
    _, B, H, Smax, _ = kv.shape
    q, kn, vn = decode_split(qkv_new, B, H)
    k, v = kv[0].double().clone(), kv[1].double().clone()
    for b in range(B):
        k[b, :, pos[b]] = kn[b]
        v[b, :, pos[b]] = vn[b]
    return q, k, v


def decode_edge_inputs(case, seed):
    """(qkv_new [B, 3 * H * 64], kv [2, B, H, Smax, 64], pos int32 [B]) of one edge case, bf16 on the CPU; kv is
    the cache BEFORE the call. Random data, and for every (b, h) with b + h even three sentinels:
      * the new token's key is a multiple of q whose base-2 score leads by about 40: it carries the row, t_O is at
        fp32 level there and losing it is an error of order |v|;
      * cache row pos + 1 (stale, where it exists) is the same multiple: if it leaked it would carry the row;
      * cache row pos holds, before the call, the NEGATIVE of that multiple (and an unrelated value row): a kernel
        that reads the cache instead of the new token loses the lead.
    The other (b, h) are plain random rows, where the output is a genuine average over all the keys."""
    B, H, Smax, pos, scale = case
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B, 3, H, 64, generator=g) * 0.5).to(BF16).float()
    kv = (torch.randn(2, B, H, Smax, 64, generator=g) * 0.5)
    for b in range(B):
        for h in range(H):
            if (b + h) % 2:
                continue
            qv = qkv[b, 0, h].double()
            lead = (qv * (40.0 / (qv.pow(2).sum().item() * scale * _LOG2E))).float()
            qkv[b, 1, h] = lead
            kv[0, b, h, pos[b]] = -lead
            if pos[b] + 1 < Smax:
                kv[0, b, h, pos[b] + 1] = lead
    return qkv.view(B, 3 * H * 64).to(BF16), kv.to(BF16), torch.tensor(pos, dtype=torch.int32)


def _dot(q, k):
    """q [64] . k [..., 64] in the kernel's order: per lane (8 dims) an fma chain from 0 (the bf16 x bf16 products
    are exact in fp32), then the xor butterfly 4, 2, 1 over the 8 lanes of the group."""
    pr = (q * k).view(*k.shape[:-1], 8, 8)
    s = torch.zeros(pr.shape[:-1])
    for d in range(8):
        s = s + pr[..., d]
    a = s[..., :4] + s[..., 4:]
    a = a[..., :2] + a[..., 2:]
    return a[..., 0] + a[..., 1]


def _fma(a, b, c):  # one rounding: the fp64 product of two fp32 values is exact
    return (a.double() * b.double() + c.double()).float()


def emulate_attn_decode(qkv_new, kv, pos, H, scale, mut=None):
    """The kernel's fp32 value before its store, [B, H * 64] fp32, computed in the kernel's order: per-state
    online softmax over the key split above, then the fixed-order merge. kv is the cache before the call and
    is not modified. Mutations (plausible kernel defects):
      drop_new_key    the new token never enters the softmax (its score still seeds m)
      plus_1          cache row pos + 1, where it exists, is taken for a cached key
      stale_new_key   the new token's k / v are read back from cache row pos as it was before the call"""
    assert mut in (None, "drop_new_key", "plus_1", "stale_new_key"), mut
    _, B, _, Smax, _ = kv.shape
    x = qkv_new.float().view(B, 3, H, 64)
    sl2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    out = torch.zeros(B, H, 64)
    w_i, u_i, g_i = torch.meshgrid(torch.arange(WAVES), torch.arange(UNROLL), torch.arange(GROUPS), indexing="ij")
    for b in range(B):
        n = int(pos[b])
        for h in range(H):
            q, kn, vn = x[b, 0, h], x[b, 1, h], x[b, 2, h]
            Kc, Vc = kv[0, b, h].float(), kv[1, b, h].float()
            if mut == "stale_new_key":
                kn, vn = Kc[n], Vc[n]
            sn = _dot(q, kn)
            m = (sn * sl2).expand(WAVES, GROUPS).clone()
            l = torch.zeros(WAVES, GROUPS)
            O = torch.zeros(WAVES, GROUPS, 64)
            if mut != "drop_new_key":
                p = torch.exp2(_fma(sn, sl2, -m[0, 0]))
                l[0, 0] = p
                O[0, 0] = p * vn
            jv = torch.arange(Smax)
            visible = jv < n
            if mut == "plus_1" and n + 1 < Smax:
                visible = visible | (jv == n + 1)
            bound = n + 2 if (mut == "plus_1" and n + 1 < Smax) else n
            for base in range(0, bound, BLOCK_KEYS):
                j = base + w_i * WAVE_KEYS + u_i * GROUPS + g_i  # [W, U, G]
                ok = (j < Smax) & visible[j.clamp_max(Smax - 1)]
                jc = j.clamp_max(Smax - 1)
                s = _dot(q, torch.where(ok[..., None], Kc[jc], torch.zeros(())))
                V = torch.where(ok[..., None], Vc[jc], torch.zeros(()))
                xs = torch.where(ok, s * sl2, torch.full((), float("-inf")))
                mx = torch.maximum(m, xs.amax(1))
                alpha = torch.exp2(m - mx)
                m = mx
                l = l * alpha
                O = O * alpha[..., None]
                for u in range(UNROLL):
                    p = torch.where(ok[:, u], torch.exp2(_fma(s[:, u], sl2, -m)), torch.zeros(()))
                    l = l + p
                    O = _fma(p[..., None], V[:, u], O)
            M = m.max()
            a = torch.exp2(m - M)
            l = l * a
            O = O * a[..., None]
            # xor 8, 16, 32 over the lanes = xor 1, 2, 4 over the groups
            l = l[:, 0::2] + l[:, 1::2]
            O = O[:, 0::2] + O[:, 1::2]
            l = l[:, 0::2] + l[:, 1::2]
            O = O[:, 0::2] + O[:, 1::2]
            l = l[:, 0] + l[:, 1]
            O = O[:, 0] + O[:, 1]
            L, T = l[0], O[0]
            for w in range(1, WAVES):
                L = L + l[w]
                T = T + O[w]
            out[b, h] = T * (torch.ones(()) / L)
    return out.view(B, H * 64)


def nan_stale_rows(kv, pos):
    """A copy of the cache with every row j > pos[b] filled with NaN."""
    kv = kv.clone()
    for b, n in enumerate(pos):
        kv[:, b, :, int(n) + 1:] = float("nan")
    return kv
