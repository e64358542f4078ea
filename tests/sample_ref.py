"""A brute-force oracle of the sampler's definition (csrc/include/mlt_sample.h) in Python ints. No tests here.

It is independent of ``ops.decode.sample_step_reference`` (no torch, no radix select, no prefix sums over tensors):
given a row's logits, its INTEGER weights and its argmax it sorts the indices by ``(z descending, index ascending)``
and applies steps 3-5 of the definition literally, one element at a time. The weights are an input because the
selection is exact only given the weights: ``weight_bound`` is the separate statement about the weights themselves.

``weight_bound`` - derivation. The device computes ``w = floor(2^24 * e)``, ``e = min(exp2f(t), 1)``,
``t = fl(s * fl(z - m))`` in fp32 (u = 2^-24 the unit roundoff), against the exact ``w* = 2^24 * 2^(s (z - m))``:
  * the subtract: ``fl(z - m) = (z - m)(1 + d1)``, ``|d1| <= u``;
  * the multiply: ``t = s (z - m)(1 + d1)(1 + d2)``, ``|d2| <= u``, so with ``t* = s (z - m)``:
    ``|t - t*| <= |t*| (2u + u^2)`` (a product that underflows adds at most 2^-150: far below the +1 of the floor);
  * ``exp2f``: at most 1 ulp as HIP documents it, a relative error ``|d3| <= 2^-23``; ``min(., 1)`` moves the value
    towards the exact one (``t* <= 0`` so ``2^t* <= 1``) and cannot add error;
  * ``* 2^24`` is exact; the floor loses less than 1: ``w in (2^24 e - 1, 2^24 e]``.
So ``|w - w*| <= w* (2^(|t*| (2u + u^2)) (1 + 2^-23) - 1) + 1``, plus the fp64 evaluation of ``w*`` itself
(``<= w* (1 + |t*|) 2^-45``, generous). Where ``z == m`` the weight is 2^24 exactly and NaN logits weigh 0: no bound.

The mutants are wrong samplers that a fixture must be able to tell from the right one.
"""
from __future__ import annotations

import math

import numpy as np

SAMPLE_SITE = 0x53414D50
ONE = 1 << 24
MUTANTS = ("k_off_by_one", "ties_dropped", "p_before_k", "seq_ids_ignored", "cached_draws")


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _top_k(order, zc, k, V, mutant):
    if not 0 < k < V:
        return list(order)
    if mutant == "ties_dropped":
        return list(order[:k])
    t_k = zc[order[k if mutant == "k_off_by_one" else k - 1]]
    return [i for i in order if zc[i] >= t_k]


def _top_p(cand, zc, w, p16):
    """``cand`` sorted by (z desc, index asc). The members with z >= T_p."""
    if p16 >= 65536:
        return list(cand)
    need = (p16 * sum(w[i] for i in cand) + 65535) >> 16
    if need == 0:
        return list(cand)
    cum, n = 0, 0
    while n < len(cand):  # one tie group at a time: the candidate thresholds are the distinct values
        t = zc[cand[n]]
        while n < len(cand) and zc[cand[n]] == t:
            cum += w[cand[n]]
            n += 1
        if cum >= need:
            return list(cand[:n])
    raise AssertionError("need <= W_K: unreachable")


def candidates(z, w, host, mutant=None):
    """S of steps 3-4: the indices kept, for one row's V logits ``z`` and integer weights ``w``."""
    V = len(z)
    zc = [(-math.inf if math.isnan(x) else float(x)) for x in z]
    order = sorted(range(V), key=lambda i: (-zc[i], i))
    if mutant == "p_before_k":
        S = _top_p(order, zc, w, host["p16"])
        return _top_k(S, zc, host["top_k"], len(S), None)
    return _top_p(_top_k(order, zc, host["top_k"], V, mutant), zc, w, host["p16"])


def sample_row(z, w, a, host, draw, seq_id, mutant=None, S=None):
    """(token, n_kept) of one row: ``z`` its V logits (floats), ``w`` its V integer weights, ``a`` its argmax;
    ``S`` = ``candidates(z, w, host, mutant)`` when the caller has it already (it does not depend on the draw)."""
    if host["inv_t_log2e"] == 0:
        return int(a), 1
    if S is None:
        S = candidates(z, w, host, mutant)
    W = sum(int(w[i]) for i in S)
    if W == 0:
        return int(a), len(S)
    seed = host["seed"]
    x = philox4x32_10((draw & 0xFFFFFFFF, 0 if mutant == "seq_ids_ignored" else seq_id & 0xFFFFFFFF, SAMPLE_SITE, 0),
                      (seed & 0xFFFFFFFF, seed >> 32))[0]
    r = ((x >> 8) * W) >> 24
    cum = 0
    for i in sorted(S):
        cum += int(w[i])
        if cum > r:
            return i, len(S)
    raise AssertionError("r < W_S: unreachable")


def new_state(B, T, seq_ids=None, finished=None):
    return dict(draws=[0] * B, seq_ids=list(range(B)) if seq_ids is None else [int(x) for x in seq_ids],
                finished=[0] * B if finished is None else [int(x) for x in finished], lengths=[0] * B,
                tokens=[[0] * T for _ in range(B)], next_ids=[0] * B, n_kept=[0] * B)


def sample_step(logits, V, weights, argmax, host, st, mutant=None, memo=None):
    """One step over all rows, with step 6's bookkeeping on the dict ``st`` (``new_state``). ``logits`` [B, >= V],
    ``weights`` [B, V] and ``argmax`` [B] are array-likes. ``memo``: a dict that keeps every row's candidate set
    between the steps of one (logits, weights, setting): consecutive draws then sort once."""
    logits = np.asarray(logits, dtype=np.float64)
    weights = np.asarray(weights).astype(np.int64)
    for b in range(logits.shape[0]):
        draw = 0 if mutant == "cached_draws" else st["draws"][b]
        zb, wb = logits[b, :V].tolist(), weights[b].tolist()
        S = None
        if host["inv_t_log2e"] != 0 and memo is not None:
            S = memo[b] if b in memo else memo.setdefault(b, candidates(zb, wb, host, mutant))
        tok, kept = sample_row(zb, wb, int(argmax[b]), host, draw, st["seq_ids"][b], mutant, S)
        if st["finished"][b]:
            tok = host["fill_id"]
        else:
            st["lengths"][b] += 1
            if tok == host["eos_id"]:
                st["finished"][b] = 1
        T = len(st["tokens"][b])
        st["tokens"][b][min(max(st["draws"][b], 0), T - 1)] = tok
        st["next_ids"][b] = tok
        st["draws"][b] += 1
        st["n_kept"][b] = kept


def weight_bound(z, m, s):
    """(w* fp64, bound fp64) per element for fp32 arrays ``z`` [..., V], ``m`` [..., 1] and the fp32 scale ``s``;
    meaningful where z is not NaN and z != m (see the module docstring)."""
    z = np.asarray(z, dtype=np.float64)
    m = np.asarray(m, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        t = float(np.float32(s)) * (z - m)
        w = 16777216.0 * np.exp2(t)
        u = 2.0 ** -24
        at = np.minimum(np.abs(t), 1e6)  # beyond that w* is 0 anyway: keep 2^(..) finite
        bound = w * (np.exp2(at * (2 * u + u * u)) * (1 + 2.0 ** -23) - 1) + 1 + w * (1 + at) * 2.0 ** -45
    return w, bound


# ----------------------------------------------------------------------------- the shared fixture
K_CASES = (1, 2, 5, "V", "V+3")            # top_k (V and V + 3: everything kept)
P_CASES = (2.0 ** -16, 0.5, 0.9, 1.0)      # top_p
T_CASES = (1e-3, 1.0, 100.0)               # temperature
FIXTURE_ROWS = 6                           # 0-2 plain, 3 with NaNs (one on its maximum), 4 all -inf, 5 finished
FILL_ID = 7


def fixture_logits(V, seed=0):
    """fp32 [6, ldz] (ldz = V rounded up to 4, the padding poisoned with NaN): logits quantised to multiples of
    0.25 (normal, sigma 1.5), so ties sit on the top-k and the top-p thresholds; row 3 carries NaNs, one of them
    where its maximum was; row 4 is all -inf."""
    rng = np.random.default_rng(seed + V)
    ldz = -(-V // 4) * 4
    z = np.full((FIXTURE_ROWS, ldz), np.nan, dtype=np.float32)
    z[:, :V] = np.round(rng.normal(0.0, 1.5, (FIXTURE_ROWS, V)) * 4) / 4
    z[1, :V][z[1, :V] == 0] = -0.0  # -0 must count as +0
    z[3, int(np.argmax(z[3, :V]))] = np.nan
    z[3, V // 2] = np.nan
    z[4, :V] = -np.inf
    return z


def fixture_settings(V):
    for k in K_CASES:
        for p in P_CASES:
            for t in T_CASES:
                yield (V if k == "V" else V + 3 if k == "V+3" else k), p, t
