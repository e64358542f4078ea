"""``C.sample_step`` / ``C.sample_weights`` (csrc/kernels/sample.hip) on the GPU.

Two separate statements: (a) the device's integer weights are within the DERIVED bound of the exact value
(tests/sample_ref.py: the subtract, the multiply, exp2f's stated ulp, the floor); (b) GIVEN those weights, everything
the kernel writes equals the brute-force oracle exactly. State tensors sit in guarded allocations and the logits'
padding columns are NaN throughout."""
import numpy as np
import pytest
import torch

from ml_trainer_amd.ops import decode as DC
from tests import sample_ref as R

pytestmark = pytest.mark.gpu

_PAT32, _PAT64, _PAD = 0x5A5AA5A5, 0x5A5AA5A55A5AA5A5, 16


def _guarded(shape, dtype, dev):
    """(buf, view): ``view`` (zeros) in the middle of a pattern-filled 1-D allocation, 16 elements on each side."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * _PAD,), _PAT32 if dtype == torch.int32 else _PAT64, dtype=dtype, device=dev)
    view = buf[_PAD:_PAD + n].view(*shape)
    view.zero_()
    return buf, view


def _guards_intact(bufs):
    for name, (buf, view) in bufs.items():
        pat = _PAT32 if buf.dtype == torch.int32 else _PAT64
        n = view.numel()
        assert bool((buf[:_PAD] == pat).all()) and bool((buf[_PAD + n:] == pat).all()), f"guard of {name} overwritten"


def _guarded_state(B, T, dev, seq_ids=None, **params):
    """A SamplerState whose every tensor is a view inside its own guarded allocation."""
    i32, i64 = torch.int32, torch.int64
    bufs = dict(params=_guarded((8,), i32, dev), draws=_guarded((B,), i32, dev), seq_ids=_guarded((B,), i32, dev),
                finished=_guarded((B,), i32, dev), n_kept=_guarded((B,), i32, dev), lengths=_guarded((B,), i64, dev),
                next_ids=_guarded((B,), i64, dev), tokens=_guarded((B, T), i64, dev))
    st = DC.SamplerState(**{k: v[1] for k, v in bufs.items()}, host={})
    st.seq_ids.copy_(torch.arange(B) if seq_ids is None else torch.tensor(seq_ids))
    st.set_params(**params)
    return st, bufs


def _assert_state(st, ref, what):
    for name in ("draws", "finished", "lengths", "next_ids", "n_kept", "tokens"):
        assert getattr(st, name).tolist() == ref[name], f"{what}: {name}"


def _run_against_oracle(C, z, V, settings, draws, dev, eos_from_row=None, finished_row=None):
    """``z`` numpy fp32 [B, ldz] (padding NaN). For every (top_k, top_p, temperature): ``draws`` consecutive steps of
    the kernel against the oracle fed the device's own weights; everything the kernel writes must be equal."""
    zt = torch.from_numpy(z).to(dev)
    B = z.shape[0]
    weights = {}
    for top_k, top_p, temp in settings:
        st, bufs = _guarded_state(B, draws, dev, seed=1234, temperature=temp, top_k=top_k, top_p=top_p, fill_id=R.FILL_ID)
        s = st.host["inv_t_log2e"]
        if s not in weights:
            w, a = C.sample_weights(zt, V, s)
            weights[s] = (w.cpu().numpy(), a.cpu().numpy())
        w, a = weights[s]
        eos = None if eos_from_row is None else int(a[eos_from_row])
        st.set_params(seed=1234, temperature=temp, top_k=top_k, top_p=top_p, eos_id=eos, fill_id=R.FILL_ID)
        ref = R.new_state(B, draws)
        if finished_row is not None:
            st.finished[finished_row] = 1
            ref["finished"][finished_row] = 1
        memo = {}
        for _ in range(draws):
            C.sample_step(zt, V, st.params, st.draws, st.seq_ids, st.finished, st.lengths, st.tokens, st.next_ids,
                          st.n_kept)
            R.sample_step(z, V, w, a, st.host, ref, memo=memo)
        _assert_state(st, ref, f"B={B} V={V} k={top_k} p={top_p} t={temp}")
        _guards_intact(bufs)
    assert bool(torch.isnan(zt[:, V:]).all())


def _random_logits(B, V, ldz, seed):
    rng = np.random.default_rng(seed)
    z = np.full((B, ldz), np.nan, dtype=np.float32)
    z[:, :V] = np.round(rng.normal(0.0, 2.0, (B, V)) * 4) / 4
    return z


@pytest.fixture(scope="module")
def C():
    from ml_trainer_amd.ops._ext import require_native
    return require_native()


@pytest.mark.parametrize("V", [37, 1000, 1003])
def test_weights_within_derived_bound(C, dev, V):
    """(a) every weight within the bound of fp64; 2^24 on the maximum; the argmax is the first index of the maximum."""
    z = R.fixture_logits(V)
    z[0, [3, 11, 29]] = z[0, :V].max() + 1.0  # a three-way tie for the maximum: index 3 wins
    z[2, :V] += np.float32(0.1) * np.arange(V, dtype=np.float32) / V  # off the 0.25 grid: the roundings matter
    zt = torch.from_numpy(z).to(dev)
    for temp in R.T_CASES + (0.37,):
        s = DC.SamplerState.allocate(1, 1, "cpu", temperature=temp).host["inv_t_log2e"]
        w, a = C.sample_weights(zt, V, s)
        w, a = w.cpu().numpy().astype(np.int64), a.cpu().numpy()
        assert a[0] == 3
        for b in range(z.shape[0]):
            zb = z[b, :V]
            nan = np.isnan(zb)
            zc = np.where(nan, -np.inf, zb)
            m = zc.max()
            assert a[b] == int(np.argmax(zc == m)), (temp, b)  # np.argmax of a bool row: the first True
            assert (w[b][zc == m] == R.ONE).all() and w[b][a[b]] == R.ONE
            assert (w[b][nan] == 0).all() and w[b].min() >= 0 and w[b].max() <= R.ONE
            rest = ~nan & (zc != m)
            if np.isfinite(m) and rest.any():
                exact, bound = R.weight_bound(zc[rest], m, s)
                err = np.abs(w[b][rest] - exact)
                i = int(np.argmax(err - bound))
                assert (err <= bound).all(), f"t={temp} row {b}: |w - w*| = {err[i]} > bound {bound[i]} at w* = {exact[i]}"


@pytest.mark.parametrize("V", [37, 1000, 1003])
def test_step_equals_oracle_on_fixture(C, dev, V):
    """(b) + (c): the CPU fixture's settings (ties on both thresholds, NaNs, an all -inf row, an EOS that row 1
    reaches, a finished row), 8 consecutive draws, guarded state."""
    _run_against_oracle(C, R.fixture_logits(V), V, list(R.fixture_settings(V)), 8, dev, eos_from_row=1, finished_row=5)


def test_step_equals_oracle_extra_settings(C, dev):
    """Greedy, no truncation, top-k alone, top-p alone: the paths that skip passes."""
    V = 1003
    settings = [(None, None, 0.0), (None, None, 1.0), (5, None, 0.7), (None, 0.5, 0.7), (1, None, 1.0)]
    _run_against_oracle(C, R.fixture_logits(V), V, settings, 8, dev, eos_from_row=2)


def test_step_equals_oracle_vocabulary_shape(C, dev):
    """[3, 30720] with V = 30,522: the shape ``decode_logits`` writes (8 vectors per thread, every bin digit used)."""
    z = _random_logits(3, 30522, 30720, 5)
    z[1, :30522] *= 4.0  # a peaked row and two flat ones
    settings = [(50, 0.9, 1.0), (None, 0.9, 1.0), (50, None, 0.8), (None, None, 1.0), (None, None, 0.0), (5, 0.5, 100.0)]
    _run_against_oracle(C, z, 30522, settings, 8, dev)


@pytest.mark.parametrize("B", [1, 17])
def test_step_equals_oracle_batch_sizes(C, dev, B):
    settings = [(40, 0.9, 1.3), (None, 0.5, 1.0), (3, None, 2.0)]
    _run_against_oracle(C, _random_logits(B, 1003, 1008, 40 + B), 1003, settings, 8, dev)


def test_reproducible_and_batch_invariant(C, dev):
    """(d) two runs give the same bits; a row alone (seq_ids = [2]) draws what it draws as row 2 of 3."""
    V = 30522
    zt = torch.from_numpy(_random_logits(3, V, 30720, 9)).to(dev)
    kw = dict(seed=77, temperature=1.3, top_k=40, top_p=0.9)
    runs = []
    for _ in range(2):
        st = DC.SamplerState.allocate(3, 16, dev, **kw)
        for _ in range(16):
            DC.sample_step(zt, V, st)
        runs.append((st.tokens.clone(), st.n_kept.clone(), st.lengths.clone()))
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    alone = DC.SamplerState.allocate(1, 16, dev, seq_ids=[2], **kw)
    for _ in range(16):
        DC.sample_step(zt[2:3], V, alone)
    assert torch.equal(alone.tokens[0], runs[0][0][2])
    assert len(set(runs[0][0][2].tolist())) > 1
    # and the torch reference, fed the device's weights, is the same function
    ref = DC.SamplerState.allocate(3, 16, "cpu", **kw)
    w, _ = C.sample_weights(zt, V, ref.host["inv_t_log2e"])
    for _ in range(16):
        DC.sample_step_reference(zt.cpu(), V, ref, weights=w.cpu())
    assert torch.equal(ref.tokens, runs[0][0].cpu()) and torch.equal(ref.n_kept, runs[0][1].cpu())


def test_logits_view_of_a_padded_buffer(C, dev):
    """The [B, V] view of a [B, Vp] buffer (what ``decode_logits`` returns) is taken as it is, and an unaligned
    contiguous [B, V] is copied by the Python wrapper: the same tokens either way."""
    V = 1003
    z = _random_logits(4, V, 1024, 3)
    full = torch.from_numpy(z).to(dev)
    kw = dict(seed=5, temperature=1.0, top_k=30, top_p=0.95)
    a = DC.SamplerState.allocate(4, 4, dev, **kw)
    b = DC.SamplerState.allocate(4, 4, dev, **kw)
    packed = full[:, :V].contiguous()  # row stride 1003: not a multiple of 4
    for _ in range(4):
        DC.sample_step(full[:, :V], V, a)
        DC.sample_step(packed, V, b)
    assert torch.equal(a.tokens, b.tokens)


def test_binding_rejects_bad_operands(C, dev):
    """(e)"""
    V = 1003
    zt = torch.zeros(2, 1008, device=dev)
    st = DC.SamplerState.allocate(2, 4, dev)

    def call(logits=zt, V=V, **over):
        t = {k: over.get(k, getattr(st, k)) for k in ("params", "draws", "seq_ids", "finished", "lengths", "tokens",
                                                       "next_ids", "n_kept")}
        C.sample_step(logits, V, t["params"], t["draws"], t["seq_ids"], t["finished"], t["lengths"], t["tokens"],
                      t["next_ids"], t["n_kept"])

    call()  # the good call passes
    bad = [dict(logits=zt.bfloat16()), dict(logits=zt.cpu()), dict(logits=torch.zeros(2, 1006, device=dev)),
           dict(logits=zt.t().contiguous().t()), dict(V=0), dict(V=1009), dict(logits=zt[:, 1:]),
           dict(draws=st.draws.long()), dict(lengths=st.lengths.int()), dict(tokens=st.tokens.int()),
           dict(draws=torch.zeros(3, dtype=torch.int32, device=dev)), dict(tokens=torch.zeros(3, 4, dtype=torch.int64, device=dev)),
           dict(tokens=torch.zeros(8, dtype=torch.int64, device=dev)), dict(params=st.params[:4]),
           dict(params=st.params.cpu()), dict(next_ids=st.next_ids.cpu()), dict(seq_ids=st.seq_ids.float())]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
    with pytest.raises(RuntimeError):
        C.sample_weights(zt.bfloat16(), V, 1.0)
    with pytest.raises(RuntimeError):
        C.sample_weights(zt, 2000, 1.0)
    torch.cuda.synchronize()
    assert st.draws.tolist() == [1, 1]  # only the good call ran
