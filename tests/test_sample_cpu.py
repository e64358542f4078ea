"""The sampler's definition on the CPU: ``ops.decode.sample_step_reference`` (tensor arithmetic) against the
brute-force oracle of tests/sample_ref.py (Python ints, one element at a time), exactly, on a fixture with ties
on both thresholds, NaNs, an all -inf row, finished rows and a NaN-poisoned padding; the oracle's mutants must be
told apart on that fixture; and ``generate(sampler="device")`` end to end on the CPU."""
import numpy as np
import pytest
import torch

from ml_trainer_amd.ops import decode as DC
from tests import sample_ref as R


def _state(B, T, seed, temperature, top_k, top_p, eos_id, seq_ids=None, finished_row=None):
    st = DC.SamplerState.allocate(B, T, "cpu", seed=seed, temperature=temperature, top_k=top_k, top_p=top_p,
                                  eos_id=eos_id, fill_id=R.FILL_ID, seq_ids=seq_ids)
    ref = R.new_state(B, T, seq_ids=seq_ids)
    if finished_row is not None:
        st.finished[finished_row] = 1
        ref["finished"][finished_row] = 1
    return st, ref


def _assert_same(st, ref, what):
    for name in ("draws", "finished", "lengths", "next_ids", "n_kept", "tokens"):
        assert getattr(st, name).tolist() == ref[name], f"{what}: {name}"


@pytest.mark.parametrize("V", [37, 1000, 1003])
def test_reference_equals_brute_force(V):
    z = R.fixture_logits(V)
    zt = torch.from_numpy(z)
    draws = 2
    for top_k, top_p, temp in R.fixture_settings(V):
        host_s = DC.SamplerState.allocate(1, 1, "cpu", temperature=temp).host["inv_t_log2e"]
        w, a, _ = DC.sample_weights_reference(zt, V, host_s)
        eos = int(a[1])  # row 1 finishes whenever it draws its argmax
        st, ref = _state(R.FIXTURE_ROWS, draws, 1234, temp, top_k, top_p, eos, finished_row=5)
        for _ in range(draws):
            DC.sample_step_reference(zt, V, st)
            R.sample_step(z, V, w.numpy(), a.numpy(), st.host, ref)
        _assert_same(st, ref, f"V={V} k={top_k} p={top_p} t={temp}")
        assert st.tokens[5].tolist() == [R.FILL_ID] * draws and int(st.lengths[5]) == 0
        assert not np.isnan(z[3, st.tokens[3].numpy()]).any()  # a NaN column is never drawn


def test_greedy_and_no_truncation_equal_brute_force():
    V = 1003
    z = R.fixture_logits(V)
    zt = torch.from_numpy(z)
    for temp, top_k, top_p in ((0.0, None, None), (1.0, None, None), (0.7, 5, None), (0.7, None, 0.5)):
        st, ref = _state(R.FIXTURE_ROWS, 3, 99, temp, top_k, top_p, None)
        w, a, _ = DC.sample_weights_reference(zt, V, st.host["inv_t_log2e"])
        for _ in range(3):
            DC.sample_step_reference(zt, V, st)
            R.sample_step(z, V, w.numpy(), a.numpy(), st.host, ref)
        _assert_same(st, ref, f"t={temp} k={top_k} p={top_p}")


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutants_are_told_apart(mutant):
    """Each wrong sampler disagrees with the right one somewhere on the fixture: the fixture can see that bug."""
    V = 37
    z = R.fixture_logits(V)
    differs = False
    for top_k, top_p, temp in R.fixture_settings(V):
        st = DC.SamplerState.allocate(R.FIXTURE_ROWS, 4, "cpu", seed=1234, temperature=temp, top_k=top_k, top_p=top_p)
        w, a, _ = DC.sample_weights_reference(torch.from_numpy(z), V, st.host["inv_t_log2e"])
        good, bad = R.new_state(R.FIXTURE_ROWS, 4), R.new_state(R.FIXTURE_ROWS, 4)
        for _ in range(4):
            R.sample_step(z, V, w.numpy(), a.numpy(), st.host, good)
            R.sample_step(z, V, w.numpy(), a.numpy(), st.host, bad, mutant=mutant)
        differs |= good["tokens"] != bad["tokens"] or good["n_kept"] != bad["n_kept"]
    assert differs, mutant


def test_degenerate_settings_give_the_argmax():
    """k = 1, p = 2^-16 and temperature 1e-3 each leave only the columns that tie for the maximum (a 0.25 step at
    1e-3 is a factor 2^-360): the token is the argmax where the maximum is unique, one of the ties otherwise."""
    V = 1003
    z = R.fixture_logits(V)
    zt = torch.from_numpy(z)
    a = DC.sample_weights_reference(zt, V, 1.0)[1].tolist()
    unique = [b for b in range(4) if int((z[b, :V] == z[b, a[b]]).sum()) == 1]
    assert unique  # not vacuous
    for kw in (dict(temperature=1.0, top_k=1), dict(temperature=1.0, top_p=2.0 ** -16), dict(temperature=1e-3)):
        st = DC.SamplerState.allocate(R.FIXTURE_ROWS, 1, "cpu", seed=5, **kw)
        DC.sample_step_reference(zt, V, st)
        for b in range(4):
            assert z[b, int(st.tokens[b, 0])] == z[b, a[b]], (kw, b)
        for b in unique:
            assert int(st.tokens[b, 0]) == a[b], (kw, b)


def test_row_alone_equals_row_in_batch():
    V = 1000
    zt = torch.from_numpy(R.fixture_logits(V))
    kw = dict(seed=77, temperature=1.3, top_k=40, top_p=0.9)
    alone = DC.SamplerState.allocate(1, 16, "cpu", seq_ids=[2], **kw)
    batch = DC.SamplerState.allocate(3, 16, "cpu", **kw)
    for _ in range(16):
        DC.sample_step_reference(zt[2:3], V, alone)
        DC.sample_step_reference(zt[:3], V, batch)
    assert alone.tokens[0].tolist() == batch.tokens[2].tolist()
    assert len(set(batch.tokens[2].tolist())) > 1  # 16 draws from 40 candidates are not one token


def test_top_p_rounding_errors():
    with pytest.raises(ValueError):
        DC.top_p_to_p16(0.0)
    with pytest.raises(ValueError):
        DC.top_p_to_p16(1.5)
    with pytest.raises(ValueError):
        DC.top_p_to_p16(2.0 ** -18)  # rounds to 0 / 65536
    assert DC.top_p_to_p16(None) == 65536 and DC.top_p_to_p16(1.0) == 65536 and DC.top_p_to_p16(0.9) == 58982


@pytest.fixture(scope="module")
def lm():
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    m = BertLMHeadModel(bert_config("bert-tiny", vocab_size=211, max_position=32)).eval()
    ids = torch.randint(5, 211, (3, 6))
    return m, ids


def test_generate_device_sampler_cpu(lm):
    m, ids = lm
    kw = dict(temperature=0.9, top_k=20, top_p=0.8, seed=3, sampler="device")
    t1, l1 = m.generate(ids, 5, **kw)
    t2, l2 = m.generate(ids, 5, **kw)
    assert t1.shape == (3, 5) and torch.equal(t1, t2) and torch.equal(l1, l2)
    assert bool(((t1 >= 0) & (t1 < 211)).all()) and l1.tolist() == [5, 5, 5]
    t3, _ = m.generate(ids, 5, **dict(kw, seed=4))
    assert not torch.equal(t1, t3)
    # the cached and the uncached model draw the same tokens while their logits agree: greedy needs no luck
    g1, _ = m.generate(ids, 5, sampler="device")
    g0, _ = m.generate(ids, 5)
    gr, _ = m.generate_reference(ids, 5, sampler="device")
    assert torch.equal(g1, g0) and torch.equal(g1, gr)
    # a row decoded alone draws what it draws in the batch (seq_ids default to the row index: row 0 here)
    a1, _ = m.generate(ids[:1], 5, **kw)
    assert torch.equal(a1[0], t1[0])


def test_generate_argument_errors(lm):
    m, ids = lm
    with pytest.raises(ValueError):
        m.generate(ids, 2, temperature=1.0, top_p=0.9)  # top_p needs the device sampler
    for bad in (0.0, -0.1, 1.01, 2.0 ** -18):
        with pytest.raises(ValueError):
            m.generate(ids, 2, temperature=1.0, top_p=bad, sampler="device")
    with pytest.raises(ValueError):
        m.generate(ids, 2, sampler="torch")
    with pytest.raises(ValueError):
        m.generate(ids, 2, graph=True)  # no device sampler
    with pytest.raises(ValueError):
        m.generate(ids, 2, sampler="device", graph=True)  # not on a GPU
    with pytest.raises(ValueError):
        m.generate_reference(ids, 2, temperature=1.0, top_p=0.9)
