"""bf16 LeNet step with the conv1 weight gradient of role D shared by kernel column over ND
workgroups per sample (csrc/kernels/lenet_mfma.inc, lenet_ms<D, ND>): bitwise the single-block step
on every buffer the kernel writes for every shipped ND, the residency rule ((ND + 1) B blocks fit the
CUs, else the next smaller split) and the A/B switches (set_split_parts, MLT_LENET_SPLIT_D)."""
import pytest
import torch

from ml_trainer_amd.models.lenet import MLModel

SHIPPED = (1, 3)  # the ND values the extension instantiates (2 and 5 measured slower: deleted)
AUTO = 3          # what auto picks where it fits


def _engine(config, seed, max_batch, opt="sgd", lr=1e-2):
    from ml_trainer_amd.models.lenet_engine import LeNetStepEngine
    from ml_trainer_amd.ops.optim import build_optimizer
    from ml_trainer_amd.utils.flat import FlatParams
    torch.manual_seed(seed)
    m = MLModel(config).to(torch.device("cuda", 0))
    flat = FlatParams(m.parameters())
    o = build_optimizer(opt, m.parameters(), lr=lr, momentum=0.9, flat=flat)
    return LeNetStepEngine(m, flat, max_batch=max_batch, optimizer=o, precision="bf16"), flat


def _bits(t):
    """Bit pattern of a float tensor (bitwise comparison: -0.0 != 0.0, NaN == NaN)."""
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _toy_data(N, seed=0):
    g = torch.Generator().manual_seed(seed)
    targets = torch.randint(0, 10, (N,), generator=g)
    base = (targets.view(N, 1, 1, 1).float() * 25).expand(N, 32, 32, 3)
    data = (base + torch.randint(0, 30, (N, 32, 32, 3), generator=g).float()).clamp(0, 255).to(torch.uint8)
    return data, targets


_FILL = 0x7F4A5A5A  # a NaN pattern no gradient produces: an element nobody wrote keeps it

_tensor_runs = {}


def _tensor_step(config, B, nd):
    """One step from tensors at ND = nd (None: one block per sample); computed once per case."""
    key = (config, B, nd)
    if key in _tensor_runs:
        return _tensor_runs[key]
    dev = torch.device("cuda", 0)
    c1, c2, f1, f2 = (4, 8, 64, 32) if config == "tiny" else (6, 16, 120, 84)
    flatn, nc = c2 * 25, 10
    g = torch.Generator().manual_seed(100 + B)
    x = torch.randn(B, 3, 32, 32, generator=g).to(dev)
    y = torch.randint(0, 10, (B,), generator=g).to(dev)
    eng, flat = _engine(config, 3, max_batch=32)
    if nd is None:
        eng.set_split(False)
        assert eng.split_blocks(B) == 1 and not eng.split_active(B)
    else:
        eng.set_split(True)
        eng.set_split_parts(nd)
        assert eng.split_blocks(B) == nd + 1 and eng.split_active(B)
    slabn = eng.C.lenet_mfma_slab_floats(eng.model.cfg_id)
    eng.bufs["slab1"].view(torch.int32).fill_(_FILL)
    eng.reset_stats()
    eng.step_from_tensors(x, y, train=True)
    torch.cuda.synchronize()
    bufs = {"grad": flat.grad, "data": flat.data, "stats": eng.stats,
            "slab1": eng.bufs["slab1"][:B * slabn].view(B, slabn)}
    for k, n in (("p2", flatn), ("h1", f1), ("h2", f2), ("dh1", f1), ("dh2", f2), ("dflat", flatn),
                 ("logits", nc), ("dlogits", nc), ("cestat", 2)):
        bufs[k] = eng.bufs[k][:B * n]
    out = {k: _bits(v).clone() for k, v in bufs.items()}
    out["slab1_rest"] = _bits(eng.bufs["slab1"][B * slabn:]).clone()
    assert torch.isfinite(flat.grad).all()
    _tensor_runs[key] = out
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["default", "tiny"])
@pytest.mark.parametrize("B", [1, 5, 32])
@pytest.mark.parametrize("nd", SHIPPED)
def test_split_parts_step_bitwise_tensors(dev, config, B, nd):
    """One step from tensors, ND role-D parts vs one block per sample: the gradient, the updated
    weights, the sums, every buffer handed to the batch-reduction kernel, and the slab rows over
    their full length from a fixed non-zero fill (an element no part wrote, or a store outside
    the used range, differs). B = 1, 5: the smallest grids; B = 32: the benchmark's batch."""
    ref = _tensor_step(config, B, None)
    got = _tensor_step(config, B, nd)
    c1, c2 = (4, 8) if config == "tiny" else (6, 16)
    used = ((c1 * 76 + 3) & ~3) + c2 * c1 * 25 + c2
    # the fill is in place where nothing is stored: the row padding and the rows past the batch
    assert (ref["slab1"][:, used:] == _FILL).all() and (ref["slab1_rest"] == _FILL).all()
    assert (ref["slab1"][:, :c1 * 76] != _FILL).all()
    for k in ref:
        assert torch.equal(ref[k], got[k]), k


@pytest.mark.gpu
def test_split_parts_training_bitwise_dataset(dev):
    """Training from the device dataset (prepared inputs, graphs of 3 steps, two epochs, the
    partial batch of 12), auto ND vs one block per sample: weights, sums and the staging state."""
    data, targets = _toy_data(300, 7)
    runs = []
    for split in (True, False):
        eng, flat = _engine("default", 8, max_batch=32)
        eng.set_split(split)
        eng.set_dataset(data, targets, batch_size=32)
        want = AUTO + 1 if split else 1
        assert eng.split_blocks(32) == want and eng.split_blocks(12) == want
        for ep in range(2):
            eng.start_epoch(torch.randperm(300, generator=torch.Generator().manual_seed(10 + ep)))
            eng.train_steps(32, 9, use_graph=True, steps_per_graph=3)
            eng.train_steps(300 - 9 * 32, 1, use_graph=True, steps_per_graph=1)
        torch.cuda.synchronize()
        runs.append({"data": _bits(flat.data).clone(), "stats": _bits(eng.stats).clone(),
                     **{k: eng.bufs[k].clone() for k in ("meta2", "pmeta", "metaN", "stage2")}})
    assert runs[0]["meta2"].view(-1, 4)[:12, 0].min().item() > 0  # the staging ran
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


# (ND, largest batch whose (ND + 1) B blocks fit 256 CUs)
_EDGE = {3: 64}


@pytest.mark.gpu
def test_split_parts_residency_boundaries(dev):
    """(ND + 1) B blocks must fit the device's CUs at once; above that the next smaller split."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert cus == 256  # MI355X
    eng, _ = _engine("default", 1, max_batch=129)
    eng.set_split(True)
    for nd in SHIPPED:
        if nd == 1:
            continue
        eng.set_split_parts(nd)
        b = _EDGE[nd]
        assert (nd + 1) * b <= cus < (nd + 1) * (b + 1)
        assert eng.split_blocks(b) == nd + 1
        smaller = max(k for k in SHIPPED if k < nd and (k + 1) * (b + 1) <= cus)
        assert eng.split_blocks(b + 1) == smaller + 1
        assert 2 <= eng.split_blocks(b + 1) < nd + 1
        assert eng.split_blocks(128) == 2 and eng.split_blocks(129) == 1
    for n in (0, 1):
        eng.set_split_parts(n)
        assert eng.split_blocks(128) == 2 and eng.split_blocks(129) == 1
        assert eng.split_active(128) and not eng.split_active(129)
    eng.set_split_parts(0)
    assert eng.split_blocks(32) == AUTO + 1
    eng.set_split(False)
    assert eng.split_blocks(32) == 1 and eng.split_blocks(128) == 1


@pytest.mark.gpu
def test_split_parts_need_prepared_inputs(dev, monkeypatch):
    """Without the prep buffers a launch from the dataset stays at one block per sample."""
    monkeypatch.setenv("MLT_LENET_PREP", "0")
    data, targets = _toy_data(64, 3)
    eng, _ = _engine("default", 9, max_batch=32)
    eng.set_split(True)
    assert eng.split_blocks(32) == AUTO + 1  # no dataset yet: inputs come from tensors
    eng.set_dataset(data, targets, batch_size=32)
    assert eng.split_blocks(32) == 1
    for nd in SHIPPED:
        eng.set_split_parts(nd)
        assert eng.split_blocks(32) == 1


@pytest.mark.gpu
def test_split_parts_env(dev, monkeypatch):
    """MLT_LENET_SPLIT_D selects the same ND as the setter; the setter overrides it."""
    for nd in SHIPPED:
        monkeypatch.setenv("MLT_LENET_SPLIT_D", str(nd))
        eng, _ = _engine("default", 1, max_batch=32)
        assert eng.split_blocks(32) == nd + 1
        other = next(k for k in SHIPPED if k != nd)
        eng.set_split_parts(other)
        assert eng.split_blocks(32) == other + 1
        eng.set_split_parts(0)
        assert eng.split_blocks(32) == AUTO + 1
    monkeypatch.setenv("MLT_LENET_SPLIT_D", "0")
    eng, _ = _engine("default", 1, max_batch=32)
    assert eng.split_blocks(32) == AUTO + 1
    monkeypatch.delenv("MLT_LENET_SPLIT_D")
    eng, _ = _engine("default", 1, max_batch=32)
    assert eng.split_blocks(32) == AUTO + 1
    for bad in (2, 4, 5, -1):  # not built
        with pytest.raises(Exception):
            eng.set_split_parts(bad)
    assert eng.split_blocks(32) == AUTO + 1
