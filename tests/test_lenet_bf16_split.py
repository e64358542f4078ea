"""bf16 LeNet step with the per-sample kernel's tail split over two workgroups per sample
(csrc/kernels/lenet_mfma.inc, lenet_ms<D, SPLIT = true>): bitwise the single-block step on every
buffer the kernel writes, and the launch falls back to one block per sample wherever the split is
not eligible (inputs the kernel stages for itself, 2 B above the CU count, MLT_LENET_SPLIT=0)."""
import pytest
import torch

from ml_trainer_amd.models.lenet import MLModel


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


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["default", "tiny"])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_split_step_bitwise_tensors(dev, config, B):
    """One step from tensors, split on vs off: the gradient, the updated weights, the loss /
    accuracy sums and every buffer the per-sample kernel hands to the batch-reduction kernel.
    B = 1 and 5: the smallest grids, no multiple of anything; B = 64: 128 blocks."""
    c1, c2, f1, f2 = (4, 8, 64, 32) if config == "tiny" else (6, 16, 120, 84)
    flatn, nc = c2 * 25, 10
    g = torch.Generator().manual_seed(100 + B)
    x = torch.randn(B, 3, 32, 32, generator=g).to(dev)
    y = torch.randint(0, 10, (B,), generator=g).to(dev)
    out = []
    for split in (True, False):
        eng, flat = _engine(config, 3, max_batch=64)
        eng.set_split(split)
        assert eng.split_active(B) is split
        eng.reset_stats()
        eng.step_from_tensors(x, y, train=True)
        torch.cuda.synchronize()
        assert eng.split_active(B) is split
        slabn = eng.C.lenet_mfma_slab_floats(eng.model.cfg_id)
        s1 = c1 * 76
        used = ((s1 + 3) & ~3) + c2 * c1 * 25 + c2  # conv1 part, pad to 4, conv2 part (+ bias)
        bufs = {"grad": flat.grad, "data": flat.data, "stats": eng.stats,
                "slab1": eng.bufs["slab1"][:B * slabn].view(B, slabn)[:, :used]}
        for k, n in (("p2", flatn), ("h1", f1), ("h2", f2), ("dh1", f1), ("dh2", f2), ("dflat", flatn),
                     ("logits", nc), ("dlogits", nc), ("cestat", 2)):
            bufs[k] = eng.bufs[k][:B * n]
        out.append({k: _bits(v).clone() for k, v in bufs.items()})
        assert torch.isfinite(flat.grad).all()
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k


@pytest.mark.gpu
def test_split_training_bitwise_dataset(dev):
    """Training from the device dataset (prepared inputs, graphs of 3 steps, two epochs, the
    partial batch of 12), split on vs off: weights and sums bit for bit, and the staging state
    the two kernels leave behind (role W does the staging of a split step)."""
    data, targets = _toy_data(300, 7)
    runs = []
    for split in (True, False):
        eng, flat = _engine("default", 8, max_batch=32)
        eng.set_split(split)
        eng.set_dataset(data, targets, batch_size=32)
        assert eng.split_active(32) is split and eng.split_active(12) is split
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


@pytest.mark.gpu
def test_split_needs_prepared_inputs(dev, monkeypatch):
    """Without the prep buffers the per-sample kernel reads the raw images its own staging wave
    rewrites: ordered inside one block, a race across two -- such a launch stays unsplit."""
    monkeypatch.setenv("MLT_LENET_PREP", "0")
    data, targets = _toy_data(64, 3)
    eng, flat = _engine("default", 9, max_batch=32)
    eng.set_split(True)
    assert eng.split_active(32)  # no dataset yet: inputs come from tensors
    eng.set_dataset(data, targets, batch_size=32)
    assert not eng.split_active(32)
    eng.start_epoch(torch.arange(64))
    eng.reset_stats()
    eng.train_steps(32, 2, use_graph=False)
    torch.cuda.synchronize()
    loss, _ = eng.read_stats(2)
    assert loss == loss and 0.0 < loss < 10.0
    assert eng.ctrl.tolist() == [2, 2]


@pytest.mark.gpu
def test_split_needs_two_blocks_per_sample_resident(dev):
    """2 B blocks must fit the device's CUs at once."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    assert cus == 256  # MI355X
    eng, _ = _engine("default", 1, max_batch=129)
    eng.set_split(True)
    assert eng.split_active(128)
    assert not eng.split_active(129)


@pytest.mark.gpu
def test_split_env_default(dev, monkeypatch):
    monkeypatch.setenv("MLT_LENET_SPLIT", "0")
    eng, _ = _engine("default", 1, max_batch=32)
    assert not eng.split_active(32)
    eng.set_split(True)
    assert eng.split_active(32)
    monkeypatch.setenv("MLT_LENET_SPLIT", "1")
    eng, _ = _engine("default", 1, max_batch=32)
    assert eng.split_active(32)
    monkeypatch.delenv("MLT_LENET_SPLIT")
    eng, _ = _engine("default", 1, max_batch=32)
    assert eng.split_active(32)
