"""Native softmax-CE / accuracy kernels vs the plain torch fp32 reference."""
import pytest
import torch
import torch.nn.functional as F

from ml_trainer_amd.ops.losses import CrossEntropyLoss, accuracy
from tests import helpers

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B,C", [(1, 10), (33, 10), (256, 2), (64, 1000), (7, 130)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ls", [0.0, 0.1])
def test_ce_forward_backward(dev, B, C, dtype, ls):
    z = (torch.randn(B, C, device=dev) * 3).to(dtype).requires_grad_(True)
    y = torch.randint(0, C, (B,), device=dev)
    if B > 3:
        y[1] = -100  # ignore_index row
    z2 = z.detach().float().requires_grad_(True)
    loss = CrossEntropyLoss(label_smoothing=ls)(z, y)
    ref = F.cross_entropy(z2, y, label_smoothing=ls)
    torch.testing.assert_close(loss.float(), ref, rtol=1e-5, atol=1e-5)
    (loss * 1.7).backward()
    (ref * 1.7).backward()
    if dtype == torch.float32:
        torch.testing.assert_close(z.grad, z2.grad, rtol=1e-6, atol=1e-6)
    # every element against fp64 within the derived bound (helpers.ce_bound): the mean-reduced gradient is at most
    # 1.7 / B per element, so that a fixed 1e-2 passed an all-zero bf16 gradient; the bound is relative to each element
    x, t = helpers.ce_bound(z.detach().cpu(), y.cpu(), -100, ls, 1.7)
    helpers.assert_within(z.grad.cpu(), x["grad"], helpers.store_bound(x["grad"], t["grad"], dtype),
                          f"ce gradient ({B},{C}) {dtype} ls {ls}")
    if B * C > 1:
        zero = torch.zeros_like(z.grad).cpu()
        with pytest.raises(AssertionError):
            helpers.assert_within(zero, x["grad"], helpers.store_bound(x["grad"], t["grad"], dtype), "zero gradient")


def test_accuracy(dev):
    z = torch.randn(1000, 10, device=dev)
    y = torch.randint(0, 10, (1000,), device=dev)
    hits, _ = helpers.accuracy_expected(z.cpu(), y.cpu())  # the explicit first-index rule, on the CPU
    torch.testing.assert_close(accuracy(z, y).cpu(), torch.tensor(hits, dtype=torch.float32))


@pytest.mark.parametrize("shape", [(1,), (37, 3), (4096, 5), (300001,)])
@pytest.mark.parametrize("kind", ["l1", "mse"])
def test_pointwise_losses(dev, shape, kind):
    from ml_trainer_amd.ops.losses import L1Loss, MSELoss
    p = torch.randn(*shape, device=dev, requires_grad=True)
    t = torch.randn(*shape, device=dev)
    if kind == "l1":
        t.view(-1)[0] = p.detach().view(-1)[0]  # sign(0) = 0 gradient
    p2 = p.detach().clone().requires_grad_(True)
    crit, ref_fn = (L1Loss(), F.l1_loss) if kind == "l1" else (MSELoss(), F.mse_loss)
    loss, ref = crit(p, t), ref_fn(p2, t)
    torch.testing.assert_close(loss, ref, rtol=1e-5, atol=1e-6)
    (loss * 3.0).backward()
    (ref * 3.0).backward()
    torch.testing.assert_close(p.grad, p2.grad, rtol=1e-6, atol=1e-9)
    # fixed-order reductions: bitwise reproducible
    assert torch.equal(crit(p, t), loss)


@pytest.mark.parametrize("B,C", [(1, 10), (513, 7), (64, 1000)])
def test_nll_loss(dev, B, C):
    from ml_trainer_amd.ops.losses import NLLLoss
    z = torch.randn(B, C, device=dev)
    lp = F.log_softmax(z, -1).requires_grad_(True)
    y = torch.randint(0, C, (B,), device=dev)
    if B > 3:
        y[2] = -100
    lp2 = lp.detach().clone().requires_grad_(True)
    loss, ref = NLLLoss()(lp, y), F.nll_loss(lp2, y)
    torch.testing.assert_close(loss, ref, rtol=1e-5, atol=1e-6)
    (loss * 0.5).backward()
    (ref * 0.5).backward()
    torch.testing.assert_close(lp.grad, lp2.grad, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("B,C", [(1, 3), (100, 6), (5000, 2)])
def test_mcrmse(dev, B, C):
    from ml_trainer_amd.ops.losses import mcrmse
    p, t = torch.randn(B, C, device=dev), torch.randn(B, C, device=dev)
    ref = torch.mean(torch.sqrt(torch.mean(torch.square(t - p), dim=0)), dim=0)
    torch.testing.assert_close(mcrmse(p, t), ref, rtol=1e-5, atol=1e-6)


def test_custom_loss_native(dev):
    from ml_trainer_amd.utils.functions import custom_loss_function
    p, t = torch.randn(32, 10, device=dev), torch.randn(32, 10, device=dev)
    torch.testing.assert_close(custom_loss_function(p, t), torch.mean((p - t) ** 2), rtol=1e-5, atol=1e-6)
