"""The stage references and bounds of the bf16 LeNet step (tests/lenet_stage_ref.py) on the CPU, the counterpart of
test_gemm_bound_cpu.py / test_attn_decode_cpu.py: a torch fp32 emulation of the step lies inside every stage
bound in two summation orders, the stage references compose to autograd's gradients, six planted defects each leave
the check that is meant to catch them, and the exactness certificate and the ambiguity cap hold for every case
tests/test_lenet_bf16_stages_gpu.py runs."""
import math

import pytest
import torch
import torch.nn.functional as F

from ml_trainer_amd.models.lenet import MLModel
from tests import lenet_stage_ref as R

CASES = list(R.BF16_CASES)


def _id(c):
    return f"{c[0]}-B{c[1]}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_certificate_cap_and_edges_hold(case):
    """Per GPU case, on the reference alone: every forward stage's sum |terms| / quantum is below 2^24 (bf16
    rounding points; identity rounding too where the fp32 engine runs the case), the ambiguous share of the live
    nonzero d1 elements is within the cap, tied pool windows and exactly-zero pooled cells occur, and sample 0 --
    whose target is the second of the tied fc3 rows -- has the tied pair as its maximum (a miss by the
    first-arg-max rule)."""
    c = R.exact_case(*case)
    cert = R.exactness_certificate(c.P, c.x)
    print(_id(case), "log2 certificate", {k: round(math.log2(v), 2) for k, v in cert.items()})
    assert max(cert.values()) < R.CERT_LIMIT, cert
    if case in R.FP32_CASES:
        c32 = R.exactness_certificate(c.P, c.x, R.identity)
        print(_id(case), "log2 certificate, identity rounding", {k: round(math.log2(v), 2) for k, v in c32.items()})
        assert max(c32.values()) < R.CERT_LIMIT, c32
    for k, v in c.P.items():  # the parameters are bf16 points: rnd(weights) changes nothing
        assert torch.equal(R.bf16_round(v), v), k
    ch = R.chain(c.P, c.x, c.y, R.bf16_round, c.inv_B)
    print(_id(case), f"ambiguous share {ch['info']['share']:.4f}")
    assert 0 < ch["info"]["share"] <= R.AMBIGUOUS_CAP
    ec = R.edge_counts(c.fw)
    print(_id(case), ec)
    assert ec["ties1"] + ec["ties2"] > 0 and ec["zeros1"] + ec["zeros2"] > 0
    z = c.fw["logits"]
    assert bool(z[0, R.TIE[0]] == z[0].max()) and bool(z[0, R.TIE[1]] == z[0].max()) and int(c.y[0]) == R.TIE[1]
    assert float(ch["hit"][0]) == 0.0
    assert torch.equal(ch["logits"], z)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_emulation_within_every_stage_bound(case, order):
    """A torch fp32 emulation of the step, rounding where the kernel rounds, passes every check of check_step in
    torch's own summation order and in a second one; the share of each allowance it uses is printed."""
    c = R.exact_case(*case)
    ratios, failures = R.check_step(c, R.emulate_step(c, order))
    print(_id(case), "order", order, {k: round(v, 4) for k, v in ratios.items()})
    assert not failures, failures


@pytest.mark.parametrize("config", ["default", "tiny"])
def test_emulation_within_bounds_on_random_data(config):
    """The bounds do not lean on the exact inputs: random normal data and weights, no exactness claimed."""
    torch.manual_seed(5)
    m = MLModel(config)
    x, y = torch.randn(7, 3, 32, 32), torch.randint(0, 10, (7,))
    c = R.Case(config, 7, {k: v.detach().double() for k, v in m.named_parameters()}, x.double(), y)
    for order in (0, 1):
        ratios, failures = R.check_step(c, R.emulate_step(c, order), exact=False)
        print(config, "order", order, {k: round(v, 4) for k, v in ratios.items()})
        assert not failures, failures


@pytest.mark.parametrize("config", ["default", "tiny"])
def test_stage_references_compose_to_autograd(config):
    """With rnd = identity the chained stage references are the fp64 model's loss and gradients."""
    torch.manual_seed(1)
    m = MLModel(config).double()
    x = torch.randn(6, 3, 32, 32, dtype=torch.float64)
    y = torch.randint(0, 10, (6,))
    loss = F.cross_entropy(m.forward_reference(x), y)
    loss.backward()
    ch = R.chain(dict(m.named_parameters()), x, y, R.identity)
    assert abs(float(ch["loss"]) - loss.item()) < 1e-12
    for n, p in m.named_parameters():
        torch.testing.assert_close(ch["grad"][n].view_as(p), p.grad, rtol=1e-9, atol=1e-12, msg=lambda s: f"{n}: {s}")


# defect -> (the smallest case that can show it, the check that must fail)
#   fc1_drop           (a) one product dropped from one fc1 row
#   tie_last           (b) the pool tie rule takes the last maximum: the gradient lands on another cell of the window
#   live_ge            (c) liveness >= 0: a cell that is exactly 0 passes its gradient on
#   wrong_sample_*     (d) the batch reduction reads sample B - 1 in place of sample 1 (B = 5: not a multiple of 32)
#   tap_shift          (e) one conv1 weight-gradient tap takes the neighbouring kernel column's window
#   d1_trunc           (f) one non-ambiguous d1 element rounded toward zero
PLANTED = {"fc1_drop": (("tiny", 1), "h1"), "tie_last": (("tiny", 1), "slab.conv1.weight"),
           "live_ge": (("tiny", 1), "slab.conv1.weight"), "wrong_sample_fc": (("tiny", 5), "grad.fc1.weight"),
           "wrong_sample_conv": (("tiny", 5), "grad.conv1.weight"), "tap_shift": (("tiny", 1), "slab.conv1.weight"),
           "d1_trunc": (("tiny", 1), "slab.conv1.weight")}


def test_every_defect_is_planted():
    assert set(PLANTED) == set(R.DEFECTS)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect_fails_its_check(defect):
    case, check = PLANTED[defect]
    c = R.exact_case(*case)
    clean = R.emulate_step(c, 0)
    assert not R.check_step(c, clean)[1]
    pick = None
    if defect == "d1_trunc":
        pick, r = R.pick_d1_element(c, clean)
        print("d1_trunc hits", pick, f"predicted |change| / allowance {r:.2f}")
    ratios, failures = R.check_step(c, R.emulate_step(c, 0, defect, pick))
    print(defect, "fails", sorted(failures))
    assert check in failures, (check, sorted(failures))
    if defect in ("tie_last", "live_ge"):  # the forward values do not depend on either rule: only the routing does
        assert not any(k.startswith("exact.") for k in failures)
