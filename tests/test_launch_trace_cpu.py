"""The native transformer path issues the recorded ``_C`` calls: same names, same order, same scalar arguments, same
tensor operands (dtype, shape, strides, offset and which buffer feeds which call). See tests/launch_trace.py for how
a trace is taken on the CPU; scripts/record_launch_traces.py regenerates the goldens when a launch changes on
purpose."""
import json
import os

import pytest

import launch_trace as LT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_trace")


def test_every_scenario_has_a_golden_and_the_reverse():
    assert sorted(n + ".json" for n in LT.SCENARIOS) == sorted(os.listdir(GOLDEN))


@pytest.mark.parametrize("name", list(LT.SCENARIOS))
def test_launch_trace_matches_golden(name, tmp_path):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        want = json.load(f)
    rec = LT.trace(name)
    if rec.sha256() != want["sha256"] or rec.names() != want["calls"]:
        full = tmp_path / (name + ".jsonl")
        full.write_text(rec.serialise())
        assert rec.names() == want["calls"], f"the sequence of launches changed; full new trace: {full}"
        pytest.fail(f"same launches, other arguments or operands (sha256 {rec.sha256()} != {want['sha256']}); "
                    f"full new trace: {full}")


def test_recorder_sees_dataflow_and_restores_the_patches():
    """Two views of one buffer share a storage number, a new buffer gets the next one, and nothing stays patched."""
    import torch
    from ml_trainer_amd.ops import transformer as T
    before = T.require_native
    with LT.record() as rec:
        a = torch.empty(4, 8)
        assert a.is_cuda
        T.require_native().probe(a[1:], a.t(), torch.empty(2), 0.5, flag=True)
        assert T.require_native().ln_partial_blocks(7) == 2
    assert T.require_native is before and not torch.empty(1).is_cuda
    name, args, kw = rec.calls[0]
    assert name == "probe" and kw == {"flag": True} and args[3] == "0.5"
    assert args[0] == ["T", "float32", [3, 8], [8, 1], 8, 0] and args[1] == ["T", "float32", [8, 4], [1, 8], 0, 0]
    assert args[2][-1] == 1
