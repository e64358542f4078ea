"""bench.py's plain / --full split and --dump-outputs: a plain run measures the headline only, --full
adds the fp32 companion; the dumped arrays are float32 / float64 .npy files within the size limit,
identical from run to run with the same arguments; --steps sets the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_main(monkeypatch, tmp_path, tag, *argv):
    """bench.main() in this process (one rank); returns (result line, {name: array} it dumped)."""
    dump, out = tmp_path / f"dump_{tag}", tmp_path / f"line_{tag}.json"
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv, "--dump-outputs", str(dump), "--json-out", str(out)])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    arrays = {f[:-4]: np.load(dump / f) for f in sorted(os.listdir(dump))}
    return json.loads(out.read_text()), arrays


def _check_dump(arrays):
    assert arrays and all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2 ** 20
    assert all(np.isfinite(a).all() for a in arrays.values())


def test_cpu_dump_is_reproducible_and_steps_are_the_timed_steps(monkeypatch, tmp_path, capsys):
    runs = [_run_main(monkeypatch, tmp_path, t, "--device", "cpu", "--gpus", "1", "--steps", "3", "--warmup", "1")
            for t in ("a", "b")]
    (line, a), (_, b) = runs
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert set(a) == {"params", "last_logits", "last_loss", "loss_sum"}
    _check_dump(a)
    assert a["params"].shape == (62006,) and a["last_logits"].shape == (32, 10)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    # one more timed step is one more update: the dump is the LAST step's
    _, c = _run_main(monkeypatch, tmp_path, "c", "--device", "cpu", "--gpus", "1", "--steps", "4", "--warmup", "1")
    assert not np.array_equal(a["params"], c["params"])


def test_large_output_is_a_fixed_sample(monkeypatch, tmp_path):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    big = torch.arange(10000, dtype=torch.float32)
    for d in ("x", "y"):
        bench._dump_outputs(str(tmp_path / d), 0, {"big": big, "small": torch.ones(3, dtype=torch.float64)})
    x, y = np.load(tmp_path / "x" / "big.npy"), np.load(tmp_path / "y" / "big.npy")
    assert x.dtype == np.float32 and x.nbytes <= 4096 * 3 // 4 // 2 and len(x) > 100
    np.testing.assert_array_equal(x, y)
    assert (np.diff(x) >= 0).all() and x.max() > 5000  # sorted positions spread over the whole array
    assert np.load(tmp_path / "x" / "small.npy").dtype == np.float64
    bench._dump_outputs(str(tmp_path / "z"), 1, {"big": big})  # only rank 0 writes
    assert not (tmp_path / "z").exists()


def _spawn(tmp_path, tag, *argv):
    """bench.py as a fresh child process (its own HIP context, streams and device flags)."""
    dump, out = tmp_path / f"dump_{tag}", tmp_path / f"line_{tag}.json"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), *argv, "--dump-outputs", str(dump),
                          "--json-out", str(out)], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    return p, dump, out


@pytest.mark.gpu
def test_plain_run_is_the_headline_only_full_adds_the_fp32_companion(tmp_path):
    """One plain and one --full run of the LeNet headline, side by side: same arguments otherwise, so
    the headline's dumped outputs are bitwise the same; only --full carries the fp32 figures."""
    common = ("--gpus", "1", "--steps", "6", "--warmup", "2")
    runs = [_spawn(tmp_path, "plain", *common), _spawn(tmp_path, "full", *common, "--full")]
    res = []
    for p, dump, out in runs:
        text, _ = p.communicate(timeout=240)
        assert p.returncode == 0, text[-3000:]
        assert len([ln for ln in text.splitlines() if ln.startswith("{")]) == 1, text[-3000:]
        res.append((json.loads(out.read_text()), {f[:-4]: np.load(dump / f) for f in sorted(os.listdir(dump))}))
    (plain, a), (full, b) = res
    for line in (plain, full):
        assert line["steps"] == 6 and line["warmup"] == 2 and line["dtype"] == "bf16" and line["ms_per_step"] > 0
        assert line["metric"] == "samples/sec/node" and line["unit"] == "samples/s" and line["higher_is_better"]
    assert not [k for k in plain["config"] if k.startswith("fp32_")]
    for k in ("fp32_samples_per_s", "fp32_ms_per_step", "fp32_vs_baseline", "fp32_dp_transport"):
        assert k in full["config"]
    assert set(a) == set(b) == {"params", "stats", "last_step_sample_stats"}
    _check_dump(a)
    assert a["params"].dtype == np.float32 and a["params"].shape == (62006,) and a["stats"].dtype == np.float64
    assert a["stats"][0] > 0 and a["last_step_sample_stats"].any()
    for k in a:  # the dump is the headline (bf16) run's, whatever follows it
        np.testing.assert_array_equal(a[k], b[k])
