"""Per-step summary of a ``rocprofv3 --kernel-trace`` run of ``generate_bench.py --trace-steps N``.

    rocprofv3 --kernel-trace --stats --output-format csv -d out -o decode -- \\
        python benchmarks/generate_bench.py --batch 8 --trace-steps 32
    python benchmarks/decode_trace_summary.py out/decode_kernel_trace.csv

A decode step starts at its ``embed_fwd`` dispatch. The window runs from the second step's ``embed_fwd`` to the last
step's (the first step follows the prefill, the last has no successor to close it), so it holds N - 2 whole steps.
One JSON line: wall microseconds per step inside the window (start to start), GPU-busy microseconds per step (the
sum of the kernel durations), launches per step, and per kernel class the launches per step, the mean duration and
the share of the busy time. The linears are keyed by what the trace can tell apart: the kernel, its grid (the
skinny kernel: N / 16 workgroups) and the kernel in front of it (``qkv`` and ``ffn1`` follow a LayerNorm, ``out``
follows ``attn_decode``, ``ffn2`` follows ``ffn1``)."""
from __future__ import annotations

import csv
import json
import re
import sys
from collections import defaultdict


def short(name: str) -> str:
    m = re.search(r"(?:mlt::|native::)?([A-Za-z_0-9]+)\s*(?:<|\()", name.replace("void ", ""))
    return m.group(1) if m else name[:40]


def label(rows, i):
    r = rows[i]
    k = short(r["Kernel_Name"])
    if k.startswith("gemm") or k == "splitk_reduce_kernel":
        prev = short(rows[i - 1]["Kernel_Name"]) if i else ""
        wgs = int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"])) * int(r["Grid_Size_Y"])
        return f"{k}[wgs={wgs},after={prev}]"
    return k


def summarize(path: str) -> dict:
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    first_decode = next(i for i, r in enumerate(rows) if "attn_decode_kernel" in r["Kernel_Name"])
    starts = [i for i, r in enumerate(rows) if "embed_fwd_kernel" in r["Kernel_Name"] and i > first_decode]
    lo, hi, steps = starts[0], starts[-1], len(starts) - 1
    t0, t1 = int(rows[lo]["Start_Timestamp"]), int(rows[hi]["Start_Timestamp"])
    dur, cnt = defaultdict(int), defaultdict(int)
    for i in range(lo, hi):
        k = label(rows, i)
        dur[k] += int(rows[i]["End_Timestamp"]) - int(rows[i]["Start_Timestamp"])
        cnt[k] += 1
    busy = sum(dur.values())
    linear = sum(v for k, v in dur.items() if k.startswith("gemm") or k.startswith("splitk"))
    kernels = {k: {"per_step": cnt[k] / steps, "mean_us": dur[k] / cnt[k] * 1e-3, "share": dur[k] / busy}
               for k in sorted(dur, key=dur.get, reverse=True)}
    return {"trace": path, "steps": steps, "wall_us_per_step": (t1 - t0) / steps * 1e-3,
            "busy_us_per_step": busy / steps * 1e-3, "launches_per_step": (hi - lo) / steps,
            "linear_share_of_busy": linear / busy, "kernels": kernels}


if __name__ == "__main__":
    for p in sys.argv[1:]:
        print(json.dumps(summarize(p)))
