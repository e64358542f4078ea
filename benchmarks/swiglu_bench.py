"""SwiGLU kernels alone on the GPU (one JSON line per variant: median us of ``--repeats`` timed windows, spread,
bytes the algorithm needs, TB/s, share of the 6.3 TB/s streaming figure):

* ``swiglu_fwd`` (6 bytes per element of [rows, F]) and ``swiglu_bwd`` (10 bytes, with its partial reduction into the
  bias gradient) at ``--rows`` rows and ``F`` in ``--widths``, alternated in one process;
* ``gemm_skinny_glu`` against ``gemm_skinny`` (N = 2F) + ``swiglu_fwd`` at ``--batch`` rows for the (F, K) of
  ``--layers``, over rotating weight copies (``--cold-mb``) so that the weights come from HBM as in a decode step.
Random operands (no network)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchmarks.gqa_bench import _time_round_robin  # noqa: E402

STREAM_TBS = 6.3  # the achievable streaming bandwidth the other kernels here are held against (profiles/README.md)


def _emit(rec, runs, nbytes):
    us = statistics.median(runs)
    tbs = nbytes / us * 1e-6
    rec.update(us=us, spread=(max(runs) - min(runs)) / us, bytes=nbytes, tb_per_s=tbs, share=tbs / STREAM_TBS, runs=runs)
    print(json.dumps(rec), flush=True)


def bench_streaming(C, dev, args):
    for F in (int(f) for f in args.widths.split(",")):
        rows = args.rows
        h1 = torch.randn(rows, 2 * F, device=dev).to(torch.bfloat16)
        da = torch.randn(rows, F, device=dev).to(torch.bfloat16)
        a, dh1 = torch.empty_like(da), torch.empty_like(h1)
        part = torch.empty(C.swiglu_partial_blocks(rows) * 2 * F, dtype=torch.float32, device=dev)
        db = torch.zeros(2 * F, dtype=torch.float32, device=dev)
        t = _time_round_robin({"swiglu_fwd": lambda i: C.swiglu_fwd(h1, a),
                               "swiglu_bwd": lambda i: C.swiglu_bwd(da, h1, dh1, part, db, False)},
                              args.iters, args.repeats)
        _emit({"bench": "swiglu_fwd", "rows": rows, "F": F}, t["swiglu_fwd"], rows * F * 6)
        _emit({"bench": "swiglu_bwd", "rows": rows, "F": F}, t["swiglu_bwd"], rows * F * 10)


def bench_decode(C, dev, args):
    for spec in args.layers.split(","):
        F, K = (int(x) for x in spec.split(":"))
        for M in (int(m) for m in args.batch.split(",")):
            n = max(2, -(-args.cold_mb * (1 << 20) // (2 * F * K * 2)))
            W = (torch.randn(n, 2 * F, K, device=dev) * K ** -0.5).to(torch.bfloat16)
            b = torch.randn(2 * F, device=dev)
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            y, h1 = (torch.empty(M, c, dtype=torch.bfloat16, device=dev) for c in (F, 2 * F))

            def pair(i):
                C.gemm_skinny(x, W[i % n], h1, bias=b)
                C.swiglu_fwd(h1, y)

            t = _time_round_robin({"fused": lambda i: C.gemm_skinny_glu(x, W[i % n], y, bias=b), "pair": pair},
                                  args.decode_iters, args.repeats)
            for name, runs in t.items():
                _emit({"bench": "gemm_skinny_glu" if name == "fused" else "gemm_skinny+swiglu_fwd", "M": M, "F": F,
                       "K": K}, runs, 2 * F * K * 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512 * 512)
    ap.add_argument("--widths", default="2048,3072")
    ap.add_argument("--layers", default="2048:768,1024:256", help="F:K of the gated decode GEMM")
    ap.add_argument("--batch", default="1,8,16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--decode-iters", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cold-mb", type=int, default=768)
    args = ap.parse_args()
    from ml_trainer_amd.ops._ext import require_native
    C, dev = require_native(), torch.device("cuda", 0)
    torch.manual_seed(0)
    bench_streaming(C, dev, args)
    bench_decode(C, dev, args)


if __name__ == "__main__":
    main()
