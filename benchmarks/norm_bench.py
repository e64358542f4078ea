"""The row-norm kernels alone: RMSNorm (rms_fwd / dropout_add_rms_fwd / rms_bwd) next to LayerNorm (ln_fwd /
dropout_add_ln_fwd / ln_bwd) at the same ``rows x D``, the backward in the forms the blocks launch (with the fused
column sums; ``+dres``: the pre-norm blocks' residual-stream gradient; ``drop``: hidden dropout's DXM).

    python benchmarks/norm_bench.py                      # 32768 x 768: the rows of a batch-64, S = 512 step
    rocprofv3 --kernel-trace --stats -- python benchmarks/norm_bench.py --iters 20   # per-launch kernel times

One JSON line per kernel form: microseconds per launch (event-timed over ``--iters`` launches), the bytes the launch
reads and writes (the [rows, D] bf16 operands; statistics, weights and partials are left out), TB/s and the share of
the 6.3 TB/s streaming figure the README uses."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from ml_trainer_amd.ops._ext import require_native
    C = require_native()
    dev = torch.device("cuda", 0)
    rows, D = args.rows, args.width
    bf = lambda: torch.randn(rows, D, device=dev).to(torch.bfloat16)
    x, dy, res = bf(), bf(), bf()
    y, z, dx, dxm = (torch.empty_like(x) for _ in range(4))
    gamma, beta = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    dg, db, dxs = (torch.empty(D, device=dev) for _ in range(3))
    part = torch.empty(C.ln_partial_blocks(rows) * 3 * D, device=dev)
    drop = dict(p=0.1, seed=1, site=1, rank=0)
    C.ln_fwd(x, gamma, beta, y, mean, rstd, 1e-12)
    # (name, [rows, D] bf16 tensors moved, launch)
    forms = [
        ("ln_fwd", 2, lambda: C.ln_fwd(x, gamma, beta, y, mean, rstd, 1e-12)),
        ("rms_fwd", 2, lambda: C.rms_fwd(x, gamma, y, rstd, 1e-12)),
        ("dropout_add_ln_fwd", 4, lambda: C.dropout_add_ln_fwd(x, res, gamma, beta, z, y, mean, rstd, 1e-12, *drop.values())),
        ("dropout_add_rms_fwd", 4, lambda: C.dropout_add_rms_fwd(x, res, gamma, z, y, rstd, 1e-12, *drop.values())),
        ("ln_bwd dxsum", 3, lambda: C.ln_bwd(dy, x, gamma, mean, rstd, dx, part, dg, db, False, None, dxsum=dxs)),
        ("rms_bwd dxsum", 3, lambda: C.rms_bwd(dy, x, gamma, rstd, dx, part, dg, False, None, dxsum=dxs)),
        ("ln_bwd dxsum+dres", 4, lambda: C.ln_bwd(dy, x, gamma, mean, rstd, dx, part, dg, db, False, res, dxsum=dxs)),
        ("rms_bwd dxsum+dres", 4, lambda: C.rms_bwd(dy, x, gamma, rstd, dx, part, dg, False, res, dxsum=dxs)),
        ("ln_bwd drop", 4, lambda: C.ln_bwd(dy, x, gamma, mean, rstd, dx, part, dg, db, False, None, dxsum=dxs, dxm=dxm, **drop)),
        ("rms_bwd drop", 4, lambda: C.rms_bwd(dy, x, gamma, rstd, dx, part, dg, False, None, dxsum=dxs, dxm=dxm, **drop)),
        ("ln_bwd drop+dres", 5, lambda: C.ln_bwd_dropout_res(dy, x, gamma, mean, rstd, dx, part, dg, db, False, res, dxs, False, dxm, *drop.values())),
        ("rms_bwd drop+dres", 5, lambda: C.rms_bwd(dy, x, gamma, rstd, dx, part, dg, False, res, dxsum=dxs, dxm=dxm, **drop)),
    ]
    lines = []
    for name, n, fn in forms:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.iters
        nbytes = n * rows * D * 2
        tbs = nbytes / us * 1e-6
        rec = {"bench": "norm", "kernel": name, "rows": rows, "width": D, "us": us, "bytes": nbytes, "tb_s": tbs,
               "share_of_stream": tbs / STREAM_TBS}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
