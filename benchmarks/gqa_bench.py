"""Kernel timings of grouped-query attention, one JSON line per figure (profiles/gqa/README.md):

* ``attn_decode_gqa`` against ``attn_decode`` at batch ``--batch``, H heads, ``pos`` in ``--pos``, ``Hkv`` in
  ``--kv-heads`` (``Hkv == H`` is the existing kernel), and the forced chunkings of ``--gc`` (``H:Hkv:gc``, e.g.
  ``16:2:8,16:2:4``: one workgroup of 8 heads against two of 4);
* ``gqa_expand`` / ``gqa_reduce`` per launch at ``--rows`` rows.

Every variant of a group is timed in turn, ``--repeats`` times round robin in one process, with device events around
``--iters`` launches; a figure is the median over the repeats and ``spread`` is (max - min) / median. A decode
variant walks through enough copies of its cache (``--cold-mb`` in all) that no launch finds its rows in a cache
left by the launch before. Bytes are what the algorithm must move: the cached K and V rows below ``pos`` once per
KV head (decode), compact once and wide once (expand / reduce)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _time_round_robin(variants, iters, repeats):
    """variants {name: fn(i)}; returns {name: [us per launch] * repeats}."""
    out = {k: [] for k in variants}
    for fn in variants.values():  # warm-up: code objects, the allocator
        for i in range(3):
            fn(i)
    for _ in range(repeats):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for i in range(iters):
                fn(i)
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / iters)
    return out


def _emit(rec, runs, nbytes):
    us = statistics.median(runs)
    rec.update(us=us, spread=(max(runs) - min(runs)) / us, bytes=nbytes, tb_per_s=nbytes / us * 1e-6, runs=runs)
    print(json.dumps(rec), flush=True)


def bench_decode(C, dev, args, H, specs, pos):
    """specs: [(Hkv, gc)]; gc = 0 is the launcher's own choice."""
    B, Smax = args.batch, args.smax
    variants, nbytes = {}, {}
    for Hkv, gc in specs:
        per = 2 * B * Hkv * Smax * 64 * 2
        n = max(2, -(-args.cold_mb * (1 << 20) // per))
        kv = (torch.randn(n, 2, B, Hkv, Smax, 64, device=dev) * 0.5).to(torch.bfloat16)
        qkv = (torch.randn(B, (H + 2 * Hkv) * 64, device=dev) * 0.5).to(torch.bfloat16)
        p = torch.full((B,), pos, dtype=torch.int32, device=dev)
        out = torch.empty(B, H * 64, dtype=torch.bfloat16, device=dev)
        if Hkv == H:
            fn = lambda i, kv=kv, qkv=qkv, p=p, out=out, n=n: C.attn_decode(qkv, kv[i % n], p, out, H, 0.125)
        else:
            fn = lambda i, kv=kv, qkv=qkv, p=p, out=out, n=n, gc=gc: C.attn_decode_gqa(qkv, kv[i % n], p, out, H, 0.125,
                                                                                         gc=gc)
        name = f"{Hkv}:{gc}"
        variants[name], nbytes[name] = fn, 2 * B * Hkv * pos * 64 * 2
    for name, runs in _time_round_robin(variants, args.iters, args.repeats).items():
        Hkv, gc = (int(x) for x in name.split(":"))
        G = H // Hkv
        _emit({"bench": "attn_decode_gqa" if Hkv != H else "attn_decode", "batch": B, "H": H, "Hkv": Hkv, "pos": pos,
               "gc": (gc or C.attn_decode_gqa_chunk(G, Hkv, B)) if Hkv != H else 1}, runs, nbytes[name])


def bench_layout(C, dev, args):
    H, Hkv, rows = args.heads, args.layout_kv_heads, args.rows
    compact = torch.randn(rows, (H + 2 * Hkv) * 64, device=dev).to(torch.bfloat16)
    wide = torch.randn(rows, 3 * H * 64, device=dev).to(torch.bfloat16)
    nbytes = (compact.numel() + wide.numel()) * 2
    t = _time_round_robin({"gqa_expand": lambda i: C.gqa_expand(compact, wide, H, Hkv),
                           "gqa_reduce": lambda i: C.gqa_reduce(wide, compact, H, Hkv)}, max(4, args.iters // 8),
                          args.repeats)
    for name, runs in t.items():
        _emit({"bench": name, "rows": rows, "H": H, "Hkv": Hkv}, runs, nbytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--kv-heads", default="12,4,2,1")
    ap.add_argument("--pos", default="255,511")
    ap.add_argument("--smax", type=int, default=512)
    ap.add_argument("--gc", default="16:2:8,16:2:4", help="forced chunkings H:Hkv:gc, timed against each other")
    ap.add_argument("--rows", type=int, default=512 * 512)
    ap.add_argument("--layout-kv-heads", type=int, default=4)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cold-mb", type=int, default=768)
    args = ap.parse_args()
    from ml_trainer_amd.ops._ext import require_native
    C, dev = require_native(), torch.device("cuda", 0)
    torch.manual_seed(0)
    for pos in (int(p) for p in args.pos.split(",")):
        bench_decode(C, dev, args, args.heads, [(int(k), 0) for k in args.kv_heads.split(",")], pos)
        forced = [tuple(int(x) for x in s.split(":")) for s in args.gc.split(",") if s]
        for H in sorted({f[0] for f in forced}):
            bench_decode(C, dev, args, H, [(hkv, gc) for h, hkv, gc in forced if h == H], pos)
    bench_layout(C, dev, args)


if __name__ == "__main__":
    main()
