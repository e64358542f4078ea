"""Decode attention over a paged cache: ``C.attn_decode_paged`` on a shuffled block table against
``C.attn_decode_split`` on the same rows in contiguous form (both are split + merge, both launches inside the timed
region), and at 512 cached rows against the single kernel (``C.attn_decode`` / ``C.attn_decode_gqa``) too. One JSON
line per (batch, Hkv, pos) with every figure (profiles/decode_paged/README.md).

    python benchmarks/attn_decode_paged_bench.py --out profiles/decode_paged/kernels.jsonl

Method (benchmarks/attn_decode_split_bench.py): the forms alternated ``--repeats`` times round robin in one process,
device events around ``--iters`` launches, medians, ``spread`` = (max - min) / median; each form walks through
``--cold-mb`` of cache copies (the paged form through as many pools, each with a shuffled table of its own) so that no
launch finds its rows in a cache left by the launch before. Before timing, the paged output is compared with the split
kernel's bit for bit. Bytes: the cached K and V rows below ``pos`` once per KV head."""
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


def bench_shape(C, dev, args, B, H, Hkv, pos):
    R = C.attn_decode_paged_page_rows()
    pages = -(-(pos + 1) // R)
    Smax, P = pages * R, B * pages + 1
    per = 2 * B * Hkv * Smax * 64 * 2  # bytes of one cache
    n = max(2, -(-args.cold_mb * (1 << 20) // per))
    rec = {"bench": "attn_decode_paged", "page_rows": R, "batch": B, "H": H, "Hkv": Hkv, "pos": pos, "smax": Smax,
           "caches": n}
    if 2 * n * per > args.max_gb * (1 << 30):
        print(json.dumps({**rec, "skipped": f"2 x {n} caches of {per} bytes exceed --max-gb"}), flush=True)
        return None
    kv = torch.empty(n, 2, B, Hkv, Smax, 64, dtype=torch.bfloat16, device=dev)
    pool = torch.zeros(n, 2, P, Hkv, R, 64, dtype=torch.bfloat16, device=dev)
    tabs = torch.empty(n, B, pages, dtype=torch.int32, device=dev)
    for i in range(n):  # copy by copy: no fp32 temporary of the whole set; the same rows, scattered over shuffled pages
        kv[i].copy_(torch.randn(2, B, Hkv, Smax, 64, device=dev) * 0.5)
        tabs[i] = (torch.randperm(P - 1, device=dev) + 1).view(B, pages).int()
        pool[i][:, tabs[i].long()] = kv[i].view(2, B, Hkv, pages, R, 64).permute(0, 1, 3, 2, 4, 5)
    qkv = (torch.randn(B, (H + 2 * Hkv) * 64, device=dev) * 0.5).to(torch.bfloat16)
    p = torch.full((B,), pos, dtype=torch.int32, device=dev)
    out = torch.empty(B, H * 64, dtype=torch.bfloat16, device=dev)
    ws = torch.empty(C.attn_decode_split_ws(B, H, Smax), dtype=torch.float32, device=dev)
    split = lambda i: C.attn_decode_split(qkv, kv[i % n], p, out, ws, H, 0.125)
    paged = lambda i: C.attn_decode_paged(qkv, pool[i % n], tabs[i % n], p, out, ws, H, 0.125)
    split(0)
    want = out.clone()
    paged(0)
    torch.cuda.synchronize()
    if not torch.equal(out.view(torch.int16), want.view(torch.int16)):
        raise SystemExit(f"paged and split outputs differ at B={B} Hkv={Hkv} pos={pos}")
    forms = {"split": split, "paged": paged}
    if pos < 1024:  # the single kernel is the contiguous path's choice below DECODE_SPLIT_MIN_SMAX
        if Hkv == H:
            forms["single"] = lambda i: C.attn_decode(qkv, kv[i % n], p, out, H, 0.125)
        else:
            forms["single"] = lambda i: C.attn_decode_gqa(qkv, kv[i % n], p, out, H, 0.125)
    iters = args.iters if pos < 8192 else max(8, args.iters // 4)  # long caches: fewer, longer launches
    runs = _time_round_robin(forms, iters, args.repeats)
    nbytes = 2 * B * Hkv * pos * 64 * 2
    rec.update(iters=iters, bytes=nbytes)
    for name, r in runs.items():
        us = statistics.median(r)
        rec.update({f"{name}_us": us, f"{name}_spread": (max(r) - min(r)) / us, f"{name}_tb_per_s": nbytes / us * 1e-6,
                    f"{name}_runs": r})
    rec["paged_over_split"] = rec["paged_us"] / rec["split_us"]
    print(json.dumps(rec), flush=True)
    del kv, pool
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="1,8")
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--kv-heads", default="12,4,1")
    ap.add_argument("--pos", default="511,2047,8191")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cold-mb", type=int, default=768)
    ap.add_argument("--max-gb", type=int, default=64)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.repeats < 5:
        raise SystemExit("--repeats: medians of at least 5")
    from ml_trainer_amd.ops._ext import require_native
    C, dev = require_native(), torch.device("cuda", 0)
    torch.manual_seed(0)
    recs = []
    for pos in (int(x) for x in args.pos.split(",")):
        for B in (int(x) for x in args.batch.split(",")):
            for Hkv in (int(x) for x in args.kv_heads.split(",")):
                rec = bench_shape(C, dev, args, B, args.heads, Hkv, pos)
                if rec:
                    recs.append(rec)
    if args.out and recs:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for rec in recs:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
