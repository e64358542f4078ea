"""Multi-token append attention: one ``C.attn_append`` launch (unsplit, and the split form with its merge launch)
against the ``T`` successive decode launches that served ``T`` tokens before it (``C.attn_decode`` / ``_gqa`` /
``_split`` by ``ops.decode.decode_attn_path``), on the same caches. One JSON line per (T, pos, batch, Hkv)
(profiles/attn_append/README.md).

    python benchmarks/attn_append_bench.py --out profiles/attn_append/kernels.jsonl

Method (benchmarks/gqa_bench.py): the forms alternated ``--repeats`` times round robin in one process, device events
around ``--iters`` calls, medians, ``spread`` = (max - min) / median; every form walks through ``--cold-mb`` of cache
copies so that no call finds its rows in a cache left by the call before. The decode side's T launches of one call
share a cache copy (the later ones find it warm: that is how the parent commit runs them, back to back)."""
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


def bench_cache(C, dev, args, B, H, Hkv, pos, Ts):
    from ml_trainer_amd.ops.decode import decode_attn_path
    Smax = pos + 16
    per = 2 * B * Hkv * Smax * 64 * 2
    n = max(2, -(-args.cold_mb * (1 << 20) // per))
    kv = torch.empty(n, 2, B, Hkv, Smax, 64, dtype=torch.bfloat16, device=dev)
    for i in range(n):
        kv[i].copy_(torch.randn(2, B, Hkv, Smax, 64, device=dev) * 0.5)
    W = (H + 2 * Hkv) * 64
    path = decode_attn_path(Smax)
    recs = []
    for T in Ts:
        qkv = (torch.randn(B * T, W, device=dev) * 0.5).to(torch.bfloat16)
        p = [torch.full((B,), pos + t, dtype=torch.int32, device=dev) for t in range(T)]
        out = torch.empty(B * T, H * 64, dtype=torch.bfloat16, device=dev)
        out1 = torch.empty(B, H * 64, dtype=torch.bfloat16, device=dev)
        ws1 = torch.empty(C.attn_decode_split_ws(B, H, Smax), dtype=torch.float32, device=dev)
        ws = torch.empty(C.attn_append_ws(B, T, H, Smax), dtype=torch.float32, device=dev)
        rp = torch.empty(B * T, dtype=torch.int32, device=dev)
        rows = qkv.view(B, T, W)

        def decode(i):
            c = kv[i % n]
            for t in range(T):
                if path == "split":
                    C.attn_decode_split(rows[:, t], c, p[t], out1, ws1, H, 0.125)
                elif Hkv != H:
                    C.attn_decode_gqa(rows[:, t], c, p[t], out1, H, 0.125)
                else:
                    C.attn_decode(rows[:, t], c, p[t], out1, H, 0.125)

        forms = {"decode": decode,
                 "append": lambda i: C.attn_append(qkv, kv[i % n], p[0], out, B, H, 0.125),
                 "append_split": lambda i: C.attn_append(qkv, kv[i % n], p[0], out, B, H, 0.125, ws=ws, row_pos=rp)}
        iters = args.iters if pos < 8192 else max(8, args.iters // 4)
        runs = _time_round_robin(forms, iters, args.repeats)
        rec = {"bench": "attn_append", "T": T, "pos": pos, "smax": Smax, "batch": B, "H": H, "Hkv": Hkv,
               "decode_path": path, "caches": n, "iters": iters}
        for name, r in runs.items():
            us = statistics.median(r)
            rec.update({f"{name}_us": us, f"{name}_spread": (max(r) - min(r)) / us, f"{name}_runs": r})
        rec["speedup"] = rec["decode_us"] / rec["append_us"]
        rec["speedup_split"] = rec["decode_us"] / rec["append_split_us"]
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    del kv
    torch.cuda.empty_cache()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="1,2,4,8,16")
    ap.add_argument("--pos", default="511,2047,8191")
    ap.add_argument("--batch", default="1,8")
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--kv-heads", default="12,4,1")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cold-mb", type=int, default=768)
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
                recs += bench_cache(C, dev, args, B, args.heads, Hkv, pos, [int(x) for x in args.tokens.split(",")])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for rec in recs:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
