"""The fp8 key/value cache against the bf16 one (profiles/kv_f8/README.md), one JSON line per shape.

    python benchmarks/kv_f8_bench.py --out profiles/kv_f8/kernels.jsonl                       # the kernels alone
    python benchmarks/kv_f8_bench.py --generate --out profiles/kv_f8/generate.jsonl          # 128 + 128 tokens, graph
    python benchmarks/kv_f8_bench.py --generate --rotary --max-position 8192 --prompt 7936 --batch 1,8 --out ...

Kernels: ``C.attn_decode_f8`` (single, and split + merge with a workspace) against ``C.attn_decode`` /
``C.attn_decode_gqa`` and ``C.attn_decode_split`` of the same build, the four alternated ``--repeats`` times round robin
in one process (benchmarks/gqa_bench.py's method: device events around ``--iters`` launches, medians, ``spread`` =
(max - min) / median), every form walking through ``--cold-mb`` of cache copies of its own format so that no launch
finds its rows in a cache left by the one before. Bytes: the cached K and V rows below ``pos`` once per KV head, 2 x 128
per row for bf16, 2 x 68 (codes + scale) for fp8. ``--generate``: ``generate(graph=True, sampler="device")`` with
``kv_cache`` None and "fp8" alternated, ms per generation, the bytes of both caches and the peak allocation of each."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchmarks.gqa_bench import _time_round_robin  # noqa: E402


def bench_shape(C, dev, args, B, H, Hkv, pos):
    Smax = pos + 1
    rows = 2 * B * Hkv * Smax
    n16, n8 = (max(2, -(-args.cold_mb * (1 << 20) // (rows * w))) for w in (128, 68))
    rec = {"bench": "kv_f8_kernel", "batch": B, "H": H, "Hkv": Hkv, "pos": pos, "smax": Smax, "caches": [n16, n8]}
    if n16 * rows * 128 + n8 * rows * 68 > args.max_gb * (1 << 30):
        print(json.dumps({**rec, "skipped": "the cache copies exceed --max-gb"}), flush=True)
        return None
    kv = torch.empty(n16, 2, B, Hkv, Smax, 64, dtype=torch.bfloat16, device=dev)
    for i in range(n16):  # filled copy by copy: no fp32 temporary of the whole set
        kv[i].copy_(torch.randn(2, B, Hkv, Smax, 64, device=dev) * 0.5)
    # random finite codes (0x7F is the NaN code) of both signs under the scale 2^-9: values within +-0.9
    kv8 = torch.randint(0, 0x7F, (n8, 2, B, Hkv, Smax, 64), dtype=torch.uint8, device=dev)
    kv8 += torch.randint(0, 2, kv8.shape, dtype=torch.uint8, device=dev) * 128
    sc = torch.full((n8, 2, B, Hkv, Smax), 2.0 ** -9, device=dev)
    qkv = (torch.randn(B, (H + 2 * Hkv) * 64, device=dev) * 0.5).to(torch.bfloat16)
    p = torch.full((B,), pos, dtype=torch.int32, device=dev)
    out = torch.empty(B, H * 64, dtype=torch.bfloat16, device=dev)
    ws = torch.empty(C.attn_decode_split_ws(B, H, Smax), dtype=torch.float32, device=dev)
    if Hkv == H:
        single = lambda i: C.attn_decode(qkv, kv[i % n16], p, out, H, 0.125)
    else:
        single = lambda i: C.attn_decode_gqa(qkv, kv[i % n16], p, out, H, 0.125)
    variants = {"bf16_single": single,
                "f8_single": lambda i: C.attn_decode_f8(qkv, kv8[i % n8], sc[i % n8], p, out, H, 0.125),
                "bf16_split": lambda i: C.attn_decode_split(qkv, kv[i % n16], p, out, ws, H, 0.125),
                "f8_split": lambda i: C.attn_decode_f8(qkv, kv8[i % n8], sc[i % n8], p, out, H, 0.125, ws=ws)}
    iters = args.iters if pos < 8192 else max(8, args.iters // 4)  # long caches: fewer, longer launches
    runs = _time_round_robin(variants, iters, args.repeats)
    rec["iters"] = iters
    for name, r in runs.items():
        us, nbytes = statistics.median(r), 2 * B * Hkv * pos * (128 if name.startswith("bf16") else 68)
        rec.update({f"{name}_us": round(us, 2), f"{name}_spread": round((max(r) - min(r)) / us, 3),
                    f"{name}_tb_per_s": round(nbytes / us * 1e-6, 3)})
    for form in ("single", "split"):
        rec[f"speedup_{form}"] = round(rec[f"bf16_{form}_us"] / rec[f"f8_{form}_us"], 3)
    print(json.dumps(rec), flush=True)
    del kv, kv8, sc
    torch.cuda.empty_cache()
    return rec


def bench_generate(args, dev, B):
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    over = dict(rotary=True) if args.rotary else {}
    if args.max_position is not None:
        over["max_position"] = args.max_position
    if args.kv_heads is not None:
        over["kv_heads"] = args.kv_heads
    m = BertLMHeadModel(bert_config(args.model, **over)).to(dev).eval()
    c = m.config
    ids = torch.randint(5, c.vocab_size, (B, args.prompt), device=dev)
    kw = dict(temperature=0.8, top_k=50, seed=1, sampler="device", graph=True)
    rec = {"bench": "kv_f8_generate", "model": args.model, "batch": B, "prompt": args.prompt, "new": args.new,
           "rotary": bool(args.rotary), "kv_heads": c.num_kv_heads, "max_position": c.max_position}
    rows = 2 * c.layers * B * c.num_kv_heads * (args.prompt + args.new)
    rec.update(bf16_cache_bytes=rows * 128, f8_cache_bytes=rows * 68)
    runs = {"bf16": [], "f8": []}
    for name, fmt in (("bf16", None), ("f8", "fp8")):  # the captures, and the peak of one generation of each format
        m.generate(ids, args.new, kv_cache=fmt, **kw)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        m.generate(ids, args.new, kv_cache=fmt, **kw)
        torch.cuda.synchronize()
        rec[f"{name}_peak_bytes"] = torch.cuda.max_memory_allocated()
    for _ in range(args.repeats):
        for name, fmt in (("bf16", None), ("f8", "fp8")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.generate(ids, args.new, kv_cache=fmt, **kw)
            torch.cuda.synchronize()
            runs[name].append((time.perf_counter() - t0) * 1e3)
    for name, r in runs.items():
        ms = statistics.median(r)
        rec.update({f"{name}_ms": round(ms, 2), f"{name}_spread": round((max(r) - min(r)) / ms, 3)})
    rec["speedup"] = round(rec["bf16_ms"] / rec["f8_ms"], 3)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="1,8,64")
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--kv-heads", default=None, help="kernels: a list (default 12,4,1); --generate: one value")
    ap.add_argument("--pos", default="255,2047,8191,32767")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cold-mb", type=int, default=768)
    ap.add_argument("--max-gb", type=int, default=64)
    ap.add_argument("--generate", action="store_true", help="time generate(graph=True) with both caches instead")
    ap.add_argument("--model", default="bert-base")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--rotary", action="store_true")
    ap.add_argument("--max-position", type=int, default=None)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.repeats < 5:
        raise SystemExit("--repeats: medians of at least 5")
    from ml_trainer_amd.ops._ext import require_native
    C, dev = require_native(), torch.device("cuda", 0)
    torch.manual_seed(0)
    recs = []
    if args.generate:
        args.kv_heads = None if args.kv_heads is None else int(args.kv_heads)
        recs = [bench_generate(args, dev, int(B)) for B in args.batch.split(",")]
    else:
        for pos in (int(x) for x in args.pos.split(",")):
            for B in (int(x) for x in args.batch.split(",")):
                for Hkv in (int(x) for x in (args.kv_heads or "12,4,1").split(",")):
                    recs.append(bench_shape(C, dev, args, B, args.heads, Hkv, pos))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for rec in filter(None, recs):
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
