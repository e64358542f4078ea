"""Decode attention over long caches: the single kernel (``C.attn_decode`` / ``C.attn_decode_gqa``: one workgroup per
head walks the whole cache) against ``C.attn_decode_split`` (split + merge, both launches inside the timed region), one
JSON line per (batch, Hkv, pos) with both figures (profiles/decode_split/README.md).

    python benchmarks/attn_decode_split_bench.py --build-variants          # no GPU: the 512 / 1024 candidates
    python benchmarks/attn_decode_split_bench.py --out profiles/decode_split/kernels.jsonl
    python benchmarks/attn_decode_split_bench.py --ext benchmarks/bin/decode_split/_C_c512.so --out ...

The keys per split are a compile-time constant (kDecSplitKeys). ``--build-variants`` compiles attn_decode_split.hip
with ``-DMLT_DEC_SPLIT_KEYS=512`` / ``1024`` and links each into ``benchmarks/bin/decode_split/_C_c<keys>.so``; ``--ext`` times
such a build instead of the in-tree extension, in a process of its own, against the single kernel of the same build
(the single kernels do not depend on the constant). Records carry ``split_keys``.

Method (benchmarks/gqa_bench.py): the two forms alternated ``--repeats`` times round robin in one process, device events
around ``--iters`` launches, medians, ``spread`` = (max - min) / median; each form walks through ``--cold-mb`` of cache
copies so that no launch finds its rows in a cache left by the launch before. Shapes whose cache copies do not fit
``--max-gb`` are skipped and say so. Bytes: the cached K and V rows below ``pos`` once per KV head."""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchmarks.gqa_bench import _time_round_robin  # noqa: E402

VARIANT_DIR = os.path.join(ROOT, "benchmarks", "bin", "decode_split")


def build_variants(keys):
    from ml_trainer_amd.build import build
    os.makedirs(VARIANT_DIR, exist_ok=True)
    for k in keys:
        out = os.path.join(VARIANT_DIR, f"_C_c{k}.so")
        build(jobs=min(16, os.cpu_count() or 8), extra_flags={"attn_decode_split.hip": [f"-DMLT_DEC_SPLIT_KEYS={k}"]},
              out_path=out)
        print("built", os.path.relpath(out, ROOT), flush=True)
    build(jobs=min(16, os.cpu_count() or 8))  # the in-tree objects back to the in-tree constant


def load_ext(path):
    if not path:
        from ml_trainer_amd.ops._ext import require_native
        return require_native()
    spec = importlib.util.spec_from_file_location("_C", path)  # the init symbol is PyInit__C whatever the file name
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bench_shape(C, dev, args, B, H, Hkv, pos):
    Smax = pos + 1
    per = 2 * B * Hkv * Smax * 64 * 2  # bytes of one cache
    n = max(2, -(-args.cold_mb * (1 << 20) // per))
    rec = {"bench": "attn_decode_split", "split_keys": C.attn_decode_split_keys(), "batch": B, "H": H, "Hkv": Hkv,
           "pos": pos, "smax": Smax, "caches": n}
    if n * per > args.max_gb * (1 << 30):
        print(json.dumps({**rec, "skipped": f"{n} caches of {per} bytes exceed --max-gb"}), flush=True)
        return None
    kv = torch.empty(n, 2, B, Hkv, Smax, 64, dtype=torch.bfloat16, device=dev)
    for i in range(n):  # filled copy by copy: no fp32 temporary of the whole set
        kv[i].copy_(torch.randn(2, B, Hkv, Smax, 64, device=dev) * 0.5)
    qkv = (torch.randn(B, (H + 2 * Hkv) * 64, device=dev) * 0.5).to(torch.bfloat16)
    p = torch.full((B,), pos, dtype=torch.int32, device=dev)
    out = torch.empty(B, H * 64, dtype=torch.bfloat16, device=dev)
    ws = torch.empty(C.attn_decode_split_ws(B, H, Smax), dtype=torch.float32, device=dev)
    if Hkv == H:
        single = lambda i: C.attn_decode(qkv, kv[i % n], p, out, H, 0.125)
    else:
        single = lambda i: C.attn_decode_gqa(qkv, kv[i % n], p, out, H, 0.125)
    split = lambda i: C.attn_decode_split(qkv, kv[i % n], p, out, ws, H, 0.125)
    iters = args.iters if pos < 8192 else max(8, args.iters // 4)  # long caches: fewer, longer launches
    runs = _time_round_robin({"single": single, "split": split}, iters, args.repeats)
    nbytes = 2 * B * Hkv * pos * 64 * 2
    rec.update(iters=iters, bytes=nbytes)
    for name, r in runs.items():
        us = statistics.median(r)
        rec.update({f"{name}_us": us, f"{name}_spread": (max(r) - min(r)) / us, f"{name}_tb_per_s": nbytes / us * 1e-6,
                    f"{name}_runs": r})
    rec["speedup"] = rec["single_us"] / rec["split_us"]
    print(json.dumps(rec), flush=True)
    del kv
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-variants", action="store_true", help="build the --variant-keys candidates and exit (no GPU)")
    ap.add_argument("--variant-keys", default="512,1024")
    ap.add_argument("--ext", default="", help="a variant build to time instead of the in-tree extension")
    ap.add_argument("--batch", default="1,8,64")
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--kv-heads", default="12,4,1")
    ap.add_argument("--pos", default="511,2047,8191,32767")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cold-mb", type=int, default=768)
    ap.add_argument("--max-gb", type=int, default=64)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.build_variants:
        return build_variants([int(k) for k in args.variant_keys.split(",")])
    if args.repeats < 5:
        raise SystemExit("--repeats: medians of at least 5")
    C, dev = load_ext(args.ext), torch.device("cuda", 0)
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
