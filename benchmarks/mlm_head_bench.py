"""The masked-LM head alone: forward + backward of ``ops.mlm.mlm_head`` (select / gather / transform /
chunked vocabulary GEMMs + ``vocab_ce`` / scatter) against the PyTorch-eager bf16 head on the same weights
and rows (``torch.autocast``: F.linear + GELU + LayerNorm + F.linear onto the vocabulary + F.cross_entropy
over the full [R, V] logits).

    python benchmarks/mlm_head_bench.py                           # bench shape: batch 1536, seq 512, 80 slots
    python benchmarks/mlm_head_bench.py --chunk-rows 2048,4096,8192,16384 --impl native
    python benchmarks/mlm_head_bench.py --batch 256 --impl both   # a size at which the eager head fits

Every configuration (each ``chunk_rows`` of the native head, the eager head) is timed ``--repeats`` times,
alternated, and reported as the median: one JSON line each with ms (forward + backward) and the peak of
``torch.cuda.max_memory_allocated`` above what was allocated before the head ran. An eager head that runs
out of memory is recorded as such. Synthetic hidden states and weights (no network).
"""
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
import torch.nn.functional as F  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1536)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--max-predictions", type=int, default=0, help="slots per sequence (default: ceil(0.15 seq) up to 8)")
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--chunk-rows", default="", help="comma-separated chunk sizes of the native head (default: the "
                    "library default)")
    ap.add_argument("--impl", choices=["native", "torch", "both"], default="both")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from ml_trainer_amd.data.text import SyntheticMaskedLM
    from ml_trainer_amd.ops import mlm as M
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    B, S, h, V = args.batch, args.seq, args.hidden, args.vocab
    P = args.max_predictions or M.default_max_predictions(S)
    R = M.slot_rows(B, P)
    ds = SyntheticMaskedLM(B, seq_len=S, vocab_size=V, max_predictions=P, seed=1)
    labels = ds.labels.to(dev)
    hidden = torch.randn(B * S, h, device=dev).to(torch.bfloat16).requires_grad_()
    ps = [torch.randn(h, h, device=dev) * 0.02, torch.zeros(h, device=dev), torch.ones(h, device=dev),
          torch.zeros(h, device=dev), torch.randn(V, h, device=dev) * 0.02, torch.zeros(V, device=dev)]
    ps = [p.requires_grad_() for p in ps]
    params = M.MLMParams(*ps, 1e-12)

    def clear():
        hidden.grad = None
        for p in ps:
            p.grad = None

    def native(chunk):
        def f():
            clear()
            out = M.mlm_head(hidden, labels, P, params, chunk_rows=chunk)
            out.loss.backward()
            return out.loss
        return f

    def eager():
        clear()
        slot_row, slot_label, _ = M.select_reference(labels, P)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            x = M.gather_reference(hidden, slot_row)
            t = F.layer_norm(F.gelu(F.linear(x, ps[0], ps[1])), (h,), ps[2], ps[3], 1e-12)
            logits = F.linear(t, ps[4], ps[5])
            n = (slot_label != -100).sum().clamp(min=1)
            loss = F.cross_entropy(logits.float(), slot_label, ignore_index=-100, reduction="sum") / n
        loss.backward()
        return loss

    chunks = [int(c) for c in args.chunk_rows.split(",") if c] or [M.DEFAULT_CHUNK_ROWS]
    configs = []
    if args.impl in ("native", "both"):
        configs += [(f"native chunk_rows={c}", native(c), c) for c in chunks]
    if args.impl in ("torch", "both"):
        configs.append(("torch eager bf16", eager, None))

    M.padded_decoder(ps[4], ps[5])  # (the padded table is a per-update cache, not part of a step)
    results = {name: {"ms": [], "peak": [], "loss": None, "error": None} for name, _, _ in configs}
    for _ in range(args.repeats):
        for name, fn, _ in configs:
            r = results[name]
            if r["error"]:
                continue
            try:
                clear()
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                for _ in range(args.warmup):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    loss = fn()
                torch.cuda.synchronize()
                r["ms"].append((time.perf_counter() - t0) / args.steps * 1e3)
                r["peak"].append(torch.cuda.max_memory_allocated() - base)
                r["loss"] = float(loss.detach())
            except torch.OutOfMemoryError as e:
                r["error"] = "out of memory: " + str(e).split("\n")[0][:160]
                clear()
                torch.cuda.empty_cache()
    recs = []
    for name, _, chunk in configs:
        r = results[name]
        rec = {"bench": "mlm_head", "impl": name, "chunk_rows": chunk, "batch": B, "seq": S, "max_predictions": P,
               "rows": R, "targets": int((labels != -100).sum()), "hidden": h, "vocab": V,
               "ms": statistics.median(r["ms"]) if r["ms"] else None, "ms_runs": r["ms"],
               "peak_bytes": max(r["peak"]) if r["peak"] else None, "full_logits_bytes": R * V * 2,
               "loss": r["loss"], "error": r["error"]}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if args.out:
        with open(args.out, "a") as f:
            for rec in recs:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
