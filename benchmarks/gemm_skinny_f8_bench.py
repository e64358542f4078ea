"""``C.gemm_skinny_f8`` against ``C.gemm_skinny`` (and the two gated forms) at the decode shapes of a model, on the GPU.

One JSON line per (kernel, N, K, M): median us per launch of ``--repeats`` timed windows of ``--iters`` launches,
the spread (max - min over the median), the weight bytes the launch must read and the TB/s they amount to. The two
kernels of a shape alternate window by window in one process, and every launch takes the next of ``n`` rotating
weight copies (``--cold-mb`` per kernel, bf16 and fp8 alike), so that the weights come from HBM as in a decode step
and not from the caches. ``--model bert-base`` adds the whole-model token time of graph-replayed decoding with and
without ``weights="fp8"``. Random operands (no network)."""
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


def _emit(rec, runs, nbytes):
    us = statistics.median(runs)
    rec.update(us=us, spread=(max(runs) - min(runs)) / us, bytes=nbytes, tb_per_s=nbytes / us * 1e-6, runs=runs)
    print(json.dumps(rec), flush=True)


def _copies(cold_mb, nbytes):
    return max(2, -(-cold_mb * (1 << 20) // nbytes))


def bench(C, dev, args, N, K, glu):
    """One (N, K): ``glu`` takes N = 2F rows of weight into F output columns on the gated kernels."""
    from ml_trainer_amd.ops.decode import weight_quantize_reference
    n16, n8 = _copies(args.cold_mb, N * K * 2), _copies(args.cold_mb, N * K)
    W16 = (torch.randn(n16, N, K, device=dev) * K ** -0.5).to(torch.bfloat16)
    codes, scales = weight_quantize_reference(torch.randn(N, K) * K ** -0.5)
    W8 = codes.to(dev)[None].repeat(n8, 1, 1)  # the values do not change the time: one quantised weight, n8 copies
    d = scales.to(dev)
    b = torch.randn(N, device=dev)
    for M in (int(m) for m in args.batch.split(",")):
        x = torch.randn(M, K, device=dev).to(torch.bfloat16)
        y = torch.empty(M, N // 2 if glu else N, dtype=torch.bfloat16, device=dev)
        if glu:
            variants = {"gemm_skinny_glu": lambda i: C.gemm_skinny_glu(x, W16[i % n16], y, bias=b),
                        "gemm_skinny_glu_f8": lambda i: C.gemm_skinny_glu_f8(x, W8[i % n8], d, y, bias=b)}
        else:
            variants = {"gemm_skinny": lambda i: C.gemm_skinny(x, W16[i % n16], y, bias=b),
                        "gemm_skinny_f8": lambda i: C.gemm_skinny_f8(x, W8[i % n8], d, y, bias=b)}
        for name, runs in _time_round_robin(variants, args.iters, args.repeats).items():
            _emit({"bench": name, "M": M, "N": N, "K": K}, runs, N * K * (1 if name.endswith("_f8") else 2))


def bench_model(dev, args):
    """Whole-model token time: ``--new - 1`` graph replays (decode step + sampler) after a ``--prompt`` wide prompt,
    ``weights=None`` and ``"fp8"`` alternating; us per token."""
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    m = BertLMHeadModel(bert_config(args.model)).to(dev).eval()
    P, T = args.prompt, args.new
    for B in (int(b) for b in args.model_batch.split(",")):
        ids = torch.randint(5, 1000, (B, P), device=dev)
        params = m._sampler_params(0.0, None, None, None, 0)
        decs = {w: m._graphed_decoder(B, P + T, T, dev, None, w) for w in (None, "fp8")}
        runs = {w: [] for w in decs}
        for r in range(args.repeats + 1):  # (the first round warms up)
            for w, dec in decs.items():
                first = dec.start(m, ids, None, params)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                dec.run(m, first)
                b.record()
                torch.cuda.synchronize()
                if r:
                    runs[w].append(a.elapsed_time(b) * 1e3 / (T - 1))
        for w, t in runs.items():
            us = statistics.median(t)
            print(json.dumps({"bench": "graph_token", "model": args.model, "weights": w or "bf16", "B": B, "prompt": P,
                              "new": T, "us": us, "spread": (max(t) - min(t)) / us, "runs": t}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="", help="also time whole-model graph-replayed tokens of this config")
    ap.add_argument("--model-batch", default="1,8")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--layers", default="2304:768,768:768,3072:768,768:3072", help="N:K of the decode linears")
    ap.add_argument("--glu-layers", default="6144:768", help="2F:K of the gated FFN1 (F = 3072 output columns)")
    ap.add_argument("--batch", default="1,8,16")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cold-mb", type=int, default=768)
    args = ap.parse_args()
    from ml_trainer_amd.ops._ext import require_native
    C, dev = require_native(), torch.device("cuda", 0)
    torch.manual_seed(0)
    for glu, specs in ((False, args.layers), (True, args.glu_layers)):
        for spec in filter(None, specs.split(",")):
            N, K = (int(v) for v in spec.split(":"))
            bench(C, dev, args, N, K, glu)
    if args.model:
        bench_model(dev, args)


if __name__ == "__main__":
    main()
