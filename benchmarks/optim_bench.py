"""Optimizer step alone on a model's flat parameter layout (default BERT-base, with the bf16 shadow):

    adamw        one flat_optim launch (AdamW, one decay for every element)
    adamw_seg    one flat_optim_seg launch (AdamW, decay per tensor through the segment table)
    lamb         the three LAMB launches; also stage 1, finalize and stage 2 each on their own

    python benchmarks/optim_bench.py --rounds 7 --iters 20 --out profiles/lamb/optim_step.jsonl

The implementations alternate inside every round; a figure is the median over the rounds of the mean
time of ``iters`` back-to-back launches (HIP events around the batch). Bytes per element by
construction: AdamW reads p, g, m, v and writes p, m, v and the 2-byte shadow = 30; LAMB stage 1 reads
p, g, m, v and writes m, v = 24, stage 2 reads p, m, v and writes p and the shadow = 18. Prints one JSON
line per implementation.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bert-base")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from ml_trainer_amd.models.bert import BertClassifier, bert_config
    from ml_trainer_amd.ops._ext import require_native
    from ml_trainer_amd.ops.optim import SegmentTable
    from ml_trainer_amd.utils.flat import FlatParams
    C = require_native()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = BertClassifier(bert_config(args.model)).to(dev)
    fp = FlatParams(model.parameters())
    shadow = fp.refresh_shadow()
    no_decay = [p for p in fp.params if p.ndim <= 1]
    seg = SegmentTable(fp, 0.01, no_decay, adapt=True)
    d = seg.dev
    for o, n in seg.segments:  # the gaps keep g = 0
        fp.grad[o:o + n].normal_(0.0, 1e-3)
    m, v = torch.zeros_like(fp.data), torch.zeros_like(fp.data)
    seg_elems = sum((n + 3) // 4 * 4 for _, n in seg.segments)
    lr, b1, b2 = 1e-4, 0.9, 0.999

    def adamw():
        C.flat_optim(fp.data, fp.grad, m, v, 2, lr, 0.0, 0.0, 0.01, b1, b2, 1e-8, 0.0, 1.0, False, False, None, None,
                     None, 1.0, shadow, None)

    def adamw_seg():
        C.flat_optim_seg(fp.data, fp.grad, m, v, d["chunks"], d["wd"], lr, b1, b2, 1e-8, 1.0, False, None, None, None,
                         1.0, shadow, None, None, 0)

    def lamb(stages):
        def run():
            C.lamb_step(fp.data, fp.grad, m, v, d["chunks"], d["tseg"], d["wd"], d["adapt"], d["part"], d["norms"],
                        seg.last_trust, lr, b1, b2, 1e-6, 1.0, False, None, None, None, 1.0, shadow, None, None, 0,
                        stages)
        return run

    # name -> (launcher, elements touched, bytes per element)
    impls = {"adamw": (adamw, fp.numel, 30), "adamw_seg": (adamw_seg, seg_elems, 30),
             "lamb": (lamb(7), seg_elems, 42), "lamb_stage1": (lamb(1), seg_elems, 24),
             "lamb_finalize": (lamb(2), 0, 0), "lamb_stage2": (lamb(4), seg_elems, 18)}
    times = {k: [] for k in impls}
    for fn, _, _ in impls.values():  # warm-up: module load, caches
        fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, (fn, _, _) in impls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / args.iters)
    recs = []
    for name, (_, elems, bpe) in impls.items():
        us = statistics.median(times[name])
        rec = {"bench": "optim_step", "impl": name, "model": args.model, "elements": elems, "tensors": len(seg.segments),
               "chunks": int(d["chunks"].shape[0]), "bytes_per_element": bpe, "us": us, "us_min": min(times[name]),
               "us_max": max(times[name]), "tb_per_s": elems * bpe / us / 1e6, "rounds": args.rounds,
               "iters": args.iters}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
