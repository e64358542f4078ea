"""BERT classifier training-step benchmark (BASELINE.json configs 4/5: BERT-base
seq 512 bf16; "large" fp8) on one GPU, native kernels vs a PyTorch-eager bf16
baseline of the same model (torch.autocast + SDPA + hipBLASLt) for comparison.

    python benchmarks/bert_bench.py --model bert-base --batch 16 --seq 512 --steps 10
    python benchmarks/bert_bench.py --impl torch      # eager PyTorch baseline
    python benchmarks/bert_bench.py --impl native --dropout 0.1   # hidden dropout in the LayerNorm kernels
    python benchmarks/bert_bench.py --impl native --attention-dropout 0.1   # ... in the flash attention kernels
    python benchmarks/bert_bench.py --impl native --min-len 64            # variable-length rows, right-padded
    python benchmarks/bert_bench.py --impl native --min-len 64 --unpad    # ... run on the real tokens only
    python benchmarks/bert_bench.py --impl native --optimizer lamb --no-decay-1d   # LAMB, biases / LayerNorm excluded
    python benchmarks/bert_bench.py --impl native --task mlm   # masked-LM pre-training step (fused vocabulary CE head)
    python benchmarks/bert_bench.py --impl native --task clm --rotary   # rotary positions instead of the learned table
    python benchmarks/bert_bench.py --impl native --task clm --pre-ln --norm rmsnorm   # pre-norm blocks, RMSNorm

Prints one JSON line per run (samples/s, tokens/s, ms/step, model TFLOP/s; ``tokens`` = the real
tokens T of the batch, ``fill`` = T / (batch * seq), ``unpad``; tokens/s and TFLOP/s count batch * seq).
Synthetic token ids, random-init weights (no network). ``--task mlm`` trains BertForMaskedLM on
SyntheticMaskedLM rows and adds ``head_ms`` / ``head_share`` (the MLM head's forward + backward alone on
the step's hidden states, timed after the steps) and ``max_predictions`` / ``chunk_rows``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def run(args):
    from ml_trainer_amd.models.bert import BertClassifier, BertForMaskedLM, BertLMHeadModel, bert_config
    from ml_trainer_amd.ops.optim import build_optimizer
    clm = args.task == "clm"
    mlm = args.task == "mlm" or clm  # (clm: the same head, one slot per position)
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    over = {"layers": args.layers} if args.layers else {}
    if args.dropout:
        over["hidden_dropout"] = args.dropout
    if args.attention_dropout:
        over["attention_dropout"] = args.attention_dropout
    if args.unpad:
        over["unpad"] = True
    if args.min_len:
        over["pad_id"] = 0
    if args.rotary:
        over["rotary"] = True
    if args.pre_ln or args.norm != "layernorm":
        over.update(pre_ln=bool(args.pre_ln), norm=args.norm)
    cfg = bert_config(args.model, **over)
    m = (BertLMHeadModel if clm else BertForMaskedLM if mlm else BertClassifier)(cfg).to(dev)
    if mlm and args.chunk_rows:
        m.mlm_chunk_rows = args.chunk_rows
    if args.impl == "native":
        # adamw without --no-decay-1d is FusedAdamW's plain flat launch, as this benchmark always ran it
        opt = build_optimizer(args.optimizer, m.parameters(), lr=1e-4, weight_decay=0.01,
                              no_decay_1d=args.no_decay_1d)
        fwd = m
    else:
        if args.optimizer != "adamw" or args.no_decay_1d:
            raise SystemExit("--optimizer / --no-decay-1d apply to --impl native")
        opt = torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=0.01, fused=True)
        fwd = m.forward_torch_bf16
    ids = torch.randint(5, cfg.vocab_size, (args.batch, args.seq), device=dev)
    real = args.batch * args.seq
    if args.min_len:  # lengths uniform in [min_len, seq] from a seeded generator, right-padded with id 0
        g = torch.Generator().manual_seed(1)
        lens = torch.randint(args.min_len, args.seq + 1, (args.batch,), generator=g).to(dev)
        ids[torch.arange(args.seq, device=dev)[None, :] >= lens[:, None]] = 0
        real = int(lens.sum())
    y = torch.randint(0, cfg.num_labels, (args.batch,), device=dev)
    if mlm:  # masked rows (80 / 10 / 10) of the learnable synthetic text (clm: unmasked, next-token labels)
        from ml_trainer_amd.data.text import SyntheticCausalLM, SyntheticMaskedLM
        var = {"min_len": args.min_len, "pad_id": 0} if args.min_len else {}
        if clm:
            ds = SyntheticCausalLM(args.batch, seq_len=args.seq, vocab_size=cfg.vocab_size, seed=1, **var)
        else:
            ds = SyntheticMaskedLM(args.batch, seq_len=args.seq, vocab_size=cfg.vocab_size, seed=1,
                                   max_predictions=m.max_predictions(args.seq), **var)
        ids, y = ds.ids.to(dev), ds.labels.to(dev)
        real = int(ds.lengths.sum())
        loss_fn = m.mlm_loss if args.impl == "native" else m.mlm_loss_torch_bf16
    else:
        def loss_fn(out, y):
            return F.cross_entropy(out, y)

    def step():
        opt.zero_grad(set_to_none=False)
        loss = loss_fn(fwd(ids), y)
        loss.backward()
        opt.step()
        return loss

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    tokens = args.batch * args.seq
    flops = m.flops_per_token(args.seq) * tokens
    rec = {"bench": "bert_train_step", "impl": args.impl, "model": args.model, "layers": cfg.layers,
           "batch": args.batch, "seq": args.seq, "dropout": args.dropout,
           "attention_dropout": args.attention_dropout, "ms_per_step": dt * 1e3, "samples_per_s": args.batch / dt,
           "tokens_per_s": tokens / dt, "model_tflops": flops / dt / 1e12, "loss": float(loss.detach()),
           "peak_mem_gb": torch.cuda.max_memory_allocated() / 2 ** 30,
           "min_len": args.min_len, "tokens": real, "fill": real / tokens, "unpad": bool(args.unpad),
           "optimizer": args.optimizer, "no_decay_1d": bool(args.no_decay_1d), "rotary": bool(args.rotary),
           "pre_ln": bool(args.pre_ln), "norm": args.norm}
    if mlm:
        with torch.no_grad():
            hidden = fwd(ids)
        hidden = hidden.detach().requires_grad_()

        def head():
            hidden.grad = None
            loss_fn(hidden, y).backward()

        for _ in range(2):
            head()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            head()
        torch.cuda.synchronize()
        hd = (time.perf_counter() - t0) / args.steps
        rec.update({"task": args.task, "head_ms": hd * 1e3, "head_share": hd / dt,
                    "max_predictions": m.max_predictions(args.seq), "chunk_rows": m.mlm_chunk_rows,
                    "mlm_accuracy": float(m.last_mlm_accuracy) if args.impl == "native" else None})
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bert-base")
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--impl", choices=["native", "torch", "both"], default="both")
    ap.add_argument("--dropout", type=float, default=0.0, help="hidden dropout probability (default 0.0)")
    ap.add_argument("--attention-dropout", type=float, default=0.0,
                    help="attention-probability dropout, applied as round(p * 256) / 256 (default 0.0)")
    ap.add_argument("--min-len", type=int, default=0,
                    help="variable-length rows: lengths uniform in [min-len, seq], right-padded (default: full rows)")
    ap.add_argument("--unpad", action="store_true", help="BertConfig.unpad: run the encoder on the real tokens only")
    ap.add_argument("--rotary", action="store_true",
                    help="BertConfig.rotary: rotary positions on q and k (the rope_qk kernel) instead of the learned table")
    ap.add_argument("--pre-ln", action="store_true", help="BertConfig.pre_ln: pre-norm blocks and a final norm")
    ap.add_argument("--norm", choices=["layernorm", "rmsnorm"], default="layernorm",
                    help="BertConfig.norm: the norm of the pre-norm blocks (rmsnorm needs --pre-ln)")
    ap.add_argument("--optimizer", choices=["adamw", "lamb"], default="adamw",
                    help="native optimizer: adamw (one flat launch) or lamb (three launches, layer-wise trust ratio)")
    ap.add_argument("--no-decay-1d", action="store_true",
                    help="no weight decay (lamb: no trust ratio) on biases and LayerNorm parameters (ndim <= 1)")
    ap.add_argument("--task", choices=["classify", "mlm", "clm"], default="classify",
                    help="classify: BertClassifier + cross-entropy; mlm: BertForMaskedLM + the fused MLM head; "
                         "clm: BertLMHeadModel (causal attention) + that head on every position's next token")
    ap.add_argument("--chunk-rows", type=int, default=0, help="--task mlm: rows of logits alive at once (default: "
                    "ops.mlm.DEFAULT_CHUNK_ROWS)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    recs = []
    for impl in (["native", "torch"] if args.impl == "both" else [args.impl]):
        args.impl = impl
        recs.append(run(args))
    if args.out:
        with open(args.out, "a") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
