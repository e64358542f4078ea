"""Train a small causal language model on arithmetic progressions, then let it continue some.

``SyntheticCausalLM`` rows are ``5 + (a + t * d) mod (vocab - 5)`` with d in {1, 2, 3}: the next token follows
from the two before it. ``bert-tiny`` (``BertLMHeadModel``: causal attention, next-token head) is trained for a few
hundred steps; ``generate`` then continues validation rows from their first ``--prompt_len`` tokens with the
key/value cache (on the GPU: one ``attn_decode`` kernel per layer per token) and the continuations are compared
with the rows' own next tokens. Runs on the CPU or the GPU.

    python examples/04_generate.py [--steps 300] [--prompt_len 8] [--new 16] [--temperature 0]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=300)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--seq_len", type=int, default=32)
    p.add_argument("--prompt_len", type=int, default=8)
    p.add_argument("--new", type=int, default=16)
    p.add_argument("--rows", type=int, default=8)
    p.add_argument("--temperature", type=float, default=0.0)
    p.add_argument("--top_k", type=int, default=None)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--seed", type=int, default=0)
    args = p.parse_args(argv)
    if args.prompt_len + args.new > args.seq_len:
        raise ValueError("--prompt_len + --new must not exceed --seq_len")
    from ml_trainer_amd.data.text import SyntheticCausalLM
    from ml_trainer_amd.models import build_model
    from ml_trainer_amd.trainer import Trainer
    torch.manual_seed(args.seed)
    model = build_model("bert-tiny", task="clm")
    V = model.config.vocab_size
    train = SyntheticCausalLM(args.steps * args.batch_size, seq_len=args.seq_len, vocab_size=V, seed=args.seed)
    val = SyntheticCausalLM(args.rows, seq_len=args.seq_len, vocab_size=V, seed=args.seed + 1)
    tr = Trainer(model, datasets=(train, val), epochs=1, batch_size=args.batch_size, optimizer="adamw", lr=args.lr,
                 criterion="clm", metric="accuracy", is_parallel=False, options={"progress": False})
    for i in range(args.steps):
        lo = i * args.batch_size
        loss = tr.train_step((train.ids[lo:lo + args.batch_size], train.labels[lo:lo + args.batch_size]))
        if i % 50 == 0 or i == args.steps - 1:
            print(f"step {i:4d}  loss {float(loss):.4f}")
    P, N = args.prompt_len, args.new
    tokens, _ = tr.model.generate(val.ids[:, :P].to(tr.device), N, temperature=args.temperature, top_k=args.top_k,
                                  seed=args.seed)
    tokens = tokens.cpu()
    want = val.ids[:, P:P + N]
    for b in range(val.ids.shape[0]):
        marks = "".join("." if int(tokens[b, t]) == int(want[b, t]) else "x" for t in range(N))
        print(f"prompt {val.ids[b, :P].tolist()} -> {tokens[b].tolist()}  {marks}")
    acc = float((tokens == want).float().mean())
    print(f"continuation accuracy {acc:.3f} over {want.numel()} tokens")
    # nucleus sampling with the on-device sampler (reproducible for a seed, independent of the batch); on a GPU the
    # decode loop is one captured graph replayed per token
    on_gpu = tr.device.type == "cuda"
    sampled, _ = tr.model.generate(val.ids[:, :P].to(tr.device), N, temperature=0.7, top_k=20, top_p=0.9,
                                   seed=args.seed, sampler="device", graph=on_gpu)
    print(f"top-p 0.9 / top-k 20 / temperature 0.7{' (graph replay)' if on_gpu else ''}: row 0 -> "
          f"{sampled[0].tolist()}  agreement with the row {float((sampled.cpu() == want).float().mean()):.3f}")
    return acc


if __name__ == "__main__":
    main()
