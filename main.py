"""CLI entrypoint (reference ``main.py:1-84``): same flags and defaults.

    python main.py --optimizer sgd --lr 0.001 --momentum 0.9 --backend smddp ...
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 main.py ...

Fixes over the reference: ``--epochs`` / ``--batch_size``
are honoured (the reference hard-codes 250 / 32), ``--custom_function`` parses
booleans properly, the SageMaker ``SM_*`` environment variables are optional
(defaults: model_dir ``model_output``, data_dir ``cifar10-dataset``), and a
dataset without transform yields tensors instead of crashing default_collate.
When ``--data_dir`` holds no CIFAR-10 batches (there is no network to download
them) ``--synthetic`` (or a missing directory) falls back to a seeded synthetic
CIFAR-shaped dataset and says so in the log.

Extension flags (not in the reference): ``--model`` (default/tiny/bert-base/
large), ``--synthetic``, ``--per_device_batch``, ``--no_engine``,
``--no_parallel``, ``--resume``, ``--amp bf16``, ``--precision bf16``, ``--metrics_jsonl``, ``--log_jsonl``, ``--zero_stage``, ``--async_checkpoint``,
``--dropout`` (BERT hidden dropout), ``--attention_dropout`` (BERT attention-probability dropout,
inside the flash attention kernels; applied as round(p * 256) / 256), ``--unpad`` (BERT: drop the pad
tokens before the embeddings and run the encoder on the real tokens only), ``--rotary`` / ``--rope_base`` (BERT,
any ``--task``: rotary position embeddings on the queries and keys instead of the learned position table),
``--pre_ln`` / ``--norm {layernorm,rmsnorm}`` (BERT, any ``--task``: pre-norm blocks ``h + f(norm(h))`` with a final
norm, and RMSNorm instead of LayerNorm as their norm; ``--norm rmsnorm`` needs ``--pre_ln``),
``--min_seq_len L``
(variable-length synthetic text, lengths uniform in [L, seq_len], right-padded with ``--pad_id``), ``--optimizer lamb`` (layer-wise trust ratios on the flat buffer) and
``--no_decay_1d`` (adamw / lamb: biases and LayerNorm parameters take no weight decay), ``--task mlm``
(BERT masked-LM pre-training on synthetic masked text: criterion ``mlm``, ``--metric accuracy`` is the
masked-token accuracy; ``--mask_prob``, ``--max_predictions``), ``--task clm`` (BERT run as a causal
language model on synthetic next-token text: causal flash attention, criterion ``clm``, ``--metric accuracy``
is the next-token accuracy), ``--generate N`` (``--task clm``: after training, rank 0 continues up to 8
validation rows from their first ``--prompt_len`` tokens by N tokens with the key/value cache, logs a
``generate`` record with the ``continuation_accuracy`` and writes ``model_dir/generated.json``;
``--temperature`` / ``--top_k`` sample instead of the greedy argmax; ``--sampler device`` takes the on-device
sampler, which adds ``--top_p`` and, with ``--graph_decode``, a decode loop replayed from one captured graph).
"""
from __future__ import annotations

import argparse
import json
import os

from ml_trainer_amd.utils.logging import get_logger

logger = get_logger("main")


def str2bool(v) -> bool:
    if isinstance(v, bool):
        return v
    s = str(v).strip().lower()
    if s in ("1", "true", "t", "yes", "y"):
        return True
    if s in ("0", "false", "f", "no", "n", "none", ""):
        return False
    raise argparse.ArgumentTypeError(f"boolean expected, got {v!r}")


def build_datasets(args):
    from ml_trainer_amd.data.cifar10 import CIFAR10, SyntheticCIFAR10
    tf = None
    if args.custom_function:
        from ml_trainer_amd.utils.functions import custom_pre_process_function
        tf = custom_pre_process_function()
    use_synth = args.synthetic
    if not use_synth:
        try:
            train_set = CIFAR10(root=args.data_dir, train=True, download=False, transform=tf)
            val_set = CIFAR10(root=args.data_dir, train=False, download=False, transform=tf)
            return train_set, val_set
        except FileNotFoundError as e:
            logger.warning("CIFAR-10 not found; using synthetic CIFAR-shaped data", error=str(e))
    n_train = args.synthetic_size or 50000
    return (SyntheticCIFAR10(n_train, train=True, transform=tf, seed=args.seed),
            SyntheticCIFAR10(max(n_train // 5, 1), train=False, transform=tf, seed=args.seed))


def build_model_and_datasets(args):
    """(model, (train set, validation set)) of the parsed flags; flag combinations that make no sense raise."""
    import torch
    from ml_trainer_amd.models import build_model
    torch.manual_seed(args.seed)
    lenet = args.model in ("default", "tiny", "lenet")
    if lenet and args.dropout:
        raise ValueError("--dropout applies to the BERT models; the LeNet models have no dropout")
    if lenet and args.attention_dropout:
        raise ValueError("--attention_dropout applies to the BERT models; the LeNet models have no attention")
    if lenet and args.unpad:
        raise ValueError("--unpad applies to the BERT models; the LeNet models have no sequences to unpad")
    if lenet and (args.rotary or args.rope_base is not None):
        raise ValueError("--rotary / --rope_base apply to the BERT models; the LeNet models have no positions")
    if args.rope_base is not None and not args.rotary:
        raise ValueError("--rope_base applies to --rotary")
    if args.rope_base is not None and not args.rope_base > 0:
        raise ValueError(f"--rope_base must be > 0, got {args.rope_base}")
    if lenet and (args.pre_ln or args.norm != "layernorm"):
        raise ValueError("--pre_ln / --norm apply to the BERT models; the LeNet models have no transformer blocks")
    if args.norm == "rmsnorm" and not args.pre_ln:
        raise ValueError("--norm rmsnorm needs --pre_ln: post-norm RMSNorm blocks are not built")
    if lenet and args.min_seq_len is not None:
        raise ValueError("--min_seq_len applies to the synthetic text data of the BERT models")
    mlm = args.task == "mlm"
    clm = args.task == "clm"
    if lenet and (mlm or clm):
        raise ValueError(f"--task {args.task} applies to the BERT models; the LeNet models classify images")
    if not mlm and (args.mask_prob is not None or args.max_predictions is not None):
        raise ValueError("--mask_prob / --max_predictions apply to --task mlm (BERT models)")
    if args.generate and not clm:
        raise ValueError("--generate applies to --task clm (the causal language model)")
    if not args.generate and (args.temperature is not None or args.top_k is not None):
        raise ValueError("--temperature / --top_k apply to --generate")
    if not args.generate and (args.top_p is not None or args.sampler is not None or args.graph_decode):
        raise ValueError("--top_p / --sampler / --graph_decode apply to --generate")
    if args.top_p is not None and args.sampler != "device":
        raise ValueError("--top_p needs --sampler device (nucleus sampling is part of the on-device sampler)")
    if args.top_p is not None and not 0.0 < args.top_p <= 1.0:
        raise ValueError(f"--top_p must satisfy 0 < top_p <= 1, got {args.top_p}")
    if args.graph_decode and args.sampler != "device":
        raise ValueError("--graph_decode needs --sampler device (the torch sampler cannot be captured)")
    if args.generate and (args.generate < 0 or args.prompt_len < 1):
        raise ValueError("--generate and --prompt_len must be positive")
    over = {"hidden_dropout": args.dropout} if args.dropout else {}
    if args.attention_dropout:
        over["attention_dropout"] = args.attention_dropout
    if args.unpad:
        over["unpad"] = True
    if args.rotary:
        over["rotary"] = True
        if args.rope_base is not None:
            over["rope_base"] = args.rope_base
    if args.pre_ln:
        over["pre_ln"] = True
        over["norm"] = args.norm
    pad_id = args.pad_id if args.pad_id is not None else (0 if args.min_seq_len is not None else None)
    if pad_id is not None and not lenet:
        over["pad_id"] = pad_id
    if mlm and args.max_predictions is not None:
        over["max_predictions"] = args.max_predictions
    model = build_model(args.model, task=args.task, **over)
    if lenet:
        datasets = build_datasets(args)
    else:  # BERT configs: synthetic token classification (no network for GLUE downloads)
        from ml_trainer_amd.data.text import SyntheticTextClassification
        c = model.config
        seq = min(args.seq_len, c.max_position)
        if args.generate and args.prompt_len + args.generate > seq:
            raise ValueError(f"--prompt_len + --generate = {args.prompt_len + args.generate} exceeds the sequence "
                             f"length {seq}")
        n = args.synthetic_size or 4096
        var = {} if args.min_seq_len is None else {"min_len": min(args.min_seq_len, seq), "pad_id": pad_id}
        if clm:
            from ml_trainer_amd.data.text import SyntheticCausalLM
            kw = dict(seq_len=seq, vocab_size=c.vocab_size, **var)
            return model, (SyntheticCausalLM(n, seed=args.seed, **kw),
                           SyntheticCausalLM(max(n // 8, 1), seed=args.seed + 1, **kw))
        if mlm:
            from ml_trainer_amd.data.text import SyntheticMaskedLM
            kw = dict(seq_len=seq, vocab_size=c.vocab_size, mask_prob=0.15 if args.mask_prob is None else args.mask_prob,
                      max_predictions=model.max_predictions(seq), **var)
            return model, (SyntheticMaskedLM(n, seed=args.seed, **kw),
                           SyntheticMaskedLM(max(n // 8, 1), seed=args.seed + 1, **kw))
        datasets = (SyntheticTextClassification(n, seq_len=seq, vocab_size=c.vocab_size, num_labels=c.num_labels,
                                                seed=args.seed, learnable=True, **var),
                    SyntheticTextClassification(max(n // 8, 1), seq_len=seq, vocab_size=c.vocab_size,
                                                num_labels=c.num_labels, seed=args.seed + 1, learnable=True, **var))
    return model, datasets


def main(args):
    from ml_trainer_amd.trainer import Trainer
    model, datasets = build_model_and_datasets(args)
    config = {
        "seed": args.seed,
        "scheduler": args.scheduler,
        "optimizer": args.optimizer,
        "momentum": args.momentum,
        "weight_decay": args.weight_decay,
        "lr": args.lr,
        "criterion": args.task if args.task in ("mlm", "clm") else args.criterion,
        "pred_function": args.pred_function,
        "metric": args.metric,
        "model_dir": args.model_dir,
        "backend": args.backend,
    }
    options = {"per_device_batch": args.per_device_batch, "resume": args.resume,
               "metrics_jsonl": args.metrics_jsonl, "amp": args.amp, "progress": not args.no_progress,
               "precision": getattr(args, "precision", "fp32"),
               "zero_stage": args.zero_stage, "async_checkpoint": args.async_checkpoint,
               "no_decay_1d": getattr(args, "no_decay_1d", False)}
    if args.no_engine:
        options["use_engine"] = False
    if args.log_jsonl:  # every structured log record, one JSON object per line
        from ml_trainer_amd.utils.logging import add_jsonl_sink
        add_jsonl_sink(args.log_jsonl)
    trainer = Trainer(model, datasets=datasets, epochs=args.epochs, batch_size=args.batch_size,
                      is_parallel=not args.no_parallel, save_history=True, options=options, **config)
    trainer.fit()
    if args.generate and trainer.rank == 0:
        generate_after_fit(args, trainer, datasets[1])
    return trainer


def generate_after_fit(args, trainer, val_set, rows: int = 8):
    """Rank 0 only, no collective: prompt with the first min(--prompt_len, len_b) tokens of up to ``rows``
    validation rows, generate --generate tokens, log a ``generate`` record and write model_dir/generated.json.
    ``continuation_accuracy``: the share of generated tokens equal to the row's own next tokens, where it has them."""
    import torch
    model = trainer.model
    while not hasattr(model, "generate") and hasattr(model, "module"):
        model = model.module  # the data-parallel wrapper
    n = min(rows, len(val_set))
    ids, lengths = val_set.ids[:n], val_set.lengths[:n]
    P, N = args.prompt_len, args.generate
    plens = lengths.clamp(max=P)
    mask = (torch.arange(P)[None, :] < plens[:, None]).long()
    dev = trainer.device
    tokens, _ = model.generate(ids[:, :P].to(dev), N, attention_mask=mask.to(dev),
                               temperature=args.temperature or 0.0, top_k=args.top_k, seed=args.seed,
                               top_p=args.top_p, sampler=args.sampler,
                               graph=args.graph_decode and dev.type == "cuda")
    tokens = tokens.cpu()
    at = plens[:, None] + torch.arange(N)[None, :]  # where the continuation sits in the row
    has = at < lengths[:, None]
    want = ids.gather(1, at.clamp(max=ids.shape[1] - 1))
    hits, total = int(((tokens == want) & has).sum()), int(has.sum())
    acc = hits / total if total else 0.0
    logger.info("generate", rows=n, prompt_len=P, new_tokens=N, continuation_accuracy=acc, compared=total)
    os.makedirs(args.model_dir, exist_ok=True)
    with open(os.path.join(args.model_dir, "generated.json"), "w") as f:
        json.dump({"prompts": [ids[b, :int(plens[b])].tolist() for b in range(n)], "tokens": tokens.tolist(),
                   "continuation_accuracy": acc, "compared": total}, f)


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    parser.add_argument("--batch_size", type=int, default=32, help="input batch size for training (default: 32)")
    parser.add_argument("--epochs", type=int, default=10, help="number of epochs to train (default: 10)")
    parser.add_argument("--optimizer", type=str, default="sgd",
                        help="optimizer for backward pass: sgd|adam|adagrad|adamax|adamw|lamb (default: sgd)")
    parser.add_argument("--lr", type=float, default=0.001, help="learning rate (default: 0.001)")
    parser.add_argument("--momentum", type=float, default=0.9, help="Optimizer momentum (default: 0.9)")
    parser.add_argument("--weight_decay", type=float, default=0.0, help="Optimizer weight decay (default: 0.0)")
    parser.add_argument("--seed", type=int, default=32, help="random seed (default: 32)")
    parser.add_argument("--scheduler", type=str, default=None,
                        help="apply scheduler for learning rate (default: None)")
    parser.add_argument("--criterion", type=str, default="cross_entropy",
                        help="loss function to apply (default: cross_entropy)")
    parser.add_argument("--metric", type=str, default=None, help="metric for model evaluation (default: None)")
    parser.add_argument("--backend", type=str, default="smddp",
                        help="backend for dist. training: smddp|rccl|nccl (RCCL over xGMI) or gloo")
    parser.add_argument("--custom_function", type=str2bool, default=False,
                        help="apply a pre-processing function (default: False)")
    parser.add_argument("--pred_function", type=str, default=None,
                        help="probability function to apply to make predictions (default: None)")
    # SageMaker environment (optional here)
    parser.add_argument("--hosts", type=json.loads, default=json.loads(os.environ.get("SM_HOSTS", "[]")))
    parser.add_argument("--current-host", type=str, default=os.environ.get("SM_CURRENT_HOST", "localhost"))
    parser.add_argument("--model_dir", type=str, default=os.environ.get("SM_MODEL_DIR", "model_output"))
    parser.add_argument("--data_dir", type=str, default=os.environ.get("SM_CHANNEL_TRAIN", "cifar10-dataset"))
    # extensions
    parser.add_argument("--model", type=str, default="default", help="default|tiny|bert-base|large")
    parser.add_argument("--dropout", type=float, default=0.0,
                        help="BERT hidden dropout probability (embedding, attention-output and FFN-output "
                             "sites; default: 0.0). An error for the LeNet models")
    parser.add_argument("--attention_dropout", type=float, default=0.0,
                        help="BERT attention-probability dropout, inside the flash attention kernels (default: "
                             "0.0). One random byte per probability: p is applied as p_eff = round(p * 256) / 256 "
                             "(0.1 -> 26/256 = 0.1015625), kept probabilities scaled by 1 / (1 - p_eff). An error "
                             "for the LeNet models")
    parser.add_argument("--unpad", action="store_true",
                        help="BERT: drop the pad tokens once, before the embeddings, and run the encoder on the real "
                             "tokens only (needs lengths: --pad_id / --min_seq_len; one small device-to-host read "
                             "per forward; not with the fp8 `large` model). An error for the LeNet models")
    parser.add_argument("--rotary", action="store_true",
                        help="BERT, any --task: rotary position embeddings (queries and keys rotated by their "
                             "position, attention scores depend on i - j only) instead of the learned position "
                             "table; the model then has no position_embeddings.weight (not with the fp8 `large` "
                             "preset). An error for the LeNet models")
    parser.add_argument("--rope_base", type=float, default=None,
                        help="--rotary: the base of the angles, position p and pair i turn by "
                             "p * base ** (-2 i / 64) (default: 10000)")
    parser.add_argument("--pre_ln", action="store_true",
                        help="BERT, any --task: pre-norm blocks h + f(norm(h)) and a final norm (final_ln) instead "
                             "of the post-LN blocks (not with the fp8 `large` preset). An error for the LeNet models")
    parser.add_argument("--norm", choices=["layernorm", "rmsnorm"], default="layernorm",
                        help="--pre_ln: the norm of the blocks and the final norm; rmsnorm = x * rsqrt(mean(x^2) + "
                             "eps) * weight, no centring, no bias (needs --pre_ln)")
    parser.add_argument("--min_seq_len", type=int, default=None,
                        help="BERT synthetic data: variable-length rows, lengths uniform in [min_seq_len, seq_len], "
                             "right-padded with --pad_id (default: fixed length)")
    parser.add_argument("--pad_id", type=int, default=None,
                        help="BERT: token id of the right padding (key lengths are derived from it); defaults to 0 "
                             "when --min_seq_len is given")
    parser.add_argument("--no_decay_1d", action="store_true",
                        help="--optimizer adamw|lamb: no weight decay (lamb: and no trust ratio) on parameters with "
                             "ndim <= 1, i.e. biases and LayerNorm weight / bias. An error for the other optimizers "
                             "and with --zero_stage 1")
    parser.add_argument("--task", type=str, default="classify", choices=["classify", "mlm", "clm"],
                        help="BERT models: classify (default), mlm (masked-LM pre-training on synthetic masked "
                             "text with the fused vocabulary cross-entropy head) or clm (causal language model: "
                             "causal attention and next-token prediction on synthetic text; not with the fp8 "
                             "`large` preset). mlm and clm are errors for the LeNet models")
    parser.add_argument("--mask_prob", type=float, default=None,
                        help="--task mlm: share of each row's real tokens chosen as targets (default: 0.15)")
    parser.add_argument("--max_predictions", type=int, default=None,
                        help="--task mlm: target slots per sequence (default: ceil(0.15 * seq_len) rounded up to 8)")
    parser.add_argument("--generate", type=int, default=0,
                        help="--task clm: after training, generate this many tokens for up to 8 validation rows "
                             "(default: 0, off)")
    parser.add_argument("--prompt_len", type=int, default=8,
                        help="--generate: tokens of each row used as the prompt (default: 8)")
    parser.add_argument("--temperature", type=float, default=None,
                        help="--generate: sample from softmax(logits / temperature) (default: greedy argmax)")
    parser.add_argument("--top_k", type=int, default=None,
                        help="--generate with --temperature: restrict the draw to the k largest logits")
    parser.add_argument("--synthetic", action="store_true", help="use the seeded synthetic dataset")
    parser.add_argument("--top_p", type=float, default=None,
                        help="--generate with --sampler device: nucleus sampling inside the top-k set, applied as "
                             "round(top_p * 65536) / 65536")
    parser.add_argument("--sampler", choices=["device"], default=None,
                        help="--generate: 'device' samples with the sample_step kernel (reproducible, independent "
                             "of the batch); default: the torch sampler")
    parser.add_argument("--graph_decode", action="store_true",
                        help="--generate with --sampler device on a GPU: replay one captured graph per token")
    parser.add_argument("--synthetic_size", type=int, default=0)
    parser.add_argument("--seq_len", type=int, default=512)
    parser.add_argument("--per_device_batch", action="store_true",
                        help="batch_size is per GPU (weak scaling) instead of global")
    parser.add_argument("--no_engine", action="store_true", help="disable the fused LeNet step engine")
    parser.add_argument("--no_parallel", action="store_true", help="do not initialise torch.distributed")
    parser.add_argument("--resume", action="store_true")
    parser.add_argument("--async_checkpoint", action="store_true",
                        help="write model.pth / trainer_state.pt from a pinned-host snapshot in a background thread")
    parser.add_argument("--zero_stage", type=int, default=0, choices=(0, 1),
                        help="1: ZeRO-1 sharded optimizer state (reduce-scatter / all-gather) under DDP")
    parser.add_argument("--amp", type=str, default=None, choices=[None, "bf16"])
    parser.add_argument("--precision", type=str, default="fp32", choices=["fp32", "bf16"],
                        help="fused LeNet step: fp32 (reference dtype) or bf16 MFMA (fp32 masters)")
    parser.add_argument("--metrics_jsonl", type=str, default=None)
    parser.add_argument("--log_jsonl", type=str, default=None, help="mirror log records into this JSON-lines file")
    parser.add_argument("--no_progress", action="store_true")
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
