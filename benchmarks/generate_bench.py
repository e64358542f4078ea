"""Cached generation against the uncached baseline: ``BertLMHeadModel.prefill`` + ``decode_step`` (key/value
cache, the ``attn_decode`` kernel) against the native full causal forward of the growing sequence, once per token.

    python benchmarks/generate_bench.py                                   # bert-base, batch 1,8,64, 128 + 128
    python benchmarks/generate_bench.py --batch 64 --out profiles/generate/generate_bench.jsonl
    python benchmarks/generate_bench.py --kernel --batch 64 --pos 255     # attn_decode alone: microseconds, bytes/s
    python benchmarks/generate_bench.py --linear                          # gemm_skinny against gemm, decode shapes
    python benchmarks/generate_bench.py --ab --repeats 5                  # MLT_DECODE_GEMM=0 / 1 alternated
    rocprofv3 --kernel-trace --stats --output-format csv -d out -o decode -- \\
        python benchmarks/generate_bench.py --batch 8 --trace-steps 32    # per-kernel share of a decode step

Per batch one JSON line: prefill ms, ms per token over the decode steps (cached), ms per token of the uncached
baseline, tokens/s. The two are alternated ``--repeats`` times in the same process and reported as medians. The
loops feed greedy tokens and never read from the device; one synchronisation closes each timed region.
``--trace-steps N`` runs one prefill and N decode steps and nothing else (the workload of the profiler run).
``--kernel`` times ``C.attn_decode`` alone on a cache of ``--pos`` tokens per sequence, rotating over enough
caches to exceed the 256 MiB last-level cache, and reports the bytes of K and V it streams per second.
``--linear`` times ``C.gemm_skinny`` and ``C.gemm`` on the five bert-base decode linears (QKV, out-projection, FFN1,
FFN2, the padded vocabulary decoder) at M = 1, 8, 16, 32, 64, alternated, each rotating over enough weight copies to
exceed the last-level cache: microseconds per launch and weight bytes per second.
``--sampler-kernel`` times ``ops.decode.sample_step`` (one launch) against ``ops.decode.sample_tokens`` (torch ops)
alone on fp32 logits [B, 30720] with 30,522 valid columns, greedy / top-k 50 / top-p 0.9 / both (the torch sampler
has no top-p: null). One logits buffer, so the row is L2-resident as it is behind the decoder GEMM.
``--sampler-ab`` alternates three whole token loops (N samples, N - 1 decode steps, prefill outside the timed
region) in one process: eager with the torch sampler, eager with ``sample_step``, and the captured graph with
``sample_step``; medians, (max - min) / median of each, and the capture time, greedy and sampled.
``--sampler device`` / ``--graph`` select the loop of ``--trace-steps`` (the workload of a profiler run).
``--ab`` alternates the cached decode between ``MLT_DECODE_GEMM=0`` (the planner's GEMMs: the launches before the
skinny kernel) and ``1`` in one process and reports both medians and the spread of the ``0`` runs.
``--rotary`` builds the model of the model timings with rotary positions (``BertConfig.rotary``) instead of the learned
position table; the records carry ``"rotary"``. ``--pre-ln`` / ``--norm {layernorm,rmsnorm}`` build it with pre-norm
blocks (``BertConfig.pre_ln`` / ``norm``); the records carry ``"pre_ln"`` and ``"norm"``.
Random weights and prompts (no network)."""
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


def _sync_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _model(args, dev):
    from ml_trainer_amd.models.bert import BertLMHeadModel, bert_config
    torch.manual_seed(0)
    over = {"rotary": True} if args.rotary else {}
    if args.pre_ln or args.norm != "layernorm":
        over.update(pre_ln=bool(args.pre_ln), norm=args.norm)
    return BertLMHeadModel(bert_config(args.model, **over)).to(dev).eval()


def bench_model(args, dev):
    m = _model(args, dev)
    V, P, N = m.config.vocab_size, args.prompt, args.new
    recs = []
    for B in [int(b) for b in args.batch.split(",")]:
        ids = torch.randint(5, V, (B, P), device=dev)
        state = {}

        def prefill():
            state["s"] = m.prefill(ids, max_len=P + N)
            state["tok"] = m.decode_step(state["s"]).argmax(-1)

        def decode():
            tok = state["tok"]
            for _ in range(N - 1):
                tok = m.decode_step(state["s"], tok).argmax(-1)

        def uncached():
            with torch.no_grad():
                seq = torch.cat((ids, torch.zeros(B, N, dtype=ids.dtype, device=dev)), 1)
                rows = torch.arange(B, device=dev)
                for t in range(N - 1):
                    W = P + t + 1
                    seq[:, W - 1] = state["tok"] if t == 0 else tok
                    hidden = m(seq[:, :W].contiguous())
                    tok = m.mlm_logits(hidden, rows * W + W - 1).argmax(-1)

        if args.trace_steps and args.sampler == "device":  # the device sampler's loop, eager or graph replay
            m.generate(ids, args.trace_steps + 1, temperature=0.8, top_k=50, top_p=0.9, seed=1, sampler="device",
                       graph=args.graph)
            torch.cuda.synchronize()
            continue
        if args.trace_steps:
            prefill()
            tok = state["tok"]
            for _ in range(args.trace_steps):
                tok = m.decode_step(state["s"], tok).argmax(-1)
            torch.cuda.synchronize()
            continue
        settings = ["0", "1"] if args.ab else [os.environ.get("MLT_DECODE_GEMM", "1")]
        for s in settings:  # warm-up: kernel loading, the padded decoder table
            os.environ["MLT_DECODE_GEMM"] = s
            prefill(), decode()
        t_pre, t_unc, t_dec = [], [], {s: [] for s in settings}
        for _ in range(args.repeats):
            for s in settings:
                os.environ["MLT_DECODE_GEMM"] = s
                t_pre.append(_sync_ms(prefill))
                t_dec[s].append(_sync_ms(decode) / (N - 1))
            if not args.no_uncached:
                t_unc.append(_sync_ms(uncached) / (N - 1))
        ms = statistics.median(t_dec[settings[-1]])
        rec = {"bench": "generate", "model": args.model, "rotary": bool(args.rotary), "pre_ln": bool(args.pre_ln),
               "norm": args.norm, "batch": B, "prompt": P, "new": N,
               "decode_gemm": settings[-1],
               "prefill_ms": statistics.median(t_pre), "cached_ms_per_token": ms, "cached_tokens_per_s": B / ms * 1e3,
               "uncached_ms_per_token": statistics.median(t_unc) if t_unc else None,
               "cached_runs": t_dec[settings[-1]], "uncached_runs": t_unc}
        if args.ab:  # the planner's GEMMs in the same process: median, runs, (max - min) / median
            r0 = t_dec["0"]
            rec.update({"gemm0_ms_per_token": statistics.median(r0), "gemm0_runs": r0,
                        "gemm0_spread": (max(r0) - min(r0)) / statistics.median(r0)})
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


SAMPLER_SETTINGS = [("greedy", dict(temperature=0.0)), ("sampled", dict(temperature=0.8, top_k=50, top_p=0.9, seed=1))]


def _spread(runs):
    return (max(runs) - min(runs)) / statistics.median(runs)


def bench_sampler_ab(args, dev):
    """(eager, torch sampler) = the path before the device sampler, (eager, device sampler), (graph, device sampler),
    alternated in one process. A timed region is the token loop alone; prefill and capture are outside it."""
    m = _model(args, dev)
    V, P, N = m.config.vocab_size, args.prompt, args.new
    recs = []
    for B in [int(b) for b in args.batch.split(",")]:
        ids = torch.randint(5, V, (B, P), device=dev)
        dec = m._graphed_decoder(B, P + N, N, dev)
        for name, kw in SAMPLER_SETTINGS:
            torch_kw = {k: v for k, v in kw.items() if k != "top_p"}  # the torch sampler has no top-p
            params = m._sampler_params(kw["temperature"], kw.get("top_k"), kw.get("top_p"), None, kw.get("seed"))
            box = {}

            def pre_eager():
                box["s"] = m.prefill(ids, max_len=P + N)
                box["z"] = m.decode_step(box["s"])

            def step(tok):
                return m.decode_step(box["s"], tok)

            def run_torch():
                m._generate_loop(lambda: box["z"], step, B, dev, N, torch_kw["temperature"], torch_kw.get("top_k"),
                                 None, torch_kw.get("seed"), False)

            def run_device():
                st = m._new_sampler(B, N, dev, kw["temperature"], kw.get("top_k"), kw.get("top_p"), None, kw.get("seed"))
                m._device_sampler_loop(lambda: box["z"], step, st, N, False)

            def pre_graph():
                box["z"] = dec.start(m, ids, None, params)

            def run_graph():
                dec.run(m, box["z"])

            modes = [("eager_torch", pre_eager, run_torch), ("eager_device", pre_eager, run_device),
                     ("graph_device", pre_graph, run_graph)]
            for _, pre, run in modes:  # warm-up
                pre(), run()
            t = {k: [] for k, _, _ in modes}
            for _ in range(args.repeats):
                for k, pre, run in modes:
                    pre()
                    t[k].append(_sync_ms(run) / (N - 1))
            rec = {"bench": "generate_sampler_ab", "model": args.model, "rotary": bool(args.rotary),
                   "pre_ln": bool(args.pre_ln), "norm": args.norm, "batch": B,
                   "prompt": P, "new": N,
                   "setting": name, "capture_s": dec.capture_seconds}
            for k in t:
                rec[k + "_ms_per_token"] = statistics.median(t[k])
                rec[k + "_spread"] = _spread(t[k])
                rec[k + "_runs"] = t[k]
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    return recs


def bench_sampler_kernel(args, dev):
    from ml_trainer_amd.ops import decode as DC
    V, Vp, reps = 30522, 30720, 200
    recs = []
    settings = [("greedy", dict(temperature=0.0)), ("top_k_50", dict(temperature=0.8, top_k=50)),
                ("top_p_0.9", dict(temperature=0.8, top_p=0.9)), ("top_k_50_top_p_0.9", dict(temperature=0.8, top_k=50, top_p=0.9)),
                ("temperature_only", dict(temperature=0.8))]
    for B in [int(b) for b in args.batch.split(",")]:
        z = torch.randn(B, Vp, device=dev) * 3.0
        zv = z[:, :V]
        gen = torch.Generator(device=dev).manual_seed(1)
        for name, kw in settings:
            st = DC.SamplerState.allocate(B, reps, dev, seed=1, **kw)

            def device():
                st.draws.zero_()
                for _ in range(reps):
                    DC.sample_step(zv, V, st)

            def torch_ops():
                for _ in range(reps):
                    DC.sample_tokens(zv, kw["temperature"], kw.get("top_k"), gen)

            has_torch = "top_p" not in kw
            device()
            t_d, t_t = [], []
            if has_torch:
                torch_ops()
            for _ in range(args.repeats):
                t_d.append(_sync_ms(device) / reps * 1e3)
                if has_torch:
                    t_t.append(_sync_ms(torch_ops) / reps * 1e3)
            rec = {"bench": "sample_step", "batch": B, "V": V, "ldz": Vp, "setting": name,
                   "sample_step_us": statistics.median(t_d), "sample_step_spread": _spread(t_d),
                   "sample_tokens_us": statistics.median(t_t) if t_t else None,
                   "sample_tokens_spread": _spread(t_t) if t_t else None}
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    return recs


def bench_kernel(args, dev):
    from ml_trainer_amd.ops._ext import require_native
    C = require_native()
    H, Smax = args.heads, args.smax
    recs = []
    for B in [int(b) for b in args.batch.split(",")]:
        D = H * 64
        per = 2 * B * H * Smax * 64 * 2  # bytes of one cache
        ncache = max(2, -(-(512 << 20) // per))  # rotate over >= 512 MiB so no launch finds its cache in the LLC
        caches = [torch.randn(2, B, H, Smax, 64, device=dev).to(torch.bfloat16) for _ in range(ncache)]
        qkv = (torch.randn(B, 3 * D, device=dev) * 0.5).to(torch.bfloat16)
        pos = torch.full((B,), args.pos, dtype=torch.int32, device=dev)
        out = torch.empty(B, D, dtype=torch.bfloat16, device=dev)
        reps = 4 * ncache

        def run():
            for i in range(reps):
                C.attn_decode(qkv, caches[i % ncache], pos, out, H, 0.125)

        run()
        us = statistics.median(_sync_ms(run) / reps * 1e3 for _ in range(args.repeats))
        streamed = 2 * B * H * args.pos * 64 * 2  # the K and V rows below pos
        rec = {"bench": "attn_decode", "batch": B, "heads": H, "smax": Smax, "pos": args.pos, "caches": ncache,
               "us": us, "kv_bytes": streamed, "tb_per_s": streamed / us * 1e-6}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    return recs


DECODE_LINEARS = [("qkv", 2304, 768), ("out", 768, 768), ("ffn1", 3072, 768), ("ffn2", 768, 3072),
                  ("decoder", 30720, 768)]  # (name, N, K) of bert-base


def bench_linear(args, dev):
    from ml_trainer_amd.ops._ext import require_native
    C = require_native()
    recs = []
    for name, N, K in DECODE_LINEARS:
        per = N * K * 2
        ncopy = max(2, -(-(512 << 20) // per))  # rotate over >= 512 MiB of weights: none is found in the LLC
        ws = [(torch.randn(N, K, device=dev) * 0.02).to(torch.bfloat16) for _ in range(ncopy)]
        bias = torch.randn(N, device=dev)
        reps = max(2 * ncopy, 64)
        for M in [int(m) for m in args.rows.split(",")]:
            x = torch.randn(M, K, device=dev).to(torch.bfloat16)
            y = torch.empty(M, N, dtype=torch.float32 if name == "decoder" else torch.bfloat16, device=dev)

            def skinny():
                for i in range(reps):
                    C.gemm_skinny(x, ws[i % ncopy], y, bias=bias)

            def gemm():
                for i in range(reps):
                    C.gemm(x, ws[i % ncopy], y, False, False, bias=bias)

            skinny(), gemm()
            t = {"skinny": [], "gemm": []}
            for _ in range(args.repeats):
                t["skinny"].append(_sync_ms(skinny) / reps * 1e3)
                t["gemm"].append(_sync_ms(gemm) / reps * 1e3)
            us_s, us_g = statistics.median(t["skinny"]), statistics.median(t["gemm"])
            rec = {"bench": "decode_linear", "linear": name, "M": M, "N": N, "K": K, "copies": ncopy,
                   "weight_bytes": per, "skinny_us": us_s, "gemm_us": us_g, "skinny_tb_per_s": per / us_s * 1e-6,
                   "gemm_tb_per_s": per / us_g * 1e-6, "gemm_spread": (max(t["gemm"]) - min(t["gemm"])) / us_g,
                   "skinny_runs": t["skinny"], "gemm_runs": t["gemm"]}
            print(json.dumps(rec), flush=True)
            recs.append(rec)
        del ws
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bert-base")
    ap.add_argument("--batch", default="1,8,64")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-uncached", action="store_true")
    ap.add_argument("--trace-steps", type=int, default=0)
    ap.add_argument("--kernel", action="store_true", help="time C.attn_decode alone")
    ap.add_argument("--linear", action="store_true", help="time C.gemm_skinny and C.gemm on the decode linears")
    ap.add_argument("--rows", default="1,8,16,32,64", help="row counts of --linear")
    ap.add_argument("--ab", action="store_true", help="alternate MLT_DECODE_GEMM=0 / 1 in the model timing")
    ap.add_argument("--sampler", choices=["torch", "device"], default="torch", help="the sampler of --trace-steps")
    ap.add_argument("--graph", action="store_true", help="--trace-steps with --sampler device: replay the captured graph")
    ap.add_argument("--sampler-kernel", action="store_true", help="time sample_step against sample_tokens alone")
    ap.add_argument("--sampler-ab", action="store_true",
                    help="alternate (eager, torch sampler), (eager, device sampler), (graph, device sampler)")
    ap.add_argument("--rotary", action="store_true", help="rotary positions in the model timings")
    ap.add_argument("--pre-ln", action="store_true", help="pre-norm blocks in the model timings")
    ap.add_argument("--norm", choices=["layernorm", "rmsnorm"], default="layernorm",
                    help="the norm of the pre-norm blocks (rmsnorm needs --pre-ln)")
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--smax", type=int, default=256)
    ap.add_argument("--pos", type=int, default=255)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.graph and args.sampler != "device":
        raise SystemExit("--graph needs --sampler device")
    if args.sampler_kernel or args.sampler_ab:
        recs = bench_sampler_kernel(args, dev) if args.sampler_kernel else bench_sampler_ab(args, dev)
    else:
        recs = bench_linear(args, dev) if args.linear else bench_kernel(args, dev) if args.kernel else bench_model(args, dev)
    if args.out and recs:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for rec in recs:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
