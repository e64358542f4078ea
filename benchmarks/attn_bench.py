"""Fused attention throughput (fwd / bwd) vs torch SDPA on BERT shapes; one JSON line per case.
``--dropout P``: attention-probability dropout in the native kernels (applied as round(P * 256) / 256)
next to ``F.scaled_dot_product_attention(dropout_p=P)``.
``--min-len L``: variable-length sequences (lengths uniform in [L, S], seeded) through the native kernels,
as padded ``lens`` or, with ``--packed``, as one [T, 3D] matrix with ``cu_seqlens``; the SDPA columns stay
the full-length run and the TFLOP/s count the full B x S x S work, so padded and packed compare by time.
``--causal``: the causal instantiations of the native kernels next to ``F.scaled_dot_product_attention(
is_causal=True)``; the TFLOP/s still count the full B x S x S work, so causal and non-causal compare by time.
``--rope``: times ``rope_qk`` (rotary positions on the q and k columns of the QKV buffer, in place) alone and nothing
else, at B 512, S 512, H 12 unless ``ATTN_B`` / ``ATTN_S`` say otherwise: microseconds per launch, forward and
backward sign, the bytes it moves computed from the shapes (2 x rows x 2D x 2: q and k read once and written once;
1.6 GB, six times the last-level cache) over that time, and the share of the 6.3 TB/s streaming rate."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.environ.get("ATTN_BENCH_PKG") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_trainer_amd.ops._ext import require_native  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dropout", type=float, default=0.0, help="attention-probability dropout (default 0.0)")
ap.add_argument("--min-len", type=int, default=0, help="variable-length sequences, lengths in [min-len, S]")
ap.add_argument("--packed", action="store_true", help="packed rows + cu_seqlens instead of padded rows + lens")
ap.add_argument("--causal", action="store_true", help="causal attention (key <= query), SDPA with is_causal=True")
ap.add_argument("--rope", action="store_true", help="time rope_qk alone (B 512 unless ATTN_B is set)")
ARGS = ap.parse_args()
P = ARGS.dropout
DROP = dict(p=P, seed=0x123456789ABCDEF, site=0x40000000, rank=0) if P > 0 else {}
C = require_native()
dev = torch.device("cuda", 0)
B, S, H = int(os.environ.get("ATTN_B", 32)), int(os.environ.get("ATTN_S", 512)), 12
D = H * 64


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


if ARGS.rope:
    from ml_trainer_amd.ops.rope import rope_table
    B = int(os.environ.get("ATTN_B", 512))
    rows = B * S
    table = rope_table(S, 10000.0, dev)
    buf = torch.randn(rows, 3 * D, device=dev, dtype=torch.bfloat16)
    pos = (torch.arange(rows, device=dev) % S).to(torch.int32)
    nbytes = 2 * rows * 2 * D * 2
    t = {"fwd": timeit(lambda: C.rope_qk(buf, table, H, S)),
         "bwd": timeit(lambda: C.rope_qk(buf, table, H, S, sign=-1)),
         "fwd_pos": timeit(lambda: C.rope_qk(buf, table, H, S, pos=pos))}
    rec = {"bench": "rope_qk", "B": B, "S": S, "H": H, "rows": rows, "bytes": nbytes,
           **{f"{k_}_us": round(v_ * 1e3, 2) for k_, v_ in t.items()},
           **{f"{k_}_tb_per_s": round(nbytes / v_ * 1e-9, 3) for k_, v_ in t.items()},
           **{f"{k_}_share_of_6.3": round(nbytes / v_ * 1e-9 / 6.3, 3) for k_, v_ in t.items()}}
    print(json.dumps(rec), flush=True)
    sys.exit(0)

qkv = torch.randn(B * S, 3 * D, device=dev).to(torch.bfloat16)
dout = torch.randn(B * S, D, device=dev).to(torch.bfloat16)
LENS, KW, TOK = None, dict(DROP, **({"causal": True} if ARGS.causal else {})), B * S
if ARGS.packed and not ARGS.min_len:
    ap.error("--packed needs --min-len")
if ARGS.min_len:
    ln = torch.randint(ARGS.min_len, S + 1, (B,), generator=torch.Generator().manual_seed(1))
    TOK = int(ln.sum())
    if ARGS.packed:
        cu = torch.zeros(B + 1, dtype=torch.int32)
        cu[1:] = ln.cumsum(0)
        KW["cu_seqlens"] = cu.to(dev)
        nq, nd = qkv[:TOK].contiguous(), dout[:TOK].contiguous()
    else:
        LENS = ln.to(torch.int32).to(dev)
        nq, nd = qkv, dout
else:
    nq, nd = qkv, dout
out = torch.empty(nq.shape[0], D, dtype=torch.bfloat16, device=dev)
lse = torch.empty(B * H * S, device=dev)
dqkv = torch.empty_like(nq)
delta = torch.empty(nq.shape[0] * H, device=dev)
C.attn_fwd(nq, out, lse, LENS, B, S, H, 0.125, **KW)
q, k, v = qkv.view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
q, k, v = [t.contiguous().requires_grad_() for t in (q, k, v)]
o = F.scaled_dot_product_attention(q, k, v, dropout_p=P, is_causal=ARGS.causal)
go = dout.view(B, S, H, 64).transpose(1, 2).contiguous()
fl_f = 4.0 * B * H * S * S * 64

t = {
    "native_fwd": timeit(lambda: C.attn_fwd(nq, out, lse, LENS, B, S, H, 0.125, **KW)),
    "native_bwd": timeit(lambda: C.attn_bwd(nq, out, nd, lse, delta, LENS, dqkv, B, S, H, 0.125, **KW)),
    "sdpa_fwd": timeit(lambda: F.scaled_dot_product_attention(q, k, v, dropout_p=P, is_causal=ARGS.causal)),
    "sdpa_bwd": timeit(lambda: torch.autograd.grad(o, (q, k, v), go, retain_graph=True)),
}
rec = {"B": B, "S": S, "H": H, "dropout": P, "causal": ARGS.causal, "min_len": ARGS.min_len, "packed": ARGS.packed, "tokens": TOK,
       "fill": round(TOK / (B * S), 4), **{k_: round(v_, 4) for k_, v_ in t.items()},
       "native_fwd_tflops": round(fl_f / t["native_fwd"] / 1e9, 1),
       "native_bwd_tflops": round(2.5 * fl_f / t["native_bwd"] / 1e9, 1),
       "sdpa_fwd_tflops": round(fl_f / t["sdpa_fwd"] / 1e9, 1),
       "sdpa_bwd_tflops": round(2.5 * fl_f / t["sdpa_bwd"] / 1e9, 1),
       "env": {k_: v_ for k_, v_ in os.environ.items() if k_.startswith("MLT_ATTN")}}
print(json.dumps(rec), flush=True)
