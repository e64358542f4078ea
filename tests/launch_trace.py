"""Launch traces of the native transformer path, recorded on the CPU.

The native Python layer only allocates tensors and calls ``_C``. ``record()`` replaces ``require_native`` in every
``ml_trainer_amd`` module with a recorder and makes every tensor answer ``is_cuda`` with True, so the public model
methods take their native route on CPU tensors (``ops/gqa.py``, ``ops/swiglu.py``, ``ops/decode.py`` and
``ops/mlm.py`` included) and every launch lands in the trace. Nothing is computed: the outputs are whatever
``torch.empty`` held, which no control flow of the path reads.

A call is recorded as its name and every argument. A tensor argument is ``["T", dtype, shape, strides, storage
offset, storage number]`` with storages numbered in first-seen order, which makes the dataflow (which buffer feeds
which call) part of the trace; the recorder keeps every tensor it saw alive, so no address is handed out twice.
Everything else is recorded as its value.

``SCENARIOS`` are the configurations of tests/test_launch_trace_cpu.py; scripts/record_launch_traces.py writes
their goldens (tests/golden/launch_trace/) with this same code.
"""
from __future__ import annotations

import contextlib
import hashlib
import json
import sys

import torch

ENV_SWITCHES = ("MLT_DGRAD_WT", "MLT_DECODE_GEMM", "MLT_DECODE_GLU")  # read per call by the path: unset in a trace


class Recorder:
    """Stands in for the ``_C`` module: every attribute is a function that records its call. ``*_blocks`` helpers
    (partial-buffer sizing) return a small int, everything else None, as the launches do."""

    def __init__(self):
        self.calls = []
        self._storage = {}
        self._alive = []

    def _enc(self, v):
        if isinstance(v, torch.Tensor):
            self._alive.append(v)
            n = self._storage.setdefault(v.untyped_storage()._cdata, len(self._storage))
            return ["T", str(v.dtype).replace("torch.", ""), list(v.shape), list(v.stride()), v.storage_offset(), n]
        if isinstance(v, (list, tuple)):
            return [self._enc(x) for x in v]
        if v is None or isinstance(v, (bool, int, str)):
            return v
        if isinstance(v, float):
            return repr(v)
        raise TypeError(f"launch trace: no encoding for an argument of type {type(v).__name__}")

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def launch(*args, **kw):
            self.calls.append([name, [self._enc(a) for a in args], {k: self._enc(kw[k]) for k in sorted(kw)}])
            return 2 if name.endswith("_blocks") else None

        return launch

    def names(self):
        return [c[0] for c in self.calls]

    def serialise(self) -> str:
        return "".join(json.dumps(c, separators=(",", ":")) + "\n" for c in self.calls)

    def sha256(self) -> str:
        return hashlib.sha256(self.serialise().encode()).hexdigest()


@contextlib.contextmanager
def record():
    import importlib
    import os
    for m in ("transformer", "gqa", "swiglu", "decode", "mlm", "dropout", "rope"):
        importlib.import_module("ml_trainer_amd.ops." + m)
    rec = Recorder()
    patched = [(m, m.require_native) for n, m in list(sys.modules.items())
               if n.startswith("ml_trainer_amd") and m is not None and hasattr(m, "require_native")]
    env = {k: os.environ.pop(k) for k in ENV_SWITCHES if k in os.environ}
    try:
        for m, _ in patched:
            m.require_native = lambda: rec
        torch.Tensor.is_cuda = property(lambda self: True)  # shadows the base class's attribute
        yield rec
    finally:
        del torch.Tensor.is_cuda
        for m, f in patched:
            m.require_native = f
        os.environ.update(env)


# ------------------------------------------------------------------------------------------------ the scenarios
B, S, LENS, SEED = 2, 64, (64, 40), 1234
ALL_ON = dict(pre_ln=True, norm="rmsnorm", rotary=True, kv_heads=2, ffn="swiglu", intermediate=512, unpad=True,
              hidden_dropout=0.1, attention_dropout=0.1, causal=True)


def _batch():
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(5, 1000, (B, S), generator=g)
    mask = torch.arange(S)[None, :] < torch.tensor(LENS)[:, None]
    labels = torch.where(torch.rand(B, S, generator=g) < 0.15, ids, torch.full_like(ids, -100))
    return ids, mask.to(torch.int64), labels


def _model(cls_name, flat=False, **cfg):
    from ml_trainer_amd.models import bert
    torch.manual_seed(0)
    m = getattr(bert, cls_name)(bert.bert_config("bert-tiny", layers=2, **cfg))
    m.train()
    if flat:  # every gradient is a view of the flat buffer: the sink branch of _Grads
        from ml_trainer_amd.utils.flat import FlatParams
        m._flat = FlatParams(m.parameters())
    return m


def _train(cls_name="BertClassifier", flat=False, **cfg):
    def run():
        m = _model(cls_name, flat, **cfg)
        ids, mask, labels = _batch()
        out = m(ids, mask, dropout_seed=SEED)
        if cls_name == "BertForMaskedLM":  # the head and its backward as well
            out = m.mlm_loss(out, labels)
        out.float().sum().backward()
    return run


def _decode(**cfg):
    def run():
        m = _model("BertLMHeadModel", **cfg)
        ids, mask, _ = _batch()
        state = m.prefill(ids, mask, max_len=S + 2)
        m.decode_step(state)
        for t in range(2):
            m.decode_step(state, ids[:, t])
    return run


SCENARIOS = {
    "default": _train(),
    "causal": _train(causal=True),
    "unpad": _train(unpad=True),
    "dropout": _train(hidden_dropout=0.1, attention_dropout=0.1),
    "rotary": _train(rotary=True),
    "pre_ln": _train(pre_ln=True),
    "pre_ln_rmsnorm": _train(pre_ln=True, norm="rmsnorm"),
    "kv_heads": _train(kv_heads=2),
    "swiglu": _train(ffn="swiglu", intermediate=512),
    "all_on": _train(**ALL_ON),
    "mlm_default": _train("BertForMaskedLM"),
    "mlm_all_on": _train("BertForMaskedLM", **ALL_ON),
    "decode_post_ln": _decode(),
    "decode_all_on": _decode(**ALL_ON),
    "flat_default": _train(flat=True),
}


def trace(name: str) -> Recorder:
    with record() as rec:
        SCENARIOS[name]()
    return rec
