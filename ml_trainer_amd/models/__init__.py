"""Model registry.

BASELINE.json configs (the reference itself has no config system; decision
recorded in SURVEY.md §7.1 and README):

* ``tiny``      -- LeNet at reduced width (CPU / gloo plumbing config)
* ``default``   -- the reference LeNet-5 (``src/model.py``), headline benchmark
* ``bert-base`` -- 12-layer, d=768, 12-head encoder classifier (seq 512, bf16)
* ``large``     -- 24-layer, d=1024, 16-head encoder classifier with fp8 GEMMs

``task="mlm"`` builds the BERT configs as ``BertForMaskedLM`` (masked-LM pre-training head) instead,
``task="clm"`` as ``BertLMHeadModel`` (causal attention, next-token head).
"""
from __future__ import annotations

from ml_trainer_amd.models.lenet import MLModel


def build_model(name: str = "default", task: str = "classify", **kw):
    """``task`` (BERT models): "classify" -> BertClassifier, "mlm" -> BertForMaskedLM (pre-training head),
    "clm" -> BertLMHeadModel (causal language model: next-token prediction)."""
    name = name.lower()
    if task not in ("classify", "mlm", "clm"):
        raise ValueError(f"unknown task {task!r} (classify|mlm|clm)")
    if name in ("default", "tiny", "lenet"):
        if task != "classify":
            raise ValueError(f"task {task!r} applies to the BERT models; the LeNet models classify images")
        return MLModel("default" if name == "lenet" else name)
    if name in ("bert-base", "bert_base", "bert", "large", "bert-large", "bert-tiny"):
        from ml_trainer_amd.models.bert import BertClassifier, BertForMaskedLM, BertLMHeadModel, bert_config
        if task == "mlm":  # (the fp8 `large` preset is rejected by the model)
            return BertForMaskedLM(bert_config(name, **kw))
        if task == "clm":  # (likewise)
            return BertLMHeadModel(bert_config(name, **kw))
        return BertClassifier(bert_config(name, **kw))
    raise ValueError(f"unknown model {name!r}")


__all__ = ["MLModel", "build_model"]
