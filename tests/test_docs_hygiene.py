"""Docs that describe the shipped step must match it (VERDICT r5 'What's weak' #6 / #9)."""
import glob
import os
import re

import ml_trainer_amd.models.lenet_engine as le
import ml_trainer_amd.trainer as tr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lenet_docstrings_say_two_launches():
    for mod in (tr, le):
        doc = mod.__doc__
        assert re.search(r"\btwo kernels per step\b", doc, re.I), mod.__name__
        assert not re.search(r"\bone kernel per step\b", doc, re.I), mod.__name__


def test_no_one_launch_step_left():
    """The one-launch step (measured slower, r5) is gone: no translation units, no engine switch."""
    kdir = os.path.join(REPO, "ml_trainer_amd", "csrc", "kernels")
    assert not glob.glob(os.path.join(kdir, "lenet_mfma_1l_*.hip"))
    src = open(os.path.join(REPO, "ml_trainer_amd", "csrc", "bindings.cpp")).read()
    assert "onelaunch" not in src and "MLT_LENET_ONELAUNCH" not in src
    assert not hasattr(le.LeNetStepEngine, "flush") and not hasattr(le.LeNetStepEngine, "sync_error")


def test_no_retired_gemm_paths_left():
    """The persistent ping-pong GEMM (config 6), the erf-polynomial GELU fork and the switches of
    settled A/Bs are gone from the native sources; the raster override is read in one place."""
    csrc = os.path.join(REPO, "ml_trainer_amd", "csrc")
    assert not glob.glob(os.path.join(csrc, "kernels", "gemm_persist*.hip"))
    text = {}
    for d, _, files in os.walk(csrc):
        for f in files:
            text[os.path.join(d, f)] = open(os.path.join(d, f), errors="replace").read()
    for name in ("MLT_W4_GELU_TAB", "MLT_Q8_GELU_TAB", "MLT_W4_PERSIST", "MLT_GEMM_W4F8", "MLT_GEMM_W4Q8_GROUP_M",
                 "MLT_GEMM_SPLIT_EXT", "gelu_grad2", "launch_gemm_persist"):
        assert not [p for p, s in text.items() if name in s], name
    assert sum(s.count('getenv("MLT_GEMM_GROUP_M")') for s in text.values()) == 1


def test_no_retired_bert_paths_left():
    """The quantising LayerNorm backward, the packed-f32 attention fork and the switches of settled
    BERT / fp8 A/Bs are gone from the package (native sources and Python); the attention backward's
    one remaining switch is read in one place."""
    text = {}
    for d, _, files in os.walk(os.path.join(REPO, "ml_trainer_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h", ".inc")):
                text[os.path.join(d, f)] = open(os.path.join(d, f), errors="replace").read()
    assert any(p.endswith("attention.hip") for p in text) and any(p.endswith("transformer.py") for p in text)
    for name in ("ln_bwd_q8", "ln_q8_partial_blocks", "MLT_FP8_LN_Q", "fuse_ln", "MLT_ATTN_PKF32", "pk_prob_ds",
                 "MLT_FP8_CT_WIDE", "MLT_ATTN_COLSUM", "MLT_DGELU_COLSUM", "MLT_FP8_ATTN_Q", "MLT_FP8_FUSE"):
        assert not [p for p, s in text.items() if name in s], name
    assert sum(s.count('getenv("MLT_ATTN_RING")') for s in text.values()) == 1
