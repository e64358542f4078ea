#!/usr/bin/env python
"""Regenerate the launch-trace goldens (tests/golden/launch_trace/) after a launch changed on purpose.

    python scripts/record_launch_traces.py [--tree DIR] [--out DIR] [--full DIR]

``--tree``: the checkout whose ``ml_trainer_amd`` is traced (default: this one). The recorder, the scenarios and
the serialisation are always tests/launch_trace.py of THIS checkout, so two trees are compared by the same code.
``--full``: also write every full trace there, for a diff.

Adapter: none. The scenarios drive public methods only (``forward``, ``mlm_loss``, ``prefill``, ``decode_step``),
so no line of the recording names an internal entry point that differs between trees.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "launch_trace"))
    ap.add_argument("--full", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(args.tree))
    import launch_trace as LT
    import ml_trainer_amd
    print("tracing", os.path.dirname(ml_trainer_amd.__file__))
    os.makedirs(args.out, exist_ok=True)
    for name in LT.SCENARIOS:
        rec = LT.trace(name)
        with open(os.path.join(args.out, name + ".json"), "w") as f:
            json.dump({"calls": rec.names(), "sha256": rec.sha256()}, f, indent=0)
            f.write("\n")
        if args.full:
            os.makedirs(args.full, exist_ok=True)
            with open(os.path.join(args.full, name + ".jsonl"), "w") as f:
                f.write(rec.serialise())
        print(f"{name}: {len(rec.calls)} calls {rec.sha256()[:16]}")


if __name__ == "__main__":
    main()
