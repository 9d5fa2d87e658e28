#!/usr/bin/env python3
"""Generate tests/golden/deep_trees.json: per case of tests/deep_scenes.py (a
generated world, a camera of trace_depth x monte_carlo_diffusion_times, 8 x 6
or 16 x 10 pixels of one sample, seed deep_scenes.SEED) what the C oracle
counts in its trees: the peak of pending siblings over the frame's samples and
how many samples reach it, the rays per tree level, the rays in all.
tests/test_deep_trees.py holds the oracle to these values and checks them
against the Python oracle's trees on sampled pixels; tests/test_gpu_deep_trees.py
holds the bounce-level engine's per-level counts to them.

    python tests/golden/make_deep_trees.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import deep_scenes  # noqa: E402


def main():
    rows = []
    with tempfile.TemporaryDirectory() as d:
        for name, depth, pt, w, h in deep_scenes.rows():
            row = {"name": name, "depth": depth, "pt": pt, "width": w, "height": h, "seed": deep_scenes.SEED}
            row.update(deep_scenes.measure(depth, pt, d, w, h))
            rows.append(row)
            print(name, row["max_pending"], row["samples_at_max"], row["rays"])
    with open(os.path.join(HERE, "deep_trees.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")


if __name__ == "__main__":
    main()
