#!/usr/bin/env python3
"""Writes tests/golden/pointcloud_color_accuracy.json: how far the vertex colours of sphere -> mesh -> coloured cloud -> coloured
banded volume -> mesh lie from the colour function 0.5 + 0.25 p that coloured the cloud, as the numpy model of the contract
(tests/pointcloud_color_model.end_to_end) and the CPU oracle's mesher have it -- CPU only, deterministic, at the grid of
tests/golden/pointcloud_accuracy.json.  The library's mesh equals this computation bit for bit (tests/test_gpu_pointcloud_color.py),
so the recorded error is its bound without margin.

    python tools/gen_pointcloud_color_accuracy.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import pointcloud_color_model as CM   # noqa: E402


def main():
    rec = CM.accuracy_figures()
    with open(os.path.join(ROOT, "tests", "golden", "pointcloud_color_accuracy.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
