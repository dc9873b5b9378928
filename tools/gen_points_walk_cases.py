#!/usr/bin/env python3
"""Writes tests/golden/points_walk_cases.json: for every adversarial cloud of tests/points_cases.py its sizes and grid and, for the
nearest point (k = 1) and for k = 8, the candidates the KdTree's shell walk visits over the case's queries and the last shells it
walks -- as the numpy restatement of the walk (points_cases.Walk) has them.  CPU only, deterministic.  They are counts, not times:
tests/test_points_walk_model.py computes them again, tests/test_gpu_points_walk.py holds the device's candidate counter to them,
and DESIGN.md quotes the far clouds' from here.

    python tools/gen_points_walk_cases.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import points_cases as PC   # noqa: E402


def main():
    rec = PC.summary()
    with open(os.path.join(ROOT, "tests", "golden", "points_walk_cases.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for name, row in rec.items():
        print(f"{name:14s} grid {row['grid']}  distinct {row['distinct_points']:5d}  k1: {row['k1']['near_candidates_per_query']:8.1f} near, "
              f"{row['k1']['candidates']:8d} all, shell {row['k1']['mean_last_shell']:.2f}   k8: {row['k8']['near_candidates_per_query']:8.1f} near, "
              f"{row['k8']['candidates']:8d} all")


if __name__ == "__main__":
    main()
