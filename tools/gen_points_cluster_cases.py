"""Writes tests/golden/points_cluster_cases.json: the tie cloud of the border rule in its three index orders, and what the numpy
model (tests/points_cluster_model.py) gives on the seeded clouds of tests/points_cluster_cases.py -- recorded results that the
CPU tests compare the model with and the GPU tests the library.  Run from the repository root: python tools/gen_points_cluster_cases.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import points_cluster_cases as CC   # noqa: E402
from tests import points_cluster_model as CM   # noqa: E402


def summary(out):
    sizes = sorted((int(s) for s in out["sizes"]), reverse=True)
    return {"stats": [int(v) for v in out["stats"]], "largest_sizes": sizes[:4], "singletons": int(sum(1 for s in sizes if s == 1))}


def main():
    L = [[-1, 0, 0], [-1.2, 0, 0], [-1.4, 0, 0], [-1.2, 0.2, 0]]
    R = [[-x, y, z] for x, y, z in L]
    O = [[0, 0, 0]]
    orders = {"L+R+origin": L + R + O, "R+L+origin": R + L + O, "origin+R+L": O + R + L}
    tie = {"radius": 1.0, "min_points": 4, "orders": {}, "sizes": None}
    for name, pts in orders.items():
        out = CM.cluster(np.array(pts, np.float32), 1.0, 4)
        tie["orders"][name] = {"points": pts, "labels": [int(v) for v in out["labels"]]}
        sizes = [int(v) for v in out["sizes"]]
        assert tie["sizes"] in (None, sizes)
        tie["sizes"] = sizes
    doc = {"tie": tie, "cloud_a": {}, "chain": {}, "duplicates": {}, "far": {}, "two_sheets": {}}
    A, _ = CC.cloud_a()
    for r, mp in CC.A_CASES:
        doc["cloud_a"][f"{r},{mp}"] = summary(CM.cluster(A, r, mp))
    P = CC.chain()
    for name, r, mp in (("1,1", 1.0, 1), ("below_1,1", CC.BELOW_ONE, 1), ("1,3", 1.0, 3)):
        doc["chain"][name] = summary(CM.cluster(P, r, mp))
    D = CC.duplicates()
    for r, mp in ((0.0, 1), (0.0, 3), (0.0, 4), (np.inf, 1), (np.inf, 20)):
        doc["duplicates"][f"{r},{mp}"] = summary(CM.cluster(D, r, mp))
    F = CC.far_cloud()
    for r, mp in ((0.25, 1), (0.5, 4)):
        doc["far"][f"{r},{mp}"] = summary(CM.cluster(F, r, mp))
    S, _ = CC.two_sheets()
    rows = {}
    for r, mp in CC.SHEET_CASES:
        if r not in rows:
            rows[r] = CM.neighbours(S, r)
        doc["two_sheets"][f"{r},{mp}"] = summary(CM.cluster(S, r, mp, rows[r]))
    with open(CC.GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(json.dumps({k: v for k, v in doc.items() if k != "tie"}))
    print(tie["sizes"], [o["labels"] for o in tie["orders"].values()])


if __name__ == "__main__":
    main()
