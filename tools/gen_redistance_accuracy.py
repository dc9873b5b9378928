#!/usr/bin/env python3
"""Writes tests/golden/redistance_accuracy.json: the first-order error of Voxels.Redistance as the numpy model of its contract
(tests/redistance_model.py) has it -- CPU only, deterministic; tests/test_redistance_model.py recomputes the entries up to 64^3
and requires equality.  Errors are in voxels (|result - exact| / DX).

    python tools/gen_redistance_accuracy.py            # a minute or two: the 128^3 sphere is 129 numpy sweeps of 2 M voxels
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import redistance_model as M   # noqa: E402


def main():
    rec = {"units": "voxels: |result - exact distance| / DX; edge_shift in units of the grid edge",
           "sphere": {}, "mesh": {}}
    for n in (16, 32, 64):
        rec["sphere"][str(n)] = {k: M.sphere_record(n, k) for k in "abc"}
    rec["sphere"]["128"] = {"a": M.sphere_record(128, "a")}
    for name in ("box", "two_spheres"):
        rec["mesh"][name] = M.mesh_record(name)
    path = os.path.join(ROOT, "tests", "golden", "redistance_accuracy.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
