"""CPU check of the KdTree search's grid arithmetic (sdfkit_amd/csrc/points_grid.h, the functions the kernels call): every
coordinate lands in a cell of the grid and every key in the cell-start table, on collinear clouds of more than 2^24 points,
thin boxes, the whole float range and random boxes (tests/cpp/points_grid_host.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_points_grid_cells_stay_in_range(tmp_path):
    exe = str(tmp_path / "points_grid_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "points_grid_host.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "grid ok" in p.stdout, p.stdout[-3000:] + p.stderr[-1000:]
