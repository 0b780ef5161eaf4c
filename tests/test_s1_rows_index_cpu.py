"""CPU: the row-group index arithmetic of dec_gemm_rows (csrc/s1_decode_rows_index.h, which the kernel is written with)
replayed on the host by tools/rows_group_index_check.cpp: built here with the host compiler and run for the row counts
next to a b-tile or a row-group boundary (B % 16 in {15, 0, 1}, and 100) and the layer shapes -- every element of y
written exactly once, x_out once per row.  Without an argument the program replays every B in 1..128."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rows_group_index_replay(tmp_path):
    from easevoice_trainer_amd.build import HIPCC

    src = os.path.join(ROOT, "tools", "rows_group_index_check.cpp")
    exe = str(tmp_path / "rows_group_index_check")
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    cmd = [cxx, "-O2", "-std=c++17"] if cxx else [HIPCC, "-x", "c++", "-O2", "-std=c++17"]
    subprocess.run([*cmd, src, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "edges"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: 250 launches replayed, B within 1..128"), r.stdout
    # the kernel and the replay share one set of expressions
    hip = open(os.path.join(ROOT, "easevoice_trainer_amd", "csrc", "s1_decode_rows.hip")).read()
    for name in ("group_first", "group_rows", "row_offset", "b_tiles", "stage_k4", "stage_row0", "stage_offset", "epi_row",
                 "epi_col", "grid_x", "grid_y"):
        assert f"evt_rows::{name}(" in hip, name
