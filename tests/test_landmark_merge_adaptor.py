"""slide::SemanticFactorGraph::mergeLandmarks / landmarkAlias / mergeDuplicateLandmarks (include/slide_sloam_adaptor.hpp) compile
warning-free as C++17 against the header alone, link against libslide_gpu.so, and (on the GPU) do what the C calls do
(tests/landmark_merge_adaptor_check.cpp)."""
import os
import subprocess

import pytest

import slide_slam_amd as s

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "landmark_merge_adaptor_check")
    lib_dir = os.path.dirname(s.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "landmark_merge_adaptor_check.cpp"), "-o", exe, "-L" + lib_dir, "-lslide_gpu",
                        "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_landmark_merge_adaptor_compiles_and_links(tmp_path):
    assert subprocess.run([_build(tmp_path)]).returncode == 0          # no argument: link check only


@pytest.mark.gpu
def test_landmark_merge_adaptor_runs(gpu, tmp_path):
    r = subprocess.run([_build(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "landmark merge ok rows=1 moved=2 alias=0 n_lm=2 status=1,-1 chain=4" in r.stdout
