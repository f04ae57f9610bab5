"""slide::SemanticFactorGraph::predictedObservationMahalanobis and slide::SemanticFactorGraphWrapper::setAssociationGate / gateStats
(include/slide_sloam_adaptor.hpp) compile warning-free as C++17 against the header alone, link against libslide_gpu.so, and (on the
GPU) return what the C calls return (tests/predicted_gate_adaptor_check.cpp)."""
import os
import subprocess

import pytest

import slide_slam_amd as s

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "predicted_gate_adaptor_check")
    lib_dir = os.path.dirname(s.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "predicted_gate_adaptor_check.cpp"), "-o", exe, "-L" + lib_dir, "-lslide_gpu",
                        "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_predicted_gate_adaptor_compiles_and_links(tmp_path):
    assert subprocess.run([_build(tmp_path)]).returncode == 0          # no argument: link check only


@pytest.mark.gpu
def test_predicted_gate_adaptor_runs(gpu, tmp_path):
    r = subprocess.run([_build(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "predicted gate ok verdicts=10 missing=1 stats=1,1,2,0" in r.stdout
