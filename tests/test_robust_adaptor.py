"""slide::SemanticFactorGraph::setRobustLoss and ::closureWeights (include/slide_sloam_adaptor.hpp) compile warning-free as C++17
against the header alone, link against libslide_gpu.so, and (on the GPU) return what slide_graph_set_robust_loss and
slide_graph_get_closure_weights return (tests/robust_adaptor_check.cpp)."""
import os
import subprocess

import pytest

import slide_slam_amd as s

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "robust_adaptor_check")
    lib_dir = os.path.dirname(s.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "robust_adaptor_check.cpp"), "-o", exe, "-L" + lib_dir, "-lslide_gpu",
                        "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_robust_adaptor_compiles_and_links(tmp_path):
    assert subprocess.run([_build(tmp_path)]).returncode == 0          # no argument: link check only


def test_binding_numbers_the_losses_as_the_reference_does():
    """SlideGraph.set_robust_loss's names map to the kinds of slide_gpu.h's table, which tests/robust_cases.py restates."""
    import robust_cases as rc
    names = {k: v for k, v in s.SlideGraph.ROBUST_KINDS.items() if v}
    assert names == rc.KINDS and s.SlideGraph.ROBUST_KINDS[None] == 0
    assert callable(s.SlideGraph.closure_weights)


@pytest.mark.gpu
def test_robust_adaptor_runs(gpu, tmp_path):
    r = subprocess.run([_build(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "robust ok n=3 kept=10 rel=1" in r.stdout
