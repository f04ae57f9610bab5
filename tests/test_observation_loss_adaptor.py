"""slide::SemanticFactorGraph::setObservationLoss and ::observationWeights (include/slide_sloam_adaptor.hpp) compile warning-free as
C++17 against the header alone, link against libslide_gpu.so, and (on the GPU) return what slide_graph_set_observation_loss and
slide_graph_get_observation_weights return (tests/observation_loss_adaptor_check.cpp)."""
import inspect
import os
import subprocess

import pytest

import slide_slam_amd as s

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "observation_loss_adaptor_check")
    lib_dir = os.path.dirname(s.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "observation_loss_adaptor_check.cpp"), "-o", exe, "-L" + lib_dir, "-lslide_gpu",
                        "-Wl,-rpath," + lib_dir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_observation_loss_adaptor_compiles_and_links(tmp_path):
    assert subprocess.run([_build(tmp_path)]).returncode == 0          # no argument: link check only


def test_binding_takes_the_classes_by_name():
    """SlideGraph.set_observation_loss shares set_robust_loss's kinds and selects the three classes by keyword, all on by default."""
    p = inspect.signature(s.SlideGraph.set_observation_loss).parameters
    assert [p[k].default for k in ("param", "points", "cubes", "cylinders")] == [0.0, True, True, True]
    assert callable(s.SlideGraph.observation_weights)
    assert {"slide_graph_set_observation_loss", "slide_graph_get_observation_weights"} <= set(s.api.EXPORTS)


@pytest.mark.gpu
def test_observation_loss_adaptor_runs(gpu, tmp_path):
    r = subprocess.run([_build(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "observation loss ok n=8 down=1" in r.stdout
