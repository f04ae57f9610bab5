"""The merged launches of an exact joint pass's assembly stage at their edges — the padding, the border fill and the lambda rows as
regions of k_schur_lb (unequal robots in one batch: a cut band, an uncut one and an empty border; no ghost factors; a last tile without
padding) and the separator landmarks' deltas written by the back-substitution (k_backsub_sep_b): every case of
tests/assembly_region_cases.py, two exact joint passes each (the second starts from what the first left, so a border tile the clear
missed shows in pass 2) against the independent joint Gauss-Newton step exactly as test_gpu_joint_step.py takes it (gn_reference by QR,
its own tolerance).  The evidence callback asserts the claimed layout on the shards.  And merged against separate: the same passes with
SLIDE_ASM_MERGE=0 (the parent's launch sequence) and at its default must leave the same bits in every pose and landmark."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import assembly_region_cases as rc                                             # noqa: E402
import joint_graphs as jg                                                      # noqa: E402
from test_gpu_joint_step import Run, run_case                                  # noqa: E402

pytestmark = pytest.mark.gpu

KNOBS = ("SLIDE_ASM_MERGE", "SLIDE_SCHUR_WALK", "SLIDE_FULL_CLEAR", "SLIDE_SEGMENTS")


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)           # (the launchers read them whenever a pass's launch sequence is built)


@pytest.mark.parametrize("name,make", rc.CASES, ids=[c[0] for c in rc.CASES])
def test_assembly_regions(gpu, monkeypatch, name, make):
    _env(monkeypatch, {})
    J, claims = make()

    def ev(r):
        rc.check_claims(J, r.ref, claims, run=r)
        assert r.info["n_slots"] > 0
    _, ratio = run_case(gpu, J, 0, evidence=ev)
    print(f"[assembly-regions] {name}: worst scaled_error / tolerance {ratio:.3e}")


def _two_passes(gpu, J):
    import torch
    r = Run(gpu, J, 0)
    try:
        out = []
        for _ in range(2):
            r.drv.one_pass()
            torch.cuda.synchronize()
            out.append(r.values().copy())
        return out
    finally:
        r.close()


MERGED = [("unequal", lambda: rc.unequal_case()[0]), ("relmeas_2x11", lambda: jg.relmeas_case(2, 11)), ("segments", lambda: jg.segments_case())]


@pytest.mark.parametrize("name,make", MERGED, ids=[c[0] for c in MERGED])
def test_merged_equals_separate(gpu, monkeypatch, name, make):
    """Two passes with the separate launches and two with the merged ones, in one process: bitwise equal after each pass."""
    _env(monkeypatch, {"SLIDE_ASM_MERGE": "0"})
    sep = _two_passes(gpu, make())
    _env(monkeypatch, {})
    mer = _two_passes(gpu, make())
    for k, (a, b) in enumerate(zip(sep, mer)):
        assert a.shape == b.shape and np.all(np.isfinite(a))
        assert a.tobytes() == b.tobytes(), (name, k, float(np.abs(a - b).max()))
    assert not np.array_equal(sep[0], sep[1])          # (the second pass moved the graph again)
