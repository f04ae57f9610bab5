"""The joint-tree selected inverse (k_jsinv_prep, k_jsinv_tile<false / true> of joint_cov_kernels.hip) tile by tile.

The joint marginals, information gain and gates read this pass through CholBatch::ensure_joint_sigma only, on whole multi-robot graphs.
Here slide_debug_joint_selected_inverse hands caller-built systems (cov_cases.py) to launch_jsinv_prep and launch_jsinv_step in that
function's sequence: factor columns split over two stores with different leading dimensions, row lists that skip tiles and reach past
the columns into a caller-given Sigma, a lambda column factored as its negative, a step whose jobs have 3, 1 and 0 rows, two systems
with different lds and col0 in one table, and band3 of the one-store tests expressed as a joint system.  Bounds (a) and (b) of
cov_cases.py everywhere, (c) where every row is an own column (Sigma = (L D L^T)^-1).  Everything outside the lists' tiles keeps its
bits — the caller's Sigma of the rows past the columns included.

Worst |err| / bound observed on an MI355X (profiles/cov_kernels_bounds.txt): (b) Z 0.097, (b) L_kk^-T D L_kk^-1 0.084 (lambda), (a) 0.101
(two_store), (c) 0.140 (as_one_store, which came out bit-identical to slide_debug_selected_inverse).  No kernel needed a change."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cov_cases as cc                                                         # noqa: E402
from cov_cases import NB                                                       # noqa: E402

pytestmark = pytest.mark.gpu


def _report(what, **ratios):
    print(f"[joint-selected-inverse] {what}: " + "  ".join(f"{k} {v:.3e}" for k, v in ratios.items()))


def _run(api, names, steps, stage=1):
    """The systems `names` in one table; steps: lists of (system, column).  Returns (models, layouts, outputs)."""
    models = [cc.joint_model(nm) for nm in names]
    rp, rows, col0 = cc.row_lists(models)
    lay = [cc.joint_layout(m, *cc.joint_dims(nm, m), c0) for nm, m, c0 in zip(names, models, col0)]
    jobs = [jb for st in steps for jb in st]
    step_off = np.cumsum([0] + [len(st) for st in steps])
    return models, lay, api.debug_joint_selected_inverse(lay, rp, rows, jobs, step_off, stage=stage)


def _check_writes(m, lay, out, stage):
    lds = lay["lds"]
    ms, mz = cc.written_masks(m, lds)
    if stage == 0:
        ms = np.zeros_like(ms)
        for k in range(m["Tc"]):
            ms[k * NB:(k + 1) * NB, k * NB:(k + 1) * NB] = True
    Sg, Z = cc.view(out["Sg"], lds), cc.view(out["Z"], lds)
    assert not np.isnan(Sg[ms]).any(), "a NaN inside the lists' tiles of Sg"
    assert not np.isnan(Z[mz]).any(), "a NaN inside the lists' tiles of Z"
    assert cc.same_bits(Sg[~ms], cc.view(lay["Sg"], lds)[~ms]), "Sg was written outside the lists' tiles (the caller's Sigma included)"
    assert cc.same_bits(Z[~mz], cc.view(lay["Z"], lds)[~mz]), "Z was written outside the lists' tiles"
    for k in range(m["Tc"]):
        t = cc.tile(out["Sg"], lds, k, k)
        assert cc.same_bits(t, t.T), ("diagonal tile not symmetric bit for bit", k)


def _check_values(name, m, lay, prep, full):
    lds = lay["lds"]
    rz, rp = cc.check_b(m, lds, prep["Sg"], prep["Z"])
    ra = cc.check_a(m, lds, full["Sg"], full["Z"], prep["Sg"])
    rc = cc.check_c_sigma(m, lds, full["Sg"]) if m["Trow"] == m["Tc"] else 0.0
    _report(name, b_Z=rz, b_P=rp, a=ra, c=rc)
    assert rz <= 1 and rp <= 1, "bound (b): k_jsinv_prep"
    assert ra <= 1, "bound (a): a tile is not the product of what the device read"
    assert rc <= 1, "bound (c): Sigma against the long-double (L D L^T)^-1"


def _one_step(m):
    return [[(0, k) for k in range(m["Tc"])]]


@pytest.mark.parametrize("name", ["two_store", "gaps", "lambda", "uneven_step", "as_one_store"])
def test_joint_case(gpu, name):
    m = cc.joint_model(name)
    steps = _one_step(m) if name == "uneven_step" else cc.sequential_steps(m)
    (_,), (lay,), (prep,) = _run(gpu.api, [name], steps, stage=0)
    (_,), (_,), (full,) = _run(gpu.api, [name], steps, stage=1)
    _check_writes(m, lay, prep, 0)
    _check_writes(m, lay, full, 1)
    assert cc.same_bits(prep["Z"], full["Z"])
    _check_values(name, m, lay, prep, full)
    if name == "as_one_store":                        # two separately compiled kernels: reported, not asserted
        ld = lay["lds"]
        f = cc.factor_layout(cc.profile_model("band3"), ld)
        pre = np.full(ld * m["Tc"] * NB, cc.OUT_NAN)
        one = gpu.api.debug_selected_inverse(f, pre, pre, stage=1)
        print(f"[joint-selected-inverse] as_one_store: bit-identical to slide_debug_selected_inverse: Sg {cc.same_bits(one['Sg'], full['Sg'])}, "
              f"Z {cc.same_bits(one['Z'], full['Z'])}")


def test_uneven_step_jobs_alone(gpu):
    """Jobs with 3, 1 and 0 rows in one step: each job's tiles equal, bit for bit, the same job launched in a step of its own."""
    m = cc.joint_model("uneven_step")
    (_,), (lay,), (tog,) = _run(gpu.api, ["uneven_step"], _one_step(m))
    for order in ([0, 1, 2], [2, 1, 0]):
        (_,), (_,), (sep,) = _run(gpu.api, ["uneven_step"], [[(0, k)] for k in order])
        assert cc.same_bits(tog["Sg"], sep["Sg"]) and cc.same_bits(tog["Z"], sep["Z"]), order


def test_pair_in_one_table(gpu):
    """Two systems with different lds and col0 in one table, their steps side by side: each equals itself alone."""
    names = ["two_store", "gaps"]
    ms = [cc.joint_model(nm) for nm in names]
    nst = max(m["Tc"] for m in ms)
    steps = [[(s, m["Tc"] - 1 - q) for s, m in enumerate(ms) if q < m["Tc"]] for q in range(nst)]
    _, lays, outs = _run(gpu.api, names, steps)
    assert lays[0]["lds"] != lays[1]["lds"] and lays[1]["col0"] > 0
    _, _, preps = _run(gpu.api, names, steps, stage=0)
    for nm, m, lay, out, prep in zip(names, ms, lays, outs, preps):
        (_,), (_,), (alone,) = _run(gpu.api, [nm], cc.sequential_steps(m))
        assert cc.same_bits(out["Sg"], alone["Sg"]) and cc.same_bits(out["Z"], alone["Z"]), nm
        _check_writes(m, lay, out, 1)
        _check_values("pair/" + nm, m, lay, prep, out)


def test_refusals_launch_nothing(gpu):
    api = gpu.api
    m = cc.joint_model("gaps")
    rp, rows, col0 = cc.row_lists([m])
    lay = cc.joint_layout(m, *cc.joint_dims("gaps", m), 0)
    steps = cc.sequential_steps(m)
    jobs = [jb for st in steps for jb in st]
    off = list(range(len(jobs) + 1))

    def refused(rows_=rows, jobs_=jobs, off_=off, lay_=lay):
        with pytest.raises(api.SlideError) as e:
            api.debug_joint_selected_inverse([lay_], rp, rows_, jobs_, off_)
        assert e.value.code == -1

    refused(rows_=[6] + rows[1:])                     # a row at the system's tile rows
    refused(rows_=[0] + rows[1:])                     # a row <= its column
    refused(rows_=[4, 4] + rows[2:])                  # a row listed twice
    refused(jobs_=jobs[:-1] + [jobs[0]])              # a column listed twice
    refused(jobs_=jobs[:-1] + [(0, 4)])               # a column the system does not have
    refused(jobs_=jobs[:-1] + [(1, 0)])               # a system the table does not have
    refused(off_=off[:-1] + [off[-1] + 1])            # steps that leave the job table
    refused(lay_=dict(lay, lds=lay["Trow"] * NB - 2, Sg=lay["Sg"][:(lay["Trow"] * NB - 2) * lay["Trow"] * NB],
                      Z=lay["Z"][:(lay["Trow"] * NB - 2) * lay["Trow"] * NB]))
    (_,), (_,), (full,) = _run(api, ["gaps"], steps)
    assert not np.isnan(cc.view(full["Sg"], lay["lds"])[cc.written_masks(m, lay["lds"])[0]]).any()
