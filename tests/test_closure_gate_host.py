"""The individual-compatibility gate and the joint marginal of pose pairs (slide_graph_closure_mahalanobis /
slide_graph_get_pose_pair_covariances): what can be checked without a device — the symbols and the header's words, the Python and
adaptor methods, and the argument refusals, which are decided on the host before the graph handle or the device is looked at.  No
graph handle can be made without a device (slide_graph_create asks for one), so the refusals are provoked with a NULL handle: a call
whose arguments are good is refused FOR the handle, a call with a bad argument is refused for that argument, whatever the handle —
slide_last_error says which.  The same refusals on a live graph, and everything that needs the factor, are in
test_gpu_closure_gate.py.  The case generators' own assertions (tests/closure_gate_cases.py) run here too."""
import ctypes as C
import os
import re

import numpy as np

import slide_slam_amd as s

import closure_gate_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["slide_graph_get_pose_pair_covariances", "slide_graph_closure_mahalanobis"]
I7 = [0.0, 0, 0, 0, 0, 0, 1]
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def test_new_symbols_declared_exported_and_documented():
    txt = open(os.path.join(ROOT, "include", "slide_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = s.lib()
    for f in NEW:
        assert re.search(r"\bint\s+" + f + r"\s*\(", code), f
        assert hasattr(L, f), f
        assert f in s.api.EXPORTS
    comments = " ".join(re.findall(r"/\*.*?\*/", txt, flags=re.S))
    assert "jointMarginalCovariance" in comments and "16.81" in comments and "forward substitution" in comments
    assert callable(s.SlideGraph.get_pose_pair_covariances) and callable(s.SlideGraph.closure_mahalanobis)
    adaptor = open(os.path.join(ROOT, "include", "slide_sloam_adaptor.hpp")).read()
    assert "jointPoseCovariance" in adaptor and "closureMahalanobis" in adaptor


def _gate(L, a, d2, Cm=None, r=None, st=None):
    return s.lib().slide_graph_closure_mahalanobis(None, C.c_int(L), P(a["fr"]), P(a["fi"]), P(a["tr"]), P(a["ti"]), P(a["rel"]), P(a["sg"]),
                                                   P(d2), P(Cm), P(r), P(st))


def test_gate_argument_refusals_come_before_the_graph_and_write_nothing():
    good = dict(fr=np.zeros(3, np.int32), fi=np.array([30, 31, 32], np.uint64), tr=np.zeros(3, np.int32), ti=np.array([1, 2, 3], np.uint64),
                rel=np.tile(I7, (3, 1)), sg=np.full((3, 6), 0.1))

    def refused(why, L=3, d2_null=False, **change):
        a = {k: v.copy() for k, v in good.items()}
        for k, v in change.items():
            if v is None:
                a[k] = None
            else:
                v(a[k])
        d2, Cm, r, st = np.full(3, 77.0), np.full((3, 36), 77.0), np.full((3, 6), 77.0), np.full(3, 77, np.int32)
        rc = _gate(L, a, None if d2_null else d2, Cm, r, st)
        assert rc == -1, (change, rc)                                  # SLIDE_ERR_INVALID
        err = s.api.last_error()
        assert "closure_mahalanobis" in err and why in err, (change, err)
        assert (d2 == 77).all() and (Cm == 77).all() and (r == 77).all() and (st == 77).all()

    refused("the graph is NULL")                                        # good arguments: only the handle is wrong
    for name in good:
        refused("pointer is NULL", **{name: None})
    refused("pointer is NULL", d2_null=True)
    refused("L < 0", L=-1)

    def put(i, j, v):
        def f(a):
            a[i, j] = v
        return f

    def robot(a):
        a[1] = 13

    def zero_quat(a):
        a[0, 3:] = 0.0
    refused("robot outside", fr=robot)
    refused("robot outside", tr=robot)
    refused("non-finite", rel=put(1, 0, np.nan))
    refused("non-finite", rel=put(2, 6, np.inf))
    refused("zero quaternion", rel=zero_quat)
    refused("non-finite", sg=put(1, 3, np.nan))
    refused("sigma <= 0", sg=put(1, 3, 0.0))
    refused("sigma <= 0", sg=put(2, 0, -0.1))


def test_pair_argument_refusals_come_before_the_graph_and_write_nothing():
    good = dict(ra=np.zeros(2, np.int32), ia=np.array([0, 5], np.uint64), rb=np.zeros(2, np.int32), ib=np.array([9, 6], np.uint64))

    def refused(why, n=2, out_null=False, **change):
        a = {k: v.copy() for k, v in good.items()}
        for k, v in change.items():
            if v is None:
                a[k] = None
            else:
                v(a[k])
        out, st = np.full((2, 144), 77.0), np.full(2, 77, np.int32)
        rc = s.lib().slide_graph_get_pose_pair_covariances(None, C.c_int(n), P(a["ra"]), P(a["ia"]), P(a["rb"]), P(a["ib"]),
                                                           None if out_null else P(out), P(st))
        assert rc == -1, (change, rc)
        err = s.api.last_error()
        assert "get_pose_pair_covariances" in err and why in err, (change, err)
        assert (out == 77).all() and (st == 77).all()

    def robot(a):
        a[0] = -1
    refused("the graph is NULL")
    for name in good:
        refused("pointer is NULL", **{name: None})
    refused("pointer is NULL", out_null=True)
    refused("n < 0", n=-1)
    refused("robot outside", ra=robot)
    refused("robot outside", rb=robot)


def test_generators_hold_their_own_conditions():
    """The planted and the aliased list assert on themselves under d2_ref alone (closure_gate_cases): true closures below 16.81 / 2
    and false ones above 4 x 16.81; in the list shared with select_closures the four false ones above 16.81, the eight true ones
    below, the three aliased ones scored consistent with each other by the restatement of the consistency score."""
    for chart in (0, 1):
        c = gc.case("noisy40", chart)
        cl, flags, d2 = gc.planted_list(c)
        assert len(cl) == 12 and flags.sum() == 8
        cl, kinds, d2 = gc.aliased_list(c)
        assert (kinds == 0).sum() == 8 and (kinds == 1).sum() == 1 and (kinds == 2).sum() == 3
        print(f"[gate-cases] chart {chart}: aliased list d2_ref true max {d2[kinds == 0].max():.2f}, false min {d2[kinds != 0].min():.1f}")


def test_reference_has_the_orientation_of_add_loop_closure():
    """A closure measured at the estimate's own relative pose X_from^-1 X_to has a zero residual in the reference, and its swapped twin
    (the same rel with from and to exchanged) does not: ref_gate follows slide_graph_add_loop_closure's sense."""
    c = gc.case("chain40", 1)
    cl = [gc.measured(c.cpu_pose12, 0, 30, 0, 2, np.zeros(6))]
    r, _, _, d2 = gc.ref_gate(c, cl, c.cpu_pose12)
    assert np.abs(r).max() < 1e-9 and d2[0] < 1e-15
    sw = [(0, 2, 0, 30, cl[0][4], cl[0][5])]
    assert gc.ref_gate(c, sw, c.cpu_pose12)[3][0] > 100.0
