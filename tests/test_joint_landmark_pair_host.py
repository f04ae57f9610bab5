"""The duplicate-landmark queries on the JOINT graph (slide_chol_batch_landmark_pair_mahalanobis / _get_landmark_pair_covariances /
_landmark_pairs_within): what can be checked without a device — the symbols and the header's words, the Python methods, and the
argument refusals, which are the single-graph calls' own and are decided on the host before the batch handle or the device is looked
at (provoked with a NULL handle, as test_landmark_pair_host.py provokes them).  The numpy side of tests/joint_landmark_pair_cases.py
is checked against itself here too: the block form the device follows (private sides eliminated into their own robot's poses, shared
sides kept as separator rows, the lambda rows counted with D = -I) against the dense inverse of the joint H, the planted generator's
own conditions on both charts, and the brute-force search on a union of robots.  Everything that needs the factor is in
test_gpu_joint_landmark_pairs.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import slide_slam_amd as s

import joint_graphs as jg
import joint_landmark_pair_cases as jp
import joint_observation_gate_cases as jo
import landmark_pair_cases as lp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["slide_chol_batch_landmark_pair_mahalanobis", "slide_chol_batch_get_landmark_pair_covariances",
       "slide_chol_batch_landmark_pairs_within"]
P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
INVALID = -1
BLOCK_FORM_BOUND = 1e-9          # test_joint_observation_gate_host.py's bound for block_form


def test_new_symbols_declared_exported_and_documented():
    txt = open(os.path.join(ROOT, "include", "slide_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = s.lib()
    for f in NEW:
        assert re.search(r"\bint\s+" + f + r"\s*\(", code), f
        assert hasattr(L, f), f
        assert f in s.api.EXPORTS
    m = re.search(r"\bint\s+" + NEW[0] + r"\s*\(([^;]*)\)\s*;", code)
    args = [a.split()[-1].lstrip("*") for a in m.group(1).split(",")]
    assert args == ["b", "n", "cls", "slot_a", "idx_a", "slot_b", "idx_b", "sigma_point3", "sigma_cylinder7", "d2", "dof", "C81", "r9", "status"], args
    comments = re.sub(r"[\s*]+", " ", " ".join(re.findall(r"/\*.*?\*/", txt, flags=re.S)))
    for words in ("W^T D W", "separator variable the pass does not eliminate", "two replicas of one shared slot",
                  "neither a factor nor a shared slot", "no direct route off the cached Sigma", "lowest replica"):
        assert words in comments, words
    from slide_slam_amd.distributed import PassDriver
    for name in ("landmark_pair_mahalanobis", "get_landmark_pair_covariances", "landmark_pairs_within", "duplicate_landmarks"):
        assert callable(getattr(s.CholBatch, name)), name
        assert callable(getattr(PassDriver, name)), name


def _arrays(good, change):
    a = {k: (None if v is None else v.copy()) for k, v in good.items()}
    for k, v in change.items():
        if v is None:
            a[k] = None
        else:
            v(a[k])
    return a


def put(i, v):
    def f(a):
        a[i] = v
    return f


def test_pair_test_argument_refusals_come_before_the_batch_and_write_nothing():
    good = dict(cls=np.array([2, 0, 2], np.int32), sa=np.array([0, 0, 1], np.int32), ia=np.array([0, 6, 3], np.uint64),
                sb=np.array([1, 0, 1], np.int32), ib=np.array([1, 2, 4], np.uint64), s3=np.full(3, 0.05), s7=np.full(7, 0.02))

    def refused(why, n=3, d2_null=False, **change):
        a = _arrays(good, change)
        d2, dof, Cm, r, st = np.full(3, 77.0), np.full(3, 77, np.int32), np.full((3, 81), 77.0), np.full((3, 9), 77.0), np.full(3, 77, np.int32)
        rc = s.lib().slide_chol_batch_landmark_pair_mahalanobis(None, C.c_int(n), P(a["cls"]), P(a["sa"]), P(a["ia"]), P(a["sb"]), P(a["ib"]),
                                                                P(a["s3"]), P(a["s7"]), None if d2_null else P(d2), P(dof), P(Cm), P(r), P(st))
        assert rc == INVALID, (change, rc)
        err = s.api.last_error()
        assert "chol_batch_landmark_pair_mahalanobis" in err and why in err, (change, err)
        assert (d2 == 77).all() and (dof == 77).all() and (Cm == 77).all() and (r == 77).all() and (st == 77).all()

    refused("the batch is NULL")                                        # good arguments: only the handle is wrong
    for name in good:
        refused("pointer is NULL", **{name: None})
    refused("pointer is NULL", d2_null=True)
    refused("n < 0", n=-1)
    refused("neither SLIDE_CLS_ELLIPSOID nor SLIDE_CLS_CYLINDER", cls=put(1, 1))      # a cube
    refused("neither SLIDE_CLS_ELLIPSOID nor SLIDE_CLS_CYLINDER", cls=put(2, 7))
    refused("neither SLIDE_CLS_ELLIPSOID nor SLIDE_CLS_CYLINDER", cls=put(0, -1))
    for bad in (0.0, -0.05, np.nan, np.inf):
        refused("sigma that is non-finite or <= 0", s3=put(1, bad))
        refused("sigma that is non-finite or <= 0", s7=put(6, bad))


def test_pair_covariance_and_search_argument_refusals():
    good = dict(cls=np.array([2, 1], np.int32), sa=np.array([0, 1], np.int32), ia=np.array([0, 3], np.uint64), sb=np.array([1, 1], np.int32),
                ib=np.array([1, 9], np.uint64))

    def refused(why, n=2, out_null=False, **change):
        a = _arrays(good, change)
        out, st = np.full((2, 324), 77.0), np.full(2, 77, np.int32)
        rc = s.lib().slide_chol_batch_get_landmark_pair_covariances(None, C.c_int(n), P(a["cls"]), P(a["sa"]), P(a["ia"]), P(a["sb"]), P(a["ib"]),
                                                                    None if out_null else P(out), P(st))
        assert rc == INVALID, (change, rc)
        err = s.api.last_error()
        assert "chol_batch_get_landmark_pair_covariances" in err and why in err, (change, err)
        assert (out == 77).all() and (st == 77).all()

    refused("the batch is NULL")                                        # (a cube pair among them: every class is served)
    for name in good:
        refused("pointer is NULL", **{name: None})
    refused("pointer is NULL", out_null=True)
    refused("n < 0", n=-1)
    refused("not a landmark class", cls=put(1, 3))

    def search(why, cls=2, radius=1.0, cap=4, outs=True, total=True):
        sa, sb, ia, ib = np.full(4, 77, np.int32), np.full(4, 77, np.int32), np.full(4, 77, np.uint64), np.full(4, 77, np.uint64)
        dist, tot = np.full(4, 77.0), np.full(1, 77, np.int64)
        rc = s.lib().slide_chol_batch_landmark_pairs_within(None, C.c_int(cls), C.c_double(radius), C.c_int(1), C.c_int64(cap),
                                                            P(sa) if outs else None, P(ia), P(sb), P(ib), P(dist), P(tot) if total else None)
        assert rc == INVALID, (why, rc)
        err = s.api.last_error()
        assert "chol_batch_landmark_pairs_within" in err and why in err, err
        assert (sa == 77).all() and (ia == 77).all() and (dist == 77).all() and tot[0] == 77
    search("the batch is NULL")
    search("not a landmark class", cls=3)
    search("radius", radius=0.0)
    search("radius", radius=np.nan)
    search("cap < 0", cap=-1)
    search("pointer is NULL", outs=False)
    search("pointer is NULL", total=False)


def _case(name, chart):
    if name == "dup":
        return jp.dup_case(chart)
    return jo.JointObsCase(jg.shared_mix_case(2) if name == "shared_mix" else jg.relmeas_case(R=2, n_rel=3, P=14), chart)


@pytest.mark.parametrize("name", ["dup", "relmeas", "shared_mix"])
def test_pair_block_form_equals_the_dense_reference(name):
    """C = I + G0 + W^T D W on the joint system equals I + diag(1 / sigma) Sig_d diag(1 / sigma) off the dense inverse of the joint H
    for all four side combinations, points and cylinders, and the 2 D unit columns give the pair's joint marginal — the block between
    two robots' private landmarks included; a shared landmark's two names are one variable.  On relmeas the lambda rows counted
    positively miss by more than the bound: the sign is tested."""
    c = _case(name, 0)
    Y = jo.joint_system(c)
    assert Y["n_lam"] == (0 if name == "shared_mix" else 12 if name == "dup" else 18)
    worst = wrong = worst_cov = 0.0
    seen = set()
    for kind in ("point", "cylinder"):
        D = jp.DIM[kind]
        for note, row in jp.side_pairs(c, kind).items():
            seen.add(note)
            _, Cs, _ = jp.ref_pairs(c, kind, [row], c.cpu_values)
            top = float(np.abs(Cs[0]).max())
            worst = max(worst, float(np.abs(jp.pair_block_form(c, kind, row) - Cs[0]).max() / top))
            wrong = max(wrong, float(np.abs(jp.pair_block_form(c, kind, row, lambda_sign=1.0) - Cs[0]).max() / top))
            S = jp.ref_joint_cov(c, kind, row)
            worst_cov = max(worst_cov, float(np.abs(jp.pair_block_form(c, kind, row, cov=True) - S).max() / np.abs(S).max()))
            assert np.abs(S[:D, D:]).max() > 0
            for side in (0, 1):                                        # a shared side through its other replica: the same variable
                sl, i = row[2 * side], row[2 * side + 1]
                if jp.is_shared(c, sl, kind, i):
                    alt = list(row)
                    alt[2 * side:2 * side + 2] = jp.other_replica(c, kind, sl, i)
                    assert alt != list(row) and np.array_equal(jp.sel(c, kind, alt), jp.sel(c, kind, row))
    print(f"[joint-lm-pair-cases] {name}: block form against the dense inverse {worst:.2e} (covariances {worst_cov:.2e}; lambda rows counted "
          f"positively: {wrong:.2e}) over {sorted(seen)}")
    assert seen == {"private-private, one graph", "private-private, across", "private-shared", "shared-shared"}
    assert worst <= BLOCK_FORM_BOUND and worst_cov <= BLOCK_FORM_BOUND
    if name == "relmeas":
        assert wrong > BLOCK_FORM_BOUND


def test_planted_conditions_hold_on_both_charts():
    """DupJoint asserts on itself under d2_ref alone (joint_landmark_pair_cases.planted): true pairs below 0.25 of the quantile,
    distinct pairs above 1.5 of it — the cross-robot duplicates and the private re-mapping of a shared landmark among the true ones."""
    for chart in (0, 1):
        c = jp.dup_case(chart)
        for kind, n in (("point", 25), ("cylinder", 12)):
            rows, flags, cross, d2 = jp.planted(c, kind)
            q = jp.QUANTILE[jp.DIM[kind]]
            assert len(rows) == n and flags.sum() == (13 if kind == "point" else 6) and (cross & flags).sum() >= (9 if kind == "point" else 4)
            print(f"[joint-lm-pair-cases] chart {chart} {kind}: true max {d2[flags].max() / q:.4f} of the quantile, false min "
                  f"{d2[~flags].min() / q:.2f}")
        rows, flags, _, d2 = jp.planted(c, "point")
        r, gm, _, gs = c.J.remap
        assert tuple(rows[-1]) == (r, jo.local_id(c, r, 2, gm), r, jo.local_id(c, r, 2, gs)) and flags[-1]
        assert jp.is_shared(c, r, "point", int(rows[-1][3])) and not jp.is_shared(c, r, "point", int(rows[-1][1]))
        print(f"[joint-lm-pair-cases] chart {chart}: the private re-mapping of a shared point, d2_ref {d2[-1]:.4f}")


def test_brute_force_search_on_a_union_of_robots():
    """The reference of the search: every shared landmark once, through its lowest replica; cross_only drops exactly the pairs of two
    private landmarks of one robot."""
    c = jp.dup_case(0)
    for kind in ("point", "cylinder"):
        ents = jp.job_landmarks(c, kind)
        nvar = len({c.lm_var(sl, kind, i) for sl, i, _ in ents})
        assert nvar == len(ents) == sum(1 for k, *_ in c.J.lms if k == jp.CLS[kind])
        xyz = np.array([jp.anchor(kind, c.cpu_values.lm(sl, kind, i)) for sl, i, _ in ents])
        r = lp.clear_radius(xyz, 1.5)
        every, cross = jp.brute_job_pairs(ents, xyz, r), jp.brute_job_pairs(ents, xyz, r, cross_only=True)
        assert 0 < len(cross[0]) < len(every[0])
        grp = {(sl, i): g for sl, i, g in ents}
        dropped = set(zip(*[x.tolist() for x in every[:4]])) - set(zip(*[x.tolist() for x in cross[:4]]))
        assert dropped and all(grp[a, b] == grp[cc, d] >= 0 for a, b, cc, d in dropped)
        assert all(grp[a, b] != grp[cc, d] for a, b, cc, d in zip(*[x.tolist() for x in cross[:4]]))
        rows, flags, cr, _ = jp.planted(c, kind)
        found = set(zip(*[x.tolist() for x in cross[:4]]))
        for row, f, x in zip(rows.tolist(), flags, cr):                # every planted cross pair lies within the radius, in either order
            if x:
                assert tuple(row) in found or (row[2], row[3], row[0], row[1]) in found, row
