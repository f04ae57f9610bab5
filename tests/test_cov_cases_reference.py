"""cov_cases.py checked on the host: the long-double reference is an inverse, the float64 restatement of the kernels' recurrences passes
the three kinds of bound the GPU tests apply, the tolerances of kind (c) do not swamp the check, and a restatement with one planted error
of each kind fails the check that is meant to catch it.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cov_cases as cc                                                         # noqa: E402
from cov_cases import LD, NB, U                                                # noqa: E402


def _run(m, lds, plant=None, steps=None):
    buf = np.full(lds * m["Trow"] * NB, cc.OUT_NAN)
    Sg0 = buf.copy()
    for (i, j), t in m["given"].items():
        cc.put(Sg0, lds, i, j, t)
    prep = cc.restate(m, lds, Sg0, buf, stage=0, plant=plant)
    full = cc.restate(m, lds, Sg0, buf, stage=1, plant=plant, steps=steps)
    return prep, full


@pytest.mark.parametrize("name", cc.PROFILE_CASES)
def test_restatement_passes_on_profiles(name):
    m = cc.profile_model(name)
    for padded in (True, False):
        lds = cc.lds_of(m["Tc"], padded)
        (Sp, Zp, Xh), (Sg, Z, _) = _run(m, lds)
        ms, mz = cc.written_masks(m, lds)
        assert not np.isnan(cc.view(Sg, lds)[ms]).any() and not np.isnan(cc.view(Z, lds)[mz]).any()
        assert cc.same_bits(cc.view(Sg, lds)[~ms], np.full((~ms).sum(), cc.OUT_NAN))
        rx, (rz, rp), ra, rc = cc.check_xhat(m, Xh), cc.check_b(m, lds, Sp, Zp), cc.check_a(m, lds, Sg, Z, Sp), cc.check_c_sigma(m, lds, Sg)
        print(f"[cov-cases] {name} ld {lds}: Xhat {rx:.3f}  Z {rz:.3f}  P {rp:.3f}  (a) {ra:.3f}  (c) {rc:.3f}")
        assert rx <= 1 and rz <= 1 and rp <= 1 and ra <= 1 and rc <= 1


@pytest.mark.parametrize("name", cc.PROFILE_CASES)
def test_tolerances_do_not_swamp(name):
    """Kind (c)'s tolerances stay below n u kappa_2 max|ref| / 16: an error of the size conditioning alone would excuse still fails."""
    m = cc.profile_model(name)
    n, kap = m["Tc"] * NB, cc.kappa2(m)
    assert 4 <= kap <= 16, kap
    tol, err, mx = cc.sigma_tolerance(m)
    assert tol < n * U * kap * mx / 16, (tol, err, mx)
    if name in ("band3", "stairs", "dense5"):
        for kind in ("dense", "unit"):
            r = cc.solve_reference(name, kind)
            for q in ("W", "X"):
                assert r["tol_" + q] < n * U * kap * float(np.abs(r[q]).max()) / 16, (kind, q, r["tol_" + q], r["err_" + q])
    if name == "band3":
        for row0 in (0, 60, 6 * ((n - 6) // 6), n - NB):
            cov, tol, err = cc.pose_cov_reference(name, row0)
            assert tol < n * U * kap * float(np.abs(cov).max()) / 16, (row0, tol, err)


@pytest.mark.parametrize("name", cc.PROFILE_CASES)
def test_reference_is_the_inverse(name):
    """(L L^T) Sigma = I on the profile, to long-double rounding: the columns of the first, a middle and the last block column."""
    m = cc.profile_model(name)
    ref = cc.reference(m)
    L = cc.dense_L(m).astype(LD)
    Xf = ref["Xfull"]
    n = m["Tc"] * NB
    assert float(np.abs(L @ Xf - np.eye(n)).max()) < 64 * float(np.finfo(LD).eps)
    for k in sorted({0, m["Tc"] // 2, m["Tc"] - 1}):
        col = Xf.T @ Xf[:, k * NB:(k + 1) * NB]                                # Sigma(:, block column k)
        res = L @ (L.T @ col)
        res[k * NB:(k + 1) * NB] -= np.eye(NB)
        assert float(np.abs(res).max()) < 256 * n * float(np.finfo(LD).eps)
        for i in [k] + m["rows"][k]:
            assert float(np.abs(col[i * NB:(i + 1) * NB] - ref["Sigma"][(i, k)]).max()) < 64 * n * float(np.finfo(LD).eps)


@pytest.mark.parametrize("name", ["two_store", "gaps", "lambda", "uneven_step", "as_one_store"])
def test_restatement_passes_on_joint_systems(name):
    m = cc.joint_model(name)
    _, _, lds = cc.joint_dims(name, m)
    steps = [[(0, k) for k in range(m["Tc"])]] if name == "uneven_step" else None
    (Sp, Zp, Xh), (Sg, Z, _) = _run(m, lds, steps=steps)
    ms, mz = cc.written_masks(m, lds)
    assert not np.isnan(cc.view(Sg, lds)[ms]).any() and not np.isnan(cc.view(Z, lds)[mz]).any()
    rx, (rz, rp), ra = cc.check_xhat(m, Xh), cc.check_b(m, lds, Sp, Zp), cc.check_a(m, lds, Sg, Z, Sp)
    rc = cc.check_c_sigma(m, lds, Sg) if m["Trow"] == m["Tc"] else 0.0
    print(f"[cov-cases] joint {name}: Xhat {rx:.3f}  Z {rz:.3f}  P {rp:.3f}  (a) {ra:.3f}  (c) {rc:.3f}")
    assert rx <= 1 and rz <= 1 and rp <= 1 and ra <= 1 and rc <= 1
    if name == "lambda":                                                       # Sigma = (L D L^T)^-1 with D = -I on the last column
        L, d = cc.dense_L(m).astype(LD), cc.dvec(m).astype(LD)
        Xf = cc.reference(m)["Xfull"]
        S = (Xf * d[:, None]).T @ Xf
        assert float(np.abs((L * d[None, :]) @ L.T @ S - np.eye(len(d))).max()) < 1e-15


def test_solves_and_pose_covariance_restatement():
    for name in ("band3", "stairs", "dense5"):
        for kind in ("dense", "unit"):
            r = cc.solve_reference(name, kind)
            print(f"[cov-cases] solve {name} {kind}: restatement err W {r['err_W']:.2e} X {r['err_X']:.2e}  tol W {r['tol_W']:.2e} X {r['tol_X']:.2e}")
            assert r["err_W"] <= r["tol_W"] and r["err_X"] <= r["tol_X"]
            if kind == "unit":
                assert set(np.unique(r["B"])) == {0.0, 1.0} and np.all(r["B"].sum(axis=1) == 1)


PLANTS = [("drop", 3, 1), ("untransposed", 2, 1), ("skip_row", 3, 2)]


@pytest.mark.parametrize("plant", PLANTS, ids=[p[0] for p in PLANTS])
def test_planted_tile_errors_fail_check_a(plant):
    """stairs, columns 1 and 2 (I = 2 .. 4 and 3 .. 4): one k-step of four dropped, Sigma(j, i) untransposed, one row of I skipped."""
    m = cc.profile_model("stairs")
    lds = cc.lds_of(m["Tc"], True)
    (Sp, _, _), (Sg, Z, _) = _run(m, lds, plant=plant)
    ra = cc.check_a(m, lds, Sg, Z, Sp)
    print(f"[cov-cases] planted {plant}: (a) {ra:.3e}")
    assert ra > 1
    assert cc.check_c_sigma(m, lds, Sg) > 1


def test_planted_sign_fails_check_b():
    m = cc.joint_model("lambda")
    _, _, lds = cc.joint_dims("lambda", m)
    (Sp, Zp, _), (Sg, Z, _) = _run(m, lds, plant=("sign", 3))
    rz, rp = cc.check_b(m, lds, Sp, Zp)
    assert rz <= 1 and rp > 1
    assert cc.check_c_sigma(m, lds, Sg) > 1


def test_gram_reference_bound_catches_a_dropped_row():
    X, rows, _, ref, bound = cc.gram_case(17, 65, "scattered")
    used = X[:, rows]
    assert np.all(np.abs(used @ used.T - ref).astype(np.float64) <= bound)
    short = used[:, :-1]
    assert np.any(np.abs(short @ short.T - ref).astype(np.float64) > bound)
