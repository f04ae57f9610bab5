"""The lambda block of an exact joint pass (the inter-robot relative-pose factors' own system) under SLIDE_LAM_FUSE: its products over the
two leaves inside the top block's launch (bit 1, launch_border_syrk_pairs) and the one-workgroup solve of a one-tile block (bit 2,
k_lam_solve1), each at the smallest shapes at which its branches can go wrong:

  lambda coordinates   6 (one factor), 60 (ten: the tile's padding rows 60 .. 63), 66 (eleven: two tiles — bit 2 must not engage, bit 1 must)
  separator            undissected (two robots: no leaf product, bit 2 alone); dissected with leaves of 2 and 6 tiles and a top block of
                       2 (the leaves' chunk counts 1 and 3, the top block's 2: three different cuts in one launch); a leaf of ONE tile
  a cut pass           PassDriver.force_parts on one process: parts 0 and 2, the product over ALL column blocks in front of the solve

Per case, from identical state: three passes with SLIDE_LAM_FUSE=0 (the separate launches) and three with =3, in one process.  After the
first and after the third pass every pose and every landmark estimate is the same bits, and so is a pose-pair marginal taken after the
passes (it reads lamS / lam_Ld through the joint selected inverse).  The =3 run is also held, pass by pass, against the independent joint
Gauss-Newton step exactly as test_gpu_joint_step.py holds its cases (gn_reference by QR, gn_reference.tolerance).  lam_dp and the
separator's solution have no accessor: they reach the comparison through the poses they move."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import joint_graphs as jg                                                      # noqa: E402
from gn_reference import scaled_error, tolerance                              # noqa: E402
from test_gn_reference import numdiff_floor                                    # noqa: E402
from test_gpu_joint_step import Run                                            # noqa: E402

pytestmark = pytest.mark.gpu

NB = 64
PASSES = 3


def tiles_case(cubes_a, cubes_b, cubes_top, n_rel, seed=23):
    """jg.separator_tiles_case with leaves of their own sizes (cubes of 9 coordinates shared inside robots 0, 1 / inside 2, 3 / across
    the halves) and n_rel relative-pose factors, every second one across the halves."""
    J = jg.Joint([16] * 4, seed=seed)
    rng = np.random.default_rng(seed)
    for (a, b), n in (((0, 1), cubes_a), ((2, 3), cubes_b)):
        for i in range(n):
            k = i % 16
            jg._add(J, 1, jg._near(J, a, k, rng), [(a, k), (b, (k + 1) % 16)], rng)
    for i in range(cubes_top):
        k = (3 * i) % 16
        jg._add(J, 1, jg._near(J, 1, k, rng), [(1, k), (2, (k + 2) % 16)], rng)
    for i in range(n_rel):
        a = i % 4
        ka = (2 * i + i // 8) % 16       # (no pose pair twice)
        J.relative(a, ka, (a + 1) % 4, ka if i % 2 == 0 else (ka + 3) % 16)
    jg.background(J, rng, every=4)
    return J


def leaf_chunks(T, nl):
    """Chunks of a leaf's lambda-block product (host_graph.hip: lam_ks_cap, then T / 2)."""
    t = (nl + 1) * nl
    cap = 16 if t <= 32 else max(1, min(16, 256 // t))
    return max(1, min(cap, T // 2))


def top_chunks(Ta, Tb, Tt, nl):
    """Chunks of the top block's product over the leaves (prepare_separator's sep_ks)."""
    nb = Tt + nl
    njobs = sum(nb + 1 - jb for jb in range(Tt))
    return max(1, min(8, (Ta + Tb) // 4, (1024 + njobs - 1) // njobs))


# name -> (builder, lambda coordinates, (Ta, Tb, Tt) or None = undissected, cut pass)
CASES = {
    "flat_6": (lambda: jg.relmeas_case(2, 1), 6, None, False),
    "flat_60": (lambda: jg.relmeas_case(2, 10), 60, None, False),
    "flat_66": (lambda: jg.relmeas_case(2, 11), 66, None, False),
    "leaves_2_6_lam_6": (lambda: tiles_case(14, 36, 8, 1), 6, (2, 6, 2), False),
    "leaves_2_6_lam_60": (lambda: tiles_case(14, 36, 8, 10), 60, (2, 6, 2), False),
    "leaves_2_6_lam_66": (lambda: tiles_case(14, 36, 8, 11), 66, (2, 6, 2), False),
    "leaf_of_one_tile": (lambda: tiles_case(7, 43, 8, 2), 12, (1, 7, 2), False),
    "cut_pass": (lambda: tiles_case(14, 36, 8, 1), 6, (2, 6, 2), True),
}


def check_layout(r, lam, blocks):
    """The case reaches the branch it is named for."""
    assert r.drv.lam_dim == lam
    sp = r.info.get("sep_prof")
    got = sp[1] if isinstance(sp, tuple) else None
    if blocks is None:
        assert got is None
        return
    Ta, Tb, Tt = blocks
    nl = (lam + NB - 1) // NB
    assert got is not None and (got[0], got[1]) == (Ta, Tb), got
    assert (r.info["sep_dim"] - NB * (Ta + Tb) + NB - 1) // NB == Tt
    ks = (leaf_chunks(Ta, nl), leaf_chunks(Tb, nl), top_chunks(Ta, Tb, Tt, nl))
    assert ks[2] > 1, ks                 # (the top block's product is split: a whole pass takes the one-launch path)
    assert ks[0] == 1 and len(set(ks)) == 3, ks      # one system without partial tiles, three different cuts in the launch


def passes(gpu, name, against_reference):
    """PASSES passes of the case; returns the values after the first and the last pass and the pose-pair marginal read afterwards."""
    import torch
    make, lam, blocks, cut = CASES[name]
    J = make()
    r = Run(gpu, J, 0)
    try:
        check_layout(r, lam, blocks)
        r.drv.force_parts = cut
        vals = r.values()
        assert np.array_equal(vals, r.ref.values)
        kept, worst = [], 0.0
        for s in range(PASSES):
            if against_reference:
                dx, H = r.ref.step(vals)
            r.drv.one_pass()
            torch.cuda.synchronize()
            new = r.values()
            assert np.all(np.isfinite(new))
            if against_reference:
                tol, kappa = tolerance(H, dx, r.ref.magnitude(vals), numdiff_floor(r.ref, dx, H, vals))
                err = scaled_error(r.ref.tangent(vals, new), dx, H)
                print(f"[lambda-block] {name} pass {s}: scaled_error {err:.3e} tolerance {tol:.3e}")
                assert np.linalg.norm(dx) > 1e-6 and err <= tol, (s, err, tol, kappa)
                worst = max(worst, err / tol)
            if s in (0, PASSES - 1):
                kept.append(new.copy())
            vals = new
        gate = None
        if not cut:                      # (a cut pass leaves no whole factor behind for the joint marginals)
            ka, a, b, _, kb = J.relmeas[0]
            cov, status = r.drv.get_pose_pair_covariances([(a, ka, b, kb), (0, 1, 1, 2)])
            assert not np.any(status) and np.all(np.isfinite(cov))
            gate = np.ascontiguousarray(cov)
        return kept, gate
    finally:
        r.close()


@pytest.mark.parametrize("name", list(CASES))
def test_lambda_block_fused_equals_separate(gpu, monkeypatch, name):
    monkeypatch.setenv("SLIDE_LAM_FUSE", "0")      # (read whenever a pass's launch sequence is built: one process takes both sides)
    sep, gate_sep = passes(gpu, name, False)
    monkeypatch.setenv("SLIDE_LAM_FUSE", "3")
    fus, gate_fus = passes(gpu, name, True)
    for k, (a, b) in enumerate(zip(sep, fus)):
        assert a.shape == b.shape
        assert a.tobytes() == b.tobytes(), (name, k, float(np.abs(a - b).max()))
    assert not np.array_equal(sep[0], sep[1])      # (the later passes moved the graph again)
    if gate_sep is not None:
        assert gate_sep.tobytes() == gate_fus.tobytes(), (name, float(np.abs(gate_sep - gate_fus).max()))
