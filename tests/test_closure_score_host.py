"""The scoring text of the loop-closure consistency matrix on the CPU: closure_prepare_one / closure_pair_score (kernels.hpp) are host +
device functions, the very text k_closure_prepare and k_closure_csr_seg call.  tests/closure_score_check.hip wraps them in a
stand-alone host program (no device is touched); here it is compiled and run over the CSR cases of tests/closure_cases.py and compared
with the numpy restatement: the pattern exactly, symmetric bit for bit, the values within 16 x the measured float64 / longdouble
spread of the restatement (floor 1e-13) — the GPU test's bound, reasoned there."""
import os
import subprocess

import numpy as np

import closure_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_host_build_of_the_scoring_text_equals_the_restatement(tmp_path):
    exe = str(tmp_path / "closure_score_check")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "slide_slam_amd", "csrc"),
                        os.path.join(ROOT, "tests", "closure_score_check.hip"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = [cc.csr_case(L, inter=L in (5, 64)) for L in (2, 5, 65)]
    tol = max(16 * cc.precision_spread(cases), 1e-13)
    for c in cases:
        L = len(c)
        rows = np.concatenate([c.from_pose7, c.to_pose7, c.rel7, c.sigma6, c.from_idx[:, None].astype(float), c.to_idx[:, None].astype(float)], axis=1)
        assert rows.shape == (L, 29)
        blob = np.concatenate([[float(L)], rows.reshape(-1), [cc.GATE, cc.SIGMA, cc.AFFINITYEPS], cc.ODOM_SIGMA6])
        fin, fout = str(tmp_path / f"in{L}.bin"), str(tmp_path / f"out{L}.bin")
        blob.astype(np.float64).tofile(fin)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and f"closure score ok L={L}" in r.stdout, r.stdout + r.stderr
        M = np.fromfile(fout, np.float64).reshape(L, L)
        assert np.array_equal(M != 0, c.M != 0) and np.array_equal(M, M.T)
        nz = c.M != 0
        rel = np.abs(M[nz] - c.M[nz]) / np.abs(c.M[nz])
        print(f"L={L}: largest relative difference to the restatement {rel.max():.3e} (allowed {tol:.3e})")
        assert rel.max() <= tol
        assert M[0, L - 1] == 1.0
