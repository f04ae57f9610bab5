"""Timing of select_consistent_closures: 64, 512 and 4096 closures in one group and 28 groups of 64, against the numpy
restatement of tests/closure_cases.py (here evaluated row by row over whole arrays of pairs: the same formulas, checked against the
pair-by-pair text on the first case) followed by the oracle's orc_clipper_solve on the same host.  Wall times with the device
synchronised around the timed region: the median of REPS repetitions after WARM warm-ups (the 4096-closure comparand: one run, it
takes minutes).  No threshold is set on these times: there is no earlier path to compare against.

    timeout -k 10 1100 python tools/closure_select_timing.py > profiles/closure_select_timing.txt
    python tools/closure_select_timing.py --device-only      # the device times alone (seconds): for comparing two builds of the library
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPS, WARM = 7, 2


def _poses(p7):
    p = np.asarray(p7, float)
    q = p[:, 3:] / np.linalg.norm(p[:, 3:], axis=1)[:, None]
    x, y, z, w = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    return R, p[:, :3].copy()


def _mul(A, B):
    return A[0] @ B[0], (A[0] @ B[1][..., None])[..., 0] + A[1]


def _inv(A):
    Rt = np.swapaxes(A[0], -1, -2)
    return Rt, -(Rt @ A[1][..., None])[..., 0]


def restate_rows(c, cc):
    """closure_cases.restate's score matrix, one row of pairs at a time"""
    F, T, Z = _poses(c.from_pose7), _poses(c.to_pose7), _poses(c.rel7)
    U = _mul(Z, _inv(T))                         # z_k T_k^-1
    Gi = _inv(_mul(F, U))                        # T_k z_k^-1 F_k^-1
    L = len(c)
    sg2, od2 = c.sigma6 ** 2, cc.ODOM_SIGMA6 ** 2
    fi, ti = c.from_idx.astype(np.int64), c.to_idx.astype(np.int64)
    M = np.zeros((L, L))
    for i in range(L - 1):
        j = np.arange(i + 1, L)
        R, t = _mul(_mul((U[0][i], U[1][i]), (Gi[0][j], Gi[1][j])), (F[0][i], F[1][i]))
        v = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)
        s = np.linalg.norm(v, axis=1) / 2
        th = np.arctan2(s, (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1) / 2)
        small = th < 1e-7
        ths, ss = np.where(small, 1.0, th), np.where(small, 1.0, s)
        w = np.where(small[:, None], v / 2, (ths / (2 * ss))[:, None] * v)
        k = np.where(small, 0.0, (1 - ths / (2 * np.tan(ths / 2))) / (ths * ths))
        wt = np.cross(w, t)
        u = t - wt / 2 + k[:, None] * np.cross(w, wt)
        legs = np.abs(fi[i] - fi[j]) + np.abs(ti[i] - ti[j])
        s2 = sg2[i] + sg2[j] + legs[:, None] * od2
        d = np.sqrt((np.concatenate([w, u], axis=1) ** 2 / s2).sum(axis=1))
        sc = np.where(d < cc.GATE, np.exp(-0.5 * d * d / cc.SIGMA ** 2), 0.0)
        M[i, j] = M[j, i] = np.where(sc > cc.AFFINITYEPS, sc, 0.0)
    return M


def main(device_only=False):
    import torch
    torch.zeros(1, device=torch.device("cuda", 0))      # (torch initialises the device before the library's HIP runtime is loaded)
    import closure_cases as cc
    import slide_slam_amd as s
    p = s.closure_params(odom_sigma6=cc.ODOM_SIGMA6)
    small = cc.planted_case(1)
    assert np.abs(restate_rows(small, cc) - small.M).max() < 1e-9          # the row-wise evaluation is the restatement

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    print(f"select_consistent_closures against numpy restatement + orc_clipper_solve, ms wall, median of {REPS} after {WARM} warm-ups")
    shapes = [("64 closures, one group", [(64, 16)]), ("512 closures, one group", [(512, 64)]), ("4096 closures, one group", [(4096, 256)]),
              ("28 groups of 64", [(64, 16)] * 28)]
    for name, groups in shapes:
        cases = [cc.planted_case(100 + k, N=90, n_true=nt, n_false=L - nt, restated=False) for k, (L, nt) in enumerate(groups)]
        pairs = [(a, b) for a in range(8) for b in range(a + 1, 8)]
        cl, fp, tp = [], [], []
        for k, c in enumerate(cases):
            cl += c.closures(pairs[k] if len(cases) > 1 else (0, 0))
            fp.append(c.from_pose7)
            tp.append(c.to_pose7)
        fp, tp = np.concatenate(fp), np.concatenate(tp)

        def device():
            return s.select_consistent_closures(cl, fp, tp, params=p)

        def host():
            return [cc.oracle_select(restate_rows(c, cc)) for c in cases]
        big = sum(len(c) for c in cases) >= 4096 and len(cases) == 1
        for _ in range(WARM):
            out = device()
        t_dev = [timed(device) for _ in range(REPS)]
        if device_only:
            print(f"({name}) device {np.median(t_dev):9.3f} ms ({min(t_dev):.3f} - {max(t_dev):.3f}); kept {int(np.sum(out['keep']))} of {len(cl)}", flush=True)
            continue
        t_host = [timed(host)] if big else [timed(host) for _ in range(WARM + REPS)][WARM:]
        sel = host()
        at, agree = 0, 0
        for c, nodes in zip(cases, sel):
            agree += sorted(np.nonzero(out["keep"][at:at + len(c)])[0].tolist()) == nodes
            at += len(c)
        print(f"({name}) device {np.median(t_dev):9.3f} ms ({min(t_dev):.3f} - {max(t_dev):.3f}); numpy + oracle {np.median(t_host):11.3f} ms "
              f"({min(t_host):.3f} - {max(t_host):.3f}, {len(t_host)} run(s)); the two select the same set in {agree} of {len(cases)} groups", flush=True)


if __name__ == "__main__":
    main("--device-only" in sys.argv)
