"""An independent reference for ONE Gauss-Newton step of a factor graph (test infrastructure).

The graph is taken from the oracle (OracleGraph.export: variables, factors, and the sigmas graph.hpp chose for them); every factor is
linearised by the oracle's orc_linearize (pinned against central differences and the reference's vectors in test_oracle_pins.py) and
whitened there.  The FULL, unreduced Jacobian over all poses and landmarks is then solved as a least-squares problem by dense QR
(numpy.linalg.lstsq).  No Schur elimination, no tile profile and no product library are involved.

The reference is dense only: it refuses graphs of more than DENSE_MAX unknowns.  The large cases of test_gpu_gn_step.py (the Schur LDS
capacity boundary, the slot-table overflow) do not use it: the first has a per-landmark closed form, the second is refused.

Tangent vectors follow var_retract (oracle/graph.hpp): pose (+) = pose_retract in the chart, points and the scale of a cube
additive, a cylinder's tangent ordered [ray, root, radius] and additive.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import pyoracle as po

DIM = {po.V_POSE: 6, po.V_POINT: 3, po.V_CUBE: 9, po.V_CYL: 7}
DENSE_MAX = 3000
EPS = np.finfo(np.float64).eps


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pose_local(a12, b12, chart):
    out = np.zeros(6)
    po.lib().orc_pose_local(_p(np.ascontiguousarray(a12, float)), _p(np.ascontiguousarray(b12, float)), C.c_int(chart), _p(out))
    return out


def pose_retract(a12, xi, chart):
    out = np.zeros(12)
    po.lib().orc_pose_retract(_p(np.ascontiguousarray(a12, float)), _p(np.ascontiguousarray(xi, float)), C.c_int(chart), _p(out))
    return out


def local(vtype, old, new, chart):
    """Tangent vector d with new = old (+) d (var_retract)."""
    old, new = np.asarray(old, float), np.asarray(new, float)
    if vtype == po.V_POSE:
        return pose_local(old[:12], new[:12], chart)
    if vtype == po.V_POINT:
        return new[:3] - old[:3]
    if vtype == po.V_CUBE:
        return np.concatenate([pose_local(old[:12], new[:12], chart), new[12:15] - old[12:15]])
    return np.concatenate([new[3:6] - old[3:6], new[0:3] - old[0:3], new[6:7] - old[6:7]])


class Reference:
    """The graph of an OracleGraph (before its first solve) as data; step(values) is one Gauss-Newton step at `values`."""

    def __init__(self, og, chart, numdiff_delta=1e-6):
        e = og.export()
        self.chart, self.delta = chart, numdiff_delta
        self.vtype, self.vkey, self.values = e["var_type"], e["var_key"], e["var_val"].copy()
        self.ftype, self.fv, self.fz, self.fsig = e["f_type"], e["f_v"], e["f_z"], e["f_sigma"]
        dims = np.array([DIM[int(t)] for t in self.vtype], int)
        self.off = np.concatenate([[0], np.cumsum(dims)])
        self.n = int(self.off[-1])
        self.key2var = {int(k): i for i, k in enumerate(self.vkey)}

    # ---- keys as the oracle builds them (graph.hpp pose_key / lm_key) ----
    def pose_var(self, robot, idx):
        return self.key2var[_pose_key(robot, idx)]

    def lm_var(self, cls, idx):
        return self.key2var[(ord("lcu"[cls]) << 56) | int(idx)]

    def list_lengths(self):
        """Landmark factors per pose variable and per landmark variable (what the kernels' lists hold)."""
        lm = np.isin(self.ftype, (po.F_BR, po.F_CUBE, po.F_CYL))
        per_pose = np.bincount(self.fv[lm, 0], minlength=len(self.vtype))
        per_lm = np.bincount(self.fv[lm, 1], minlength=len(self.vtype))
        return per_pose, per_lm

    def linearize(self, values=None, delta=None):
        """Whitened Jacobian (COO rows, cols, vals), residual, at `values` (default: the graph's initial values)."""
        vals = self.values if values is None else values
        delta = self.delta if delta is None else delta
        L = po.lib()
        r, J0, J1 = np.zeros(9), np.zeros(81), np.zeros(81)
        pr, pJ0, pJ1 = _p(r), _p(J0), _p(J1)
        rows, cols, data, res = [], [], [], []
        m0 = 0
        for f in range(len(self.ftype)):
            t = int(self.ftype[f])
            v0, v1 = int(self.fv[f, 0]), int(self.fv[f, 1])
            x0 = np.ascontiguousarray(vals[v0])
            t1 = int(self.vtype[v1]) if v1 >= 0 else po.V_POSE
            x1 = np.ascontiguousarray(vals[v1]) if v1 >= 0 else None
            m = L.orc_linearize(C.c_int(t), _p(x0), C.c_int(t1), _p(x1) if x1 is not None else None, _p(self.fz[f]),
                                _p(self.fsig[f]), C.c_int(self.chart), C.c_double(delta), pr, pJ0, pJ1, C.c_int(1))
            res.append(r[:m].copy())
            for v, J in ((v0, J0), (v1, J1)):
                if v < 0:
                    continue
                d = DIM[int(self.vtype[v])]
                rr, cc = np.meshgrid(np.arange(m) + m0, np.arange(d) + self.off[v], indexing="ij")
                rows.append(rr.ravel()); cols.append(cc.ravel()); data.append(J[: m * d].copy())
            m0 += m
        return np.concatenate(rows), np.concatenate(cols), np.concatenate(data), np.concatenate(res)

    def step(self, values=None, delta=None):
        """dx minimising ||J dx + r|| at `values`, and H = J^T J (for scaled_error / tolerance)."""
        i, j, v, r = self.linearize(values, delta)
        m, n = len(r), self.n
        assert n <= DENSE_MAX, n          # (a dense QR: the cases keep to test sizes)
        J = np.zeros((m, n))
        np.add.at(J, (i, j), v)
        dx = np.linalg.lstsq(J, -r, rcond=None)[0]
        H = J.T @ J
        return dx, H

    def split(self, dx):
        return [dx[self.off[k]:self.off[k + 1]] for k in range(len(self.vtype))]

    def retract(self, values, dx):
        out = values.copy()
        for k, d in enumerate(self.split(dx)):
            t = int(self.vtype[k])
            if t in (po.V_POSE, po.V_CUBE):
                out[k, :12] = pose_retract(values[k, :12], d[:6], self.chart)
                if t == po.V_CUBE:
                    out[k, 12:15] = values[k, 12:15] + d[6:9]
            elif t == po.V_POINT:
                out[k, :3] = values[k, :3] + d
            else:
                out[k, 3:6] = values[k, 3:6] + d[:3]
                out[k, 0:3] = values[k, 0:3] + d[3:6]
                out[k, 6] = values[k, 6] + d[6]
        return out

    def magnitude(self, values):
        """Per tangent coordinate, the size of the value it moves (rotations: 1; translations, points, scales: their norm)."""
        out = []
        for k in range(len(self.vtype)):
            t, x = int(self.vtype[k]), values[k]
            if t in (po.V_POSE, po.V_CUBE):
                out += [1.0] * 3 + [np.linalg.norm(x[9:12])] * 3 + ([np.linalg.norm(x[12:15])] * 3 if t == po.V_CUBE else [])
            elif t == po.V_POINT:
                out += [np.linalg.norm(x[:3])] * 3
            else:
                out += [np.linalg.norm(x[3:6])] * 3 + [np.linalg.norm(x[0:3])] * 3 + [abs(x[6])]
        return np.array(out)

    def tangent(self, old, new):
        """Stacked tangent vectors new_k = old_k (+) d_k over all variables."""
        return np.concatenate([local(int(self.vtype[k]), old[k], new[k], self.chart) for k in range(len(self.vtype))])


def _pose_key(robot, idx):
    cs = "xyzmnopqrstvw"
    return (ord(cs[robot]) << 56) | int(idx)


def scaled_error(dx, dx_ref, H):
    """||W (dx - dx_ref)|| / ||W dx_ref||, W = diag(H)^(1/2): the norm in which a normal-equations solve's error is bounded by the
    condition number of the Jacobi-scaled H (van der Sluis: diagonal scaling does not change the computed Cholesky factor's
    backward error, so kappa(W^-1 H W^-1), not kappa(H), governs the forward error there)."""
    w = np.sqrt(np.diag(H))
    return float(np.linalg.norm(w * (dx - dx_ref)) / np.linalg.norm(w * dx_ref))


def tolerance(H, dx_ref, mag, nd_floor=0.0):
    """Bound on scaled_error for a solve of the normal equations (what the product and the oracle do; the reference uses QR):
      8 n eps kappa_s          -- backward error of Cholesky (c n eps, c = 8) times kappa_s = cond(W^-1 H W^-1);
      + 10 nd_floor            -- cube / cylinder Jacobians come from central differences: their rounding noise moves dx by about
                                  nd_floor (measured by the caller: dx at numdiff_delta 1e-6 against 1.00001e-6), ten times that;
      + 8 eps ||W mag||/||W dx|| -- the step is read back as the difference of two stored values, each rounded to eps |x|
                                  (mag: Reference.magnitude)."""
    w = np.sqrt(np.diag(H))
    Hs = H / np.outer(w, w)
    kappa = float(np.linalg.cond(Hs))
    n = H.shape[0]
    return 8 * n * EPS * kappa + 10 * nd_floor + 8 * EPS * float(np.linalg.norm(w * mag) / np.linalg.norm(w * dx_ref)), kappa
