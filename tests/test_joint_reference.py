"""The multi-robot builders (tests/joint_graphs.py) and the joint reference on the CPU, before any GPU run: the shards hold exactly the
joint graph's factors (their whitened residuals after the value broadcast sum to the joint graph's), and oracle shards driven by
PassDriver(arrow=True) — the exact joint pass, phases 40 / 41 / 42 — take gn_reference's joint Gauss-Newton step, pass after pass,
poses and landmarks alike."""
import copy
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import joint_graphs as jg                                                      # noqa: E402
from gn_reference import Reference, scaled_error, tolerance                     # noqa: E402
from oracle import pyoracle as po                                              # noqa: E402
from slide_slam_amd.distributed import PassDriver, setup_local_shards          # noqa: E402
from test_gn_reference import numdiff_floor                                    # noqa: E402

# (name, builder) — a representative subset of test_gpu_joint_step.py's cases
CASES = [
    ("lm_cyl_25", lambda: jg.landmark_count_case(0, 25)),
    ("lm_cube_49_shared", lambda: jg.landmark_count_case(1, 49, shared=True)),
    ("lm_point_65_shared", lambda: jg.landmark_count_case(2, 65, shared=True)),
    ("shared_mix_3", lambda: jg.shared_mix_case(3)),
    ("shared_mix_4", lambda: jg.shared_mix_case(4)),
    ("sizes_4", lambda: jg.sizes_case([10, 33, 65, 20], private_only=(2,))),
    ("relmeas_2", lambda: jg.relmeas_case(2, 3)),
    ("relmeas_4_lambda66", lambda: jg.relmeas_case(4, 11)),
]


def joint_reference(J, chart):
    og = po.OracleGraph(po.OrcParams.default(pose_chart=chart))
    J.emit_joint(og)
    return Reference(og, chart), og


def read_values(shards, gid, ref, sizes):
    """Every shard's estimate in the joint reference's variable layout: poses through get_pose12(0, k), landmarks through
    get_landmark — a shared landmark from EVERY replica, which must agree bit for bit."""
    out = ref.values.copy()
    seen = {}
    for r, sh in enumerate(shards):
        for k in range(sizes[r]):
            st, v = sh.graph.get_pose12(0, k)
            assert st == 0
            out[ref.pose_var(r, k), :12] = v
        for cls in range(3):
            for loc, g in enumerate(gid[r][cls]):
                st, v = sh.graph.get_landmark(cls, loc)
                assert st == 0
                i = ref.lm_var(cls, int(g))
                if i in seen:
                    assert np.array_equal(seen[i], v), (cls, int(g), r)
                seen[i] = v
                out[i, : len(v)] = v
    assert len(seen) == int((ref.vtype != po.V_POSE).sum())
    return out


def whitened_sq(ref, values=None, factors=None):
    """||r||^2 of the whitened residual of `ref` at `values`, over the factors `factors` (default: all)."""
    if factors is not None:
        ref = copy.copy(ref)
        ref.ftype, ref.fv, ref.fz, ref.fsig = ref.ftype[factors], ref.fv[factors], ref.fz[factors], ref.fsig[factors]
    r = ref.linearize(values)[3]
    return float(r @ r)


def oracle_setup(J, chart, before=None):
    shards, assoc = jg.build(J, lambda: po.OracleGraph(po.OrcParams.default(pose_chart=chart)))
    if before is not None:
        before(shards)
    bufs, info = setup_local_shards(shards, None, assoc=assoc)
    drv = PassDriver(shards, bufs, info["n_slots"], arrow=True, sep_dim=info["sep_dim"], sep_prof=info.get("sep_prof"))
    if J.relmeas:
        drv.setup_ghosts(J.relmeas)
    return shards, assoc[0], info, drv


def _ftype_counts(ref):
    return np.bincount(ref.ftype, minlength=5)


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_shards_hold_the_joint_graph(name, make, chart):
    """After the value broadcast every replica holds the joint graph's initial values (a shared landmark: its owner's), and the
    shards' factors are the joint graph's: counts per type, and the whitened residuals sum to ||r||^2 of the joint linearisation
    (the relative-pose factors, held by both robots as ghosts, counted once from the joint graph)."""
    J = make()
    ref, _ = joint_reference(J, chart)
    srefs = []
    shards, gid, info, _ = oracle_setup(J, chart, lambda shs: srefs.extend(Reference(sh.graph, chart) for sh in shs))
    vals = read_values(shards, gid, ref, J.sizes)
    assert np.array_equal(vals, ref.values)
    assert info["n_slots"] > 0
    total, counts, moved = 0.0, np.zeros(5, int), 0
    for r, (sh, sref) in enumerate(zip(shards, srefs)):
        svals = sref.values.copy()          # (the shard's own initial values, before the broadcast; now: the owners' values)
        for cls in range(3):
            for loc in range(len(gid[r][cls])):
                i = sref.lm_var(cls, loc)
                v = sh.graph.get_landmark(cls, loc)[1]
                moved += not np.array_equal(svals[i, : len(v)], v)
                svals[i, : len(v)] = v
        total += whitened_sq(sref, svals)
        counts += _ftype_counts(sref)
    rel = [f for f in range(len(ref.ftype)) if ref.ftype[f] == po.F_BETWEEN
           and (int(ref.vkey[ref.fv[f, 0]]) >> 56) != (int(ref.vkey[ref.fv[f, 1]]) >> 56)]
    assert len(rel) == len(J.relmeas)
    counts[po.F_BETWEEN] += len(rel)
    assert np.array_equal(counts, _ftype_counts(ref)), (counts, _ftype_counts(ref))
    assert moved > 0                    # (some replica's shared landmark started away from its owner's value)
    rel_sq = whitened_sq(ref, factors=np.array(rel, int)) if rel else 0.0
    full = whitened_sq(ref)
    assert np.isclose(total + rel_sq, full, rtol=1e-12, atol=0), (total + rel_sq, full)


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_oracle_exact_joint_pass_is_the_joint_step(name, make, chart):
    """Two exact joint passes of oracle shards, each against the reference's step at the point the pass starts from."""
    J = make()
    ref, _ = joint_reference(J, chart)
    shards, gid, info, drv = oracle_setup(J, chart)
    vals = read_values(shards, gid, ref, J.sizes)
    for s in range(2):
        dx, H = ref.step(vals)
        drv.one_pass()
        new = read_values(shards, gid, ref, J.sizes)
        got = ref.tangent(vals, new)
        tol, kappa = tolerance(H, dx, ref.magnitude(vals), numdiff_floor(ref, dx, H, vals))
        err = scaled_error(got, dx, H)
        assert np.linalg.norm(dx) > 1e-6
        assert err <= tol, (s, err, tol, kappa)
        vals = new
