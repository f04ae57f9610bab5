"""PlaceRecognition::findInterLoopClosureWithClipper (place_recognition.cpp:541-629) on the GPU: the single call against the existing
run_semantic_clipper on hand-filtered maps, the list form (k_tri_match_seg, k_affinity_csr_seg, one k_clq_solve_b launch) against the
single call bit for bit, and both against the oracle.

The new entry points return no inlier list (the C signature has no such output), so where the oracle check compares the SELECTED point
pairs it takes them from the existing semantic_clipper on the same triangles and start weights, after asserting that its counts and
transform are the new call's."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KW = dict(sigma=0.05, epsilon=0.15, num_inliers_threshold=4, matching_threshold=0.1, min_num_map_objects_to_start=5)
SEEDS = (200, 201, 202, 203)


def _seeded(seed, n=45, nq=28, span=30.0):
    """the generator of test_run_semantic_clipper_from_maps (tests/test_gpu_place.py)"""
    rng = np.random.default_rng(seed)
    ref = np.zeros((n, 7)); ref[:, 0] = 1; ref[:, 1:3] = rng.uniform(-span, span, (n, 2))
    yaw = rng.uniform(-np.pi, np.pi)
    R = np.array([[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]])
    t = rng.uniform(-5, 5, 2)
    sel = rng.permutation(n)[:nq]
    qry = np.zeros((nq, 7)); qry[:, 0] = 1
    qry[:, 1:3] = (ref[sel, 1:3] - t) @ R + rng.normal(0, 0.01, (nq, 2))
    return ref, qry, R, t


def _with_zero_rows(m, where):
    """(label, 0, 0, ...) rows mixed in at the given positions (z and the dimensions non-zero: only x and y decide)"""
    out = m
    for w in where:
        row = np.array([[2.0, 0.0, 0.0, 1.5, 0.3, 0.3, 0.3]])
        out = np.concatenate([out[:w], row, out[w:]], axis=0)
    return out


def _filtered(m):
    return m[~((m[:, 1] == 0.0) & (m[:, 2] == 0.0))]


def _load_map(name):
    a = np.loadtxt(os.path.join(HERE, "golden", name))
    out = np.zeros((a.shape[0], 7))
    out[:, :4] = a[:, :4]
    return out


def _xy_map(xy):
    m = np.zeros((len(xy), 7)); m[:, 0] = 1; m[:, 1:3] = xy
    return m


def _maps_with_triangle_counts(gpu, want_model=65):
    """a map whose Delaunay triangulation has 65 triangles, and a convex pentagon (3 triangles) holding a moved copy of the first map's
    LAST triangle — data triangle 64 of a 65-triangle scan is the one that matches.  The pentagon: the triangle and two far points on the
    line through its centroid parallel to one edge, so that all five are in convex position."""
    for seed in range(400, 600):
        big = np.random.default_rng(seed).uniform(-30, 30, (38, 2))
        tri = gpu.delaunay_2d(big)
        if len(tri) != want_model:
            continue
        last = big[tri[-1]]
        c = last.mean(axis=0)
        for e in range(3):
            d = last[(e + 1) % 3] - last[e]
            d = d / np.linalg.norm(d)
            small = np.concatenate([last, [c - 4000.0 * d, c + 4000.0 * d]], axis=0) + np.array([3.0, -2.0])
            t5 = gpu.delaunay_2d(small)
            if len(t5) == 3 and any(sorted(t) == [0, 1, 2] for t in t5.tolist()):
                return _xy_map(big), _xy_map(small)
    raise AssertionError("no 65 / 3 triangle pair found")


@pytest.fixture(scope="module")
def case(gpu):
    """ONE list with every situation the list form meets, evaluated once as a list and once pair by pair"""
    maps, pairs, u0s, names = [], [], [], []

    def add(ref, qry, name, u0=None):
        maps.extend([ref, qry])
        pairs.append((len(maps) - 2, len(maps) - 1))
        u0s.append(u0)
        names.append(name)

    p = gpu.slidegraph_params(**KW)
    big65, small3 = _maps_with_triangle_counts(gpu)
    add(big65, small3, "65x3")                                        # 65 rows: the next pair starts at wave 1 of a workgroup
    truth = {}
    for seed in SEEDS:
        ref, qry, R, t = _seeded(seed)
        add(_with_zero_rows(ref, (0, 7, 30)), _with_zero_rows(qry, (3, 28)), f"seed{seed}")
        truth[f"seed{seed}"] = (R, t)
    add(small3, big65, "3x65")                                        # 3 rows, 65 data triangles: a second 64-lane chunk of one lane
    r0, r1 = _load_map("robot0Map_indoor.txt"), _load_map("robot1Map_indoor.txt")
    maps.extend([r0, r1])
    i0 = len(maps) - 2
    for a, b, name in ((i0, i0 + 1, "robot01"), (i0 + 1, i0, "robot10")):            # each map named by two pairs
        pairs.append((a, b)); u0s.append(None); names.append(name)
    rng = np.random.default_rng(11)
    add(_xy_map(rng.uniform(-30, 30, (30, 2))), _xy_map(rng.uniform(-30, 30, (4, 2))), "gate")
    add(_xy_map(rng.uniform(-30, 30, (25, 2))), _xy_map(rng.uniform(-3e4, 3e4, (25, 2))), "far-apart scales")
    line = np.stack([np.linspace(1, 40, 25), 0.5 * np.linspace(1, 40, 25)], axis=1)
    add(_xy_map(rng.uniform(-30, 30, (25, 2))), _xy_map(line), "collinear query")
    ref, qry, _, _ = _seeded(300, n=150, nq=130, span=12.0)
    add(ref, qry, "large")                                            # >= 1024 associations: the cooperative route
    # explicit start weights for some pairs (their lengths from a first, single evaluation), NULL for the others
    singles = [gpu.find_inter_loop_closure_clipper(maps[a], maps[b], p) for a, b in pairs]
    for k, name in enumerate(names):
        if name in ("seed201", "seed203", "robot10", "65x3"):
            u0s[k] = np.random.default_rng(50 + k).uniform(0, 1, singles[k]["n_putative"])
            singles[k] = gpu.find_inter_loop_closure_clipper(maps[pairs[k][0]], maps[pairs[k][1]], p, u0s[k])
    many = gpu.find_inter_loop_closures_clipper(maps, pairs, p, u0s)
    return dict(maps=maps, pairs=pairs, u0s=u0s, names=names, p=p, singles=singles, many=many, truth=truth)


def _same(a, b):
    return (a["found"] == b["found"] and np.array_equal(a["tf"], b["tf"]) and a["n_putative"] == b["n_putative"] and a["n_inliers"] == b["n_inliers"]
            and a["n_ref_used"] == b["n_ref_used"] and a["n_qry_used"] == b["n_qry_used"])


def test_wrapper_against_the_existing_call(gpu, case):
    """found / n_putative / n_inliers equal run_semantic_clipper's on the hand-filtered maps, tf is the inverse of its tf, and where
    found it is (R, t) within the parent test's tolerances turned round.  Checked for EVERY pair of the list that passes the gate
    (the existing call has no gate), so the 65-triangle chunk boundary and the cooperative route are held against the old kernels too."""
    found = 0
    for k, name in enumerate(case["names"]):
        if name == "gate":
            continue
        a, b = case["pairs"][k]
        ref, qry = _filtered(case["maps"][a]), _filtered(case["maps"][b])
        new = case["singles"][k]
        old = gpu.run_semantic_clipper(ref, qry, sigma=KW["sigma"], epsilon=KW["epsilon"], min_num_pairs=KW["num_inliers_threshold"],
                                       matching_threshold=KW["matching_threshold"], u0=case["u0s"][k])
        print(f"{name}: kept {new['n_ref_used']}/{new['n_qry_used']} putative {new['n_putative']} inliers {new['n_inliers']} found {new['found']}")
        assert (new["n_ref_used"], new["n_qry_used"]) == (len(ref), len(qry)), name
        assert new["found"] == old["found"] and new["n_putative"] == old["n_putative"] and new["n_inliers"] == old["n_inliers"], name
        assert np.abs(new["tf"] - np.linalg.inv(old["tf"])).max() <= 1e-12, name
        if name in case["truth"] and new["found"]:
            found += 1
            R, t = case["truth"][name]
            assert np.abs(new["tf"][:2, :2] - R).max() < 0.02 and np.abs(new["tf"][:2, 3] - t).max() < 0.3, name
    assert found >= 3
    names = case["names"]
    assert case["singles"][names.index("seed200")]["n_ref_used"] == 45 and case["singles"][names.index("seed200")]["n_qry_used"] == 28


def test_batch_equals_the_single_call_bit_for_bit(gpu, case):
    names, singles, many = case["names"], case["singles"], case["many"]
    assert len(many) == len(singles) == 12
    for name, one, m in zip(names, singles, many):
        assert m["status"] == 0, name
        assert _same(one, m), (name, one, m)
    by = dict(zip(names, many))
    assert by["large"]["n_putative"] >= 1024                                   # the cooperative route was taken
    assert by["gate"]["n_qry_used"] == 4 and not by["gate"]["found"] and by["gate"]["n_putative"] == 0
    assert by["far-apart scales"]["n_putative"] == 0 and not by["far-apart scales"]["found"]
    assert by["collinear query"]["n_putative"] == 0 and by["collinear query"]["n_qry_used"] == 25
    assert by["3x65"]["n_putative"] >= 3 and by["65x3"]["n_putative"] >= 3      # the planted triangle: data triangle 64 / model row 64
    for name in ("gate", "far-apart scales", "collinear query"):
        assert np.array_equal(by[name]["tf"], np.eye(4))
    assert sum(by[f"seed{s}"]["found"] for s in SEEDS) >= 3
    tri = lambda m: len(gpu.delaunay_2d(m[:, 1:3]))
    a, b = case["pairs"][0]
    assert (tri(case["maps"][a]), tri(case["maps"][b])) == (65, 3)


def test_a_pair_does_not_depend_on_the_list(gpu, case):
    """alone, first of 3 and last of 17: the same bits"""
    k = case["names"].index("seed201")
    a, b = case["pairs"][k]
    ref, qry, u0 = case["maps"][a], case["maps"][b], case["u0s"][k]
    fill = [_seeded(500 + i)[:2] for i in range(16)]
    alone = gpu.find_inter_loop_closures_clipper([ref, qry], [(0, 1)], case["p"], [u0])[0]
    maps3 = [ref, qry, fill[0][0], fill[0][1], case["maps"][case["pairs"][-1][0]], case["maps"][case["pairs"][-1][1]]]
    first = gpu.find_inter_loop_closures_clipper(maps3, [(0, 1), (2, 3), (4, 5)], case["p"], [u0, None, None])[0]
    maps17 = [m for f in fill for m in f] + [ref, qry]
    last = gpu.find_inter_loop_closures_clipper(maps17, [(2 * i, 2 * i + 1) for i in range(17)], case["p"], [None] * 16 + [u0])[-1]
    for other in (alone, first, last, case["many"][k]):
        assert _same(case["singles"][k], other) and other["status"] == 0
    assert case["singles"][k]["n_putative"] > 0


def test_same_bits_on_two_runs(gpu, case):
    again = gpu.find_inter_loop_closures_clipper(case["maps"], case["pairs"], case["p"], case["u0s"])
    for a, b in zip(case["many"], again):
        assert _same(a, b) and a["status"] == b["status"]


def test_status_is_per_pair(gpu, case):
    """a wrong n_u0[k]: SLIDE_ERR_INVALID for that pair alone (found 0, identity), its neighbours unchanged"""
    k = case["names"].index("seed202")
    u0s = list(case["u0s"])
    u0s[k] = np.ones(case["many"][k]["n_putative"] + 1)
    got = gpu.find_inter_loop_closures_clipper(case["maps"], case["pairs"], case["p"], u0s)
    assert got[k]["status"] == -1 and not got[k]["found"] and np.array_equal(got[k]["tf"], np.eye(4))
    for j, (a, b) in enumerate(zip(case["many"], got)):
        if j != k:
            assert _same(a, b) and b["status"] == 0
    with pytest.raises(gpu.SlideError):            # the single call reports the pair's fault as its return value
        a, b = case["pairs"][k]
        gpu.find_inter_loop_closure_clipper(case["maps"][a], case["maps"][b], case["p"], u0s[k])


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_against_the_oracle(gpu, case):
    """orc_semantic_clipper on scipy-qhull triangles under the conditions of test_semantic_clipper_pipeline: inlier counts equal, the
    selected point pairs as sets within 2, the transform within 1e-3 after inversion.  The start weights follow the associations from
    the product's triangle order to qhull's (a matched triangle pair is known by its twelve coordinates)."""
    from test_gpu_place import _oracle_clipper_params, _triangles
    for seed in SEEDS:
        k = case["names"].index(f"seed{seed}")
        a, b = case["pairs"][k]
        ref, qry = _filtered(case["maps"][a])[:, 1:3], _filtered(case["maps"][b])[:, 1:3]
        tm_g = np.ascontiguousarray(ref[gpu.delaunay_2d(ref)]); td_g = np.ascontiguousarray(qry[gpu.delaunay_2d(qry)])
        tm_o = np.ascontiguousarray(_triangles(ref).reshape(-1, 6)); td_o = np.ascontiguousarray(_triangles(qry).reshape(-1, 6))
        pts_g, _ = gpu.match_triangles(tm_g, td_g, KW["matching_threshold"])
        cap = len(tm_o) * len(td_o)
        pts_o = np.zeros((cap, 3, 4)); od = np.zeros(cap)
        n_o = po.lib().orc_match_triangles(_p(tm_o), C.c_int(len(tm_o)), _p(td_o), C.c_int(len(td_o)), C.c_double(KW["matching_threshold"]), _p(pts_o),
                                           _p(od), C.c_int(cap))
        pts_o = pts_o[:n_o]
        m = 3 * len(pts_g)
        assert n_o == len(pts_g) and m > 0
        where = {tuple(r.ravel()): i for i, r in enumerate(pts_g)}
        u0_g = np.random.default_rng(seed).uniform(0, 1, m)
        u0_o = np.concatenate([u0_g[3 * where[tuple(r.ravel())]:3 * where[tuple(r.ravel())] + 3] for r in pts_o])
        new = gpu.find_inter_loop_closure_clipper(case["maps"][a], case["maps"][b], case["p"], u0_g)
        cp = gpu.clipper_params(sigma=KW["sigma"], epsilon=KW["epsilon"])
        old = gpu.semantic_clipper(tm_g, td_g, cp, min_num_pairs=KW["num_inliers_threshold"], matching_threshold=KW["matching_threshold"], u0=u0_g)
        assert (new["found"], new["n_putative"], new["n_inliers"]) == (old["found"], old["n_putative"], old["n_inliers"]) and new["n_putative"] == m
        assert np.abs(new["tf"] - np.linalg.inv(old["tf"])).max() <= 1e-12
        op = _oracle_clipper_params(sigma=KW["sigma"], epsilon=KW["epsilon"])
        tf = np.zeros(16); counts = np.zeros(2, np.int32); inl = np.zeros(m, np.int32)
        ok = po.lib().orc_semantic_clipper(_p(tm_o), C.c_int(len(tm_o)), _p(td_o), C.c_int(len(td_o)), C.byref(op), C.c_int(KW["num_inliers_threshold"]),
                                           C.c_double(KW["matching_threshold"]), _p(u0_o), _p(tf), _p(counts), _p(inl))
        assert counts[0] == m and new["found"] == bool(ok)
        assert new["n_inliers"] == counts[1]
        sel_g = {tuple(pts_g.reshape(-1, 4)[i]) for i in old["inliers"]}
        sel_o = {tuple(pts_o.reshape(-1, 4)[i]) for i in inl[:counts[1]]}
        assert len(sel_g ^ sel_o) <= 2
        assert np.abs(new["tf"] - np.linalg.inv(tf.reshape(4, 4))).max() < 1e-3


def test_list_is_not_slower_than_the_loop(gpu):
    """7 query maps of 45 objects against one reference, median of five after a warm-up: the list form against the loop over the existing
    run_semantic_clipper (the parent's path).  Held: not slower.  How much faster is printed, not held (profiles/slidegraph_batch_timing.txt)."""
    ref = _seeded(700)[0]
    qrys = []
    for i in range(7):                                   # seven robots' views of the same 45 objects
        rng = np.random.default_rng(710 + i)
        yaw, t = rng.uniform(-np.pi, np.pi), rng.uniform(-5, 5, 2)
        R = np.array([[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]])
        q = np.zeros((45, 7)); q[:, 0] = 1
        q[:, 1:3] = (ref[rng.permutation(45), 1:3] - t) @ R + rng.normal(0, 0.01, (45, 2))
        qrys.append(q)
    p = gpu.slidegraph_params(**KW)
    maps, pairs = [ref] + qrys, [(0, i + 1) for i in range(7)]

    def loop():
        return [gpu.run_semantic_clipper(ref, q, sigma=KW["sigma"], epsilon=KW["epsilon"], min_num_pairs=KW["num_inliers_threshold"],
                                         matching_threshold=KW["matching_threshold"]) for q in qrys]

    def batch():
        return gpu.find_inter_loop_closures_clipper(maps, pairs, p)

    def median_ms(f):
        f()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), min(ts), max(ts)

    lo, bo = loop(), batch()
    assert [r["n_putative"] for r in lo] == [r["n_putative"] for r in bo] and [r["found"] for r in lo] == [r["found"] for r in bo]
    assert bo[0]["found"]
    t_loop, t_batch = median_ms(loop), median_ms(batch)
    print(f"7 x 45 objects: loop of run_semantic_clipper {t_loop[0]:.2f} ms [{t_loop[1]:.2f}, {t_loop[2]:.2f}], "
          f"one list call {t_batch[0]:.2f} ms [{t_batch[1]:.2f}, {t_batch[2]:.2f}], ratio {t_loop[0] / t_batch[0]:.2f}")
    assert t_batch[0] <= t_loop[0]
