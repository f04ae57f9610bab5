"""The plain numpy references of tests/place_cases.py held against the oracle (CPU only), and every case's claimed edges asserted on
the reference's results — so that tests/test_gpu_place_edges.py can hold the kernels against these references and trust the cases."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import place_cases as pc  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

SWEEP = pc.sweep_cases()
TRIANGLES = pc.triangle_cases()
AFFINITY = pc.affinity_cases()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class OPlace(C.Structure):
    _fields_ = [("dilation_factor", C.c_double), ("xy_step", C.c_double), ("yaw_half_range", C.c_double),
                ("yaw_step", C.c_double), ("match_threshold", C.c_double), ("match_threshold_dimension", C.c_double),
                ("disable_yaw_search", C.c_int), ("ignore_dimension", C.c_int), ("min_num_inliers", C.c_int),
                ("use_lsq", C.c_int), ("min_num_map_objects_to_start", C.c_int), ("max_rings", C.c_int)]


def oracle_place_params(p):
    return OPlace(p["dilation_factor"], p["search_xy_step_size"], p["match_yaw_half_range"], p["search_yaw_step_size"],
                  p["match_threshold_position"], p["match_threshold_dimension"], p["disable_yaw_search"], p["ignore_dimension"],
                  p["min_num_inliers"], p["use_nonlinear_least_squares"], p["min_num_map_objects_to_start"], p["max_rings"])


def oracle_match_maps(case):
    ref, qry = np.ascontiguousarray(case["ref7"]), np.ascontiguousarray(case["qry7"])
    op = oracle_place_params(case["params"])
    best = np.zeros(3)
    pr, pq = np.full(max(len(qry), 1), -1, np.int32), np.full(max(len(qry), 1), -1, np.int32)
    inl = po.lib().orc_match_maps(_p(ref), C.c_int(len(ref)), _p(qry), C.c_int(len(qry)), C.byref(op), _p(best), _p(pr), _p(pq))
    k = max(inl, 0)
    return inl, best, pr[:k], pq[:k]


def oracle_counts(case, n):
    """orc_match_maps_counts: the oracle's count of every candidate (OpenMP over candidates) and its candidate triples."""
    ref, qry = np.ascontiguousarray(case["ref7"]), np.ascontiguousarray(case["qry7"])
    op = oracle_place_params(case["params"])
    counts, xyyaw = np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 3))
    got = po.lib().orc_match_maps_counts(_p(ref), C.c_int(len(ref)), _p(qry), C.c_int(len(qry)), C.byref(op), _p(counts), _p(xyyaw),
                                         C.c_longlong(n))
    assert got == n, (got, n)
    return counts[:n], xyyaw[:n]


def assert_claims(claimed, measured):
    assert claimed, "a case must claim at least one edge"
    for k, v in claimed.items():
        assert k in measured, k
        assert measured[k] == v, (k, v, measured[k])


@pytest.mark.parametrize("name", sorted(SWEEP))
def test_sweep_reference_matches_oracle(name):
    case = SWEEP[name]
    lat = pc.lattice(case["ref7"], case["qry7"], case["params"])
    fh = pc.first_hits(case["ref7"], case["qry7"], lat, case["params"])
    counts = (fh >= 0).sum(axis=1).astype(np.int32)
    measured = pc.sweep_edges(case, lat, fh)
    if name == "argmax_ties":
        measured.update(pc.argmax_tie_edges(counts))
    if "targets" in case:          # threshold cases: each pair sits on the side of the threshold the builder says
        assert pc.threshold_targets_hit(case, lat, fh) == case["expect_hit"]
        for k in case["edges"]:
            measured[k] = True
    assert_claims(case["edges"], measured)
    inl, best, pr, pq = oracle_match_maps(case)
    bi = pc.first_argmax(counts)
    if lat["n"] == 0:
        assert bi == -1 and inl == -10000
        return
    oc, oxy = oracle_counts(case, lat["n"])
    assert np.array_equal(oxy, pc.cand_xyyaw(lat))                   # the lattice, bit for bit
    assert np.array_equal(oc, counts)                                # every candidate
    assert counts[bi] == inl
    assert np.array_equal(pc.cand_xyyaw(lat)[bi], best)              # best_xyyaw, bit for bit
    r, q = pc.pairs_at(case["ref7"], case["qry7"], lat, case["params"], bi)
    assert np.array_equal(r, pr) and np.array_equal(q, pq)


def test_sweep_cases_cover_the_kernel_edges():
    """Every edge the sweep kernels have is claimed (and, above, reached) by some case: removing a claim from a builder fails here."""
    claims = set()
    for case in SWEEP.values():
        for k, v in case["edges"].items():
            claims.add((k, tuple(v) if isinstance(v, list) else v))
    sizes = set()
    for case in SWEEP.values():
        sizes |= set(case["edges"].get("bucket_sizes", []))
    assert {1, 3, 4, 5, 15, 16, 17, 33} <= sizes and max(sizes) >= 400
    for nq in (1, 63, 64, 65, 128, 130, 200):
        assert ("nq", nq) in claims, nq
    for need in [("early_exit", True), ("closed_and_open_lanes_in_one_bucket", True), ("query_label_absent_from_ref", True),
                 ("ref_label_absent_from_query", True), ("n_labels_ref", 1), ("n_labels_ref", 3), ("n_labels_ref", 40), ("n_yaw", 1),
                 ("candidates", 0), ("max_buckets_in_later_chunk", 2), ("max_buckets_in_later_chunk", 3), ("last_chunk_fill", 1),
                 ("pair_at_threshold", True), ("pair_at_v_crit", True), ("pair_one_below_v_crit", True), ("pair_above_threshold", True),
                 ("dim_at_threshold_one_branch", True), ("dim_at_threshold_avg_branch", True),
                 ("ties_further_than_a_grid_stride", True), ("ties_in_other_workgroups", True), ("ties_inside_one_workgroup", True)]:
        assert need in claims, need
    labels = np.concatenate([c["ref7"][:, 0] for c in SWEEP.values()])
    assert (labels < 0).any() and (labels != np.round(labels)).any()           # negative and fractional labels
    rings = {c["params"]["max_rings"] for c in SWEEP.values()}
    assert {0, 1, -1} <= rings
    assert {c["params"]["ignore_dimension"] for c in SWEEP.values()} == {0, 1}


def test_yaw_tables_are_the_c_librarys():
    """The kernels' cos / sin tables are filled on the host by std::cos / std::sin; the reference's lattice() takes math.cos / math.sin
    (the same C library) rather than numpy's vectorised versions, which may differ in the last bit.  How often they do on the yaw tables
    used here is printed; the comparison with the oracle above is what holds the choice."""
    import math
    diff = total = 0
    for case in SWEEP.values():
        lat = pc.lattice(case["ref7"], case["qry7"], case["params"])
        yaws = lat["yaw"][:lat["n_yaw"]]
        total += 2 * len(yaws)
        diff += int((np.cos(yaws) != np.array([math.cos(v) for v in yaws])).sum() + (np.sin(yaws) != np.array([math.sin(v) for v in yaws])).sum())
    print(f"numpy cos/sin differ from the C library's in {diff} of {total} table entries")


def test_full_size_sweep_oracle_counts_vouched_by_numpy():
    """The 792 x 554 pair over FULL_SIZE_RINGS rings is too large for numpy at every candidate; the oracle's loop counts all of them
    (what the GPU test compares with) and numpy vouches for it on an evenly spread sub-sample plus the winner."""
    case = pc.full_size_pair(pc.FULL_SIZE_RINGS)
    lat = pc.lattice(case["ref7"], case["qry7"], case["params"])
    t0 = time.perf_counter()
    oc, oxy = oracle_counts(case, lat["n"])
    dt = time.perf_counter() - t0
    print(f"full-size sweep: {pc.FULL_SIZE_RINGS} rings, {lat['n']} candidates, oracle loop {dt:.1f} s")
    assert np.array_equal(oxy, pc.cand_xyyaw(lat))
    bi = pc.first_argmax(oc)
    sel = np.unique(np.concatenate([np.linspace(0, lat["n"] - 1, 150).astype(np.int64), [bi]]))
    assert np.array_equal(pc.sweep_counts(case["ref7"], case["qry7"], lat, case["params"], sel), oc[sel])
    L = pc.bucket_layout(case["ref7"], case["qry7"])
    assert_claims(case["edges"], dict(nq=len(case["qry7"]), chunks=len(L["chunks"]), last_chunk_fill=len(case["qry7"]) - 64 * (len(L["chunks"]) - 1)))
    assert oc[bi] == oc.max() and not (oc[:bi] == oc.max()).any() and oc[bi] > 0
    # (orc_match_maps itself is not run here: its single-threaded loop over this lattice takes longer than the whole module)


def oracle_triangles(case):
    tm, td = np.ascontiguousarray(case["tm"].reshape(-1, 6)), np.ascontiguousarray(case["td"].reshape(-1, 6))
    cap = max(len(tm) * len(td), 1)
    op, od = np.zeros((cap, 3, 4)), np.zeros(cap)
    n = po.lib().orc_match_triangles(_p(tm), C.c_int(len(tm)), _p(td), C.c_int(len(td)), C.c_double(case["thr"]), _p(op), _p(od), C.c_int(cap))
    return op[:n], od[:n]


@pytest.mark.parametrize("name", sorted(TRIANGLES))
def test_triangle_reference_matches_oracle(name):
    case = TRIANGLES[name]
    assert_claims(case["edges"], pc.triangle_edges(case))
    pts, diffs, _ = pc.triangle_rows(case["tm"], case["td"], case["thr"])
    op, od = oracle_triangles(case)
    assert len(od) == len(diffs)
    assert np.array_equal(pts, op) and np.array_equal(diffs, od)               # row for row


def test_triangle_cases_cover_the_kernel_edges():
    claims = {(k, v) for c in TRIANGLES.values() for k, v in c["edges"].items()}
    for ntd in (0, 1, 63, 64, 65, 129):
        assert ("ntd", ntd) in claims
    assert ("ntm", 0) in claims and any(k == "ntm" and v % 4 for k, v in claims)
    for need in [("unmatched_model_between_matched", True), ("all_pairs", True), ("rank_carries_across_rounds", True),
                 ("two_equal_distances", True), ("three_equal_distances", True), ("pair_at_thr_excluded", True),
                 ("pair_below_thr_included", True)]:
        assert need in claims, need


class OClipper(C.Structure):
    _fields_ = [("tol_u", C.c_double), ("tol_F", C.c_double), ("maxiniters", C.c_int), ("maxoliters", C.c_int),
                ("beta", C.c_double), ("maxlsiters", C.c_int), ("eps", C.c_double), ("affinityeps", C.c_double),
                ("rescale_u0", C.c_int), ("sigma", C.c_double), ("epsilon", C.c_double), ("mindist", C.c_double)]


def oracle_affinity(case):
    D1, D2, A = np.ascontiguousarray(case["D1"]), np.ascontiguousarray(case["D2"]), np.ascontiguousarray(case["A"], np.int32).copy()
    m = len(A)
    p = OClipper()
    po.lib().orc_clipper_default_params(C.byref(p))
    p.sigma, p.epsilon, p.mindist, p.affinityeps = (case["kw"][k] for k in ("sigma", "epsilon", "mindist", "affinityeps"))
    M = np.zeros((m, m))
    po.lib().orc_clipper_affinity(_p(D1), C.c_int(len(D1)), _p(D2), C.c_int(len(D2)), C.c_int(D1.shape[1]), _p(A), C.c_int(m), C.byref(p), _p(M))
    return M


def reference_affinity(case):
    kw = case["kw"]
    return pc.affinity(case["D1"], case["D2"], case["A"], kw["sigma"], kw["epsilon"], kw["mindist"], kw["affinityeps"])


@pytest.mark.parametrize("name", sorted(AFFINITY))
def test_affinity_reference_matches_oracle(name):
    case = AFFINITY[name]
    ref = reference_affinity(case)
    assert_claims(case["edges"], pc.affinity_edges(case, ref))
    assert ref["margin"] >= 1e-12              # no decision hangs on exp's last bit (a condition on the inputs)
    Mo = oracle_affinity(case)
    assert np.array_equal(Mo != 0, ref["M"] != 0)                              # the sparsity pattern: every decision
    assert np.array_equal(ref["M"] != 0, ref["M_hp"] != 0)
    assert np.allclose(Mo, ref["M_hp"], rtol=1e-14, atol=0)
    assert not np.tril(Mo).any()


def test_affinity_cases_cover_the_kernel_edges():
    claims = {(k, v) for c in AFFINITY.values() for k, v in c["edges"].items()}
    for m in (1, 127, 128, 129, 257):
        assert ("m", m) in claims
    for need in [("dim", 2), ("dim", 3), ("shared_points", True), ("c_equals_eps", True), ("below_affinityeps", True), ("at_mindist", True)]:
        assert need in claims, need
