"""The map-matcher kernels (csrc/place_kernels.hip) against the plain references of tests/place_cases.py, candidate by candidate and row
by row, on the cases whose edges tests/test_place_reference.py asserts (and whose references it holds against the oracle).

Exact equality everywhere except the affinity VALUES (exp is the one inexact operation: rtol 1e-14 against a higher-precision exp).
The yaw tables: both sides take the C library's cos / sin on the host (place_cases.lattice), so the counts compare exactly."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import place_cases as pc  # noqa: E402
from test_place_reference import AFFINITY, SWEEP, TRIANGLES, oracle_counts, reference_affinity  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SLIDE_ERR_CAPACITY = -3


def _where(case, lat, got, want):
    """First differing candidate, with the chunks of 64 query objects and the buckets each chunk scans."""
    bad = np.nonzero(got != want)[0]
    c = int(bad[0])
    L = pc.bucket_layout(case["ref7"], case["qry7"])
    fh = pc.first_hits(case["ref7"], case["qry7"], lat, case["params"], [c])[0][L["order"]]
    per_chunk = [(ci, int((fh[64 * ci:64 * ci + 64] >= 0).sum()), [(b, L["sizes"][b]) for b in ch]) for ci, ch in enumerate(L["chunks"])]
    return (f"{len(bad)} of {len(want)} candidates differ; first: candidate {c} (x, y, yaw) = {pc.cand_xyyaw(lat)[c].tolist()}: kernel {int(got[c])}, "
            f"reference {int(want[c])}; per chunk (chunk, reference hits, [(bucket, size)]): {per_chunk}")


def check_sweep(case, r, lat, counts):
    assert r["status"] == 0 and r["candidates"] == lat["n"]
    assert np.array_equal(r["xyyaw"], pc.cand_xyyaw(lat))                                   # the lattice, bit for bit
    assert np.array_equal(r["inliers"], counts), _where(case, lat, r["inliers"], counts)    # EVERY candidate
    assert r["best_index"] == pc.first_argmax(counts)


@pytest.mark.parametrize("name", sorted(SWEEP))
def test_sweep_every_candidate(gpu, name):
    case = SWEEP[name]
    gp = gpu.place_default_params(**case["params"])
    lat = pc.lattice(case["ref7"], case["qry7"], case["params"])
    counts = pc.sweep_counts(case["ref7"], case["qry7"], lat, case["params"])
    r = gpu.match_maps_sweep(case["ref7"], case["qry7"], gp)
    g = gpu.match_maps(case["ref7"], case["qry7"], gp)
    if lat["n"] == 0:
        assert r["status"] == 0 and r["candidates"] == 0 and r["best_index"] == -1 and g["inliers"] == -10000
        return
    check_sweep(case, r, lat, counts)
    bi = r["best_index"]
    assert g["inliers"] == counts[bi] and np.array_equal(g["xyyaw"], pc.cand_xyyaw(lat)[bi]) and g["candidates"] == lat["n"]
    pr, pq = pc.pairs_at(case["ref7"], case["qry7"], lat, case["params"], bi)
    assert np.array_equal(g["ref_idx"], pr) and np.array_equal(g["qry_idx"], pq)


def test_sweep_read_back_capacity(gpu):
    """Candidate buffers too small: SLIDE_ERR_CAPACITY with the count filled in, nothing launched, nothing written."""
    case = SWEEP["q64_three_labels_15_16_17"]
    gp = gpu.place_default_params(**case["params"])
    lat = pc.lattice(case["ref7"], case["qry7"], case["params"])
    r = gpu.match_maps_sweep(case["ref7"], case["qry7"], gp, capacity=lat["n"] - 1)
    assert r["status"] == SLIDE_ERR_CAPACITY and r["candidates"] == lat["n"] and r["best_index"] == -1
    r = gpu.match_maps_sweep(case["ref7"], case["qry7"], gp, capacity=lat["n"])
    assert r["status"] == 0 and len(r["inliers"]) == lat["n"]


def test_full_size_sweep_every_candidate(gpu):
    """The benchmark's 792 x 554 pair over FULL_SIZE_RINGS rings (nine chunks of query objects per candidate, the last holding 42):
    every candidate against the oracle's loop, which tests/test_place_reference.py vouches for with numpy."""
    case = pc.full_size_pair(pc.FULL_SIZE_RINGS)
    gp = gpu.place_default_params(**case["params"])
    lat = pc.lattice(case["ref7"], case["qry7"], case["params"])
    counts, _ = oracle_counts(case, lat["n"])
    r = gpu.match_maps_sweep(case["ref7"], case["qry7"], gp)
    check_sweep(case, r, lat, counts)
    g = gpu.match_maps(case["ref7"], case["qry7"], gp)
    bi = r["best_index"]
    assert g["inliers"] == counts[bi] and np.array_equal(g["xyyaw"], pc.cand_xyyaw(lat)[bi])
    pr, pq = pc.pairs_at(case["ref7"], case["qry7"], lat, case["params"], bi)
    assert np.array_equal(g["ref_idx"], pr) and np.array_equal(g["qry_idx"], pq)


@pytest.mark.parametrize("ignore_dimension", [1, 0])
def test_bucketed_kernel_capacity(gpu, ignore_dimension):
    """The bucketed kernel's LDS image (16 B per object with ignore_dimension, 40 B without, + 8 B per query object + 16, 150 KiB): the
    largest reference map it admits (9594 / 3836 objects against three query objects — one bucket of that size; the old condition, the
    PLAIN kernel's 48 B per reference object, refused anything above 3200) is swept and agrees with the reference at every candidate;
    one object more is refused with a clean status."""
    nr = pc.bucketed_max_nr(3, ignore_dimension)
    assert nr == (9594 if ignore_dimension else 3836)
    case = pc.capacity_case(nr, ignore_dimension)
    gp = gpu.place_default_params(**case["params"])
    lat = pc.lattice(case["ref7"], case["qry7"], case["params"])
    counts = pc.sweep_counts(case["ref7"], case["qry7"], lat, case["params"])
    assert lat["n"] > 30 and 0 < counts.max() and len(np.unique(counts)) > 1
    check_sweep(case, gpu.match_maps_sweep(case["ref7"], case["qry7"], gp), lat, counts)
    over = pc.capacity_case(nr + 1, ignore_dimension)
    r = gpu.match_maps_sweep(over["ref7"], over["qry7"], gp)
    assert r["status"] == SLIDE_ERR_CAPACITY and r["best_index"] == -1
    with pytest.raises(gpu.SlideError, match="SLIDE_ERR_CAPACITY"):
        gpu.match_maps(over["ref7"], over["qry7"], gp)


PLAIN_CASES = ["q64_three_labels_15_16_17", "q65_dims_3_4_5_absent_labels", "q128_forty_labels", "q200_dims_three_labels",
               "threshold_position", "threshold_dimension"]


def test_plain_kernel_same_cases_and_capacity(gpu, tmp_path):
    """SLIDE_PLACE_PLAIN=1 (the one-wavefront-per-candidate kernel without buckets, kept for comparison) on a subset of the cases, and
    its own capacity: 48 B per reference object, so 3200 objects are swept (150 KiB of dynamic LDS, which needs the kernel's
    MaxDynamicSharedMemorySize opt-in) and 3201 refused.  The switch is read once per process: one fresh child, no retry."""
    out = str(tmp_path / "plain.npz")
    nr = pc.plain_max_nr()
    assert nr == 3200
    names = PLAIN_CASES + [f"capacity:{nr}:1", f"capacity:{nr + 1}:1"]
    env = dict(os.environ, SLIDE_PLACE_PLAIN="1")
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "place_plain_child.py"), out, *names], env=env, timeout=600)
    assert r.returncode == 0
    z = np.load(out)
    for name in names:
        key = name.replace(":", "_")
        got = dict(status=int(z[key + "/status"]), candidates=int(z[key + "/candidates"]), best_index=int(z[key + "/best_index"]),
                   xyyaw=z[key + "/xyyaw"], inliers=z[key + "/inliers"])
        if name == f"capacity:{nr + 1}:1":
            assert got["status"] == SLIDE_ERR_CAPACITY and got["best_index"] == -1
            continue
        case = pc.capacity_case(nr, 1) if name.startswith("capacity:") else SWEEP[name]
        lat = pc.lattice(case["ref7"], case["qry7"], case["params"])
        check_sweep(case, got, lat, pc.sweep_counts(case["ref7"], case["qry7"], lat, case["params"]))


@pytest.mark.parametrize("name", sorted(TRIANGLES))
def test_triangle_rows(gpu, name):
    case = TRIANGLES[name]
    pts, diffs, _ = pc.triangle_rows(case["tm"], case["td"], case["thr"])
    gp, gd = gpu.match_triangles(case["tm"], case["td"], case["thr"])
    assert len(gd) == len(diffs)
    assert np.array_equal(gp, pts) and np.array_equal(gd, diffs)          # same pairs, same order, same vertex order, same bits


def _affinity_poisoned(gpu, case):
    """slide_clipper_affinity into a host matrix pre-filled with NaN.  The DEVICE buffer the kernel writes is allocated inside the entry
    point (uninitialised hipMalloc memory) and cannot be poisoned through the binding; an element the kernel skipped would come back
    as whatever that memory held, and an element the read-back skipped as NaN."""
    from slide_slam_amd import api
    D1, D2, A = api._d(case["D1"]), api._d(case["D2"]), api._i(case["A"])
    m, kw = len(A), case["kw"]
    M = np.full((m, m), np.nan)
    rc = gpu.lib().slide_clipper_affinity(api._p(D1), C.c_int(len(D1)), api._p(D2), C.c_int(len(D2)), C.c_int(D1.shape[1]), api._p(A), C.c_int(m),
                                          C.c_double(kw["sigma"]), C.c_double(kw["epsilon"]), C.c_double(kw["mindist"]),
                                          C.c_double(kw["affinityeps"]), api._p(M))
    assert rc == 0
    return M


@pytest.mark.parametrize("name", sorted(AFFINITY))
def test_affinity_pattern_and_values(gpu, name):
    """Largest relative difference from the higher-precision value seen on the MI355X: 2.2e-16 (one unit in the last place), m = 257."""
    case = AFFINITY[name]
    ref = reference_affinity(case)
    M = _affinity_poisoned(gpu, case)
    assert not np.isnan(M).any()
    assert np.array_equal(M != 0, ref["M_hp"] != 0)                       # every decision
    assert not np.tril(M).any()                                           # strict lower triangle and diagonal: zeros
    nz = ref["M_hp"] != 0
    rel = float(np.max(np.abs(M[nz] - ref["M_hp"][nz]) / ref["M_hp"][nz])) if nz.any() else 0.0
    print(f"affinity {name}: largest relative difference {rel:.3e} over {int(nz.sum())} entries")
    assert np.allclose(M, ref["M_hp"], rtol=1e-14, atol=0)
    assert np.array_equal(gpu.clipper_affinity(case["D1"], case["D2"], case["A"], **case["kw"]), M)
