"""Lists of map pairs for the list form of SlideMatch (slide_find_inter_loop_closures, the loop of sloamNode.cpp:600-694 over
findInterLoopClosure, place_recognition.cpp:498-538) and their per-pair reference.  Plain numpy on top of place_cases: no GPU, no
product import, no oracle import.  The reference of a pair is what the method does before the refinement: the object-count gate, both
maps centred on their XY centroids (sums in row order in Python floats — np.mean sums pairwise and may differ in the last bit), then
place_cases' lattice, per-candidate counts and first-of-maximum arg-max.  Every lattice swept here stays below 1e8 pair tests (coarse
steps or max_rings).  tests/test_slidematch_list_reference.py asserts every edge a case claims on the reference's results;
tests/test_gpu_slidematch_list.py holds the library against them."""
import math
import os

import numpy as np

import place_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
COARSE = dict(search_xy_step_size=1.0, search_yaw_step_size=math.pi / 4, match_threshold_position=1.0)
MAX_PAIR_TESTS = 1e8


def load_map(name):
    """place_recognition_test.cpp:88-95 layout: 'label x y z' rows -> Vector7d with zero dimensions."""
    a = np.loadtxt(os.path.join(HERE, "golden", name))
    out = np.zeros((a.shape[0], 7))
    out[:, :4] = a[:, :4]
    return out


def centre(m):
    """(centred copy, centroid): findTransformation :752-765 with the sums taken row by row"""
    m = np.array(m, np.float64).reshape(-1, 7)
    sx = sy = 0.0
    for row in m:
        sx += float(row[1])
        sy += float(row[2])
    n = len(m)
    c = (sx / n, sy / n) if n else (0.0, 0.0)
    m[:, 1] = np.subtract(m[:, 1], c[0])
    m[:, 2] = np.subtract(m[:, 2], c[1])
    return m, c


def pair_reference(ref7, qry7, params):
    """dict(gated, candidates, best_index, counts, max_count) of ONE pair by itself."""
    nr, nq = len(ref7), len(qry7)
    if nr < params["min_num_map_objects_to_start"] or nq < params["min_num_map_objects_to_start"] or nr == 0 or nq == 0:
        return dict(gated=True, candidates=0, best_index=-1, counts=np.zeros(0, np.int32), max_count=None, lat=None)
    r, _ = centre(ref7)
    q, _ = centre(qry7)
    lat = pc.lattice(r, q, params)
    assert lat["n"] * nr * nq <= MAX_PAIR_TESTS, (lat["n"], nr, nq)
    counts = pc.sweep_counts(r, q, lat, params)
    bi = pc.first_argmax(counts)
    return dict(gated=False, candidates=lat["n"], best_index=bi, counts=counts, max_count=int(counts[bi]) if bi >= 0 else None, lat=lat)


_REF_CACHE = {}


def list_reference(case):
    """One pair_reference per pair of the case (computed once per distinct pair and case name, shared by every test)."""
    out = []
    for a, b in case["pairs"]:
        key = (case["name"], a, b)
        if key not in _REF_CACHE:
            _REF_CACHE[key] = pair_reference(case["maps"][a], case["maps"][b], case["params"])
        out.append(_REF_CACHE[key])
    return out


def _view_of(rng, ref, take, extra, yaw, shift, noise=0.03):
    """`take` objects of ref seen from a frame rotated by yaw and shifted, with dimensions drawn anew, plus `extra` objects of its own"""
    sel = rng.permutation(len(ref))[:take]
    q = ref[sel].copy()
    c, s = math.cos(-yaw), math.sin(-yaw)
    xy = q[:, 1:3] - np.array(shift)
    q[:, 1] = c * xy[:, 0] - s * xy[:, 1]
    q[:, 2] = s * xy[:, 0] + c * xy[:, 1]
    q[:, 1:3] += rng.normal(0, noise, (take, 2))
    e = np.zeros((extra, 7))
    e[:, 0] = rng.integers(1, 4, extra)
    e[:, 1:3] = rng.uniform(-12.0, 12.0, (extra, 2))
    e[:, 3] = rng.normal(0, 0.2, extra)
    out = np.concatenate([q, e])
    out[:, 4:7] = rng.uniform(0.3, 2.0, (len(out), 3))
    out[rng.integers(0, 3, len(out)) == 0, 5:7] = 0.0              # some take the one-dimension branch as reference objects
    return np.ascontiguousarray(out[rng.permutation(len(out))])


def mixed_list(ignore_dimension):
    """Four maps: the two golden indoor maps, a 60-object map with dimensions (25 of its objects are map 0 seen from another frame), a
    3-object map.  (0, 1), (1, 0), a self pair, seven pairs with reference 0."""
    rng = np.random.default_rng(60)
    m0, m1 = load_map("robot0Map_indoor.txt"), load_map("robot1Map_indoor.txt")
    m2 = _view_of(rng, m0, 25, 35, 0.8, (1.5, -2.0))
    m3 = np.zeros((3, 7))
    m3[:, 0] = (1.0, 2.0, 3.0)
    m3[:, 1:3] = ((4.0, 1.0), (-3.0, 2.5), (0.5, -6.0))
    pairs = [(0, 1), (1, 0), (2, 2), (0, 2), (0, 3), (0, 0), (0, 1), (0, 2), (0, 3), (3, 2), (2, 1)]
    return dict(name=f"mixed_ig{ignore_dimension}", maps=[m0, m1, m2, m3], pairs=pairs,
                params=pc.place_params(ignore_dimension=ignore_dimension, **COARSE),
                edges=dict(n_maps=4, n_pairs=11, pairs_with_reference_0=7, self_pair=True, sizes=[32, 35, 60, 3], found_at_least=3))


def tie_maps():
    """One query object and two mirrored reference objects: after centring the reference objects sit at (-6.25, 0.25) and
    (6.25, -0.25) exactly, the query object at the origin, so every candidate within the threshold of either counts 1 — equal maxima
    at the low and at the high end of the x loop of one ring, every yaw of such a cell included."""
    ref = np.zeros((2, 7))
    ref[0, :3] = (1.0, -4.25, 3.25)
    ref[1, :3] = (1.0, 8.25, 2.75)
    qry = np.zeros((1, 7))
    qry[0, :3] = (1.0, 5.0, -7.0)
    return ref, qry


def tie_lists():
    """name -> case: the tie pair alone, between two heavy pairs (which shrinks its share of workgroups), three times in one list"""
    ref, qry = tie_maps()
    h = pc.sweep_cases()["q64_three_labels_15_16_17"]
    params = pc.place_params(ignore_dimension=1, **COARSE)
    maps = [ref, qry, h["ref7"], h["qry7"]]
    edges = dict(nq=1, max_count=1, ties_far_apart=True, ties_at_neighbouring_yaws=True)
    return {
        "alone": dict(name="tie_alone", maps=maps, pairs=[(0, 1)], tie_at=[0], params=params, edges=edges),
        "between_heavy": dict(name="tie_between_heavy", maps=maps, pairs=[(2, 3), (0, 1), (2, 3)], tie_at=[1], params=params, edges=edges),
        "three_times": dict(name="tie_three_times", maps=maps, pairs=[(0, 1), (0, 1), (0, 1)], tie_at=[0, 1, 2], params=params, edges=edges),
    }


def tie_edges(ref):
    counts = ref["counts"]
    tied = np.nonzero(counts == counts.max())[0]
    n_yaw = ref["lat"]["n_yaw"]
    return dict(nq=1, max_count=int(counts.max()), ties_far_apart=bool(tied[-1] - tied[0] > 1024 and len(tied) >= 2),
                ties_at_neighbouring_yaws=bool(n_yaw > 1 and (np.diff(tied) == 1).any()), first=int(tied[0]), n_tied=int(len(tied)))


def chunk_list(ignore_dimension):
    """The maps of three place_cases sweep cases with 64, 65 and 128 query objects (one full chunk of a wavefront, one object into the
    second chunk, two full chunks) under ONE parameter set, ring 0 only."""
    sc = pc.sweep_cases()
    names = ["q64_three_labels_15_16_17", "q65_dims_3_4_5_absent_labels", "q128_forty_labels"]
    maps = []
    for n in names:
        maps += [sc[n]["ref7"], sc[n]["qry7"]]
    return dict(name=f"chunks_ig{ignore_dimension}", maps=maps, pairs=[(0, 1), (2, 3), (4, 5)],
                params=pc.place_params(ignore_dimension=ignore_dimension, search_xy_step_size=1.0, search_yaw_step_size=math.pi / 2,
                                       match_threshold_position=2.0, match_threshold_dimension=0.6, max_rings=1),
                edges=dict(nq=[64, 65, 128]))


def status_list(ignore_dimension):
    """Every per-pair outcome in one list, at place_cases.capacity_case's parameters (49 candidates, no yaw search), gate at 3
    objects, one inlier enough to be found.  Maps: 0 the capacity map at the largest size whose image fits beside 3 query objects,
    1 its 3 query objects, 2 map 0 with one object more, 3 an empty map, 4 five objects, 5 four objects at ONE point (centred: all
    at the origin, half ranges 0, no lattice), 6 two objects (below the gate)."""
    ig = ignore_dimension
    nr = pc.bucketed_max_nr(3, ig)
    cap = pc.capacity_case(nr, ig)
    over = np.concatenate([cap["ref7"], cap["ref7"][-1:] + np.array([[0, 0.125, -0.25, 0, 0, 0, 0]])])
    rng = np.random.default_rng(77)
    five = np.zeros((5, 7))
    five[:, 0] = 1.0
    five[:, 1:3] = rng.uniform(-5.0, 5.0, (5, 2))
    five[:, 4:7] = rng.uniform(0.3, 2.0, (5, 3))
    spot = np.zeros((4, 7))
    spot[:, 0] = 1.0
    spot[:, 1:3] = (2.0, 3.0)
    two = five[:2].copy()
    params = dict(cap["params"])
    params.update(min_num_map_objects_to_start=3, min_num_inliers=1)
    pairs = [(4, 1), (6, 1), (0, 1), (3, 1), (1, 4), (1, 3), (2, 1), (5, 5), (4, 4), (1, 6)]
    return dict(name=f"status_ig{ig}", maps=[cap["ref7"], cap["qry7"], over, np.zeros((0, 7)), five, spot, two], pairs=pairs, params=params,
                expect=dict(gated=[1, 3, 5, 9], empty_lattice=[7], capacity=[6], at_capacity=[2], live=[0, 2, 4, 8]),
                edges=dict(capacity_nr=nr, over_nr=nr + 1, image_bytes_at=lds_image_bytes(nr, 3, ig), image_bytes_over=lds_image_bytes(nr + 1, 3, ig)))


def lds_image_bytes(nr, nq, ignore_dimension):
    """the bucketed sweep's on-chip image (place_cases.LDS_BYTES is its limit)"""
    return (16 if ignore_dimension else 40) * (nr + nq) + 8 * nq + 16


def full_size_list():
    """The 792 / 554 forest pair over its first ring(s), twice, with a small pair between: no numpy reference at this size, the list
    is held against the single call."""
    f = pc.full_size_pair(pc.FULL_SIZE_RINGS)
    small = tie_maps()
    return dict(name="full_size", maps=[f["ref7"], f["qry7"], small[0], small[1]], pairs=[(0, 1), (2, 3), (0, 1)], params=f["params"])
