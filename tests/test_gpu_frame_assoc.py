"""k_assoc_frame (csrc/assoc_kernels.hip, launched by HostBackend::associate in csrc/host_backend.hip) detection by detection.

Every case of tests/frame_cases.py runs through gpu.SlideBackend and po.OracleBackend; per frame and per detection *_match (the
match's position in the nearest-first submap, which the device COUNTS — assoc_core rank_mode — instead of sorting), *_id, counts()
and status are identical.  FOREIGN-only cases are also held against the numpy restatement of the frame (margin rule of
frame_cases.check_against_numpy) on the map read back from the device, and the landmarks they create against R b + t from numpy
(projectModels).  tests/test_frame_reference.py proves the cases and the reference on the CPU first.
"""
import functools

import numpy as np
import pytest

import frame_cases as fc
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


def _oracle(case):
    ob = po.OracleBackend(po.OrcParams.default(), case.n_robots)
    if case.knn != fc.K_DEFAULT:
        ob.set_knn(*case.knn)
    return ob


def _device(gpu, case):
    p = gpu.default_params(knn_cylinder=case.knn[0], knn_cube=case.knn[1], knn_ellipsoid=case.knn[2], number_of_robots=case.n_robots)
    return gpu.SlideBackend(p, case.n_robots)


def _snapshot(backend):
    """hits, labels and scales of every landmark, as map_model reports them."""
    cnt = backend.counts()
    out = {}
    for ci, c in enumerate(fc.CLS):
        rows = [backend.map_model(ci, i) for i in range(cnt[fc.COUNT_KEY[ci]])]
        out[c] = dict(hits=np.array([r[2] for r in rows], np.int64), label=np.array([r[3] for r in rows], np.int64),
                      scale=np.array([r[1][3:6] for r in rows]).reshape(len(rows), -1))
    return out


@functools.lru_cache(maxsize=None)
def _oracle_run(name):
    """The oracle's results of a case, computed once (and, after every call that refreshes the map, its hits / labels / scales)."""
    case = fc.get_case(name)
    ob = _oracle(case)
    snaps = {}

    def after(k, op, r):
        if not case.foreign_only and _refreshes(op):
            snaps[k] = _snapshot(ob)

    return fc.run_case(ob, case, after_op=after), snaps


def _refreshes(op):
    return op["op"] == "end_frame" or (op["op"] == "frame" and op["mode"] == fc.FRAME_HOST)


def _run_foreign(gpu, name):
    case = fc.get_case(name)
    res, under = fc.check_against_numpy(_device(gpu, case), case)
    assert under == [], f"{name}: detections under the margin outside the named ties: {under}"
    fc.compare_results(case, res, _oracle_run(name)[0])
    return case, res


@pytest.mark.parametrize("counts", fc.DET_COUNTS, ids=lambda c: "_".join(map(str, c)))
def test_detections_per_class(gpu, counts):
    """A map of 120 / 80 / 1500 landmarks seeded by one FOREIGN frame (n_det = 1500: dozens of rounds of the ungrouped box loop; all
    three gates select afterwards, K = 50 / 30 / 1000: knn_select's histogram + candidate ranks, one dynamic-LDS size shared by a
    cylinder, a cube and an ellipsoid layout), then a frame of `counts` = (cylinders, cubes, ellipsoids) detections on 16 waves:
    cylinders 0 1 16 | 17 32 | 33 40: no detection, one wave, every wave once | the second detection of a wave (`two`), all of them |
      a second round of the cylinder loop, with and without `two` in it — on the LDS-staged gated cylinder submap;
    cubes 0 1 16 | 17 33 48 | 49 65: first detection of a wave | detections 2 and 3 of a wave (HM = 3), partly and fully | a second
      round — on the gated, staged cube submap with label_gate = 0 (the ungrouped staged path: float screening + exact rule);
    ellipsoids 0 1 16 17 49 64 | 65 100: the label-grouped staged submap (n_det <= ASSOC_GMAX = 64: one detection per wave and round,
      up to four rounds) | the ungrouped staged path, three per wave, two and three rounds.
    Each frame holds detections far from every landmark (new landmarks), labels no landmark has, cylinders with the right place and
    the wrong label, and objects beyond the gate; a third, small frame matches landmarks the second one created (the map grows across
    ClassMap::sync_device's incremental uploads).  (0, 0, 0) is the frame without any detection, followed by a normal one."""
    _run_foreign(gpu, "det_counts_" + "_".join(map(str, counts)))


@pytest.mark.parametrize("n_rel", ["K-1", "K", "K+1", "3K"])
@pytest.mark.parametrize("K", fc.KNN_K)
def test_knn_and_map_size(gpu, K, n_rel):
    """default_params(knn_* = K) / set_knn(K) against maps of n = K - 1, K, K + 1, 3 K landmarks per class: K >= n takes no selection
    at all (knn_select: fbin < 0, shift = 64, every key placed), K < n the histogram select with Ksub = K; Kp = 64 (the floor) for
    K <= 64, a power of two exactly at K = 64 and 128, one above at 65 and 129 (the padding keys ~0 behind Ksub); K = 1: a submap of
    one landmark, rank 0 or no match; K = 1, n = 0: detections on empty maps."""
    n = dict(zip(["K-1", "K", "K+1", "3K"], fc.knn_sizes(K)))[n_rel]
    _run_foreign(gpu, f"knn_K{K}_n{n}")


def test_ellipsoid_submap_beyond_the_staging_budget(gpu):
    """K = 5000 of 6000 ellipsoids, 40 detections: Ksub > 4 x 1024, and 40 B per survivor no longer fit ASSOC_LDS_BUDGET, so
    assoc_plan clears `staged` — the submap is neither grouped nor staged although n_det <= 64, and the box loop takes its
    global-memory branch WITH the gate's keys (sel[] / C.model gathers), which no pure matcher reaches; Kp = 8192 > 1024 threads."""
    _run_foreign(gpu, "ell_K5000_n6000")


def test_map_beyond_the_distance_cache(gpu):
    """Ellipsoids only.  assoc_plan: fixed = Kp * 8 + 256 * 4 = 1024 * 8 + 1024 = 9216 B at K = 1000, and the n distance words are
    cached while fixed + 4 n <= ASSOC_LDS_BUDGET = 143360, i.e. n <= 33536: the map has n = 33537 landmarks, the smallest for which
    `cached` is cleared and knn_select recomputes the distances in every pass (key_at -> dist_bits).  Frames of 20 (grouped) and 70
    (ungrouped) detections."""
    assert fc.BEYOND_CACHE_N == (140 * 1024 - (1024 * 8 + 256 * 4)) // 4 + 1
    _run_foreign(gpu, "beyond_cache")


@pytest.mark.parametrize("which", ["all", "cyl", "cube", "ell", "no_dets_first"])
def test_empty_sides(gpu, which):
    """all: every class's map empty with detections present (the first FOREIGN frame: assoc_core with n = 0, Ksub = 0, every write -1);
    cyl / cube / ell: that class's map empty (assoc_plan returns Kp = 0 for it) next to two selecting classes in the same launch;
    no_dets_first: a frame with no detections at all on empty maps (n_det = 0 in all three workgroups, d_det sized 1), then a normal
    one.  (The frame without detections on a FULL map is test_detections_per_class[0_0_0].)"""
    _run_foreign(gpu, "empty_maps_" + which)


def test_ties(gpu):
    """Exactly equal distances (identity rotation, dyadic coordinates).  Two and five landmarks created at one position in one frame
    (cloud keys equal up to the index); a later detection there: the lowest map index wins and its rank counts only the keys below
    it (reduce_write: the lexicographic (distance, key) minimum, rank = keys below the winner's).  A detection exactly halfway
    between two landmarks of its label, the farther-from-the-robot one created first: the earlier SUBMAP position wins, not the lower
    index.  A coincident landmark of another label in front of the match: skipped for ellipsoids (and counted in the rank), the
    winner for cubes (label_gate = 0).  A cylinder detection equidistant from two map cylinders.  The detections built to tie are
    compared with the oracle only (and with the ids the rule dictates), the others with numpy as well."""
    case, res = _run_foreign(gpu, "ties")
    for k in (1, 2):
        for c in fc.CLS:
            assert list(res[k][c + "_id"]) == case.expect_id[c], (k, c, res[k][c + "_id"])
    assert res[1]["ell_match"][3] == res[1]["ell_match"][4] + 1


def test_ties_within_a_lane(gpu):
    """130 coincident landmarks of one label per class behind gates of K = 200 / 200 / 1000: a submap longer than a wavefront, so a
    LANE holds two or three exactly tied candidates — in whatever order the select's compaction left them — and must keep the lowest
    key itself: the in-lane tie rules of the cylinder loop (d == best && key < bkey), of `exact` (ungrouped staged cubes) and of
    `exact1` (label-grouped ellipsoids), which a tie between fewer than 65 candidates never reaches (one candidate per lane, the
    tie is then reduce_write's).  Landmark 3, the first of the 130, wins at submap position 3."""
    case, res = _run_foreign(gpu, "ties_many")
    for k in (1, 2):
        for c in fc.CLS:
            assert list(res[k][c + "_id"]) == case.expect_id and res[k][c + "_match"][3] == 3, (k, c, res[k][c + "_id"], res[k][c + "_match"])


def test_gate_tie(gpu):
    """K = 2, the second and third cloud point equidistant from the pose (r = 4.0 exactly): the gate keeps the lower index (the
    select's keys carry the index below the distance bits), so the detection at landmark 2 finds nothing within the threshold and
    becomes a new landmark; in the next frame three cloud points tie behind the cut."""
    case, res = _run_foreign(gpu, "gate_tie")
    for k in (1, 2):
        for c in fc.CLS:
            assert list(res[k][c + "_id"]) == case.expect_id[k - 1] and list(res[k][c + "_match"]) == case.expect_match, (k, c)


def _check_refresh(gb, osnap, where):
    """k_map_refresh is a copy: after a refresh every landmark's map model equals the graph's optimised landmark bit for bit (all 7
    cylinder values; cube positions = entries 9:12, point positions = entries 0:3).  hits and labels equal the oracle's exactly,
    ellipsoid scales to 1e-13 relative (at most 10 updates of the 0.2 moving average here, an ulp each at worst if one side contracts
    the multiply-add)."""
    cnt = gb.counts()
    snap = _snapshot(gb)
    for ci, c in enumerate(fc.CLS):
        n = cnt[fc.COUNT_KEY[ci]]
        assert n == len(osnap[c]["hits"]) and n > 0, (where, c)
        for i in range(n):
            st, model, _, _ = gb.map_model(ci, i)
            st2, lm = gb.graph.get_landmark(ci, i)
            assert st == 0 and st2 == 0, (where, c, i)
            want = lm[0:7] if ci == 0 else (lm[9:12] if ci == 1 else lm[0:3])
            got = model[0:7] if ci == 0 else model[0:3]
            assert got.tobytes() == want.tobytes(), (where, c, i, got, want)
        assert np.array_equal(snap[c]["hits"], osnap[c]["hits"]), (where, c, "hits")
        assert np.array_equal(snap[c]["label"], osnap[c]["label"]), (where, c, "labels")
    assert np.all(np.abs(snap["ell"]["scale"] - osnap["ell"]["scale"]) <= 1e-13 * np.abs(osnap["ell"]["scale"])), (where, "ellipsoid scales")


def _run_host(gpu, name, on_frame=None):
    case = fc.get_case(name)
    ores, osnaps = _oracle_run(name)
    gb = _device(gpu, case)
    state = {}

    def before(k, op, prev):
        if on_frame and op["mode"] != fc.FRAME_FOREIGN:
            state["maps"] = fc.read_new_models(gb, fc.empty_maps())
            Ra, ta = fc.pose7_Rt(prev)
            Rb, tb = fc.pose7_Rt(op["rel7"])
            state["pose"] = fc.pose7(Ra @ Rb, Ra @ tb + ta)

    def after(k, op, r):
        if _refreshes(op):
            assert r["status"] == 0
            _check_refresh(gb, osnaps[k], (name, k))
        if on_frame and op["op"] == "frame" and op["mode"] != fc.FRAME_FOREIGN and k > 0:
            on_frame(state["maps"], state["pose"], r)

    res = fc.run_case(gb, case, before, after)
    fc.compare_results(case, res, ores)
    return case, res


def test_rank_against_distance_order(gpu):
    """Four HOST-mode frames, 0.04 m detection noise, K = 20 / 10 / 100 of 40 / 30 / 300 landmarks.  The first HOST frame takes the
    first-scan shortcut of HostBackend::associate (all -1, the map seeded).  Every solve moves the models (k_map_refresh) off the
    first-seen float32 cloud, so a match's position in the nearest-first submap — the number of selected keys below its own,
    assoc_core rank_mode — is not its position by model distance: the sequence is asserted to contain such matches.  The third
    frame is FRAME_HOST_DEFERRED followed by end_frame once.  After every HOST frame and after end_frame the refresh is checked
    exactly (_check_refresh)."""
    off = []
    case, res = _run_host(gpu, "host_rank", lambda maps, pose, r: off.append(fc.ranks_off_distance_order(maps, pose, r)))
    for c in fc.CLS:
        assert (res[0][c + "_match"] == -1).all() and np.array_equal(res[0][c + "_id"], np.arange(len(res[0][c + "_id"])))
    assert len(off) == 3 and sum(off) >= 3, off


def test_multi_robot_flow_on_one_map(gpu):
    """The order replay_multi uses: the host's frame (deferred refresh; the first scan: all -1), three FOREIGN frames of robot 1 that
    match the host's landmarks and add their own (the map grows across four ClassMap::sync_device calls while the landmark-id table
    stays behind), ingest_solve, end_frame (refresh_maps extends the lid table by everything the four frames added, then
    k_map_refresh), one more HOST frame.  Matches, ids and counts per frame equal the oracle's; the refresh is checked exactly."""
    case, res = _run_host(gpu, "multi_robot")
    grown = [res[k]["counts"]["point"] for k in range(4)]
    assert grown == sorted(grown) and grown[3] > grown[0]
    assert sum(int((res[-1][c + "_match"] >= 0).sum()) for c in fc.CLS) >= 20
