"""Landmark fusion without a device: merge_clusters, the Rekey reference of tests/landmark_merge_cases.py, the refusals
slide_graph_merge_landmarks decides on the host before any graph or device is looked at, and the binding's argument errors."""
import ctypes as C

import numpy as np
import pytest

import landmark_merge_cases as lm
import slide_slam_amd as s
from oracle import pyoracle as po


def _rows(r):
    return [tuple(int(v) for v in row) for row in np.asarray(r).reshape(-1, 2)]


def test_merge_clusters_chains_triangles_repeats():
    assert _rows(s.merge_clusters([], [])) == []
    assert s.merge_clusters([], []).shape == (0, 2) and s.merge_clusters([], []).dtype == np.uint64
    assert _rows(s.merge_clusters([5], [3])) == [(3, 5)]                                  # reversed: the smallest key survives
    assert _rows(s.merge_clusters([1, 2, 3], [2, 3, 4])) == [(1, 2), (1, 3), (1, 4)]      # a chain
    assert _rows(s.merge_clusters([7, 7, 8], [8, 9, 9])) == [(7, 8), (7, 9)]              # a triangle
    assert _rows(s.merge_clusters([4, 4, 6, 4], [6, 6, 4, 4])) == [(4, 6)]                # repeated, reversed and a == b
    assert _rows(s.merge_clusters([10, 1, 20], [11, 2, 21])) == [(1, 2), (10, 11), (20, 21)]
    # two clusters joined late by their largest members
    assert _rows(s.merge_clusters([1, 5, 3, 7], [3, 7, 5, 9])) == [(1, 3), (1, 5), (1, 7), (1, 9)]
    with pytest.raises(s.SlideError):
        s.merge_clusters([1, 2], [3])


def test_merge_clusters_does_not_depend_on_the_order():
    rng = np.random.default_rng(4)
    n = 30
    a = rng.integers(0, 60, n)
    b = rng.integers(0, 60, n)
    want = _rows(s.merge_clusters(a, b))
    assert len(want) > 10 and len({k for k, _ in want}) > 3 and len(want) > len({k for k, _ in want})      # several clusters, some of three or more
    for k, m in want:
        assert k < m
    assert all(k not in {m for _, m in want} for k, _ in want)       # a survivor is no one's member
    for seed in range(5):
        p = np.random.default_rng(seed).permutation(n)
        flip = np.random.default_rng(seed + 50).random(n) < 0.5
        aa, bb = np.where(flip, b[p], a[p]), np.where(flip, a[p], b[p])
        assert _rows(s.merge_clusters(aa, bb)) == want


@pytest.mark.parametrize("chart", [0, 1])
def test_rekeyed_reference_is_the_merged_graph(chart):
    """dup40 with every true pair of both classes merged, as data: (variables - drops) variables, the same factors in the same order,
    and every factor of a dropped key on its survivor."""
    plain, W = lm.reference("dup40", chart)
    rows = {kind: lm.true_pairs(W, kind) for kind in ("point", "cylinder")}
    drop = lm.drop_map(rows)
    assert len(drop) == 13 + 6
    merged, _ = lm.reference("dup40", chart, drop)
    assert len(merged.vtype) == len(plain.vtype) - len(drop)
    assert len(merged.ftype) == len(plain.ftype) and np.array_equal(merged.ftype, plain.ftype)
    assert np.array_equal(merged.fz, plain.fz) and np.array_equal(merged.fsig, plain.fsig)
    key_of = {(cls, d): (ord(lm.KEY_TAG[cls]) << 56) | k for (cls, d), k in drop.items()}
    dropped_keys = {(ord(lm.KEY_TAG[cls]) << 56) | d for (cls, d) in drop}
    assert not dropped_keys & {int(k) for k in merged.vkey}
    moved = 0
    for f in range(len(plain.ftype)):
        assert int(merged.vkey[merged.fv[f, 0]]) == int(plain.vkey[plain.fv[f, 0]])
        if int(plain.ftype[f]) not in (po.F_BR, po.F_CUBE, po.F_CYL):
            assert int(merged.fv[f, 1]) < 0 or int(merged.vkey[merged.fv[f, 1]]) == int(plain.vkey[plain.fv[f, 1]])
            continue
        key = int(plain.vkey[plain.fv[f, 1]])
        cls, idx = "lcu".index(chr(key >> 56)), key & ((1 << 56) - 1)
        want = key_of.get((cls, idx), key)
        moved += want != key
        assert int(merged.vkey[merged.fv[f, 1]]) == want
    assert moved == 2 * len(drop)                                  # every dropped landmark of dup40 has two factors
    # the survivors keep their own initial values
    for (cls, d), k in drop.items():
        assert np.array_equal(merged.values[merged.lm_var(cls, k)], plain.values[plain.lm_var(cls, k)])


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_host_refusals_need_no_device():
    L = s.lib()
    cls, keep, drop = np.array([2, 0], np.int32), np.array([1, 2], np.uint64), np.array([3, 4], np.uint64)
    into, moved, status = np.full(2, 77, np.uint64), np.full(2, 77, np.int32), np.full(2, 77, np.int32)
    g = C.c_void_p(None)

    def call(n=2, c=cls, k=keep, d=drop, fuse=0):
        rc = L.slide_graph_merge_landmarks(g, C.c_int(n), _p(c) if c is not None else None, _p(k) if k is not None else None,
                                           _p(d) if d is not None else None, C.c_int(fuse), _p(into), _p(moved), _p(status))
        return rc, s.api.last_error()

    for kw, reason in ((dict(), "the graph is NULL"), (dict(n=-1), "n < 0"), (dict(c=None), "a needed pointer is NULL"),
                       (dict(k=None), "a needed pointer is NULL"), (dict(d=None), "a needed pointer is NULL"),
                       (dict(c=np.array([2, 3], np.int32)), "not a landmark class"), (dict(c=np.array([-1, 0], np.int32)), "not a landmark class"),
                       (dict(fuse=2), "fuse"), (dict(fuse=-1), "fuse")):
        rc, msg = call(**kw)
        assert rc == -1 and "merge_landmarks" in msg and reason in msg, (kw, rc, msg)
    assert (into == 77).all() and (moved == 77).all() and (status == 77).all()       # nothing written
    out = C.c_uint64(5)
    assert L.slide_graph_landmark_alias(g, C.c_int(2), C.c_uint64(1), C.byref(out)) == -1 and out.value == 5


def test_binding_argument_errors():
    G = object.__new__(s.SlideGraph)           # (no handle: the binding must refuse before it reaches the library)
    with pytest.raises(s.SlideError, match="not a landmark class"):
        s.SlideGraph.merge_landmarks(G, 3, [(0, 1)])
    with pytest.raises(s.SlideError, match="rows of"):
        s.SlideGraph.merge_landmarks(G, 2, [0, 1, 2])
    with pytest.raises(s.SlideError, match="rows of"):
        s.SlideGraph.merge_landmarks(G, 2, [(0, 1, 2)])
    with pytest.raises(s.SlideError, match="negative"):
        s.SlideGraph.merge_landmarks(G, 2, [(0, -1)])
    with pytest.raises(s.SlideError, match="negative"):
        s.merge_clusters([0], [-4])
