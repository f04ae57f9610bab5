"""The layout tables of a set of graphs (tile profile, border profile, segments, segment table, the shards' chol_dim) against the
arrays recorded at the commit before the layout planning moved into csrc/host_layout.hpp (tests/golden/layout_parent.npz, written by
tests/golden/make_layout_golden.py on the GPU; the commit's hash is stored in the file).  Every array must match exactly: moving the
planner changed no table.  The graphs: robots of mixed sizes (64 poses as the threshold for a cut, an empty border), bands cut into 1 - 4
segments, borders of 63 - 129 coordinates, ghost factors, a strip wider than 256 poses, a column past the LDS cap, a stream whose S is
re-allocated, a graph before and after merge_landmarks."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import make_layout_golden as mk                                                # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(HERE, "golden", "layout_parent.npz")) as f:
        return {k: f[k] for k in f.files if k != "parent"}, str(f["parent"])


@pytest.mark.parametrize("name", mk.CASE_NAMES)
def test_layout_tables_match_the_recorded_parent(gpu, recorded, name):
    want = {k[len(name) + 1:]: v for k, v in recorded[0].items() if k.startswith(name + "/")}
    got = mk.cases(gpu)[name]()
    assert want and sorted(got) == sorted(want)
    differ = [k for k in sorted(want) if got[k].dtype != want[k].dtype or not np.array_equal(got[k], want[k])]
    print(f"[layout] {name}: {len(want)} arrays, {sum(a.size for a in want.values())} words against commit {recorded[1]}: {len(differ)} differ")
    assert not differ, differ


def test_recorded_cases_reach_their_edges(recorded):
    """The recorded file covers every case, and the cases what they are there for: bands cut into 2, 3 and 4 segments and an uncut one,
    an empty border, ghost rows, a stream that outgrows its first allocation, a merge that widens the profile."""
    want = recorded[0]
    assert {k.split("/")[0] for k in want} == set(mk.CASE_NAMES) == set(mk.cases(None))
    assert [len(want[f"segments{n}/r0/segs"]) // 2 for n in (1, 2, 3, 4)] == [0, 2, 3, 4]
    assert len(want["sizes_private/r1/bfirst"]) == 0 and len(want["relmeas/r0/bfirst"]) > 0
    assert want["stream/prof_len"].min() == 1 and want["stream/prof_len"].max() > 4
    assert want["merge/after/prof"][0] > want["merge/before/prof"][0]
