"""Each streaming update of the product (SlideGraph.solve(): iSAM2-style, one per key frame) against an independent least-squares
step: with the wildfire bound off an update is exactly one Gauss-Newton step of the full linearisation at the per-variable
linearisation points theta, and tests/stream_graphs.py restates theta from the product's read-backs (test_stream_reference.py
checks that restatement against the oracle's own solve).  A c_d or pose0 one column too high, a wrong prediction or a stale CSR
table leaves stale blocks in the factor: that changes the path to the optimum, not the optimum, so parity after a few more frames
does not see it; one update does.

Per update: every pose (the newest one from the closing pack's cache) and landmark read back and compared with gn_reference's step
at theta, within its bound; stats()["n_relin"] equals the variables the tracker relinearised; incremental_stats()'s first
re-factored column is at most 6 pmin / 64, pmin being the test's restatement of the dirty rule.  Every case asserts that it reached
its edge.  The four switches (SLIDE_NO_PREDICT, SLIDE_NO_LIN_SKIP, SLIDE_NO_FUSED_FINAL, SLIDE_NO_INCREMENTAL; each read once per
process) run the drift case in a child process each."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stream_graphs as sg                                                       # noqa: E402

pytestmark = pytest.mark.gpu

NB = sg.NB
NOTHING = 1 << 30


def check_updates(R):
    """The per-update assertions beyond the step itself (Run.solve checked that).  -> (worst error / tolerance, per-update
    increments of the incremental and full counters)."""
    inc, full = [], []
    prev = dict(incremental=0, full=0)
    for n, u in enumerate(R.updates):
        assert u.gpu_relin == u.n_relin, (n, u)
        assert u.block_columns == u.T, (n, u)
        bound = u.T if u.pmin >= NOTHING else 6 * u.pmin // NB
        assert u.last_first_column <= bound, (n, u)
        inc.append(u.incremental - prev["incremental"])
        full.append(u.full - prev["full"])
        assert inc[-1] + full[-1] == 1, (n, u)
        prev = dict(incremental=u.incremental, full=u.full)
    return max(u.ratio for u in R.updates), inc, full


def run(gpu, chart, case, *a, **kw):
    S, R, G = sg.stream_pair(gpu, chart, 60, **kw)
    marks = case(S, R, *a, **({"set_incremental": G.set_incremental} if case is sg.case_toggle else {}))
    worst, inc, full = check_updates(R)
    print(f"[stream-step] {case.__name__}{a} chart {chart}: {len(R.updates)} updates, worst scaled_error / tolerance {worst:.3e}")
    return R, marks, inc, full


def column(u):
    """The first re-factored block column the dirty rule asks for."""
    return u.T if u.pmin >= NOTHING else 6 * u.pmin // NB


@pytest.mark.parametrize("chart", [0, 1])
def test_plain(gpu, chart):
    """P = 1 .. 50: T <= 2 (full path), the first incremental updates, the band gaining block columns (at T = 5 S is re-allocated:
    full path), T > 4."""
    R, _, inc, full = run(gpu, chart, sg.case_plain)
    U = R.updates
    for n, u in enumerate(U):
        if u.T <= 2:
            assert full[n] == 1, (n, u)
    first_inc = next(n for n in range(len(U)) if inc[n])
    assert U[first_inc].T == 3 and U[first_inc - 1].T <= 2
    grow = next(n for n in range(len(U)) if U[n].T == 5)
    assert full[grow] == 1 and U[grow].last_first_column == 0      # (S re-allocated: nothing of the last factor survives)
    assert sum(inc[n] for n in range(len(U)) if U[n].T == 5) >= 5
    for n, u in enumerate(U):
        if inc[n]:
            assert u.last_first_column == column(u), (n, u)


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("cls", ["point", "cube", "cyl"])
def test_reobserve(gpu, chart, cls):
    """An old landmark re-observed, first observer 42 / 32 / 31 / 11 / 10: pmin from its first observer (h_lm_first), the CSR tail
    rebuilt from an old list.  Pose 10 spans columns 0 and 1 (coordinates 60 .. 65): c_d = 0 through the incremental branch."""
    _, marks, _, _ = run(gpu, chart, sg.case_reobserve, cls)
    for f, u in marks.items():
        assert u.pmin_fac == f and u.last_first_column == column(u), (f, u)
    assert [column(marks[f]) for f in (10, 11, 31, 32)] == [0, 1, 2, 3]


@pytest.mark.parametrize("chart", [0, 1])
def test_late_observation(gpu, chart):
    """A landmark observed from a pose older than its first observer (30 -> 25); its relinearisation at the next update dirties
    from the new first observer: column 6 * 25 / 64 = 2, not 6 * 30 / 64."""
    _, m, _, _ = run(gpu, chart, sg.case_late)
    assert m["late"].last_first_column == 2 and m["key"] in m["after"].moved
    assert m["after"].pmin_rel == 25 and m["after"].last_first_column == 2


@pytest.mark.parametrize("chart", [0, 1])
def test_loop(gpu, chart):
    """A loop closure from the newest pose to pose P-2, 21, 11, 10, 0: c_d from a between factor (0 through the incremental
    branch), the profile's reach."""
    R, marks, _, _ = run(gpu, chart, sg.case_loop)
    for i, u in marks.items():
        assert u.last_first_column == column(u), (i, u)
    assert [marks[i].last_first_column for i in (0, 10, 11, 21)] == [0, 0, 1, 1]


@pytest.mark.parametrize("chart", [0, 1])
def test_drift_correction(gpu, chart):
    """Drifting odometry, a loop closure to pose 0 with a large correction; the next update relinearises many old poses and
    landmarks, and its first dirty column comes from the prediction (pred_pose), below the merged factors' (dirty_min_pose).  That
    frame also closes a loop to, and re-observes, variables predicted to relinearise ("factors merged since the prediction only
    add")."""
    _, m, _, _ = run(gpu, chart, sg.case_drift, yaw_bias=0.02)
    nxt = m["next"]
    assert nxt.n_relin > 30 and m["lm"] in nxt.moved
    assert nxt.last_first_column == column(nxt) < 6 * nxt.pmin_fac // NB


@pytest.mark.parametrize("chart", [0, 1])
def test_repeat(gpu, chart):
    """solve() with no new factors: at T = 3 until nothing is dirty (c_d = T: the substitutions repeated); at T = 5 the captured
    hipGraph is replayed (same_as_prev; k_relin inside it: a full update)."""
    _, m, inc, full = run(gpu, chart, sg.case_repeat)
    last = m["small"][-1]
    assert last.pmin == NOTHING and last.last_first_column == last.T == 3 and inc[25 + 4] == 1
    for u in m["big"]:
        assert u.T == 5 and u.last_first_column == 0
    assert full[-2:] == [1, 1] and m["big"][0].n_relin > 0


@pytest.mark.parametrize("chart", [0, 1])
def test_incremental_toggle(gpu, chart):
    """set_incremental(False) before frame 30, back on before frame 36, on the same graph: the non-incremental branch in process."""
    R, _, inc, full = run(gpu, chart, sg.case_toggle)
    assert all(full[k] == 1 for k in range(30, 36))
    assert sum(inc[:30]) > 0 and sum(inc[36:]) > 0


CHILD = r'''
import json, os, sys
import torch
torch.zeros(1, device="cuda:0")
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import slide_slam_amd as s
import stream_graphs as sg
from chart_env import chart_kw
from test_gpu_stream_step import check_updates
s.device_check()
chart = chart_kw(s).get("pose_chart", s.CHART_CAYLEY)
S, R, G = sg.stream_pair(s, chart, 60, yaw_bias=0.02)
m = sg.case_drift(S, R)
worst, inc, full = check_updates(R)
nxt = m["next"]
json.dump(dict(worst=worst, inc=inc, full=full, n=len(R.updates), next_col=nxt.last_first_column, next_fac_col=6 * nxt.pmin_fac // 64,
               next_relin=nxt.n_relin), open(sys.argv[2], "w"))
'''


@pytest.mark.parametrize("switch", ["SLIDE_NO_PREDICT", "SLIDE_NO_LIN_SKIP", "SLIDE_NO_FUSED_FINAL", "SLIDE_NO_INCREMENTAL"])
def test_switch(gpu, switch, tmp_path):
    """The drift case in a fresh process with one fallback switch on (chart: SLIDE_TEST_CHART, tests/chart_env.py)."""
    out = str(tmp_path / "r.json")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, out], env=dict(os.environ, **{switch: "1"}), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    print(f"[stream-step] drift, {switch}=1: {res['n']} updates, worst scaled_error / tolerance {res['worst']:.3e}")
    assert res["next_relin"] > 30
    if switch == "SLIDE_NO_INCREMENTAL":
        assert sum(res["inc"]) == 0 and res["next_col"] == 0
    else:
        assert sum(res["inc"]) > 10 and res["next_col"] == 0 < res["next_fac_col"]
