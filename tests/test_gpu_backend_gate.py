"""The association gate of the streaming back-end (slide_backend_set_association_gate / slide_backend_gate_stats): a frame's matches
tested at the predicted pose inside slide_backend_process_frame, before they are added.

The stream: 16 key frames (14 of them the main run, two for after a foreign packet) along a gently turning path, twelve landmarks
(four points, four cubes, four cylinders, at least 4 m apart) all detected in every frame with 1 cm of detection noise, odometry
noise at closure_cases.ODOM_SIGMA6 x the step; the back-end runs with bearing_range_sigma 0.05, cylinder_sigma 0.1 and those odometry sigmas (under the defaults — 1 m / 1 rad and
400 — the gate passes anything).  Frame 10 carries one EXTRA ellipsoid detection 0.6 m behind point landmark 2 as seen from the
robot: inside the Euclidean gate (0.75 m), nearer to that landmark than to any other, twelve range sigmas out."""
import numpy as np
import pytest

import closure_cases as cc
import gn_graphs as gg

pytestmark = pytest.mark.gpu

P_FRAMES, MAIN, PLANT_FRAME, PLANT_LM, PLANT_OFF = 16, 14, 10, 2, 0.6
PROB = 0.99
POINTS = np.array([[1.0, 4.0, 0.5], [5.0, -4.0, 1.0], [9.0, 4.0, 0.8], [13.0, -4.0, 0.6]])
CUBES = np.array([[3.0, -5.0, 0.5], [7.0, 5.0, 0.7], [11.0, -5.5, 0.4], [15.0, 4.5, 0.6]])
CYLS = np.array([[-1.0, -4.0, 0.0], [3.0, 8.0, 0.0], [7.0, -8.0, 0.0], [12.0, 8.5, 0.0]])
CUBE_YAW = [0.3, -1.1, 2.0, 0.7]
CUBE_SCALE = np.array([0.8, 1.5, 0.6])
ELL_SCALE = np.array([0.5, 0.5, 0.9])
RAY = np.array([0.0, 0.05, 1.0]) / np.linalg.norm([0.0, 0.05, 1.0])
PARAMS = dict(noise_model_odom_vec=list(cc.ODOM_SIGMA6), bearing_range_sigma=0.05, cylinder_sigma=0.1)


def truth(k):
    return gg.rot([0.0, 0.0, 0.05 * k]), np.array([1.0 * k, 0.3 * np.sin(0.4 * k), 0.0])


def stream(plant=True, seed=7):
    """[(rel7, detections, planted ellipsoid's index or -1)] per frame; rel7 of frame 0 is the first pose itself (prev = identity)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(P_FRAMES):
        R, t = truth(k)
        if k == 0:
            rel = (R, t)
        else:
            Rp, tp = truth(k - 1)
            step = (Rp.T @ R, Rp.T @ (t - tp))
            n = rng.normal(0, 1, 6) * cc.ODOM_SIGMA6 * np.linalg.norm(step[1])
            rel = cc._mul(step, (cc._rotvec(n[:3]), n[3:]))
        body = lambda pw: R.T @ (pw - t) + rng.normal(0, 0.01, 3)
        ell = [gg.p7(R.T, body(p)) for p in POINTS]
        cube = [gg.p7(R.T @ gg.rot([0.0, 0.0, y]), body(p)) for p, y in zip(CUBES, CUBE_YAW)]
        roots = [body(p) for p in CYLS]
        planted = -1
        if plant and k == PLANT_FRAME:
            d = POINTS[PLANT_LM] - t
            planted = len(ell)
            ell.append(gg.p7(R.T, R.T @ (POINTS[PLANT_LM] + PLANT_OFF * d / np.linalg.norm(d) - t)))
        det = dict(cyl_root=np.array(roots), cyl_ray=np.array([R.T @ RAY] * len(CYLS)), cyl_radius=np.full(len(CYLS), 0.25),
                   cyl_label=np.ones(len(CYLS), np.int32), cube_pose7=np.array(cube), cube_scale=np.array([CUBE_SCALE] * len(CUBES)),
                   cube_label=np.ones(len(CUBES), np.int32), ell_pose7=np.array(ell), ell_scale=np.array([ELL_SCALE] * len(ell)),
                   ell_label=np.ones(len(ell), np.int32))
        out.append((cc.p7(rel), det, planted))
    return out


def backend(gpu, gate=None, on_reject="drop"):
    B = gpu.SlideBackend(gpu.default_params(**PARAMS), 2)
    if gate is not None:
        B.set_association_gate(gate, on_reject)
    return B


def replay(B, frames, upto=None):
    prev, res = np.array([0.0, 0, 0, 0, 0, 0, 1]), []
    for rel7, det, _ in frames[:upto]:
        r = B.process_frame(0, rel7, prev, det)
        assert r["status"] == 0
        prev = r["pose7"].copy()
        res.append(r)
    return res, prev


def candidates(est7, det):
    """The tuples predicted_observation_mahalanobis takes for EVERY detection of the frame against the landmark of its own number (the
    ground truth's; the planted extra one against PLANT_LM), with the measurement process_frame passes: the detection taken to the
    world frame at the predicted pose."""
    X = cc._pose(est7, np.float64)
    out = {"cyl": [], "cube": [], "ell": []}
    for i, (root, ray, rad) in enumerate(zip(det["cyl_root"], det["cyl_ray"], det["cyl_radius"])):
        out["cyl"].append(("cylinder", 0, 0, i, est7, X[0] @ root + X[1], X[0] @ ray, rad))
    for i, (c7, sc) in enumerate(zip(det["cube_pose7"], det["cube_scale"])):
        out["cube"].append(("cube", 0, 0, i, est7, cc.p7(cc._mul(X, cc._pose(c7, np.float64))), sc))
    for i, e7 in enumerate(det["ell_pose7"]):
        pb = X[0].T @ ((X[0] @ e7[:3] + X[1]) - X[1])
        out["ell"].append(("point", 0, 0, i if i < len(POINTS) else PLANT_LM, pb / np.linalg.norm(pb), float(np.linalg.norm(pb))))
    return out


def test_gate_off_is_the_back_end_as_it_was(gpu):
    """A back-end that never sets the gate and one that sets it to 0 give the same ids, matches and poses bit for bit, and count
    nothing; the planted detection is matched to its neighbour by both (the Euclidean gate lets it in)."""
    frames = stream()
    A, B = backend(gpu), backend(gpu, 0.0)
    ra, _ = replay(A, frames, MAIN)
    rb, _ = replay(B, frames, MAIN)
    for a, b in zip(ra, rb):
        for f in ("pose7", "cyl_id", "cube_id", "ell_id", "cyl_match", "cube_match", "ell_match"):
            assert np.array_equal(a[f], b[f]), f
    assert ra[PLANT_FRAME]["ell_id"][-1] == PLANT_LM and ra[PLANT_FRAME]["ell_match"][-1] >= 0
    for k in range(1, MAIN):
        assert ra[k]["ell_id"][:4].tolist() == [0, 1, 2, 3] and ra[k]["cube_id"].tolist() == [0, 1, 2, 3] and ra[k]["cyl_id"].tolist() == [0, 1, 2, 3]
    assert A.gate_stats() == B.gate_stats() == dict(frames_gated=0, frames_skipped=0, tested=0, rejected=0)
    ca, cb = A.counts(), B.counts()
    assert all(np.array_equal(ca[f], cb[f]) for f in ca) and ca["point"] == 4 and ca["cube"] == 4 and ca["cyl"] == 4


@pytest.mark.parametrize("on_reject", ["drop", "new"])
def test_gate_decides_as_the_predicted_gate_does(gpu, on_reject):
    """With the gate on, every decision of process_frame equals thresholding predicted_observation_mahalanobis, called on the back-end's
    own graph with the same inputs just before the frame; the planted detection gets MATCH_GATED and every true match is kept; a drop
    leaves the landmark count as it was and adds no factor, a new adds one landmark and one factor; gate_stats counts frame 0 and
    the frame after an unsolved foreign packet as skipped."""
    frames = stream()
    B = backend(gpu, PROB, on_reject)
    q = {d: gpu.chi2_quantile(PROB, d) for d in (3, 7, 9)}
    prev = np.array([0.0, 0, 0, 0, 0, 0, 1])
    tested = rejected = gated = 0
    for k, (rel7, det, planted) in enumerate(frames[:MAIN]):
        want = None
        if k > 0:
            est7 = cc.p7(cc._mul(cc._pose(prev, np.float64), cc._pose(rel7, np.float64)))
            cl = candidates(est7, det)
            flat = cl["cyl"] + cl["cube"] + cl["ell"]
            pre = B.graph.predicted_observation_mahalanobis(0, k - 1, rel7, est7, flat)
            assert (pre["status"] == 0).all()
            want = pre["d2"] > np.array([q[int(d)] for d in pre["dof"]])
            print(f"[backend-gate] frame {k}: d2 / quantile from {(pre['d2'] / [q[int(d)] for d in pre['dof']]).min():.3g} to "
                  f"{(pre['d2'] / [q[int(d)] for d in pre['dof']]).max():.3g}")
        before = B.counts()
        r = B.process_frame(0, rel7, prev, det, gpu.FRAME_HOST_DEFERRED if k % 2 else gpu.FRAME_HOST)
        assert r["status"] == 0
        if k % 2:
            st, pose = B.end_frame(0)
            assert st == 0
            r["pose7"] = pose
        prev = r["pose7"].copy()
        after = B.counts()
        if k == 0:
            continue
        match = np.concatenate([r["cyl_match"], r["cube_match"], r["ell_match"]])
        ids = np.concatenate([r["cyl_id"], r["cube_id"], r["ell_id"]])
        assert ((match == gpu.MATCH_GATED) == want).all(), (k, match, want)
        assert (match != -1).all()                                       # (every detection of frames 1 .. is a candidate)
        gated += 1
        tested += len(match)
        rejected += int(want.sum())
        n_new = int(want.sum()) if on_reject == "new" else 0
        kept = ~want
        assert (ids[kept] == np.array([c[3] for c in flat])[kept]).all()
        if planted >= 0:
            assert want[-1] and want.sum() == 1, want                    # the planted one, and every true match kept
            assert r["ell_match"][planted] == gpu.MATCH_GATED
            assert r["ell_id"][planted] == (-1 if on_reject == "drop" else before["point"])
        else:
            assert not want.any(), (k, want)
        assert after["point"] == before["point"] + n_new and after["cyl"] == before["cyl"] and after["cube"] == before["cube"]
        assert after["factors"] == before["factors"] + 1 + int(kept.sum()) + n_new
    assert rejected == 1
    assert B.gate_stats() == dict(frames_gated=gated, frames_skipped=1, tested=tested, rejected=rejected)
    # a foreign packet (robot 1, no solve), then a host frame: associated ungated and counted as skipped; the frame after it is gated
    none = dict(cyl_root=np.zeros((0, 3)), cyl_ray=np.zeros((0, 3)), cyl_radius=np.zeros(0), cyl_label=np.zeros(0, np.int32),
                cube_pose7=np.zeros((0, 7)), cube_scale=np.zeros((0, 3)), cube_label=np.zeros(0, np.int32), ell_pose7=np.zeros((0, 7)),
                ell_scale=np.zeros((0, 3)), ell_label=np.zeros(0, np.int32))
    rf = B.process_frame(1, [0.0, 0, 0, 0, 0, 0, 1], [20.0, 3.0, 0, 0, 0, 0, 1], none, gpu.FRAME_FOREIGN)
    assert rf["status"] == 0
    assert B.gate_stats()["frames_skipped"] == 1                        # (a foreign frame is neither tested nor counted)
    for n in range(2):
        rel7, det, _ = frames[MAIN + n]
        r = B.process_frame(0, rel7, prev, det)
        assert r["status"] == 0 and (np.concatenate([r["cyl_match"], r["cube_match"], r["ell_match"]]) >= 0).all()
        prev = r["pose7"].copy()
        assert B.gate_stats() == dict(frames_gated=gated + n, frames_skipped=2, tested=tested + 12 * n, rejected=rejected)
    # the gate switched off again: nothing more is counted
    B.set_association_gate(0.0)
    B.process_frame(1, [0.0, 0, 0, 0, 0, 0, 1], [21.0, 3.0, 0, 0, 0, 0, 1], none, gpu.FRAME_FOREIGN)
    assert B.gate_stats()["frames_gated"] == gated + 1
    with pytest.raises(gpu.SlideError):
        B.set_association_gate(1.0)
    with pytest.raises(gpu.SlideError):
        B.set_association_gate(0.5, "keep")
