"""Multi-robot graphs at the edges of the assembly kernels of an exact joint pass — k_schur_lb (reduced system from pair lists),
k_lin_lf_b (linearisation of the landmark factors) and k_pose_b (H_pp and g_p per pose) — built on joint_graphs.Joint (test infrastructure for test_assembly_cases_reference.py and
test_gpu_assembly_edges.py).  Every builder returns (J, claims); check_claims(J, ref, claims) asserts on the host, from the
reference's own factor lists and from J.observers, that the graph reaches what its builder says it reaches.

What the kernels do at these edges (solver_kernels.hip):

  k_schur_lb   a block's pairs are shared out to eight lanes (pair x of the list to lane x mod 8); a lane loads its pair entries THREE at
               a time before the first record — 24 pairs of a block make one batch, the 25th opens a second one — and the records' columns
               two at a time (D = 3, 7, 9: one pair of columns and a single one, three and one, four and one).  The adjacency words of a
               32-pose chunk come straight from the bitmap: a strip that reaches 31, 32 or 33 poses below the diagonal ends in the first
               chunk, on its last row, or with one live block in the second chunk (the workgroups y >= 1 otherwise only write zeros).
  k_lin_lf_b   the cubes and cylinders are linearised 32 lanes per factor over each graph's list of them (lf_nbr), in one launch sized for
               the longest list of the batch.
  k_pose_b     one lane per entry of a pose: the graph's unary factors (in these graphs the one prior, whatever pose it sits on), the
               pose's between factors, its landmark factors; the 64 lanes' partial sums cross in one LDS transpose, so 63, 64, 65
               entries are the last lane, a full wave and a second entry on lane 0, and 130 is three entries on the first lanes.

Every builder is deterministic."""
from __future__ import annotations

import numpy as np

import joint_graphs as jg
from oracle import pyoracle as po

PAIR_BATCH = 24           # k_schur_listed_body: eight lanes load three pair entries each before the first record (x0 += 24)

PAIR_COUNTS = [1, 7, 8, 9, 16, 17, 24, 25]
POSE_LANES = [31, 32, 33, 34, 63, 64, 65, 66, 130, 131]
STRIP_REACH = [31, 32, 33]


def pair_counts(J, r):
    """{(pi, pj): pairs} of robot r's lower blocks, pi >= pj: over the landmarks only robot r observes (a separator landmark's F is
    zero, its pairs are not listed), (factors on pose pi) x (factors on pose pj)."""
    out = {}
    for cls, g, _, obs in J.lms:
        if {a for a, _ in obs} != {r}:
            continue
        ks = np.array([k for _, k in obs])
        poses, cnt = np.unique(ks, return_counts=True)
        for i, pi in enumerate(poses):
            for j, pj in enumerate(poses[: i + 1]):
                out[(int(pi), int(pj))] = out.get((int(pi), int(pj)), 0) + int(cnt[i] * cnt[j])
    return out


def pose_lanes(J, ref, r, k):
    """Lanes of k_pose_b's wave that hold an entry of pose k of robot r: the shard's prior, the pose's odometry factors, its landmark
    factors (no relative-pose factors in these graphs: no ghosts)."""
    assert not J.relmeas
    per_pose, _ = ref.list_lengths()
    P = J.sizes[r]
    return 1 + (k > 0) + (k < P - 1) + int(per_pose[ref.pose_var(r, k)])


def _partner(J, rng):
    """Robot 1 shares two points with robot 0's first poses (the batch has a separator), and every robot gets background landmarks."""
    c = jg._near(J, 0, 0, rng, 5.0)
    J.point(c + np.array([1.0, -2.0, 0.3]), [(0, 0), (0, 1), (1, 0), (1, 1)])
    J.point(c + np.array([-1.0, 1.5, 0.2]), [(0, 1), (1, 2)])


def pair_count_case(seed=41):
    """Robot 0: block (10 i + 3, 10 i) holds PAIR_COUNTS[i] pairs (that many points seen from exactly those two poses): one pair on one
    lane; seven; one per lane; a second entry on lane 0; two per lane; a third entry on lane 0; a full batch of 24; a second batch.
    Block (88, 85) holds 8 points, 8 cylinders, 8 cubes created in that order, so the three entries of every lane's share lie on
    landmarks of three different dimensions (the pair list is ordered by landmark, and landmarks of a class are numbered in creation
    order).  Pose 94 .. 96 observe nothing: their columns hold the diagonal block and a block with a between factor and NO pair; the
    last pose's column holds the diagonal block only.  Background landmarks span three consecutive poses and never two poses three
    apart."""
    P = 97
    J = jg.Joint([P, 9], seed=seed, step=0.3)
    rng = np.random.default_rng(seed)
    claims = {"pairs": {}, "empty_cols": [P - 1]}
    for i, n in enumerate(PAIR_COUNTS):
        pj, pi = 10 * i, 10 * i + 3
        for _ in range(n):
            J.point(jg._near(J, 0, pj, rng), [(0, pj), (0, pi)])
        claims["pairs"][(pi, pj)] = n
    for cls in (2, 0, 1):
        for _ in range(8):
            jg._add(J, cls, jg._near(J, 0, 85, rng), [(0, 85), (0, 88)], rng)
    claims["pairs"][(88, 85)] = 24
    claims["mixed_block"] = (88, 85)
    claims["pairs"][(95, 94)] = 0
    _partner(J, rng)
    # (background: every fourth pose, seen from poses k, k + 1, k + 2 — stops before the poses that are to observe nothing)
    n = 0
    for r in range(J.R):
        for k in range(1, J.sizes[r] - (5 if r == 0 else 0), 4):
            jg._add(J, n % 3, jg._near(J, r, k, rng), [(r, j) for j in range(k, min(J.sizes[r] - (4 if r == 0 else 0), k + 3))], rng)
            n += 1
    return J, claims


def strip_case(seed=42):
    """Robot 0 (70 poses): the columns of poses 2, 4 and 6 re-observe a landmark 31, 32 and 33 poses later — a point, a cylinder, a cube —
    so their strips end on row 31 of the first chunk, on row 0 of the second (its only live block) and on row 1 of the second."""
    P = 70
    J = jg.Joint([P, 10], seed=seed, step=0.25)
    rng = np.random.default_rng(seed)
    claims = {"pairs": {}, "reach": {}}
    for cls, (pj, d) in zip((2, 0, 1), zip((2, 4, 6), STRIP_REACH)):
        jg._add(J, cls, jg._near(J, 0, pj, rng), [(0, pj), (0, pj + d)], rng)
        claims["pairs"][(pj + d, pj)] = 1
        claims["reach"][pj] = d
    _partner(J, rng)
    jg.background(J, rng, every=4)
    return J, claims


def pose_lane_case(seed=43):
    """Robot 0: pose 6 i + 2 holds POSE_LANES[i] lanes' worth of entries (the prior's lane, two odometry factors, the rest points that
    pose 6 i + 3 sees too): half of the wave's lanes, give or take (31, 32, 33 incident factors), the 64 lanes of the wave give or
    take (63, 64, 65 incident factors: a second entry on lane 0), and more than two entries per lane (130).  The last pose
    observes nothing: one incident factor.  (The blocks (6 i + 3, 6 i + 2) carry up to 128 pairs: six batches of k_schur_lb.)"""
    P = 6 * len(POSE_LANES) + 3
    J = jg.Joint([P, 11], seed=seed, step=0.3)
    rng = np.random.default_rng(seed)
    claims = {"lanes": {}, "pairs": {}}
    for i, n in enumerate(POSE_LANES):
        k = 6 * i + 2
        for _ in range(n - 3):
            J.point(jg._near(J, 0, k, rng), [(0, k), (0, k + 1)])
        claims["lanes"][k] = n
        claims["pairs"][(k + 1, k)] = n - 3
    claims["lanes"][P - 1] = 2          # (the prior's lane and the one odometry factor)
    _partner(J, rng)
    for k in range(5, P - 2, 6):         # (poses 6 i + 5, 6 i + 6 = 6 (i + 1): away from the counted poses)
        jg._add(J, (k // 6) % 3, jg._near(J, 0, k, rng), [(0, k), (0, k + 1)], rng)
    for k in range(3, 10, 3):
        jg._add(J, k % 3, jg._near(J, 1, k, rng), [(1, k), (1, k + 1)], rng)
    return J, claims


def landmark_order_case(seed=44):
    """Two robots of 13 and 10 poses whose landmarks are created cylinder, cube, point, cylinder, ... : any four consecutive landmarks
    of a robot (one workgroup of k_landmark_b) are of three different classes, and neither a robot's pose count nor its landmark count
    is a multiple of four (the last workgroup of k_landmark_b and of k_pose_b is partly empty)."""
    J = jg.Joint([13, 10], seed=seed)
    rng = np.random.default_rng(seed)
    jg.background(J, rng, every=2)
    J.point(jg._near(J, 0, 3, rng), [(0, 3), (0, 4), (1, 2), (1, 3)])
    J.cylinder(jg._near(J, 0, 6, rng), [0.05, -0.02, 1.0], 0.3, [(0, 6), (1, 5)])
    return J, {"three_classes": True}


def factor_classes(J, r):
    """(bearing-range factors, cube and cylinder factors) of robot r."""
    br = sum(sum(1 for a, _ in obs if a == r) for cls, _, _, obs in J.lms if cls == 2)
    nbr = sum(sum(1 for a, _ in obs if a == r) for cls, _, _, obs in J.lms if cls != 2)
    return br, nbr


def lin_list_case(seed=45):
    """k_lin_lf_b's 32-lane region runs over each graph's list of cube and cylinder factors, the launch sized for the longest list of
    the batch: robot 0 holds bearing-range factors only (an empty list), robot 1 cubes and cylinders only (every factor listed),
    robot 2 a mix; robots 1 and 2 list 13 and 11 factors (no multiple of eight: the last workgroup of the region is partly empty, and
    robot 2's list ends inside robot 1's).  Robot 2 shares a point with robot 0 and a cylinder with robot 1."""
    J = jg.Joint([9, 10, 11], seed=seed)
    rng = np.random.default_rng(seed)
    for k in range(0, 8, 2):
        J.point(jg._near(J, 0, k, rng), [(0, k), (0, k + 1)])
    for i, k in enumerate(range(0, 8, 2)):
        jg._add(J, i % 2, jg._near(J, 1, k, rng), [(1, k), (1, k + 1), (1, k + 2)], rng)
    for i, k in enumerate(range(0, 9, 2)):
        jg._add(J, (2, 0, 2, 1, 2)[i], jg._near(J, 2, k, rng), [(2, k), (2, k + 1), (2, k + 2)], rng)
    J.point(jg._near(J, 0, 4, rng), [(0, 4), (0, 5), (2, 3), (2, 4)])
    J.cylinder(jg._near(J, 1, 5, rng), [0.05, -0.02, 1.0], 0.3, [(1, 5), (2, 6), (2, 7), (2, 8), (2, 9), (2, 10)])
    return J, {"factor_classes": [(10, 0), (0, 13), (11, 11)]}


CASES = [("pair_counts", pair_count_case), ("strip_reach", strip_case), ("pose_lanes", pose_lane_case),
         ("landmark_order", landmark_order_case), ("lin_list", lin_list_case)]


def check_claims(J, ref, claims):
    """Assert on the host that J reaches what its builder claims."""
    pc = pair_counts(J, 0)
    for blk, n in claims.get("pairs", {}).items():
        assert pc.get(blk, 0) == n, (blk, pc.get(blk, 0), n)
    if "mixed_block" in claims:
        pi, pj = claims["mixed_block"]
        dims = [jg.SLOT_DIM[cls] for cls, _, _, obs in J.lms if sorted(obs) == [(0, pj), (0, pi)]]
        assert len(dims) == PAIR_BATCH and [dims[x] for x in (0, 8, 16)] == [3, 7, 9]
        assert all(len({dims[s], dims[s + 8], dims[s + 16]}) == 3 for s in range(8))
    for pj in claims.get("empty_cols", []):
        assert [b for b in pc if b[1] == pj and b[0] > pj] == [] and pj == J.sizes[0] - 1
    for pj, d in claims.get("reach", {}).items():
        assert max(b[0] for b in pc if b[1] == pj) - pj == d
    for k, n in claims.get("lanes", {}).items():
        assert pose_lanes(J, ref, 0, k) == n, (k, pose_lanes(J, ref, 0, k), n)
    for r, want in enumerate(claims.get("factor_classes", [])):
        assert factor_classes(J, r) == want, (r, factor_classes(J, r), want)
        br, nbr = want
        assert (r != 0 or nbr == 0) and (r != 1 or br == 0) and (nbr == 0 or nbr % 8)
        lm = np.isin(ref.ftype, (po.F_CUBE, po.F_CYL))
        assert int(lm.sum()) == sum(w[1] for w in claims["factor_classes"])
    if claims.get("three_classes"):
        _, per_lm = ref.list_lengths()
        for r in range(J.R):
            order = [cls for cls, _, _, obs in J.lms if r in {a for a, _ in obs}]
            assert len(order) % 4 and J.sizes[r] % 4, (len(order), J.sizes[r])
            assert all(len(set(order[i:i + 4])) == 3 for i in range(0, len(order) - 4))
        assert per_lm.sum() > 0
