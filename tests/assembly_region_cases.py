"""Multi-robot graphs at the edges of the merged launches of an exact joint pass's assembly stage, built on joint_graphs.Joint (test
infrastructure for test_assembly_region_cases_reference.py and test_gpu_assembly_regions.py).  Every builder returns (J, claims);
check_claims(J, ref, claims, run=None) asserts that the graph reaches what its builder says — on the host from J alone, and, given the
GPU run (test_gpu_joint_step.Run), also from the layout the shards report (border_profile, segment_table).

What the launches do at these edges (solver_kernels.hip, launch_phase3_arrow_batched / launch_arrow_finish_batched):

  k_border_clear_b     runs in front of the Schur launch when the fills are merged into it (behind it otherwise): per robot over the
                       tiles of the segment table when the band is cut, else linearly over the border rows.
  k_schur_lb           behind its pose columns three regions sized for the largest robot of the batch: the right-hand-side row and the
                       padding of the last tile (none when 6 P is a multiple of 64), the border fill (four slots per workgroup, over the
                       batch's slot count whatever a robot observes of them) and the lambda rows of the ghost factors (no workgroup at all
                       when no robot has one).  A robot with an empty border leaves all of them at once.
  k_backsub_sep_b      a separator landmark of any class takes its delta from the separator's solution instead of its factor sum.

SLIDE_ASM_MERGE=0 selects the separate launches; both must give the same bits.

Every builder is deterministic."""
from __future__ import annotations

import numpy as np

import joint_graphs as jg

NB = 64


def shared_by_robot(J):
    """Per robot, the (cls, gid) of the landmarks it observes that another robot observes too: its live slots."""
    out = [[] for _ in range(J.R)]
    for cls, g, _, obs in J.lms:
        robots = {a for a, _ in obs}
        if len(robots) > 1:
            for r in sorted(robots):
                out[r].append((cls, g))
    return out


def landmarks_by_robot(J):
    return [sum(1 for _, _, _, obs in J.lms if r in {a for a, _ in obs}) for r in range(J.R)]


def ghosts_by_robot(J):
    """Ghost factors per robot: a relative-pose measurement is a factor on both its robots."""
    return [sum((a == r) + (b == r) for _, a, b, _, _ in J.relmeas) for r in range(J.R)]


def _unequal(with_rel):
    J = jg.sizes_case([150, 10, 33], private_only=(1,))
    # (as jg.segments_case: a point seen from poses 14 apart around each place the default three segments are cut at — the separator
    # behind a cut must span more than a tile, or the band stays whole)
    rng = np.random.default_rng(77)
    for q in (50, 100):
        J.point(jg._near(J, 0, q, rng), [(0, q - 2), (0, q + 12)])
    if with_rel:
        J.relative(0, 5, 2, 7)
    claims = {
        "cut": [True, False, False],              # robot 0's band is cut (the segment-table clear), robot 2's is not (the linear clear)
        "empty_border": [False, True, False],     # robot 1 shares nothing and is too short to cut: its pad, fill and lambda workgroups leave at once
        "n_ghost": [1, 0, 1] if with_rel else [0, 0, 0],
        "slots": [6, 0, 6],
        # Only two robots share, so both hold every slot: the robot with the most landmarks (0) holds no more slots than robot 2, which
        # has under a fifth of its landmarks — the fill region is sized by the batch's slot count, not by any robot's landmarks.
        "most_landmarks": 0, "as_many_slots": 2,
    }
    return J, claims


def unequal_case():
    """150, 10 and 33 poses, robot 1 private, one relative-pose factor between robots 0 and 2."""
    return _unequal(True)


def no_ghost_case():
    """The same batch without the relative-pose factor: the lambda region has no workgroup."""
    return _unequal(False)


def padding_case():
    """32 poses = 192 columns = three full tiles (the pad region writes the right-hand-side row only) next to 33 poses (padding)."""
    J = jg.sizes_case([32, 33])
    return J, {"pad_cols": [0, NB - (6 * 33) % NB], "slots": [6, 6], "n_ghost": [0, 0]}


def separator_delta_case():
    """Four robots; separator landmarks of all three classes seen by two robots and by all of them."""
    J = jg.shared_mix_case(4)
    return J, {"slot_classes": True}


CASES = [("unequal", unequal_case), ("no_ghost", no_ghost_case), ("padding", padding_case), ("separator_deltas", separator_delta_case)]


def check_claims(J, ref, claims, run=None):
    """Assert that J reaches what its builder claims; run: the GPU run, for the claims about the shards' layout."""
    shared = shared_by_robot(J)
    if "slots" in claims:
        assert [len(x) for x in shared] == claims["slots"], [len(x) for x in shared]
    if "n_ghost" in claims:
        assert ghosts_by_robot(J) == claims["n_ghost"]
        if run is not None:
            assert getattr(run.drv, "lam_dim", 0) == 6 * len(J.relmeas)
    if "most_landmarks" in claims:
        lm = landmarks_by_robot(J)
        a, b = claims["most_landmarks"], claims["as_many_slots"]
        assert lm[a] == max(lm) and lm[a] >= 5 * lm[b] and len(shared[b]) >= len(shared[a]) > 0, (lm, [len(x) for x in shared])
    if "empty_border" in claims:
        for r, empty in enumerate(claims["empty_border"]):
            assert (len(shared[r]) == 0) == empty and (not empty or (J.sizes[r] < 64 and ghosts_by_robot(J)[r] == 0))
            if run is not None:
                assert (len(run.shards[r].graph.border_profile()) == 0) == empty
    if "pad_cols" in claims:
        assert [(-6 * P) % NB for P in J.sizes] == claims["pad_cols"] and claims["pad_cols"][0] == 0 < claims["pad_cols"][1]
    if "cut" in claims:
        for r, cut in enumerate(claims["cut"]):
            assert not cut or J.sizes[r] >= 64          # (upload_new cuts no band under 64 poses)
            if run is not None:
                assert (run.shards[r].graph.segment_table() is not None) == cut, r
    if claims.get("slot_classes"):
        for r in range(J.R):
            assert {cls for cls, _ in shared[r]} == {0, 1, 2}, r
        seen = [len({a for a, _ in obs}) for _, _, _, obs in J.lms]
        assert 2 in seen and J.R in seen
    assert ref is None or ref.n > 0
