"""The launch shapes of the batched Cholesky step launches, decided on the host from the CU count (launch_chol_batch, chol_kernels.hip):
a_split = two type-A workgroups per tile, a_joins = the type-A workgroups drain the queue after their chain.  slide_debug_chol_plan runs
the planning code of the real launches without a device, for an assumed CU count; test_gpu_chol_batch.py then checks that the device
takes exactly these shapes and factors correctly in each.  The expected traces were worked out by hand from plan_step / plan_pair and
the two conditions (a_split: k > 0 and (2 nA + nB) * 100 <= n_cu * share; a_joins: nB > max(n_cu - nAw, 8)) for the mixed batch of
chol_cases.MIXED; the host entry agreed with every one of them."""
import itertools

import numpy as np
import pytest

import chol_cases as cc
from slide_slam_amd import api


@pytest.fixture(scope="module")
def mixed():
    return [cc.tables(cc.CASES[c], c) for c in cc.MIXED]


def _shapes(trace):
    return [(int(r[1]), int(r[2])) for r in trace]


def test_mixed_batch_is_the_documented_one():
    assert cc.MIXED == ["segment", "one_column", "leaf", "segment_odd", "second_level_T5", "segment_decoupled", "two_columns", "second_level_T4"]
    assert sorted(cc.MIXED) == sorted(cc.CASES)


@pytest.mark.parametrize("cus,share,want", [
    (64, 100, [(0, 0)] + [(0, 1)] * 4 + [(0, 0)] * 3 + [(1, 0)] * 4),
    (256, 100, [(0, 0)] + [(1, 0)] * 11),
    (256, 25, [(0, 0)] * 8 + [(1, 0)] * 4),
    (8, 100, [(0, 1) if k in (1, 2, 3, 4, 5, 6, 7, 8, 10) else (0, 0) for k in range(12)]),
    (8, 25, [(0, 1) if k in (1, 2, 3, 4, 5, 6, 7, 8, 10) else (0, 0) for k in range(12)]),
    (8, 0, [(0, 1) if k in (1, 2, 3, 4, 5, 6, 7, 8, 10) else (0, 0) for k in range(12)]),
])
def test_step_kernel_trace(mixed, cus, share, want):
    tr = api.debug_chol_plan(mixed, method=0, cu_share=share, assumed_cus=cus)
    assert tr[:, 0].tolist() == list(range(12))             # one launch per block column of the longest system
    assert _shapes(tr) == want


def test_64_cus_cover_every_reachable_shape(mixed):
    tr = api.debug_chol_plan(mixed, method=0, cu_share=100, assumed_cus=64)
    assert set(_shapes(tr)) == {(0, 0), (0, 1), (1, 0)}


@pytest.mark.parametrize("cus,want", [(64, [0, 1, 1, 1, 0, 0]), (256, [0] * 6)])
def test_pair_kernel_trace(mixed, cus, want):
    tr = api.debug_chol_plan(mixed, method=2, cu_share=100, assumed_cus=cus)
    assert tr[:, 0].tolist() == [0, 2, 4, 6, 8, 10]
    assert tr[:, 1].tolist() == [0] * 6                     # (the pair kernel has no a_split)
    assert tr[:, 2].tolist() == want


def test_split_and_join_exclude_each_other(mixed):
    """a_split needs 2 nA + nB <= n_cu * share / 100 <= n_cu, a_joins needs nB > max(n_cu - 2 nA, 8) >= n_cu - 2 nA."""
    seen = set()
    for cus, share, method in itertools.product((8, 32, 64, 104, 256), (0, 25, 33, 50, 100), (0, 2)):
        for batch in (mixed, mixed[:1] * 32, mixed[2:3], mixed[4:5] * 8):
            sh = _shapes(api.debug_chol_plan(batch, method=method, cu_share=share, assumed_cus=cus))
            assert (1, 1) not in sh, (cus, share, method)
            seen |= set(sh)
    assert seen == {(0, 0), (0, 1), (1, 0)}


def test_trace_is_invariant_under_permuting_the_batch(mixed):
    rng = np.random.default_rng(7)
    for cus, share, method in ((64, 100, 0), (256, 25, 0), (8, 100, 0), (64, 100, 2)):
        want = api.debug_chol_plan(mixed, method=method, cu_share=share, assumed_cus=cus)
        for perm in ([7, 6, 5, 4, 3, 2, 1, 0], *(rng.permutation(8).tolist() for _ in range(3))):
            got = api.debug_chol_plan([mixed[i] for i in perm], method=method, cu_share=share, assumed_cus=cus)
            assert np.array_equal(got, want), (cus, share, method, perm)


def test_short_systems_have_no_work_in_late_launches(mixed):
    """The totals of a launch are sums over the systems: a launch k is that of the systems with T > k alone (nAw = nB = 0 from the rest)."""
    for cus, share in ((64, 100), (256, 100), (8, 100)):
        full = api.debug_chol_plan(mixed, method=0, cu_share=share, assumed_cus=cus)
        for k in range(12):
            alive = [s for s in mixed if s["T"] > k]
            assert 0 < len(alive) < len(mixed) or k == 0
            sub = api.debug_chol_plan(alive, method=0, cu_share=share, assumed_cus=cus)
            assert np.array_equal(sub[k], full[k]), (cus, share, k)
    # and a system alone, then beside a longer one: the launches past its end are the longer one's own
    short, long_ = mixed[6], mixed[0]                        # two_columns (T = 2), segment (T = 12)
    both = api.debug_chol_plan([short, long_], assumed_cus=64)
    alone = api.debug_chol_plan([long_], assumed_cus=64)
    assert np.array_equal(both[2:, 3:], alone[2:, 3:]) and not np.array_equal(both[:2, 3:], alone[:2, 3:])
    pair_both = api.debug_chol_plan([short, long_], method=2, assumed_cus=64)
    pair_alone = api.debug_chol_plan([long_], method=2, assumed_cus=64)
    assert np.array_equal(pair_both[1:, 3:], pair_alone[1:, 3:]) and not np.array_equal(pair_both[:1, 3:], pair_alone[:1, 3:])


def test_32_band_segments_take_the_joining_shape():
    """The batch size CHOL_STEP_BATCH_MAX is documented for: 32 band segments in one launch sequence run (a_split, a_joins) = (0, 1) on a
    256-CU device while their trailing passes last — the shape n_copies <= 8 of one system never reaches at 256 CUs."""
    seg = cc.tables(cc.CASES["segment"], "segment")
    tr = api.debug_chol_plan([seg] * 32, method=0, cu_share=100, assumed_cus=256)
    assert (0, 1) in _shapes(tr) and (1, 1) not in _shapes(tr)
    assert tr[:, 3].max() > 256


def _exact_output(d):
    """What a factorisation without rounding would hand back for build()'s system d, in the layout check_system reads."""
    T, nbr, n = d["T"], d["nbr"], d["T"] * cc.NB
    NB, B0 = cc.NB, (d["b0"] or d["T"]) * cc.NB
    pf = d["prof"] if d["prof"] is not None else [T - 1] * T
    So = d["S"].copy().reshape(n, d["ld"])
    for c in range(T):
        for r in range(c + 1, pf[c] + 1):
            So[c * NB:(c + 1) * NB, r * NB:(r + 1) * NB] = d["L0"][r * NB:(r + 1) * NB, c * NB:(c + 1) * NB].T
    So[:, B0:B0 + nbr * NB] = d["W0"].T
    So[:, B0 + nbr * NB] = d["y0"]
    Ld, Wi = np.zeros((T, NB, NB)), np.zeros((T, 4, 16, 16))
    for k in range(T):
        D = d["L0"][k * NB:(k + 1) * NB, k * NB:(k + 1) * NB]
        Ld[k] = D.T
        for b in range(4):
            Wi[k, b] = np.linalg.inv(D[16 * b:16 * b + 16, 16 * b:16 * b + 16]).T
    return dict(S=So.ravel(), Ld=Ld.ravel(), Winv=Wi.ravel(), status=np.zeros(8, np.int32))


@pytest.mark.parametrize("case", ["leaf", "segment_decoupled"])
def test_checker_accepts_the_known_factor_and_rejects_a_wrong_one(case):
    """check_system is what every kernel-level Cholesky test rests on: the exact factor passes, and one wrong element anywhere it looks
    (a band tile, a border row in its physical place, the right-hand side, Ld, Winv, the rows it must leave alone, the zeros outside the
    profile, the status word) does not."""
    d = cc.build(cc.CASES[case], case)
    NB, T, n, ld = cc.NB, d["T"], d["T"] * cc.NB, d["ld"]
    B0 = (d["b0"] or T) * NB
    good = _exact_output(d)
    cc.check_system(d, good)

    def wrong(key, index, value=None, add=1e-6):
        bad = {k: v.copy() for k, v in good.items()}
        flat = bad[key]
        flat[index] = value if value is not None else flat[index] + add
        with pytest.raises(AssertionError):
            cc.check_system(d, bad)
    pf = d["prof"] if d["prof"] is not None else [T - 1] * T
    wrong("S", (0 * NB + 5) * ld + 1 * NB + 7)                              # band tile (1, 0)
    wrong("S", ((T - 2) * NB + 63) * ld + (T - 1) * NB + 63)                # the last band tile
    live = int(np.flatnonzero(np.abs(d["W0"]).sum(axis=1))[-1])             # a border row that is not all zero
    wrong("S", (n - 1) * ld + B0 + live)
    wrong("S", 3 * ld + B0 + d["nbr"] * NB)                                 # right-hand side
    wrong("Ld", (1 * NB + 2) * NB + 40)                                     # Ld[1][col 2][row 40]: sub-tile (2, 0)
    wrong("Winv", (T - 1) * 1024 + 3 * 256 + 17)
    wrong("status", 1, value=1)
    if d["b0"] > T:
        wrong("S", 9 * ld + T * NB + 1, value=0.0)                          # between the band and the view's border
    if pf[0] < T - 1:
        wrong("S", 2 * ld + (pf[0] + 1) * NB + 3, value=1e-300)             # outside the profile


def test_plan_refusals(mixed):
    for kw in (dict(assumed_cus=0), dict(assumed_cus=-1), dict(cu_share=101), dict(cu_share=-1), dict(method=1)):
        with pytest.raises(api.SlideError, match="SLIDE_ERR_INVALID"):
            api.debug_chol_plan(mixed, **{"assumed_cus": 64, **kw})
    with pytest.raises(api.SlideError, match="SLIDE_ERR_INVALID"):
        api.debug_chol_plan([], assumed_cus=64)
    with pytest.raises(api.SlideError, match="SLIDE_ERR_INVALID"):
        api.debug_chol_plan(mixed[:1] * 33, assumed_cus=64)
