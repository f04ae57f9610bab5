"""The batched Cholesky step launches (k_chol_step_batched, opt-in k_chol_pair_batched) on MIXED batches, in every launch shape.

test_gpu_chol_bordered.py factors n_copies of ONE system per launch sequence: every entry of the kernel's per-system tables is then equal,
so a workgroup that reads system r's TvB with system r + 1's nbB, or decodes an item against the wrong b_base, goes unnoticed; and the
launch shape (a_split: two type-A workgroups per tile; a_joins: the type-A workgroups drain the queue after their chain) follows from
the device's CU count alone.  Here the systems of a launch sequence differ in T, profile, border order, first columns, b0 and kofs
(chol_cases.MIXED: shorter systems have no work in late launches), the launches are planned for an assumed CU count and a CU share so
that every reachable shape is taken (the device's trace must equal the host-only plan, test_chol_plan.py), and the packed f32 factor copy
L32 the joint solve's preconditioner streams is compared with the f64 factor.  Bounds: chol_cases.check_system, the ones of
test_gpu_chol_bordered.py — the systems are built from a known factor; new are the code paths and the bit-for-bit conditions."""
import itertools

import numpy as np
import pytest

import chol_cases as cc
from chol_cases import CASES, MIXED, NB

pytestmark = pytest.mark.gpu

SETTINGS = [(0, 100), (64, 100), (64, 0), (8, 100), (0, 25)]      # (assumed_cus, cu_share)
PREFILL = 0x7fc0dead


@pytest.fixture(scope="module")
def mixed():
    return [cc.build(CASES[c], c) for c in MIXED]


@pytest.fixture(scope="module")
def runs(gpu, mixed):
    """The mixed batch through debug_chol_batch, once per (method, assumed_cus, cu_share): shared by the tests below, never modified."""
    done = {}

    def run(method, cus, share):
        if (method, cus, share) not in done:
            done[method, cus, share] = gpu.api.debug_chol_batch(mixed, method=method, cu_share=share, assumed_cus=cus)
            assert gpu.pair_timeouts() == 0
        return done[method, cus, share]
    return run


def _shapes(trace):
    return [(int(r[1]), int(r[2])) for r in trace]


def _check_all(systems, out):
    for i, (d, o) in enumerate(zip(systems, out["systems"])):
        try:
            cc.check_system(d, o)
        except AssertionError as e:
            raise AssertionError(f"system {i} (T {d['T']}, nbr {d['nbr']}, b0 {d['b0']}, kofs {d['kofs']}): {e}") from e


def _same_bits(a, b):
    return all(np.array_equal(a[key].view(np.uint64), b[key].view(np.uint64)) for key in ("S", "Ld", "Winv"))


@pytest.mark.parametrize("cus,share", SETTINGS)
@pytest.mark.parametrize("method", [0, 2])
def test_mixed_batch_in_every_shape(gpu, mixed, runs, method, cus, share):
    out = runs(method, cus, share)
    n_cu = out["n_cu"]
    assert n_cu == cus or (cus == 0 and n_cu > 0)
    plan = gpu.api.debug_chol_plan(mixed, method=method, cu_share=share, assumed_cus=n_cu)
    print(f"method {method}, assumed_cus {cus} (planned for {n_cu}), cu_share {share}: (k, a_split, a_joins, nAw, nB) = {[tuple(r) for r in out['trace'].tolist()]}")
    assert np.array_equal(out["trace"], plan), "the device took other launch shapes than the plan"
    assert len(out["trace"]) == (12 if method == 0 else 6)
    if cus == 64 and method == 0:       # a run that silently tested one shape fails
        want = {(0, 0), (0, 1), (1, 0)} if share == 100 else {(0, 0), (0, 1)}
        assert set(_shapes(out["trace"])) == want
    if cus == 64 and method == 2:
        assert out["trace"][:, 2].tolist() == [0, 1, 1, 1, 0, 0]
    if cus == 8:
        assert not out["trace"][:, 1].any() and out["trace"][:, 2].sum() == (9 if method == 0 else 3)
    _check_all(mixed, out)
    assert gpu.pair_timeouts() == 0


@pytest.mark.parametrize("cus,share", [(64, 100), (0, 100)])
@pytest.mark.parametrize("method", [0, 2])
def test_a_system_does_not_depend_on_its_place_in_the_batch(gpu, mixed, runs, method, cus, share):
    """The totals that decide the shape are sums over the systems: the reversed batch takes the same launches, with other a_base / b_base
    for every system — each system's S, Ld and Winv must come out bit for bit the same."""
    fwd = runs(method, cus, share)
    rev = gpu.api.debug_chol_batch(mixed[::-1], method=method, cu_share=share, assumed_cus=cus)
    assert gpu.pair_timeouts() == 0
    assert np.array_equal(fwd["trace"], rev["trace"])
    _check_all(mixed[::-1], rev)
    for i, (a, b) in enumerate(zip(fwd["systems"], rev["systems"][::-1])):
        assert _same_bits(a, b), f"system {i} ({MIXED[i]}) differs between the batch and the reversed batch"


@pytest.mark.parametrize("method", [0, 2])
def test_a_system_does_not_depend_on_its_neighbours(gpu, mixed, runs, method):
    """one_column and two_columns replaced by two more band segments (other seeds): every a_base / b_base behind them moves, the launches
    change (the shapes may, too: a_split follows the totals) — the systems that stayed are still the known factor.  Whether they also stayed
    bit-equal is printed, not asserted."""
    other = list(mixed)
    other[MIXED.index("one_column")] = cc.build(CASES["segment"], "segment, a second one")
    other[MIXED.index("two_columns")] = cc.build(CASES["segment"], "segment, a third one")
    assert other[1]["bfirst"] != mixed[0]["bfirst"] and other[6]["ord"] != other[1]["ord"]
    out = gpu.api.debug_chol_batch(other, method=method, cu_share=100, assumed_cus=64)
    assert gpu.pair_timeouts() == 0
    assert np.array_equal(out["trace"], gpu.api.debug_chol_plan(other, method=method, cu_share=100, assumed_cus=64))
    _check_all(other, out)
    ref = runs(method, 64, 100)
    same = [_same_bits(a, b) for i, (a, b) in enumerate(zip(ref["systems"], out["systems"])) if i not in (1, 6)]
    print(f"method {method}: unreplaced systems bit-equal beside other neighbours: {same}; shapes {_shapes(ref['trace'])} -> {_shapes(out['trace'])}")


@pytest.mark.parametrize("cus", [0, 8])
@pytest.mark.parametrize("method", [0, 2])
def test_same_kind_different_parameters(gpu, method, cus):
    """Four band segments of one size (T = 12, nbr = 9, profile three tiles wide) that differ in what the kernel reads per system: kofs,
    b0, the first columns and order of the border rows, and the values — the mix-up that identical copies hide."""
    systems = [cc.build(dict(T=12, nbr=9, band=3, first="sorted", b0=b0, kofs=kofs), f"same kind {i}")
               for i, (kofs, b0) in enumerate(zip((21, 0, 5, 40), (16, 12, 13, 20)))]
    assert len({tuple(s["bfirst"]) for s in systems}) == 4 and len({tuple(s["ord"]) for s in systems}) == 4
    out = gpu.api.debug_chol_batch(systems, method=method, cu_share=100, assumed_cus=cus)
    assert gpu.pair_timeouts() == 0
    assert np.array_equal(out["trace"], gpu.api.debug_chol_plan(systems, method=method, cu_share=100, assumed_cus=out["n_cu"]))
    _check_all(systems, out)


@pytest.mark.parametrize("method", [0, 2])
def test_across_shapes(mixed, runs, method):
    """The same batch in the five settings: each passes the checker (asserted), and the largest difference of any band tile, border row or
    right-hand side between any two settings is printed.  Measured on an MI355X (256 CUs), step and pair kernels alike: all five settings
    are BIT-EQUAL in S, Ld and Winv of every system (largest difference 0.0) — a_split divides a tile's rows between two workgroups and
    a_joins only changes which workgroup draws an item, neither touches the order of a sum.  A change that alters a summation order with
    the launch shape gives that up."""
    worst = dict(band=0.0, border=0.0, rhs=0.0)
    bits = True
    for (ca, sa), (cb, sb) in itertools.combinations(SETTINGS, 2):
        a, b = runs(method, ca, sa), runs(method, cb, sb)
        for d, x, y in zip(mixed, a["systems"], b["systems"]):
            n, B0 = d["T"] * NB, (d["b0"] or d["T"]) * NB
            X, Y = x["S"].reshape(n, d["ld"]), y["S"].reshape(n, d["ld"])
            E = np.abs(X - Y)
            worst["band"] = max(worst["band"], float(E[:, :n].max()))
            if d["nbr"]:
                worst["border"] = max(worst["border"], float(E[:, B0:B0 + d["nbr"] * NB].max()))
            worst["rhs"] = max(worst["rhs"], float(E[:, B0 + d["nbr"] * NB].max()))
            bits = bits and _same_bits(x, y)
    print(f"method {method}: largest difference between any two of {SETTINGS}: {worst}; S, Ld, Winv bit-equal throughout: {bits}")
    for cus, share in SETTINGS:
        _check_all(mixed, runs(method, cus, share))


@pytest.fixture(scope="module")
def l32_batch():
    names = ["second_level_T4", "second_level_T5", "segment_decoupled", "one_column", "two_columns"]
    systems = [cc.build(CASES[c], c) for c in names] + [cc.build(dict(T=6, nbr=0), "dense_T6")]
    assert all(s["b0"] == 0 for s in systems)
    return systems


def _check_l32(d, o):
    """Every packed tile (j, c), c < j <= prof[c], is np.float32 of the f64 tile in S; every other float still holds the prefill."""
    T, n = d["T"], d["T"] * NB
    pf = d["prof"] if d["prof"] is not None else [T - 1] * T
    L32 = o["L32"]
    assert L32.size == T * (T - 1) // 2 * 4096 + 4
    So = o["S"].reshape(n, d["ld"])
    written = np.zeros(L32.size, bool)
    for c in range(T):
        for j in range(c + 1, pf[c] + 1):
            off = 4096 * (c * (T - 1) - c * (c - 1) // 2 + j - c - 1)
            want = So[c * NB:(c + 1) * NB, j * NB:(j + 1) * NB].astype(np.float32).ravel()      # [col][row]: element (row, col) at col * 64 + row
            got = L32[off:off + 4096]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("L32 tile", j, c, float(np.abs(got - want).max()))
            written[off:off + 4096] = True
    assert np.all(L32.view(np.uint32)[~written] == PREFILL), "a float of L32 outside the profile's tiles was written"


def test_l32_is_the_f32_of_the_factor(gpu, l32_batch):
    """The type-A workgroups write the packed f32 copy beside the panel (panel_rows); under a_split two workgroups each write half of a
    packed tile.  (0, 100): a_split = 1 after column 0; (8, 100): a_split = 0 in every column that has band tiles, a_joins = 1 while the
    trailing passes last.  Both stores take the same register value, so the copy is compared bit for bit with np.float32 of the f64 factor
    read back from S — and on an MI355X it is exact, in both shapes."""
    outs = {}
    for cus in (0, 8):
        out = outs[cus] = gpu.api.debug_chol_batch(l32_batch, method=0, cu_share=100, assumed_cus=cus, want_l32=True)
        assert np.array_equal(out["trace"], gpu.api.debug_chol_plan(l32_batch, method=0, cu_share=100, assumed_cus=out["n_cu"]))
        print(f"L32, assumed_cus {cus} (planned for {out['n_cu']}): {[tuple(r) for r in out['trace'].tolist()]}")
        _check_all(l32_batch, out)
        for d, o in zip(l32_batch, out["systems"]):
            _check_l32(d, o)
    assert outs[0]["trace"][1:, 1].all(), "the run on the device's own CU count was to split every column after the first"
    # at 8 CUs no column with off-diagonal band tiles is split (the last launch, column 7 of segment_decoupled alone, is: 2 * 4 + 0 <= 8 —
    # it has border and right-hand-side rows only, nothing of L32), and the first trailing passes are drained by the type-A workgroups
    assert not outs[8]["trace"][:7, 1].any() and outs[8]["trace"][1:4, 2].all()
    # the pair kernel does not write L32: method 2 runs the step kernels, launch for launch
    pair = gpu.api.debug_chol_batch(l32_batch, method=2, cu_share=100, assumed_cus=0, want_l32=True)
    assert gpu.pair_timeouts() == 0
    assert np.array_equal(pair["trace"], outs[0]["trace"]) and len(pair["trace"]) == 8
    for a, b in zip(outs[0]["systems"], pair["systems"]):
        assert _same_bits(a, b) and np.array_equal(a["L32"].view(np.uint32), b["L32"].view(np.uint32))
    # and a system with b0 > 0 in such a batch gets no copy
    seg = cc.build(CASES["segment_odd"], "segment_odd")
    both = gpu.api.debug_chol_batch([l32_batch[1], seg], method=0, assumed_cus=8, want_l32=True)
    assert both["systems"][1]["L32"] is None
    _check_all([l32_batch[1], seg], both)
    _check_l32(l32_batch[1], both["systems"][0])


def test_refusals(gpu, mixed, runs):
    n_cu = runs(0, 0, 100)["n_cu"]
    small = cc.build(CASES["one_column"], "one_column")
    short = dict(mixed[2], ld=mixed[2]["ld"] - NB)
    short["S"] = np.zeros(short["ld"] * short["T"] * NB)
    refused = [
        ("more CUs than the device has", dict(systems=mixed, assumed_cus=n_cu + 1)),
        ("negative CU count", dict(systems=mixed, assumed_cus=-1)),
        ("no system", dict(systems=[])),
        ("33 systems", dict(systems=[small] * 33)),
        ("cu_share 101", dict(systems=mixed, cu_share=101)),
        ("an ld too small for one system of the batch", dict(systems=[mixed[0], mixed[1], short, mixed[3]])),
    ]
    for what, kw in refused:
        with pytest.raises(gpu.api.SlideError, match="SLIDE_ERR_INVALID") as e:
            gpu.api.debug_chol_batch(**kw)
        assert e.value.code == -1 and e.value.n_launches == 0, what
    # the largest count that is allowed is the device's own: the same plan as 0
    out = gpu.api.debug_chol_batch(mixed, assumed_cus=n_cu)
    assert np.array_equal(out["trace"], runs(0, 0, 100)["trace"])
    assert gpu.pair_timeouts() == 0
