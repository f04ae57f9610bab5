"""The test of the border tests (border_cases.py), without a device: the long-double reference and its a-priori bound must catch the
smallest mistakes a border kernel can make — one k-step of four columns left out of one tile, one chunk boundary off by one block column,
one mask bit decoded wrongly — on every case, must pass an honest float64 evaluation in another order, and every case must really hold
the edge it is named after (its empty chunk, its inactive segment, its pair without a common segment, its mask bit at 32 or above)."""
import numpy as np
import pytest

import border_cases as bc
from border_cases import NB, INACTIVE


def _launch(name):
    systems, kw, ev = bc.product_case(name)
    return systems[0], kw.get("ks", 1), kw.get("jb_end"), ev


def _summed_tiles(d, jb_end=None):
    return [(ib, jb) for jb in range(d["nbr"] if jb_end is None else jb_end) for ib in range(jb, d["nbr"] + 1) if bc.pair_ranges(d, ib, jb)]


@pytest.fixture(scope="module")
def refs():
    done = {}

    def get(name):
        if name not in done:
            d, ks, jb_end, _ = _launch(name)
            done[name] = bc.product_reference(d, ks=ks, jb_end=jb_end)
        return done[name]
    return get


@pytest.mark.parametrize("name", bc.PRODUCT_CASES)
def test_a_dropped_k_step_breaks_the_bound(refs, name):
    d, ks, jb_end, _ = _launch(name)
    ref, bound, _ = refs(name)
    where = bc.lower_tile_mask(d, jb_end)
    assert bc.worst_ratio(ref.astype(np.float64), ref, bound, where) < 1.0
    rng = np.random.default_rng(7)
    tiles = _summed_tiles(d, jb_end)
    ib, jb = tiles[rng.integers(len(tiles))]
    steps = 16 * sum(hi - lo for lo, hi in bc.pair_ranges(d, ib, jb))
    wrong, _, _ = bc.product_reference(d, ks=ks, jb_end=jb_end, drop=(ib, jb, int(rng.integers(steps))))
    ratio = bc.worst_ratio(wrong.astype(np.float64), ref, bound, where)
    print(f"{name}: tile ({ib}, {jb}) without one k-step: worst |err| / bound {ratio:.3e}")
    assert ratio > 1e3


@pytest.mark.parametrize("name", [c for c in bc.PRODUCT_CASES if c.startswith(("split", "segtab"))])
def test_a_shifted_boundary_breaks_the_bound(refs, name):
    d, ks, jb_end, _ = _launch(name)
    ref, bound, _ = refs(name)
    # a tile whose sum has more than one piece (chunk or segment)
    pick = None
    for ib, jb in _summed_tiles(d, jb_end):
        pieces = []
        for lo, hi in bc.pair_ranges(d, ib, jb):
            pieces += [c for c in bc.chunk_ranges(d["T"], lo, ks) if c is not None] if ks > 1 else [(lo, hi)]
        if len(pieces) > 1:
            pick = (ib, jb)
    assert pick is not None
    wrong, _, _ = bc.product_reference(d, ks=ks, jb_end=jb_end, shift=pick)
    ratio = bc.worst_ratio(wrong.astype(np.float64), ref, bound, bc.lower_tile_mask(d, jb_end))
    print(f"{name}: tile {pick} with one block column summed twice: worst |err| / bound {ratio:.3e}")
    assert ratio > 1e3


@pytest.mark.parametrize("name", ["sum:5:2", "segtab", "split:9:8", "bfirst_src"])
def test_float64_in_another_order_is_inside_the_bound(refs, name):
    """The bound is no tighter than float64 allows: the same sums in plain float64, column blocks DESCENDING, pass it."""
    d, ks, jb_end, _ = _launch(name)
    ref, bound, _ = refs(name)
    cols, ldb = d["bord_cols"], d["ldb"]
    got = d["bord"].reshape(cols, ldb).copy()
    cin = (d["bord_src"] if d.get("bord_src") is not None else d["bord"]).reshape(cols, ldb)
    for ib, jb in [(ib, jb) for jb in range(d["nbr"]) for ib in range(jb, d["nbr"] + 1)]:
        rg = bc.pair_ranges(d, ib, jb)
        if not rg and d.get("bord_src") is None:
            continue
        acc = cin[jb * NB:(jb + 1) * NB, ib * NB:(ib + 1) * NB].T.copy()
        for lo, hi in reversed(rg):
            for c in reversed(range(lo, hi)):
                acc -= bc.wt_tile(d, ib, c, c + 1).astype(np.float64) @ bc.wt_tile(d, jb, c, c + 1).astype(np.float64).T
        got[jb * NB:(jb + 1) * NB, ib * NB:(ib + 1) * NB] = acc.T
    ratio = bc.worst_ratio(got, ref, bound, bc.lower_tile_mask(d, jb_end))
    print(f"{name}: float64, descending: worst |err| / bound {ratio:.3e}")
    assert 0 < ratio < 1.0


@pytest.mark.parametrize("name", bc.PRODUCT_CASES)
def test_the_product_cases_hold_their_edges(name):
    d, ks, jb_end, ev = _launch(name)
    T, nbr = d["T"], d["nbr"]
    B0 = d["b0"] or T
    S = d["S"].reshape(T * NB, d["ld"])
    assert np.all(S[:, (B0 + nbr) * NB + 1:(B0 + nbr + 1) * NB] == 0.0), "rows 1 .. 63 of the right-hand-side row tile"
    assert np.all(S[:, T * NB:B0 * NB] >= 1e30) and np.all(S[:, (B0 + nbr + 1) * NB:] >= 1e30)
    assert d["ld"] % 2 == 0 and d["ldb"] % 2 == 0 and d["ld"] >= (B0 + nbr + 1) * NB
    if d.get("bfirst") is not None:
        assert list(d["bfirst"][:nbr]) == sorted(d["bfirst"][:nbr])
    if "empty_sum" in ev:
        assert bc.pair_ranges(d, *ev["empty_sum"]) == [] and T in d["bfirst"]
    if "inactive" in ev:          # (tile row, segment)
        row, seg = ev["inactive"]
        assert bc.parse_segtab(d["segtab"], nbr)[1][seg][row] == INACTIVE
    if "disjoint" in ev:
        assert bc.pair_ranges(d, *ev["disjoint"]) == []
        assert bc.pair_ranges(d, ev["disjoint"][0], ev["disjoint"][0]) and bc.pair_ranges(d, ev["disjoint"][1], ev["disjoint"][1])
    if name.startswith("segtab"):
        ends, firsts, masks = bc.parse_segtab(d["segtab"], nbr)
        assert [e - s for s, e in zip([0] + ends[:-1], ends)] == [3, 1, 3] and T == 7
        assert [f[nbr] for f in firsts] == [0] + ends[:-1], "the right-hand side rides from each segment's first column"
        assert len(bc.pair_ranges(d, 0, 0)) == 3 and (3, 4) in bc.pair_ranges(d, 0, 0), "no sum crosses the one-column segment"
        assert masks is not None and len(masks) == T
    if "empty_chunk" in ev:
        assert any(None in bc.chunk_ranges(T, lo, ks) for ib, jb in _summed_tiles(d) for lo, _ in bc.pair_ranges(d, ib, jb))
    elif ks > 1 and d.get("bfirst") is None:
        assert None not in bc.chunk_ranges(T, 0, ks)
    if "c0_positive" in ev:
        (lo, hi), = bc.pair_ranges(d, *ev["c0_positive"])
        own, zero = bc.chunk_ranges(T, lo, ks), bc.chunk_ranges(T, 0, ks)
        assert lo > 0 and own[1] is not None and own[1] != zero[1], "a reduction that cuts from column 0 would add another chunk"
    if jb_end is not None:
        assert 0 < jb_end < nbr


@pytest.mark.parametrize("T,c0,ks", [(T, c0, ks) for T in (1, 2, 4, 5, 6, 9) for c0 in range(0, T + 1) for ks in (1, 2, 3, 4, 8)])
def test_chunk_model(T, c0, ks):
    """The kernel's own arithmetic (len, c0 + q len, min(T, ..)) restated in numpy against chunk_ranges: the chunks tile [c0, T) in order,
    and the rule by which the reduction skips a chunk (c0 + q len >= T) names exactly the empty ones."""
    q = np.arange(ks)
    length = (T - c0 + ks - 1) // ks
    lo = c0 + q * length
    hi = np.minimum(T, lo + length)
    got = bc.chunk_ranges(T, c0, ks)
    for k in range(ks):
        assert (got[k] is None) == bool(lo[k] >= hi[k]) == bool(lo[k] >= T or length == 0)
        if got[k] is not None:
            assert got[k] == (int(lo[k]), int(hi[k]))
    cover = [c for r in got if r is not None for c in range(*r)]
    assert cover == list(range(c0, T))


def test_fused_and_eight_systems():
    a, b = bc.fused_systems()
    assert (a["T"], b["T"]) == (4, 6) and a["nbr"] == b["nbr"] == 3 and a["bfirst"] is None and b["bfirst"] is None
    assert bc.chunk_ranges(6, 0, 3) == [(0, 2), (2, 4), (4, 6)] and bc.chunk_ranges(4, 0, 2) == [(0, 2), (2, 4)]
    eight = bc.eight_systems()
    assert len(eight) == 8 and len({(d["T"], d["nbr"]) for d in eight}) == 8
    codes = bc.job_table(eight)
    assert len(codes) == len(set(codes)) == sum((d["nbr"] + 1) * d["nbr"] // 2 + d["nbr"] for d in eight)
    assert max(c >> 20 for c in codes) == 7


@pytest.mark.parametrize("name", bc.APPLY_CASES)
def test_the_apply_cases(name):
    systems = bc.apply_case(name)
    for d in systems:
        ref, bound = bc.apply_reference(d)
        assert np.all(np.abs(ref.astype(np.float64) - ref) <= bound)
        assert np.all(d["x_loc"] != 0.0)
        # one product left out of one column breaks the bound
        T, nbr = d["T"], d["nbr"]
        masks = bc.parse_segtab(d["segtab"], nbr)[2] if d.get("segtab") is not None else None
        col = T * NB - 3
        t = next(t for t in range(nbr) if masks is None or (masks[col // NB] >> t) & 1)
        S = d["S"].reshape(T * NB, d["ld"])
        wrong = ref.copy()
        wrong[col] += S[col, (d["b0"] or T) * NB + t * NB + 5] * d["x_loc"][t * NB + 5]
        assert abs(float(wrong[col] - ref[col])) > 1e3 * bound[col]
    if name == "three":
        assert [d["T"] for d in systems] == [1, 3, 2] and {d["nbr"] for d in systems} == {1, 3}
    if name == "view":
        assert systems[0]["b0"] > systems[0]["T"]
    if name.startswith("masks"):
        d = systems[0]
        masks = bc.parse_segtab(d["segtab"], d["nbr"])[2]
        assert d["nbr"] == 34 and any(m >> 32 for m in masks) and any((m >> 32) & 1 for m in masks) and any((m >> 33) & 1 for m in masks)
        assert all(m & 0xffffffff for m in masks) and any(m != masks[0] for m in masks)
        S = d["S"].reshape(d["T"] * NB, d["ld"])
        W = S[:, d["T"] * NB:(d["T"] + d["nbr"]) * NB]
        outside = np.ones_like(W, bool)
        for c, m in enumerate(masks):
            for t in range(d["nbr"]):
                if (m >> t) & 1:
                    outside[c * NB:(c + 1) * NB, t * NB:(t + 1) * NB] = False
        assert outside.any() and np.all(W[outside] == (1e30 if name == "masks_decode" else 0.0)) and np.all(W[~outside] != 0.0)
        # decoding one bit wrongly (a tile row outside the mask taken in) breaks the bound of the sentinel case
        if name == "masks_decode":
            ref, bound = bc.apply_reference(d)
            c = 0
            t = next(t for t in range(d["nbr"]) if not (masks[c] >> t) & 1)
            extra = W[:NB, t * NB:(t + 1) * NB].astype(bc.LD) @ d["x_loc"][t * NB:(t + 1) * NB].astype(bc.LD)
            assert np.all(np.abs(extra.astype(np.float64)) > 1e3 * bound[:NB])
    if name == "no_masks":
        d = systems[0]
        assert d["nbr"] == 65 and bc.parse_segtab(d["segtab"], 65)[2] is None
        assert d["segtab"][1 + 2 + 2 * 66] == 0, "msk[0] == 0: the full walk"
