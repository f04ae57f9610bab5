"""Systems AFTER their steps for the border product's and the border apply's tests (test_gpu_border_product.py, test_gpu_border_apply.py,
test_border_cases_reference.py), as the exact joint passes hand them to launch_border_syrk / launch_border_syrk_jobs / launch_border_apply
(DESIGN.md 3 / 4): W^T in the border row tiles of S, y^T in row 0 of the tile behind them, the border block C in bord, the tables that
cut the sum (bfirst, the segments' table with its per-column masks).  Everything is drawn from an rng seeded by the case's name, entries
normal(0, 1) — also OUTSIDE the ranges the tables name, so that a kernel that sums a column block too many is wrong by O(1).  Rows 1 .. 63 of
the right-hand-side row tile of S are zero (the kernels' contract); what no kernel may touch holds a sentinel (values around 1e30).

The reference is numpy in np.longdouble (the operation the reference project delegates to GTSAM's elimination of the separator:
ISAM2Params::CHOLESKY, backend/sloam/src/factorgraph/graph.cpp:15):
    bord(ib, jb) = C(ib, jb) - sum over the pair's column blocks of W^T(ib, c) W^T(jb, c)^T        ib >= jb, ib = nbr: the right-hand side
    yv          -= W x                                                                             over the active tile rows
and the bound is the a-priori one of a dot product in ANY order, with or without fused multiply-add: per element
    |got - ref| <= (K + ks + 4) * 2^-53 * (|C| + sum |a| |b|)
K products (each product and each addition rounds once: K u to first order, u = 2^-53), ks - 1 further additions of the split-K
partials, the rest for the terms of second order (K u < 1e-12 here).  Nothing in it comes from a kernel's output."""
import zlib

import numpy as np

NB = 64
INACTIVE = 1 << 30
U = 2.0 ** -53
LD = np.longdouble


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _sentinel(rng, shape):
    return (1.0 + rng.uniform(0, 1, shape)) * 1e30


# ---- tables --------------------------------------------------------------------------------------------------------------------------

def make_segtab(T, nbr, ends, firsts):
    """HostGraph::seg_tab's flat layout: nseg, the segments' end columns, per segment the first column of every border tile row + the
    right-hand side (INACTIVE: zero in that segment), then the masks' head: T and per block column (low, high) of the 64-bit set of
    tile rows some segment works on there — or 0 when there are more than 64 tile rows."""
    nseg = len(ends)
    assert len(firsts) == nseg and all(len(f) == nbr + 1 for f in firsts)
    tab = [nseg] + list(ends)
    for f in firsts:
        tab += list(f)
    if nbr <= 64:
        tab.append(T)
        for m in column_masks(T, nbr, ends, firsts):
            tab += [m & 0xffffffff, m >> 32]
    else:
        tab.append(0)
    return tab


def column_masks(T, nbr, ends, firsts):
    """Per block column the set of border tile rows some segment works on there (bit t = tile row t)."""
    starts = [0] + list(ends[:-1])
    out = []
    for c in range(T):
        m = 0
        for q, f in enumerate(firsts):
            if starts[q] <= c < ends[q]:
                for t in range(nbr):
                    if f[t] <= c:
                        m |= 1 << t
        out.append(m)
    return out


def parse_segtab(tab, nbr):
    """(ends, firsts, masks or None) of a flat table."""
    nseg = tab[0]
    ends = list(tab[1:1 + nseg])
    firsts = [list(tab[1 + nseg + q * (nbr + 1):1 + nseg + (q + 1) * (nbr + 1)]) for q in range(nseg)]
    head = 1 + nseg + nseg * (nbr + 1)
    Tb = tab[head]
    masks = None
    if Tb > 0:
        masks = [(tab[head + 1 + 2 * c] & 0xffffffff) | ((tab[head + 2 + 2 * c] & 0xffffffff) << 32) for c in range(Tb)]
    return ends, firsts, masks


def pair_ranges(sysd, ib, jb):
    """The block-column ranges [lo, hi) the sum of tile (ib, jb) runs over, ascending."""
    T = sysd["T"]
    if sysd.get("segtab") is not None:
        ends, firsts, _ = parse_segtab(sysd["segtab"], sysd["nbr"])
        out = []
        for q, f in enumerate(firsts):
            lo = max(f[ib], f[jb])
            if lo < ends[q]:
                out.append((lo, ends[q]))
        return out
    c0 = 0
    if sysd.get("bfirst") is not None:
        c0 = max(sysd["bfirst"][ib], sysd["bfirst"][jb])
    return [(c0, T)] if c0 < T else []


def chunk_ranges(T, c0, ks):
    """Split K as launch_border_syrk cuts it: chunk q sums the block columns [c0 + q len, min(T, c0 + (q + 1) len)), len =
    ceil((T - c0) / ks); a chunk that starts at or behind T is empty (neither summed nor reduced)."""
    length = -((c0 - T) // ks) if T > c0 else 0
    out = []
    for q in range(ks):
        lo = c0 + q * length
        hi = min(T, lo + length)
        out.append((lo, hi) if lo < hi else None)
    return out


def job_table(systems, jb_end=None):
    """system << 20 | ib << 10 | jb for every lower tile and right-hand-side row tile (tile columns < jb_end only), system-major."""
    codes = []
    for r, d in enumerate(systems):
        for jb in range(d["nbr"] if jb_end is None else jb_end):
            for ib in range(jb, d["nbr"] + 1):
                codes.append(r << 20 | ib << 10 | jb)
    return codes


# ---- systems -------------------------------------------------------------------------------------------------------------------------

def make_system(rng, T, nbr, b0=0, bfirst=None, segtab=None, src=False, ld_pad=2, rows_beyond=NB + 2, cols_beyond=NB):
    """One system after its steps.  S[col, row] (flat: column-major ld x T*64), bord[col, row] (ldb x bord_cols).  Between a view's
    band and its border (b0 > T), behind the right-hand-side tile (ld_pad), above the diagonal of bord and beyond its border block:
    sentinels.  src: the tiles' values before the product live in bord_src, bord itself holds sentinels everywhere."""
    n, B0 = T * NB, b0 or T
    ld = (B0 + nbr + 1) * NB + ld_pad
    S = _sentinel(rng, (n, ld))
    S[:, :T * NB] = rng.normal(size=(n, T * NB))            # the band itself: no business of the product's
    S[:, B0 * NB:(B0 + nbr) * NB] = rng.normal(size=(n, nbr * NB))
    S[:, (B0 + nbr) * NB:(B0 + nbr + 1) * NB] = 0.0
    S[:, (B0 + nbr) * NB] = rng.normal(size=n)
    ldb, cols = (nbr + 1) * NB + rows_beyond, nbr * NB + cols_beyond
    Cm = _sentinel(rng, (cols, ldb))
    for jb in range(nbr):
        Cm[jb * NB:(jb + 1) * NB, jb * NB:(nbr + 1) * NB] = rng.normal(size=(NB, (nbr + 1 - jb) * NB))
    d = dict(T=T, nbr=nbr, b0=b0, ld=ld, S=S.ravel(), ldb=ldb, bord_cols=cols, bfirst=bfirst, segtab=segtab)
    if src:
        d["bord_src"] = Cm.ravel()
        d["bord"] = _sentinel(rng, (cols, ldb)).ravel()
    else:
        d["bord"] = Cm.ravel()
    return d


def wt_tile(sysd, ib, lo, hi):
    """W^T(ib, block columns lo .. hi - 1) as (64, 64 (hi - lo)) in long double: row = border row, column = the band's column."""
    B0 = sysd["b0"] or sysd["T"]
    S = sysd["S"].reshape(sysd["T"] * NB, sysd["ld"])
    return S[lo * NB:hi * NB, (B0 + ib) * NB:(B0 + ib + 1) * NB].T.astype(LD)


def product_reference(sysd, ks=1, jb_end=None, drop=None, shift=None):
    """(ref, bound, given): the block after the product in long double, the bound per element, and the block's input as float64, all
    (bord_cols, ldb) like bord.  What is no lower tile of the border block (in a tile column < jb_end), and every tile with an empty
    sum and no separate source, is `given` in ref and has bound 0; so has a tile with an empty sum that is copied from its source.
    The sums run chunk by chunk as launch_border_syrk cuts them (ks; with a segments' table ks is 1), which changes no value.
    Mutations for the test of the test: drop = (ib, jb, k): the tile's k-th k-step of four columns is left out; shift = (ib, jb):
    the end of the tile's first chunk (or segment) moves one block column up, so that one block column is summed twice."""
    T, nbr, ldb, cols = sysd["T"], sysd["nbr"], sysd["ldb"], sysd["bord_cols"]
    given = sysd["bord"].reshape(cols, ldb)
    has_src = sysd.get("bord_src") is not None
    cin = sysd["bord_src"].reshape(cols, ldb) if has_src else given
    ref = given.astype(LD)
    bound = np.zeros((cols, ldb))
    for jb in range(nbr if jb_end is None else jb_end):
        for ib in range(jb, nbr + 1):
            ranges = pair_ranges(sysd, ib, jb)
            if not ranges and not has_src:
                continue                                      # an empty sum: the tile is not touched
            Cij = cin[jb * NB:(jb + 1) * NB, ib * NB:(ib + 1) * NB].T.astype(LD)          # (row, column) of the tile
            acc, mag, K = Cij.copy(), np.abs(Cij), 0
            pieces = []
            for lo, hi in ranges:
                pieces += [c for c in chunk_ranges(T, lo, ks) if c is not None] if ks > 1 else [(lo, hi)]
            if shift is not None and shift == (ib, jb):
                assert len(pieces) > 1
                pieces[0] = (pieces[0][0], pieces[0][1] + 1)
            step = 0
            for lo, hi in pieces:
                A, B = wt_tile(sysd, ib, lo, hi), wt_tile(sysd, jb, lo, hi)
                if drop is not None and drop[:2] == (ib, jb) and 0 <= drop[2] - step < (hi - lo) * 16:
                    keep = np.ones(A.shape[1], bool)
                    keep[4 * (drop[2] - step):4 * (drop[2] - step) + 4] = False
                    A, B = A[:, keep], B[:, keep]
                step += (hi - lo) * 16
                acc -= A @ B.T
                mag += np.abs(A) @ np.abs(B).T
                K += A.shape[1]
            ref[jb * NB:(jb + 1) * NB, ib * NB:(ib + 1) * NB] = acc.T
            if K > 0:
                bound[jb * NB:(jb + 1) * NB, ib * NB:(ib + 1) * NB] = ((K + ks + 4) * U * mag).astype(np.float64).T
    return ref, bound, given


def lower_tile_mask(sysd, jb_end=None):
    """True on the elements of the border block's lower tiles and right-hand-side row tiles (tile columns < jb_end), (bord_cols, ldb)."""
    nbr = sysd["nbr"]
    m = np.zeros((sysd["bord_cols"], sysd["ldb"]), bool)
    for jb in range(nbr if jb_end is None else jb_end):
        m[jb * NB:(jb + 1) * NB, jb * NB:(nbr + 1) * NB] = True
    return m


def worst_ratio(got, ref, bound, where):
    """max |got - ref| / bound over `where` (elements with bound 0 must be equal)."""
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    exact = where & (bound == 0)
    assert np.all(err[exact] == 0), "an element with an empty sum differs from what was given"
    sel = where & (bound > 0)
    return float((err[sel] / bound[sel]).max()) if sel.any() else 0.0


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


# ---- the product's cases --------------------------------------------------------------------------------------------------------------
# name -> (systems, launch keywords of debug_border_product without the table, evidence the CPU suite checks)

SUM_LENGTH = [(T, nbr) for T in (1, 2, 3, 5) for nbr in (1, 2, 5)]
SPLIT_K = [(5, 2), (5, 4), (2, 2), (9, 8)]
SEG_ENDS = [3, 4, 7]                                  # three segments over T = 7: 3, 1 and 3 block columns
SEG_FIRSTS = [[0, 1, 0, INACTIVE, 0],                 # tile rows 0 .. 3 and the right-hand side, which rides from each segment's first column
              [3, INACTIVE, INACTIVE, INACTIVE, 3],   # row 1 is inactive in the one-column segment
              [4, 5, INACTIVE, 4, 4]]                 # rows 2 and 3 share no segment


def product_case(name):
    rng = _rng(name)
    kind = name.split(":")[0]
    if kind == "sum":
        _, T, nbr = name.split(":")
        return [make_system(rng, int(T), int(nbr))], {}, {}
    if kind == "bfirst":                               # non-decreasing first columns, row 3 starts at T: every sum with it is empty
        return [make_system(rng, 5, 4, bfirst=[0, 1, 3, 5, 0])], {}, dict(empty_sum=(3, 0))
    if kind == "bfirst_src":
        return [make_system(rng, 5, 4, bfirst=[0, 1, 3, 5, 0], src=True)], {}, dict(empty_sum=(3, 0))
    if kind == "bfirst_view":                          # the border starts further down than T
        return [make_system(rng, 3, 3, b0=5, bfirst=[0, 0, 2, 1])], {}, {}
    if kind == "segtab":
        return [make_system(rng, 7, 4, segtab=make_segtab(7, 4, SEG_ENDS, SEG_FIRSTS))], {}, dict(inactive=(1, 1), disjoint=(3, 2))
    if kind == "segtab_src":
        return [make_system(rng, 7, 4, segtab=make_segtab(7, 4, SEG_ENDS, SEG_FIRSTS), src=True)], {}, dict(inactive=(1, 1), disjoint=(3, 2))
    if kind == "split":
        _, T, ks = name.split(":")
        ev = dict(empty_chunk=True) if (int(T), int(ks)) in ((5, 4), (9, 8)) else {}
        return [make_system(rng, int(T), 2)], dict(ks=int(ks)), ev
    if kind == "split_bfirst":                         # c0 > 0: the kernel and the reduction must cut the same len; row 2's second chunk is empty
        return [make_system(rng, 5, 3, bfirst=[0, 2, 4, 0])], dict(ks=2), dict(empty_chunk=True, c0_positive=(1, 0))
    if kind == "split_view":
        return [make_system(rng, 5, 2, b0=8)], dict(ks=2), {}
    if kind == "split_jb_end":
        return [make_system(rng, 5, 3)], dict(ks=2, jb_end=2), {}
    raise KeyError(name)


PRODUCT_CASES = ([f"sum:{T}:{nbr}" for T, nbr in SUM_LENGTH] + ["bfirst", "bfirst_src", "bfirst_view", "segtab", "segtab_src"] +
                 [f"split:{T}:{ks}" for T, ks in SPLIT_K] + ["split_bfirst", "split_view", "split_jb_end"])
FUSED = [(2, 3), (1, 3)]                              # ks_sys of the fused launches, T = (4, 6), nbr = 3


def fused_systems(name="fused"):
    rng = _rng(name)
    return [make_system(rng, 4, 3), make_system(rng, 6, 3)]


def eight_systems(name="eight"):
    """Eight different systems for one launch: every T and nbr of the sum-length family, one with first columns."""
    rng = _rng(name)
    shapes = [(1, 5), (5, 1), (2, 2), (3, 5), (5, 2), (1, 1), (3, 1), (2, 5)]
    out = [make_system(rng, T, nbr) for T, nbr in shapes]
    out[3]["bfirst"] = [0, 0, 1, 2, 3, 0]
    return out


# ---- the apply's cases ----------------------------------------------------------------------------------------------------------------

def make_apply_system(rng, T, nbr, b0=0, segtab=None, outside=None):
    """S with W in the border rows (normal(0, 1); with a table whose masks are in use: inside the masks only, `outside` elsewhere),
    yv, x_loc (non-zero everywhere, padding included)."""
    n, B0 = T * NB, b0 or T
    ld = (B0 + nbr + 1) * NB
    S = _sentinel(rng, (n, ld))
    S[:, :T * NB] = rng.normal(size=(n, T * NB))
    W = rng.normal(size=(n, nbr * NB))
    masks = parse_segtab(segtab, nbr)[2] if segtab is not None else None
    if masks is not None:
        for c in range(T):
            for t in range(nbr):
                if not (masks[c] >> t) & 1:
                    W[c * NB:(c + 1) * NB, t * NB:(t + 1) * NB] = 0.0 if outside is None else outside
    S[:, B0 * NB:(B0 + nbr) * NB] = W
    S[:, (B0 + nbr) * NB:(B0 + nbr + 1) * NB] = 0.0
    S[:, (B0 + nbr) * NB] = rng.normal(size=n)
    return dict(T=T, nbr=nbr, b0=b0, ld=ld, S=S.ravel(), segtab=segtab, yv=rng.normal(size=n), x_loc=rng.normal(size=nbr * NB))


def apply_reference(sysd):
    """(ref, bound): yv - W x over the active tile rows in long double (the masks' tile rows where masks are in use, else every row)."""
    T, nbr = sysd["T"], sysd["nbr"]
    B0 = sysd["b0"] or T
    S = sysd["S"].reshape(T * NB, sysd["ld"])
    masks = parse_segtab(sysd["segtab"], nbr)[2] if sysd.get("segtab") is not None else None
    x = sysd["x_loc"].astype(LD)
    ref, bound = sysd["yv"].astype(LD), np.zeros(T * NB)
    for c in range(T):
        rows = [t for t in range(nbr) if masks is None or (masks[c] >> t) & 1]
        idx = np.concatenate([np.arange(t * NB, (t + 1) * NB) for t in rows]) if rows else np.zeros(0, int)
        Wc = S[c * NB:(c + 1) * NB, B0 * NB + idx].astype(LD)
        ref[c * NB:(c + 1) * NB] -= Wc @ x[idx]
        mag = np.abs(sysd["yv"][c * NB:(c + 1) * NB]).astype(LD) + np.abs(Wc) @ np.abs(x[idx])
        bound[c * NB:(c + 1) * NB] = ((NB * len(rows) + 1 + 4) * U * mag).astype(np.float64)
    return ref, bound


def mask_segtab(T=3, nbr=34):
    """Two segments over three block columns whose masks reach into the high word: tile row 33 is active in the first segment, 32 in
    the second."""
    firsts = [[0 if t % 3 == 0 else (1 if t % 3 == 1 else INACTIVE) for t in range(nbr)] + [0],
              [2 if t % 2 == 0 else INACTIVE for t in range(nbr)] + [2]]
    return make_segtab(T, nbr, [2, 3], firsts)


def apply_case(name):
    rng = _rng(name)
    if name == "one":
        return [make_apply_system(rng, 2, 3)]
    if name == "three":                                # T = 1, 3, 2 in one grid: the shorter systems' workgroups leave early
        return [make_apply_system(rng, 1, 1), make_apply_system(rng, 3, 3), make_apply_system(rng, 2, 1)]
    if name == "view":
        return [make_apply_system(rng, 2, 3, b0=4)]
    if name == "masks":
        return [make_apply_system(rng, 3, 34, segtab=mask_segtab())]
    if name == "masks_decode":                         # a finite sentinel outside the masks: a wrongly decoded bit adds 1e30 x
        return [make_apply_system(rng, 3, 34, segtab=mask_segtab(), outside=1e30)]
    if name == "no_masks":                             # more than 64 tile rows: the table carries no masks, the full walk
        firsts = [[0] * 65 + [0], [1] * 65 + [1]]
        return [make_apply_system(rng, 2, 65, segtab=make_segtab(2, 65, [1, 2], firsts))]
    raise KeyError(name)


APPLY_CASES = ["one", "three", "view", "masks", "masks_decode", "no_masks"]
