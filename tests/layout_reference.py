"""The layout planner (slide_slam_amd/csrc/host_layout.hpp) restated in plain Python from what its tables MEAN (the header's comments,
DESIGN.md 4, "Where the layout is planned") — test infrastructure for test_layout_plan_host.py, not a test.  Sets, sorts and
definitions where the C++ keeps running maxima and fills tables in passes.

Conventions: a pose owns the six coordinates 6 p .. 6 p + 5 of the reduced system; a tile is NB = 64 coordinates, so pose p lies in
block columns col(p) = 6 p // 64 and (6 p + 5) // 64 (two of them when it straddles a tile edge).  INF = 1 << 30 stands for "never"."""
from __future__ import annotations

NB = 64
INF = 1 << 30
VT_POINT, VT_CUBE, VT_CYL = 1, 2, 3
DIM = {VT_POINT: 3, VT_CUBE: 9, VT_CYL: 7}

REFUSE_GHOST_IDS = "exact joint step: slide_graph_set_ghost_ids must name every ghost factor of the graph"
REFUSE_CLASSES = "separator offsets do not match the landmark classes of the shared slots"
REFUSE_OVERLAP = "separator offsets: the coordinate ranges of two shared slots overlap"
REFUSE_TWICE = "exact joint step: two ghost factors of one graph name the same measurement"


def col(p):
    return 6 * p // NB


def tiles(n):
    return -(-n // NB)


def tiles_of(lo, n):
    """The tile rows the coordinates lo .. lo + n - 1 touch."""
    return range(lo // NB, (lo + n - 1) // NB + 1)


# ---- the tile profile ------------------------------------------------------------------------------------------------------------------
def tile_profile(reach, Pn, dense):
    """prof[c]: the last tile row of block column c inside the profile — the column itself, the tile rows its poses' couplings reach,
    and everything an earlier column reaches (the fill of the factorisation).  first[r]: the first column that reaches tile row r."""
    T = tiles(6 * Pn)
    if dense:
        prof = [T - 1] * T
    else:
        rows = [{c} for c in range(T)]                      # tile rows block column c couples to by itself
        for p in range(Pn):
            for c in {col(p), (6 * p + 5) // NB}:
                rows[c].add((6 * reach[p] + 5) // NB)
        prof = [max(set().union(*rows[:c + 1])) for c in range(T)]
    first = [min(c for c in range(T) if prof[c] >= r) for r in range(T)]
    return prof, first


# ---- the border ------------------------------------------------------------------------------------------------------------------------
def couplings(Pn, lf_pose, lf_lm, bt_i, bt_j):
    """reach[p]: the last pose that pose p is coupled to — itself, an observer of a landmark it observes, the later pose of a between
    factor whose earlier pose it is."""
    observers = {}
    for p, l in zip(lf_pose, lf_lm):
        observers.setdefault(l, set()).add(p)
    partners = [{p} for p in range(Pn)]
    for p, l in zip(lf_pose, lf_lm):
        partners[p] |= observers[l]
    for i, j in zip(bt_i, bt_j):
        partners[min(i, j)].add(max(i, j))
    return [max(s) for s in partners]


def cuts_of(Pn, reach, want_seg):
    """-> (segments as tile ranges, windows [q0, q1) of separator poses); ([], []) when the chain is not cut.  The chain is cut at
    Pn i / want_seg, i = 1 .. want_seg - 1; the window behind a cut at q0 ends behind the last pose anything before q0 couples to.  A cut
    too close (8 poses) to the start of its segment, one nothing couples across, and one whose window ends within 8 poses of the chain's
    end are skipped.  Segments own whole tiles: if two would share a tile, the chain stays uncut."""
    if want_seg < 2 or Pn < 64:
        return [], []
    windows, start = [], 0
    for i in range(1, want_seg):
        q0 = Pn * i // want_seg
        q1 = max(reach[:q0]) + 1 if q0 > 0 else 0
        if q0 <= start + 8 or q1 <= q0 or q1 + 8 >= Pn:
            continue
        windows.append((start, q0, q1))
        start = q1
    if not windows:
        return [], []
    segs = [(col(s0), tiles(6 * q0)) for s0, q0, _ in windows] + [(col(start), tiles(6 * Pn))]
    if any(b[0] < a[1] for a, b in zip(segs, segs[1:])):
        return [], []
    return segs, [(q0, q1) for _, q0, q1 in windows]


def border(Pn, lf_pose, lf_lm, lm_type, lm_fids, bt_i, bt_j, sh_lid, sep_off, gh_pose, gh_gid, lam_total, want_seg):
    """-> {"refused": message} or the tables of BorderPlan by name."""
    Ln, m = len(lm_type), sep_off[-1]
    if lam_total > 0 and len(gh_gid) != len(gh_pose):
        return {"refused": REFUSE_GHOST_IDS}
    reach = couplings(Pn, lf_pose, lf_lm, bt_i, bt_j)
    segs, windows = cuts_of(Pn, reach, want_seg)
    window_poses = [q for q0, q1 in windows for q in range(q0, q1)]
    pose_sep = [-1] * max(Pn, 1)
    for k, q in enumerate(window_poses):
        pose_sep[q] = 6 * k
    nsep = tiles(6 * len(window_poses))

    # the items: (first block column, kind, id, coordinates, global offset, the poses it couples to)
    items, used = [], set()
    for i, lid in enumerate(sh_lid):
        if not 0 <= lid < Ln:
            continue
        d = DIM[lm_type[lid]]
        if sep_off[i] + d > m:
            return {"refused": REFUSE_CLASSES}
        mine = set(range(sep_off[i], sep_off[i] + d))
        if mine & used:
            return {"refused": REFUSE_OVERLAP}
        used |= mine
        poses = [lf_pose[f] for f in lm_fids[lid]]
        items.append((col(min(poses)) if poses else 0, 0, lid, d, sep_off[i], poses))
    if lam_total > 0:
        if len(set(gh_gid)) != len(gh_gid):
            return {"refused": REFUSE_TWICE}
        for q, (p, g) in enumerate(zip(gh_pose, gh_gid)):
            items.append((col(p), 1, q, 6, m + 6 * g, [p]))
    items.sort(key=lambda it: it[0])                        # (stable: equal first columns keep slot order, landmarks before ghosts)

    lm_bord, gh_bord, sep_map = [-1] * max(Ln, 1), [-1] * max(len(gh_pose), 1), [-1] * max(m + lam_total, 1)
    o = nsep * NB
    placed = []                                             # (border offset, item)
    for it in items:
        (lm_bord if it[1] == 0 else gh_bord)[it[2]] = o
        for k in range(it[3]):
            sep_map[it[4] + k] = o + k
        placed.append((o, it))
        o += it[3]
    nbr = tiles(o)
    on_tile = {t: {it[0] for at, it in placed if t in tiles_of(at, it[3])} for t in range(nbr)}
    bfirst, high = [], 0
    for t in range(nbr):
        high = max(high, min(on_tile[t]) if t >= nsep and on_tile[t] else 0)      # (never decreasing, by force)
        bfirst.append(high)
    bfirst.append(0)
    out = dict(refused="", nbr=nbr, nsep=nsep, nsep_dim=6 * len(window_poses), n_sep_poses=len(window_poses), lm_bord=lm_bord, sep_map=sep_map,
               gh_bord=gh_bord, bfirst=bfirst, segs=[v for s in segs for v in s], pose_sep=pose_sep, seg_ord=[], seg_sfirst=[], flat_ord=[],
               seg_tab=[], seg_tab_head=0)
    if not segs:
        return out

    # active[q][t]: the block columns of segment q in which border tile row t is non-zero
    NS = len(segs)
    seg_of = {c: q for q, (t0, t1) in enumerate(segs) for c in range(t0, t1)}
    active = [[set() for _ in range(nbr + 1)] for _ in range(NS)]
    for at, it in placed:
        for p in it[5]:
            if 0 <= p < Pn and pose_sep[p] < 0 and col(p) in seg_of:
                for t in tiles_of(at, it[3]):
                    active[seg_of[col(p)]][t].add(col(p))
    at = 0
    for w, (q0, q1) in enumerate(windows):
        rows = tiles_of(6 * at, 6 * (q1 - q0))
        before = [p for p in range(q0) if col(p) >= segs[w][0] and reach[p] >= q0]      # the poses of segment w coupled into the window
        for t in rows:
            if before:
                active[w][t].add(col(min(before)))
            active[w + 1][t].add(segs[w + 1][0])            # behind it: from the segment's first block column on
        at += q1 - q0
    sf = [[min(active[q][t], default=INF) for t in range(nbr)] + [segs[q][0]] for q in range(NS)]      # (last: the right-hand side)
    out["seg_ord"] = [sorted(range(nbr), key=lambda t, q=q: sf[q][t]) for q in range(NS)]
    out["seg_sfirst"] = [[sf[q][t] for t in out["seg_ord"][q]] + [segs[q][0]] for q in range(NS)]
    out["flat_ord"] = [t for o_ in out["seg_ord"] for t in o_]
    tab = [NS] + [t1 for _, t1 in segs] + [v for row in sf for v in row]
    out["seg_tab_head"] = len(tab)
    if nbr <= 64:
        Tb = tiles(6 * Pn)
        tab.append(Tb)
        for c in range(Tb):
            # segment q works on border tile row t at column c: c is one of its columns and the row is non-zero there already
            bits = {t for q, (t0, t1) in enumerate(segs) if t0 <= c < t1 for t in range(nbr) if sf[q][t] <= c}
            mask = sum(1 << t for t in bits)
            tab += [_i32(mask & 0xffffffff), _i32(mask >> 32)]
    else:
        tab.append(0)
    out["seg_tab"] = tab
    return out


def _i32(u):
    return u - (1 << 32) if u >= 1 << 31 else u


# ---- the segments' own profiles ------------------------------------------------------------------------------------------------------------
def segment_profiles(prof, segs):
    """Per segment (t0, t1): its columns' profile, cut off at its last tile row, in its own numbering."""
    return [[min(prof[c], t1 - 1) - t0 for c in range(t0, t1)] for t0, t1 in segs]


# ---- the Schur pair lists ----------------------------------------------------------------------------------------------------------------
def schur_pairs(pose_fids, lm_fids, prof, lf_pose, lf_lm, lf_eoff, lm_type, lm_bord, ebuf_used):
    """-> (walk, W, idx, pairs).  Block (pi, pj), pj <= pi < p_end(pj), lists every pair of factors (x on pose pi, y on pose pj) on one
    landmark that is not a border landmark, ordered by (x's landmark, x, y); p_end(pj): the first pose past the tile rows that the
    block column of pj's LAST coordinate reaches.  W: the widest strip.  idx[2 (pj W + d)]: first pair and pair count of block (pj + d, pj)."""
    Pn = len(pose_fids)
    if Pn == 0 or not prof:
        return True, 1, [], []
    p_end = [min(Pn, ((prof[(6 * pj + 5) // NB] + 1) * NB + 5) // 6) for pj in range(Pn)]
    W = max([1] + [p_end[pj] - pj for pj in range(Pn)])
    if W > 256 or ebuf_used >= 1 << 29:
        return True, W, [], []
    ed = [(lf_eoff[f] << 4) | DIM[lm_type[lf_lm[f]]] for f in range(len(lf_lm))]
    blocks = {}
    for l, fids in enumerate(lm_fids):
        if lm_bord and l < len(lm_bord) and lm_bord[l] >= 0:
            continue
        for y in fids:
            for x in fids:
                pi, pj = lf_pose[x], lf_pose[y]
                if pj <= pi < p_end[pj]:
                    blocks.setdefault((pj, pi - pj), []).append((l, x, y))
    idx, pairs = [0] * (2 * Pn * W), []
    for (pj, d) in sorted(blocks):
        idx[2 * (pj * W + d)] = len(pairs) // 2
        idx[2 * (pj * W + d) + 1] = len(blocks[pj, d])
        for _, x, y in sorted(blocks[pj, d]):
            pairs += [ed[x], ed[y]]
    return False, W, idx, pairs


# ---- the slot table ----------------------------------------------------------------------------------------------------------------------
def lm_slot(sh_lid, Ln):
    """-> (slot per landmark: the last slot that names it, or -1; onto: no named slot out of range, no landmark named twice)."""
    slot = [-1] * max(Ln, 1)
    for i, l in enumerate(sh_lid):
        if 0 <= l < Ln:
            slot[l] = i
    named = [l for l in sh_lid if l >= 0]
    return slot, all(l < Ln for l in named) and len(set(named)) == len(named)
