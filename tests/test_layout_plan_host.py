"""The layout planner (slide_slam_amd/csrc/host_layout.hpp: tile profile, border and cuts, segment profiles, Schur pair lists, slot
table) on the CPU.  tests/layout_plan_check.hip wraps the five functions in a stand-alone host program (no device is touched); here it is
compiled twice — plain, and with -fsanitize=address,undefined -fno-sanitize-recover=all on the host side — and every case goes through
both: every table must equal the restatement in tests/layout_reference.py, and the sanitized program must end clean.  The cases are the
smallest at which each piece can go wrong (poses that straddle a tile, items that straddle a border tile, the 64-pose and one-tile
thresholds of the cuts, 64 / 65 border tiles for the masks, strips of 256 / 257 poses)."""
import os
import subprocess

import numpy as np
import pytest

import layout_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
POINT, CUBE, CYL = lr.VT_POINT, lr.VT_CUBE, lr.VT_CYL
ESIZE = {POINT: 42, CUBE: 114, CYL: 90}          # doubles of a factor's Schur record (graph_dev.hpp lf_esize)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """(the plain program, the sanitized one, a scratch directory)"""
    d = tmp_path_factory.mktemp("layout_plan")
    out = []
    for name, flags in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g"] + SANITIZE)):
        exe = str(d / f"layout_plan_check_{name}")
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "slide_slam_amd", "csrc"),
                            os.path.join(ROOT, "tests", "layout_plan_check.hip"), "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        out.append(exe)
    return out[0], out[1], d


_n = [0]


def run(programs, op, arrays):
    """One case through both programs -> the output arrays (lists of int); the two must agree and the sanitized one end clean."""
    plain, sanitized, d = programs
    words = [op]
    for a in arrays:
        a = [int(v) for v in a]
        words += [len(a)] + a
    _n[0] += 1
    fin = str(d / f"in{_n[0]}.bin")
    np.array(words, np.int64).tofile(fin)
    got = []
    for exe in (plain, sanitized):
        fout = str(d / f"out{_n[0]}_{os.path.basename(exe)}.bin")
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and f"layout plan ok op={op}" in r.stdout and not r.stderr.strip(), (exe, r.returncode, r.stdout, r.stderr[-3000:])
        w = np.fromfile(fout, np.int64).tolist()
        out, at = [], 0
        while at < len(w):
            out.append(w[at + 1:at + 1 + w[at]])
            at += 1 + w[at]
        got.append(out)
    assert got[0] == got[1]
    return got[0]


def csr(lists):
    ptr = [0]
    for l in lists:
        ptr.append(ptr[-1] + len(l))
    return ptr, [v for l in lists for v in l]


def unflatten(lens, flat):
    out, at = [], 0
    for n in lens:
        out.append(flat[at:at + n])
        at += n
    assert at == len(flat)
    return out


class Graph:
    """Pn poses in a chain of between factors (without those in `gaps`: k means no factor k - 1 -> k) and landmarks (type, observers);
    the factors are numbered pose by pose, as a stream adds them."""

    def __init__(self, Pn, lms, gaps=(), extra_bt=()):
        self.Pn, self.lm_type = Pn, [t for t, _ in lms]
        self.lf_pose, self.lf_lm, self.lf_eoff = [], [], []
        self.lm_fids, self.pose_fids = [[] for _ in lms], [[] for _ in range(Pn)]
        used = 0
        for p in range(Pn):
            for l, (t, obs) in enumerate(lms):
                for _ in range(list(obs).count(p)):
                    f = len(self.lf_pose)
                    self.lf_pose.append(p); self.lf_lm.append(l); self.lf_eoff.append(used)
                    self.lm_fids[l].append(f); self.pose_fids[p].append(f)
                    used += ESIZE[t]
        self.ebuf_used = used
        bt = [(k - 1, k) for k in range(1, Pn) if k not in gaps] + list(extra_bt)
        self.bt_i, self.bt_j = [a for a, _ in bt], [b for _, b in bt]

    def border(self, programs, sh_lid, sep_off, gh_pose=(), gh_gid=(), lam_total=0, want_seg=1):
        """plan_border through the programs against the restatement -> the restatement's tables."""
        args = (self.Pn, self.lf_pose, self.lf_lm, self.lm_type, self.lm_fids, self.bt_i, self.bt_j, list(sh_lid), list(sep_off), list(gh_pose),
                list(gh_gid), lam_total, want_seg)
        want = lr.border(*args)
        got = run(programs, 1, [[self.Pn, lam_total, want_seg], self.lf_pose, self.lf_lm, self.lm_type, *csr(self.lm_fids), self.bt_i, self.bt_j,
                                sh_lid, sep_off, gh_pose, gh_gid])
        msg = bytes(got[0]).decode()
        assert msg == want["refused"]
        if msg:
            assert all(len(a) == 0 or a == [0] * 5 for a in got[1:]), got      # a refusal carries nothing else
            return want
        assert got[1] == [want[k] for k in ("nbr", "nsep", "nsep_dim", "n_sep_poses", "seg_tab_head")]
        for k, a in zip(("lm_bord", "sep_map", "gh_bord", "bfirst", "segs", "pose_sep"), got[2:8]):
            assert a == want[k], k
        assert unflatten(got[8], got[9]) == want["seg_ord"] and unflatten(got[10], got[11]) == want["seg_sfirst"]
        assert got[12] == want["flat_ord"] and got[13] == want["seg_tab"]
        return want


def chain_lms(Pn, span=2):
    """A private point per pose, seen from it and the next `span` poses."""
    return [(POINT, range(p, min(Pn, p + span + 1))) for p in range(Pn)]


def slots(g, shared, order=None):
    """sh_lid and separator offsets for the shared landmarks `shared` (in slot order; -1: a slot that names no landmark, 3 coordinates
    wide), the coordinates laid out in the order `order` of the slots."""
    dims = [3 if l < 0 else lr.DIM[g.lm_type[l]] for l in shared]
    off, o = [0] * len(shared), 0
    for i in (order or range(len(shared))):
        off[i] = o
        o += dims[i]
    return list(shared), off + [o]


# ---- the tile profile ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Pn,far,dense", [(1, None, False), (10, None, False), (11, None, False), (32, None, False), (40, 39, False),
                                          (32, None, True), (0, None, False)],
                         ids=["1", "10-one-tile", "11-straddle", "32-three-tiles", "pose0-reaches-the-end", "dense", "empty"])
def test_tile_profile(programs, Pn, far, dense):
    reach = [min(p + 2, Pn - 1) for p in range(Pn)]
    if far is not None:
        reach[0] = far
    prof, first = run(programs, 0, [[Pn, int(dense)], reach])
    want = lr.tile_profile(reach, Pn, dense)
    assert (prof, first) == (list(want[0]), list(want[1]))
    T = -(-6 * Pn // 64)
    assert len(prof) == T
    if Pn == 11:
        assert prof == [1, 1]                      # pose 10 lies in both tiles
    if far is not None or dense:
        assert prof == [T - 1] * T and first == [0] * T


# ---- the border, uncut -----------------------------------------------------------------------------------------------------------------
def _mixed_border_graph():
    # eight cylinders and a cube (56 + 9 coordinates: the cube straddles border tiles 0 and 1); first columns out of order; landmark 3
    # has no factor; pose 10 straddles block columns 0 and 1
    lms = [(CYL, [25, 26]), (CYL, [0, 1]), (CYL, [12]), (CYL, []), (CYL, [22]), (CYL, [3]), (CYL, [11]), (CYL, [10]), (CUBE, [15, 2]),
           (POINT, [5, 6])]
    return Graph(30, lms)


@pytest.mark.parametrize("ghosts", ["none", "named", "unnamed"])
def test_border_without_cuts(programs, ghosts):
    g = _mixed_border_graph()
    sh_lid, sep_off = slots(g, [0, 1, 2, -1, 3, 4, 5, 6, 7, 8], order=[4, 9, 0, 3, 7, 1, 2, 8, 6, 5])
    kw = {"named": dict(gh_pose=[20, 4], gh_gid=[2, 0], lam_total=18),       # (measurement 1 is another robot pair's: its coordinates map nowhere)
          "unnamed": dict(gh_pose=[20, 4]), "none": {}}[ghosts]
    w = g.border(programs, sh_lid, sep_off, **kw)
    assert w["nbr"] == 2 and w["nsep"] == 0 and w["segs"] == []                       # (65 coordinates, 77 with the ghosts' twelve)
    cols = [0 if l == 3 else lr.col(min(g.lf_pose[f] for f in g.lm_fids[l])) for l in range(9)]
    order = sorted(range(9), key=lambda l: (cols[l], sh_lid.index(l)))
    assert [w["lm_bord"][l] for l in order] == sorted(w["lm_bord"][:9]) and w["lm_bord"][9] == -1          # stable, by first column
    assert w["bfirst"][:-1] == sorted(w["bfirst"][:-1]) and w["bfirst"][-1] == 0
    assert w["sep_map"][sep_off[3]:sep_off[3] + 3] == [-1] * 3                                            # the slot without a landmark
    if ghosts == "named":
        m = sep_off[-1]
        assert -1 not in w["sep_map"][m:m + 6] + w["sep_map"][m + 12:m + 18] and w["sep_map"][m + 6:m + 12] == [-1] * 6
        assert w["gh_bord"][1] < w["gh_bord"][0]                                                          # pose 4 before pose 20
    else:
        assert w["gh_bord"] == [-1] * max(len(kw.get("gh_pose", [])), 1)


def test_border_refusals(programs):
    g = _mixed_border_graph()
    sh_lid, off = slots(g, [0, 1, 8])
    past = off[:2] + [off[3] - 8, off[3]]                                           # the cube's nine coordinates start eight before the end
    assert g.border(programs, sh_lid, past)["refused"] == lr.REFUSE_CLASSES
    overlap = [off[0], off[0] + 6] + off[2:]                                       # slot 1 starts on slot 0's last coordinate
    assert g.border(programs, sh_lid, overlap)["refused"] == lr.REFUSE_OVERLAP
    assert g.border(programs, sh_lid, off, gh_pose=[3, 9], gh_gid=[1, 1], lam_total=12)["refused"] == lr.REFUSE_TWICE
    assert g.border(programs, sh_lid, off, gh_pose=[3, 9], gh_gid=[1], lam_total=12)["refused"] == lr.REFUSE_GHOST_IDS
    # offsets laid out for other classes (three points' worth of coordinates): the cube in the last slot does not fit
    assert g.border(programs, sh_lid, [0, 3, 6, 9])["refused"] == lr.REFUSE_CLASSES
    assert g.border(programs, sh_lid, off)["refused"] == ""


# ---- the cuts --------------------------------------------------------------------------------------------------------------------------
def wide(q):
    """A point seen from poses q - 2 and q + 12: the window behind a cut at q holds 13 poses, more than a tile."""
    return (POINT, [q - 2, q + 12])


def _cut_graph(Pn, wides=(), gaps=(), extra=()):
    lms = chain_lms(Pn) if not gaps else [(t, [p for p in obs if not any(min(obs) < k <= p for k in gaps)]) for t, obs in chain_lms(Pn)]
    n = len(lms)
    lms += [wide(q) for q in wides] + list(extra) + [(CYL, [1, 2]), (CUBE, [Pn // 2, Pn // 2 + 1]), (POINT, [Pn - 2]), (CYL, [])]
    g = Graph(Pn, lms, gaps=gaps)
    g.shared = list(range(len(lms) - 4, len(lms)))
    assert n == Pn
    return g


@pytest.mark.parametrize("Pn,want_seg,n_segs", [(63, 2, 0), (64, 2, 2), (65, 2, 2), (150, 2, 2), (150, 3, 3), (150, 4, 4)])
def test_cuts(programs, Pn, want_seg, n_segs):
    g = _cut_graph(Pn, wides=sorted({Pn * i // n for n in (2, 3, 4) for i in range(1, n)}) if Pn == 150 else ())
    w = g.border(programs, *slots(g, g.shared), want_seg=want_seg)
    assert len(w["segs"]) == 2 * n_segs
    if n_segs:
        assert w["nsep"] > 0 and w["seg_tab"][0] == n_segs and w["seg_tab"][w["seg_tab_head"]] == -(-6 * Pn // 64)
        if want_seg >= 3:
            assert any(lr.INF in row[:-1] for row in w["seg_sfirst"])      # a window's rows never touch the segments it does not adjoin


def test_cut_skipped_near_the_end(programs):
    """Three segments asked for; the window behind the second cut (pose 100) would end at pose 143 of 150: two segments."""
    g = _cut_graph(150, wides=[50], extra=[(POINT, [98, 142])])
    w = g.border(programs, *slots(g, g.shared), want_seg=3)
    assert len(w["segs"]) == 4 and w["n_sep_poses"] == 13


@pytest.mark.parametrize("want_seg", [2, 3])
def test_window_narrower_than_a_tile(programs, want_seg):
    """Windows of two poses: the segments on either side would share a tile, so the band stays uncut."""
    g = _cut_graph(150)
    w = g.border(programs, *slots(g, g.shared), want_seg=want_seg)
    assert w["segs"] == [] and w["nsep"] == 0 and w["seg_tab"] == [] and w["pose_sep"] == [-1] * 150


def test_gap_nothing_couples_across(programs):
    """Four segments asked for; nothing couples pose 74 to pose 75 (no between factor, no landmark), so no window is needed there."""
    g = _cut_graph(150, wides=[37, 112], gaps=(75,))
    assert lr.couplings(150, g.lf_pose, g.lf_lm, g.bt_i, g.bt_j)[74] == 74
    w = g.border(programs, *slots(g, g.shared), want_seg=4)
    assert len(w["segs"]) == 6 and w["n_sep_poses"] == 26


@pytest.mark.parametrize("cubes,nbr", [(440, 64), (448, 65)])
def test_masks_at_64_and_65_border_tiles(programs, cubes, nbr):
    g = _cut_graph(150, wides=[75], extra=[(CUBE, [(7 * k) % 148, (7 * k) % 148 + 1]) for k in range(cubes)])
    shared = list(range(151, 151 + cubes))
    w = g.border(programs, *slots(g, shared), want_seg=2)
    assert w["nbr"] == nbr and w["nsep"] == 2 and len(w["segs"]) == 4
    tail = w["seg_tab"][w["seg_tab_head"]:]
    if nbr == 64:
        assert tail[0] == 15 and len(tail) == 1 + 2 * 15 and min(tail) < 0          # (row 63: the sign bit of a high word)
    else:
        assert tail == [0]


# ---- the segments' profiles ------------------------------------------------------------------------------------------------------------
def test_segment_profiles(programs):
    prof = [1, 2, 3, 4, 5, 6, 8, 8, 9, 10, 11, 12, 13, 14, 14]
    for segs in ([(0, 8), (8, 15)], [(0, 5), (5, 10), (10, 15)], [(0, 4), (4, 8), (8, 11), (11, 15)], []):
        lens, flat, off, flat2 = run(programs, 2, [prof, [v for s in segs for v in s]])
        want = lr.segment_profiles(prof, segs)
        assert unflatten(lens, flat) == want and flat2 == [v for p in want for v in p]
        assert off == [sum(len(p) for p in want[:k]) for k in range(len(want))]


# ---- the Schur pair lists --------------------------------------------------------------------------------------------------------------
def _pairs(programs, g, prof, lm_bord, ebuf_used=None):
    ebuf_used = g.ebuf_used if ebuf_used is None else ebuf_used
    got = run(programs, 3, [[ebuf_used], *csr(g.pose_fids), *csr(g.lm_fids), prof, g.lf_pose, g.lf_lm, g.lf_eoff, g.lm_type, lm_bord])
    walk, W, idx, pairs = lr.schur_pairs(g.pose_fids, g.lm_fids, prof, g.lf_pose, g.lf_lm, g.lf_eoff, g.lm_type, lm_bord, ebuf_used)
    assert got == [[int(walk), W], idx, pairs]
    return walk, W, idx, pairs


def test_schur_pairs_inside_one_strip(programs):
    """Landmark 0 (a cube) seen by poses 1, 2 and 4 (pose 2 twice), landmark 1 a border landmark, a point on each later pose besides."""
    g = Graph(12, [(CUBE, [1, 2, 2, 4]), (CYL, [1, 3])] + [(POINT, [p]) for p in range(5, 12)])
    prof, _ = lr.tile_profile([min(p + 3, 11) for p in range(12)], 12, False)
    bord = [-1] * len(g.lm_type)
    walk, W, idx, pairs = _pairs(programs, g, prof, bord)
    with_border = list(bord)
    with_border[1] = 0
    _, _, idx_b, pairs_b = _pairs(programs, g, prof, with_border)
    assert not walk and W == 12 and len(pairs_b) == len(pairs) - 2 * 3               # the cylinder's (1,1) (3,1) (3,3) are gone
    assert idx[2 * (1 * W + 1) + 1] == 2 and idx[2 * (1 * W + 3) + 1] == 1           # blocks (2, 1): pose 2's two factors; (4, 1)
    _pairs(programs, g, prof, [])                                                    # (no border table at all)


def test_schur_pairs_walk_flag(programs):
    def graph(Pn):
        return Graph(Pn, [(POINT, [0, Pn - 1])] + chain_lms(Pn, span=1))
    g = graph(256)
    assert _pairs(programs, g, [23] * 24, [])[:2] == (False, 256)
    assert _pairs(programs, g, [23] * 24, [], ebuf_used=1 << 29)[0] is True
    assert _pairs(programs, g, [23] * 24, [], ebuf_used=(1 << 29) - 1)[0] is False
    assert _pairs(programs, graph(257), [24] * 25, [])[:2] == (True, 257)
    assert _pairs(programs, Graph(0, []), [], [])[0] is True                         # an empty graph
    assert _pairs(programs, graph(4), [], [])[0] is True                             # no profile yet


# ---- the slot table --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh_lid,Ln,onto", [([2, 0, -1, 3], 5, True), ([2, 0, 2], 5, False), ([1, 7], 5, False), ([-1, -1], 0, True),
                                            ([0], 0, False)],
                         ids=["clean", "two-slots-one-landmark", "out-of-range", "no-landmarks", "out-of-range-empty-graph"])
def test_slot_table(programs, sh_lid, Ln, onto):
    got = run(programs, 4, [[Ln], sh_lid])
    slot, want_onto = lr.lm_slot(sh_lid, Ln)
    assert got == [[int(want_onto)], slot] and want_onto == onto
    if sh_lid == [2, 0, 2]:
        assert slot[2] == 2                         # the later slot holds the entry
