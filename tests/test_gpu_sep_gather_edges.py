"""The data-movement kernels between the stages of an exact joint pass — k_border_fill_b (E rows into the border), k_sep_extract_b
(cut poses out of the band) and k_sep_gather (the robots' border blocks summed into the separator system) — at their edges, each
case one exact joint pass (two, in fact: the second starts from the first's result) against the independent joint Gauss-Newton step
exactly as test_gpu_joint_step.py takes it (gn_reference by QR, its tolerance).

Cases (gather_case below builds them with joint_graphs.Joint; every shared landmark is seen by exactly two robots, so the separator's
landmark part has exactly the dimension the mix asks for wherever the layout is not dissected — 7 per cylinder, 9 per cube, 3 per
point: the TANGENT dimensions the separator is laid out in; 15 is a cube's stored value, not its coordinate count):

  separator dimension 63 / 64 / 65 / 129      one tile less one, one tile, one tile plus one, two tiles plus one (k_sep_gather works
                                              on 64-row tiles in strips of 16 columns; 65 and 129 leave a strip with one live column)
  2, 3 and 8 robots                           3: no dissection, robots without a partner in a pair; 8: the dissected layout with the
                                              per-half partial sums (split_col) and the hole between the leaves
  with / without relative-pose factors        lambda coordinates behind the landmarks' (18 and 66 of them: one and two lambda tiles)
  bands uncut / cut into three segments       k_sep_extract_b's three kinds of strip; a robot of 30 poses beside one of 100: a band
                                              too short to cut in the same launch
  reversed order                              every case: a robot whose border orders two of its coordinates the other way round than
                                              the separator does (the borders are ordered by first observing block column), asserted
                                              on the host from the layout rule — k_sep_gather then fetches that pair through its
                                              transposed path

and one exact-equality run: the same job as two ranks of four robots over the local-rank rehearsal (every rank sums its robots into
the PACKED exchange layout, the halves are exchanged and unpacked) against one process holding all eight — 1e-12, DESIGN.md 6: the
invariant the fixed summation tree protects.  A restricted robot_mask is not reachable from Python (launch_sep_gather always passes
all robots of the GPU); the ranks' subsets of the robots are what exercises partial sums."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import joint_graphs as jg                                                      # noqa: E402
from test_gpu_joint_step import run_case                                       # noqa: E402

pytestmark = pytest.mark.gpu

NB = 64
MIX = {63: (3, 3, 5), 64: (1, 5, 4), 65: (2, 5, 2), 129: (3, 10, 6)}          # (cylinders, cubes, points) -> 7 a + 9 b + 3 c coordinates


def gather_case(sizes, mix, n_rel=0, seed=31):
    """Robots of `sizes` poses; the n-th shared landmark is seen by the n-th pair of the ring (r, r + 1) — twice by the first robot,
    once by the second — first from pose 12 (block column 1 of the band) when n is even and from pose 1 (block column 0) when n is odd:
    a robot's border, ordered by first observing block column, then runs against the separator's order for many pairs.  Robots of 64
    poses and more get jg.segments_case's points around the cuts (the separator behind a cut must span more than a tile)."""
    J = jg.Joint(sizes, seed=seed, step=0.5 if max(sizes) > 64 else 1.0)
    rng = np.random.default_rng(seed)
    R = J.R
    for r in range(R):
        P = sizes[r]
        if P >= 64:
            for q in sorted({P * i // n for n in (2, 3, 4) for i in range(1, n)}):
                J.point(jg._near(J, r, q, rng), [(r, q - 2), (r, q + 12)])
    pairs = [(0, 1)] if R == 2 else [(a, (a + 1) % R) for a in range(R)]
    n = 0
    for cls, cnt in enumerate(mix):
        for _ in range(cnt):
            a, b = pairs[n % len(pairs)]
            ka = 12 if n % 2 == 0 else 1
            kb = 13 if (n // 2) % 2 == 0 else 2
            jg._add(J, cls, jg._near(J, a, ka, rng), [(a, ka), (a, ka + 1), (b, kb)], rng)
            n += 1
    for i in range(n_rel):
        a = i % R
        b = (a + 1) % R
        ka = (2 * i) % min(sizes)
        J.relative(a, ka, b, ka if i % 2 == 0 else (ka + 3) % min(sizes))
    jg.background(J, rng, every=4)
    return J


def reversed_pairs(J, gid, n_global, sep_off):
    """Per robot, the number of pairs of its shared slots that its border holds in the opposite order to the separator's.  The border's
    order is the layout rule of HostGraph (slots by the first block column of the band in which their coupling row is non-zero — the
    first observing pose's — and by slot index among equals); the separator's is sep_off."""
    slots = []
    for cls in range(3):
        for g in range(n_global[cls]):
            who = [r for r in range(J.R) if g in set(map(int, gid[r][cls]))]
            if len(who) >= 2:
                slots.append((cls, g, who))
    assert len(slots) + 1 == len(sep_off)
    out = []
    for r in range(J.R):
        mine = [i for i, (_, _, who) in enumerate(slots) if r in who]
        cb = {i: 6 * min(k for a, k in J.observers(slots[i][0], slots[i][1]) if a == r) // NB for i in mine}
        local = sorted(mine, key=lambda i: (cb[i], i))
        rank = {i: p for p, i in enumerate(local)}
        out.append(sum(1 for i in mine for j in mine if rank[i] < rank[j] and sep_off[i] > sep_off[j]))
    return out


def _run(gpu, J, ev, monkeypatch=None, seg=None):
    if monkeypatch is not None:
        if seg is None:
            monkeypatch.delenv("SLIDE_SEGMENTS", raising=False)
        else:
            monkeypatch.setenv("SLIDE_SEGMENTS", seg)

    def evidence(r):
        rev = reversed_pairs(J, r.gid, r.info["n_global"], r.info["sep_off"])
        assert max(rev) > 0, rev                 # (the lr < lc path of k_sep_gather is certain to run)
        ev(r)
    _, ratio = run_case(gpu, J, 0, evidence=evidence)
    print(f"[sep-movement] worst scaled_error / tolerance {ratio:.3e}")
    return ratio


@pytest.mark.parametrize("n_rel", [0, 3], ids=["no-lambda", "lambda18"])
@pytest.mark.parametrize("dim", sorted(MIX))
def test_two_robots_separator_tile_edges(gpu, monkeypatch, dim, n_rel):
    """Two robots, bands uncut; the separator's landmark part holds 63 / 64 / 65 / 129 coordinates, without and with 18 lambda
    coordinates behind them."""
    mix = MIX[dim]
    assert sum(n * d for n, d in zip(mix, (7, 9, 3))) == dim
    J = gather_case([24, 24], mix, n_rel=n_rel)

    def ev(r):
        assert r.info["sep_dim"] == dim and not isinstance(r.info["sep_prof"], tuple)
        assert (r.drv.lam_dim if n_rel else 0) == 6 * n_rel
        assert all(sh.graph.segments()[0] == [] for sh in r.shards)
    _run(gpu, J, ev, monkeypatch)


@pytest.mark.parametrize("dim,n_rel", [(65, 0), (129, 11)], ids=["65", "129-lambda66"])
def test_three_robots_no_dissection(gpu, monkeypatch, dim, n_rel):
    """Three robots in a ring of pairs: no dissection (the tree's leaves 3 .. 7 stay empty, every tile pair has one or two candidate
    robots); 129 coordinates with 66 lambda coordinates = two lambda tiles."""
    J = gather_case([20, 20, 20], MIX[dim], n_rel=n_rel)

    def ev(r):
        assert r.info["sep_dim"] == dim and not isinstance(r.info["sep_prof"], tuple)
        assert (r.drv.lam_dim if n_rel else 0) == 6 * n_rel
    _run(gpu, J, ev, monkeypatch)


@pytest.mark.parametrize("n_rel", [0, 11], ids=["no-lambda", "lambda66"])
def test_eight_robots_dissected_split(gpu, monkeypatch, n_rel):
    """Eight robots in a ring of pairs, the layout dissected into the halves 0 .. 3 | 4 .. 7: the pairs (3, 4) and (7, 0) make the top
    block, whose columns take the per-half partial sums (split_col, mask_b); both leaves and the top block are past one tile and end
    inside a tile; the tile rows of leaf b under leaf a's columns are the hole nobody writes."""
    J = gather_case([16] * 8, (8, 32, 8), n_rel=n_rel)

    def ev(r):
        assert isinstance(r.info["sep_prof"], tuple)
        Ta, Tb, used_a, used_b = r.info["sep_prof"][1]
        top = r.info["sep_dim"] - NB * (Ta + Tb)
        assert used_a > NB and used_b > NB and top > NB, (used_a, used_b, top)
        assert used_a % NB and used_b % NB and top % NB
        assert (r.drv.lam_dim if n_rel else 0) == 6 * n_rel
    _run(gpu, J, ev, monkeypatch)


@pytest.mark.parametrize("sizes,dim,n_rel", [([100, 30], 63, 0), ([100, 30], 129, 3)], ids=["63", "129-lambda18"])
def test_cut_bands_beside_a_band_too_short_to_cut(gpu, monkeypatch, sizes, dim, n_rel):
    """A robot of 100 poses, its band cut into three segments (k_sep_extract_b moves the cut poses' column strips, row strips and
    border rows — the shared landmarks' and lambdas' rows among them — into the border), beside a robot of 30 poses whose band stays
    whole: the same launch, sized for the largest."""
    J = gather_case(sizes, MIX[dim], n_rel=n_rel)

    def ev(r):
        assert r.info["sep_dim"] == dim
        for P, sh in zip(sizes, r.shards):
            segs, _ = sh.graph.segments()
            assert len(segs) == (3 if P >= 64 else 0), (P, segs)
    _run(gpu, J, ev, monkeypatch, seg=None)


def test_two_ranks_of_four_robots_equal_one_process(gpu, tmp_path):
    """C8tiny (eight robots on C4's 2 x 4 grid, with relative-pose factors) as two thread ranks of four robots — each rank gathers its
    four robots' partial sums into the packed exchange layout, which is exchanged and unpacked — against one process whose single
    launch sums all eight with the per-half split: the same poses to 1e-12 after three passes."""
    out = str(tmp_path / "r2.json")
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "gpu_scenarios.py"), "rank_threads", out, "C8tiny", "2", "3", "1"],
                       cwd=ROOT, timeout=600)
    assert r.returncode == 0
    z = json.load(open(out))
    assert z["finite"] and len(set(z["n_slots"])) == 1 and z["n_slots"][0] > 0 and z["n_relmeas"] > 0
    assert all(z["owned"])                       # (the ranks split along the dissection: packed partial sums, leaves owned)
    assert z["rel"] < 1e-12, z["rel"]
