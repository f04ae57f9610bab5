"""The border product (k_border_syrk, k_border_syrk_reduce, k_border_syrk_reduce2 of chol_kernels.hip) tile by tile, in every launch shape.

The exact joint passes reach this code only through whole Gauss-Newton steps under a conditioning-scaled tolerance, on borders of one to
three tiles and in whatever launch shape the layout picks.  Here slide_debug_border_product hands caller-built systems (border_cases.py)
to the passes' own launchers — plain (ib, jb, system) grid or job table, first columns, the segments' table, split K with guarded scratch,
the fused two-system launch, views (b0 > T), a separate source block — and every element is compared with a long-double reference under
the a-priori bound of border_cases.py: |got - ref| <= (K + ks + 4) 2^-53 (|C| + sum |a| |b|).  Where the code promises the same bits
(table order, grid against table, a system alone against the same system in a batch, the prefetch depth SLIDE_SYRK_RD, the fused launch
against two single ones) the comparison is bit for bit.  Every run also checks what must not be written: the tiles above the diagonal,
bord beyond tile row nbr and tile column nbr - 1, S, and (inside the hook) one guard tile on either side of the split-K scratch.

The question of the idle half (test_prefilled_scratch): a table launch never writes rows 32 .. 63 of a right-hand-side row tile's partial,
the reductions add them all the same, and HostGraph reuses one scratch buffer under different ks, i.e. different indexings.  Observed on
an MI355X with the scratch pre-filled with 3.0: rows 0 .. 31 of every tile and all of every other tile come out bit-identical to the
zeroed run; rows 32 .. 63 of the right-hand-side row tiles receive 3.0 once per non-empty chunk behind the first (the test pins exactly
that).  Those rows have no reader: k_lam_prepare, k_sep_top_add and k_chol_extract_y read row 0 of the tile only, and the step kernels
treat the tile's rows independently of each other — so this is no defect, but neither are those rows "zero and stay zero"."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import border_cases as bc                                                      # noqa: E402
from border_cases import NB                                                    # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = -1                                                                   # SLIDE_ERR_INVALID


def _report(family, ratio):
    print(f"[border-product] {family}: worst |err| / bound {ratio:.3e}")


def _blk(d, flat):
    return flat.reshape(d["bord_cols"], d["ldb"])


def _launch(api, systems, table, order=None, **kw):
    """The systems through the plain grid (table False) or a job table (system-major, or permuted by `order`)."""
    jobs = None
    if table:
        jobs = bc.job_table(systems, kw.get("jb_end"))
        if order is not None:
            jobs = [jobs[i] for i in order]
    return api.debug_border_product(systems, jobs=jobs, **kw)


def _check(d, out, ref, bound, given, jb_end=None):
    """One system's result: inside the bound on the lower tiles, bit-identical everywhere else, S as it was.  Returns worst err / bound."""
    got, where = _blk(d, out["bord"]), bc.lower_tile_mask(d, jb_end)
    assert bc.same_bits(out["S"], d["S"]), "S was written"
    assert bc.same_bits(got[~where], given[~where]), "written above the diagonal or beyond the border block"
    ratio = bc.worst_ratio(got, ref, bound, where)
    if ratio > 1.0:
        err = np.abs(got.astype(bc.LD) - ref).astype(np.float64)
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0) * where
        col, row = np.unravel_index(np.argmax(r), r.shape)
        raise AssertionError(f"tile ({row // NB}, {col // NB}) element ({row % NB}, {col % NB}): |err| {err[col, row]:.3e}, bound {bound[col, row]:.3e}")
    return ratio


@pytest.fixture(scope="module")
def refs():
    """Case name -> (systems, launch keywords, [(ref, bound, given)]): computed once, shared, never modified."""
    done = {}

    def get(name):
        if name not in done:
            systems, kw, _ = bc.product_case(name)
            done[name] = (systems, kw, [bc.product_reference(d, ks=kw.get("ks", 1), jb_end=kw.get("jb_end")) for d in systems])
        return done[name]
    return get


def _both_shapes(gpu, refs, name, family):
    """A one-system case on the plain grid and on a table: both inside the bound, and bit-identical to each other."""
    systems, kw, rf = refs(name)
    outs = [_launch(gpu.api, systems, table, **kw)[0] for table in (False, True)]
    worst = max(_check(systems[0], o, *rf[0]) for o in outs)
    assert bc.same_bits(outs[0]["bord"], outs[1]["bord"]), "the plain grid and the job table differ in bits"
    _report(f"{family} {name}", worst)


# ---- sum length, first columns, segments ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,nbr", bc.SUM_LENGTH)
def test_sum_length(gpu, refs, T, nbr):
    """T = 1 is 16 k-steps: one round of the prefetch ring at depth 16, the prologue alone holds 15 of them."""
    _both_shapes(gpu, refs, f"sum:{T}:{nbr}", "sum length")


@pytest.mark.parametrize("name", ["bfirst", "bfirst_src", "bfirst_view"])
def test_first_columns(gpu, refs, name):
    """The sum starts at max(bfirst[ib], bfirst[jb]); a row that starts at T has empty sums: its tiles are untouched (bound 0: bit for
    bit), or copied from bord_src; one system's border starts further down than T."""
    _both_shapes(gpu, refs, name, "bfirst")


@pytest.mark.parametrize("name", ["segtab", "segtab_src"])
def test_segments(gpu, refs, name):
    """Three segments of 3, 1 and 3 block columns: the prefetch ring crosses the one-column segment, one row is inactive there, one
    pair shares no segment (its tile is rewritten as it was, or copied)."""
    _both_shapes(gpu, refs, name, "segtab")


# ---- split K ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [f"split:{T}:{ks}" for T, ks in bc.SPLIT_K] + ["split_bfirst", "split_view"])
def test_split_k(gpu, refs, name):
    """(5, 4) and (9, 8) leave trailing chunks empty; with first columns the tiles' chunk lengths differ and one row's second chunk is
    empty: the kernel and the reduction must skip by the same rule."""
    _both_shapes(gpu, refs, name, "split K")


def test_split_k_stops_at_jb_end(gpu, refs):
    """Tile columns >= jb_end are neither in the table nor reduced: bit-identical (they are outside _check's mask)."""
    systems, kw, rf = refs("split_jb_end")
    out = _launch(gpu.api, systems, True, **kw)[0]
    _report("split K jb_end", _check(systems[0], out, *rf[0], jb_end=kw["jb_end"]))


# ---- the fused two-system launch --------------------------------------------------------------------------------------------------

def _fused_and_singles(api, ks=1, ks_sys=None):
    pair = bc.fused_systems()
    each = ks_sys if ks_sys is not None else (ks, ks)
    singles = [_launch(api, [d], True, ks=k)[0] for d, k in zip(pair, each)]
    fused = _launch(api, pair, True, ks=ks, ks_sys=ks_sys, fuse_add=True)
    return pair, each, singles, fused


@pytest.mark.parametrize("ks,ks_sys", [(1, s) for s in bc.FUSED] + [(2, None)], ids=lambda v: str(v))
def test_fused_two_systems(gpu, ks, ks_sys):
    """System 0's block after the fused launch = (system 0 alone, cut its way) + (system 1 alone, cut its way) as a + b in float64, bit
    for bit; ks_sys = (1, 3): one system unsplit inside a split launch."""
    pair, each, singles, fused = _fused_and_singles(gpu.api, ks, ks_sys)
    worst = 0.0
    for d, k, o in zip(pair, each, singles):
        worst = max(worst, _check(d, o, *bc.product_reference(d, ks=k)))
    _report(f"fused, the single launches ks {tuple(each)}", worst)
    where = bc.lower_tile_mask(pair[0])
    want = _blk(pair[0], pair[0]["bord"]).copy()
    want[where] = _blk(pair[0], singles[0]["bord"])[where] + _blk(pair[1], singles[1]["bord"])[where]
    assert bc.same_bits(_blk(pair[0], fused[0]["bord"]), want), "the fused launch is not the sum of the two single ones, bit for bit"
    other = _blk(pair[1], fused[1]["bord"])
    assert bc.same_bits(other[~where], _blk(pair[1], pair[1]["bord"])[~where])
    assert all(bc.same_bits(o["S"], d["S"]) for o, d in zip(fused, pair))


# ---- the same bits ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["eight", "segtab", "split:5:4"])
def test_table_order(gpu, refs, name):
    """The workgroups' order is the dispatcher's business: a reversed and a seeded random table give the same bits, and so does a
    launch with idle LDS that bounds the workgroups per CU."""
    if name == "eight":
        systems, kw = bc.eight_systems(), {}
    else:
        systems, kw, _ = refs(name)
    n = len(bc.job_table(systems))
    base = _launch(gpu.api, systems, True, **kw)
    for order in (list(range(n))[::-1], [int(i) for i in np.random.default_rng(11).permutation(n)]):
        out = _launch(gpu.api, systems, True, order=order, **kw)
        assert all(bc.same_bits(a["bord"], b["bord"]) for a, b in zip(base, out))
    # nor is the residency: 32 KB of idle LDS per workgroup (SLIDE_SYRK_LDS) changes no bit
    out = _launch(gpu.api, systems, True, lds_pad=32768, **kw)
    assert all(bc.same_bits(a["bord"], b["bord"]) for a, b in zip(base, out))


@pytest.mark.parametrize("table", [False, True], ids=["grid", "table"])
def test_eight_systems_each_as_alone(gpu, table):
    """Eight different systems in one launch: each inside the bound and bit-identical to itself launched alone (a workgroup that read
    system r's T with system r + 1's nbr would show)."""
    systems = bc.eight_systems()
    outs = _launch(gpu.api, systems, table)
    worst = 0.0
    for d, o in zip(systems, outs):
        worst = max(worst, _check(d, o, *bc.product_reference(d)))
        alone = _launch(gpu.api, [d], table)[0]
        assert bc.same_bits(alone["bord"], o["bord"]), f"T {d['T']}, nbr {d['nbr']}: differs from itself launched alone"
    _report(f"eight systems, {'table' if table else 'grid'}", worst)


RD_CASES = ["segtab", "split:5:4"]


def _rd_digests(api):
    """Per case of RD_CASES and launch shape: worst err / bound and a digest of the result's bits."""
    out = []
    for name in RD_CASES:
        systems, kw, _ = bc.product_case(name)
        rf = bc.product_reference(systems[0], ks=kw.get("ks", 1))
        for table in (False, True):
            o = _launch(api, systems, table, **kw)[0]
            out.append([_check(systems[0], o, *rf), hashlib.sha256(o["bord"].tobytes()).hexdigest()])
    return out


def _child(rd):
    """A fresh process: launch_syrk_kernel reads SLIDE_SYRK_RD once into a static."""
    e = dict(os.environ)
    e["SLIDE_SYRK_RD"] = str(rd)
    r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), str(rd)], cwd=ROOT, env=e, timeout=300, capture_output=True, text=True)
    sys.stdout.write(r.stdout[-2000:])
    sys.stderr.write(r.stderr[-2000:])
    assert r.returncode == 0, r.returncode
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_prefetch_depth_same_bits(gpu):
    """border_syrk_body<4>, <8> and <16>: 'same order of the sum: same bits' on the segments' case and on a split-K case, grid and
    table — one child process per depth, one at a time."""
    runs = {rd: _child(rd) for rd in (4, 8, 16)}
    for rd, res in runs.items():
        _report(f"SLIDE_SYRK_RD={rd}", max(r for r, _ in res))
        assert [h for _, h in res] == [h for _, h in runs[16]], f"SLIDE_SYRK_RD={rd} differs in bits from 16"
    if "SLIDE_SYRK_RD" not in os.environ:
        assert [h for _, h in _rd_digests(gpu.api)] == [h for _, h in runs[16]], "the default depth is not 16"


# ---- the idle half of a right-hand-side row tile's partials --------------------------------------------------------------------------

PREFILL = 3.0


def _chain(start, times):
    v = start.copy()
    for _ in range(times):
        v = v + PREFILL
    return v


def _idle_half(d):
    """Rows 32 .. 63 of the right-hand-side row tiles, (bord_cols, ldb)."""
    m = np.zeros((d["bord_cols"], d["ldb"]), bool)
    m[:d["nbr"] * NB, d["nbr"] * NB + 32:(d["nbr"] + 1) * NB] = True
    return m


@pytest.mark.parametrize("name", ["split:5:4", "split:9:8", "split:5:2"])
def test_prefilled_scratch_split_k(gpu, refs, name):
    """Split K with the scratch pre-filled with 3.0 in place of zero.  Plain grid: every partial that is read was written — nothing
    changes.  Table: rows 32 .. 63 of the right-hand-side row tile's partials are never written and the reduction adds them: the
    pre-fill arrives there once per non-empty chunk behind the first, and nowhere else."""
    systems, kw, _ = refs(name)
    d = systems[0]
    zero = {t: _launch(gpu.api, systems, t, **kw)[0] for t in (False, True)}
    fill = {t: _launch(gpu.api, systems, t, prefill=PREFILL, **kw)[0] for t in (False, True)}
    assert bc.same_bits(zero[False]["bord"], fill[False]["bord"]), "plain grid: a partial was read that nobody wrote"
    idle = _idle_half(d)
    z, f = _blk(d, zero[True]["bord"]), _blk(d, fill[True]["bord"])
    assert bc.same_bits(z[~idle], f[~idle]), "the pre-fill reached row 0 .. 31 of a right-hand-side tile or another tile"
    chunks = sum(c is not None for c in bc.chunk_ranges(d["T"], 0, kw["ks"]))
    got = np.unique(f[idle] - z[idle])
    print(f"[border-product] pre-filled scratch, {name}, table: rows 32 .. 63 of the right-hand-side tiles change by {got.tolist()} "
          f"({chunks} non-empty chunks)")
    assert bc.same_bits(f[idle], _chain(z[idle], chunks - 1)), "rows 32 .. 63: not the pre-fill once per later non-empty chunk"


@pytest.mark.parametrize("ks_sys", bc.FUSED, ids=str)
def test_prefilled_scratch_fused(gpu, ks_sys):
    """The same for the fused launch: each system's idle half takes the pre-fill once per later non-empty chunk of its own."""
    pair = bc.fused_systems()
    zero = _launch(gpu.api, pair, True, ks_sys=ks_sys, fuse_add=True)
    fill = _launch(gpu.api, pair, True, ks_sys=ks_sys, fuse_add=True, prefill=PREFILL)
    idle = _idle_half(pair[0])
    z, f = _blk(pair[0], zero[0]["bord"]), _blk(pair[0], fill[0]["bord"])
    assert bc.same_bits(z[~idle], f[~idle]), "the pre-fill reached row 0 .. 31 of a right-hand-side tile or another tile"
    # (A + its partials) + (B + its partials), each in chunk order; the idle halves of A and B themselves are as given
    ca, cb = _blk(pair[0], pair[0]["bord"])[idle], _blk(pair[1], pair[1]["bord"])[idle]
    na, nb = (sum(c is not None for c in bc.chunk_ranges(d["T"], 0, k)) - 1 for d, k in zip(pair, ks_sys))
    print(f"[border-product] pre-filled scratch, fused ks_sys {ks_sys}: rows 32 .. 63 of the right-hand-side tiles change by "
          f"{np.unique(f[idle] - z[idle]).tolist()} ({na} + {nb} later chunks)")
    assert bc.same_bits(f[idle], _chain(ca, na) + _chain(cb, nb))


# ---- what the launchers do not define ---------------------------------------------------------------------------------------------

def _refused(api, systems, table=True, **kw):
    with pytest.raises(api.SlideError) as e:
        _launch(api, systems, table, **kw)
    assert e.value.code == INVALID, e.value


def test_refused_combinations(gpu):
    api = gpu.api
    rng = np.random.default_rng(3)
    one = lambda **kw: bc.make_system(rng, 2, 2, **kw)
    seg = bc.make_segtab(2, 2, [1, 2], [[0, 0, 0], [1, 1, 1]])
    for table in (False, True):
        _refused(api, [one(segtab=seg)], table, ks=2)                                    # split K with a segments' table
        _refused(api, [one(), one()], table, ks=2)                                       # split K, two systems, not fused
        _refused(api, [one(ld_pad=1)], table)                                            # an odd ld
        _refused(api, [one(rows_beyond=NB + 1)], table)                                  # an odd ldb
        short = one(ld_pad=0)
        short["ld"] -= 2
        short["S"] = np.zeros(short["ld"] * short["T"] * NB)
        _refused(api, [short], table)                                                    # ld < (B0 + nbr + 1) * 64
    _refused(api, [one()], ks=2, fuse_add=True)                                          # fused: n != 2
    _refused(api, [one(), one(), one()], ks=2, fuse_add=True)
    _refused(api, [one(), bc.make_system(rng, 2, 3)], ks=2, fuse_add=True)               # fused: unequal nbr
    _refused(api, [one(), one(bfirst=[0, 1, 0])], ks=2, fuse_add=True)                   # fused: a bfirst
    _refused(api, [one(segtab=seg), one()], ks=2, fuse_add=True)                         # fused: a segments' table
    with pytest.raises(api.SlideError) as e:                                             # a job names system 1 of 1
        api.debug_border_product([one()], jobs=[0, 1 << 20])
    assert e.value.code == INVALID
    with pytest.raises(api.SlideError) as e:                                             # the fused launch has no plain grid
        api.debug_border_product([one(), one()], ks=2, fuse_add=True)
    assert e.value.code == INVALID
    # and what IS defined still runs after all the refusals
    d = one()
    _check(d, _launch(api, [d], True)[0], *bc.product_reference(d))


if __name__ == "__main__":
    import torch  # noqa: F401   (torch before the product library: tests/conftest.py)
    torch.zeros(1, device="cuda:0")
    import slide_slam_amd as s
    assert os.environ.get("SLIDE_SYRK_RD") == sys.argv[1]
    print(json.dumps(_rd_digests(s.api)))
