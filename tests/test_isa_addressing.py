"""How the batched pass's kernels address memory, read from their gfx950 assembly (tools/isa_addressing.py; CPU only, hipcc
cross-compiles).  A kernel that takes the graphs as a table in memory (const GraphDev* Gs) reads its pointers from memory; were they
plain pointers, every access through them would be a flat_* instruction, which counts on the vector-memory AND the LDS counter, so
that every wait drains every outstanding load.  graph_dev.hpp declares the views' pointer members as global pointers for
the device: no such kernel of solver_kernels.hip, pcg_kernels.hip or obs_gate_kernels.hip may contain a flat_load, flat_store or
flat_atomic, and none may use scratch."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import isa_addressing as isa                                                   # noqa: E402

FILES = ["solver_kernels.hip", "pcg_kernels.hip", "obs_gate_kernels.hip"]

pytestmark = pytest.mark.skipif(not isa.hipcc_available(), reason="hipcc is not installed")


@pytest.fixture(scope="module")
def rows():
    """One compile of the three files (side by side), every kernel that takes a pointer to GraphDev."""
    with ThreadPoolExecutor(len(FILES)) as ex:
        return [r for part in ex.map(lambda f: isa.table([f]), FILES) for r in part]


def test_parser_counts_what_it_is_given():
    asm = """
\t.protected\t_Z1kPKN2sl8GraphDevE
_Z1kPKN2sl8GraphDevE:                   ; @_Z1kPKN2sl8GraphDevE
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tflat_load_dword v1, v[2:3]
\tglobal_load_dwordx2 v[4:5], v0, s[0:1]
\ts_waitcnt vmcnt(0) lgkmcnt(0)
\tglobal_load_dword v6, v0, s[0:1]
\tglobal_load_dword v7, v0, s[0:1] offset:4
\ts_waitcnt vmcnt(1)
\tds_write_b32 v0, v6
\ts_waitcnt vmcnt(0)
\tflat_atomic_add v0, v[2:3], v7
\tglobal_store_dword v0, v7, s[0:1]
\ts_endpgm
.Lfunc_end0:
\t.size\t_Z1kPKN2sl8GraphDevE, .Lfunc_end0-_Z1kPKN2sl8GraphDevE
; NumVgprs: 8
; ScratchSize: 16
; Occupancy: 8
\t.amdhsa_kernel _Z1kPKN2sl8GraphDevE
\t.end_amdhsa_kernel
"""
    (name, c), = isa.parse(asm).items()
    assert name == "_Z1kPKN2sl8GraphDevE"
    assert (c["flat"], c["flat_load"], c["flat_store"], c["flat_atomic"], c["glob"], c["ds"]) == (2, 1, 0, 1, 4, 1)
    assert (c["wait_full"], c["wait_vm0"], c["wait_partial"]) == (1, 1, 1)
    assert (c["vgprs"], c["scratch"], c["waves"]) == (8, 16, 8)


def test_the_batched_kernels_are_found(rows):
    names = {isa.short(r["kernel"]) for r in rows}
    for k in ("k_relin_b", "k_lin_lf_b", "k_lin_lf_robust_b", "k_landmark_b<3>", "k_pose_b", "k_schur_b", "k_schur_lb", "k_backsub_b<0>",
              "k_backsub_sep_b", "k_border_clear_b", "k_sep_extract_b", "k_estimate_b", "k_ghost_refresh_local", "k_robust_reweight_b",
              "k_pcg_tl_symv", "k_pcg_cross", "k_joint_obs_gate_lin"):
        assert k in names, k
    assert all(isa.GRAPH_ARG.search(r["kernel"]) for r in rows)
    # (the counts are read: every one of these kernels touches global memory, and the resource comments were found)
    assert all(r["glob"] > 0 and r["vgprs"] is not None and r["scratch"] is not None and r["waves"] is not None for r in rows)


def test_no_flat_access_and_no_scratch(rows):
    bad = [(isa.short(r["kernel"]), r["flat_load"], r["flat_store"], r["flat_atomic"], r["scratch"]) for r in rows
           if r["flat_load"] or r["flat_store"] or r["flat_atomic"] or r["scratch"]]
    assert not bad, f"(kernel, flat_load, flat_store, flat_atomic, scratch bytes): {bad}"


def test_the_waits_leave_loads_in_flight(rows):
    """With global loads the compiler waits for vmcnt(N), N > 0, where later loads are not needed yet; flat loads allowed no such
    wait.  The three longest assembly kernels of an exact joint pass keep three waves per SIMD."""
    by = {isa.short(r["kernel"]): r for r in rows}
    for k in ("k_schur_lb", "k_landmark_b<3>", "k_lin_lf_b", "k_pose_b", "k_backsub_sep_b"):
        assert by[k]["wait_partial"] > 0, (k, by[k])
    for k in ("k_schur_lb", "k_landmark_b<3>", "k_lin_lf_b"):
        assert by[k]["waves"] >= 3, (k, by[k])
