"""The selected inverse of the resident factor (k_sinv_prep, k_sinv_tile<false / true> of cov_kernels.hip) tile by tile.

The marginals, the information gain and every Mahalanobis gate read this pass, and the suite reached it only through whole queries on
graphs of at most four tiles under a conditioning-scaled tolerance.  Here slide_debug_selected_inverse hands caller-built factors
(cov_cases.py: known L0, long-double Winv, NaN sentinels wherever the kernels must not read) to launch_selected_inverse itself: every
profile case (one tile, dense, band 0, bands 2 and 3, a decoupled chain, a staircase whose columns are shorter than the band) with the
padded and the minimal leading dimension.  Stage 0 (k_sinv_prep alone) is held to bound (b), stage 1 to bound (a) — every tile as the
product of what the device itself read — and to (c) against the long-double Sigma.  Sg and Z are pre-filled with a second NaN payload:
every tile of the profile must be fully written and everything else — tiles outside the profile, the upper tiles, the rows from T*64
on, Z outside the profile — must keep the pre-fill's bits; S, Ld and Winv come back unchanged; the diagonal tiles are symmetric bit for
bit.

Worst |err| / bound observed on an MI355X (profiles/cov_kernels_bounds.txt): (b) Z 0.115 (band2), (b) L_kk^-T L_kk^-1 0.107 (decoupled),
(a) 0.151 (decoupled), (c) 0.140 (one, band3; 0.125 = the restatement's own error elsewhere).  No kernel needed a change."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cov_cases as cc                                                         # noqa: E402
from cov_cases import NB                                                       # noqa: E402

pytestmark = pytest.mark.gpu


def _report(what, **ratios):
    print(f"[selected-inverse] {what}: " + "  ".join(f"{k} {v:.3e}" for k, v in ratios.items()))


def _run(api, m, ld, stage, explicit_prof=True):
    f = cc.factor_layout(m, ld, explicit_prof=explicit_prof)
    pre = np.full(ld * m["Tc"] * NB, cc.OUT_NAN)
    out = api.debug_selected_inverse(f, pre, pre, stage=stage)
    assert cc.same_bits(out["S"], f["S"]) and cc.same_bits(out["Ld"], f["Ld"]) and cc.same_bits(out["Winv"], f["Winv"]), "the factor was written"
    return out


def _check_writes(m, ld, out, stage):
    """Every tile of the profile fully written with numbers, everything else as pre-filled; diagonal tiles symmetric bit for bit."""
    ms, mz = cc.written_masks(m, ld)
    Sg, Z = cc.view(out["Sg"], ld), cc.view(out["Z"], ld)
    if stage == 0:                                    # (k_sinv_prep writes the diagonal tiles and Z only)
        ms = np.zeros_like(ms)
        for k in range(m["Tc"]):
            ms[k * NB:(k + 1) * NB, k * NB:(k + 1) * NB] = True
    assert not np.isnan(Sg[ms]).any(), "a NaN inside the profile of Sg: a tile not fully written, or a read outside the contract"
    assert not np.isnan(Z[mz]).any(), "a NaN inside the profile of Z"
    pre = np.full(1, cc.OUT_NAN)
    assert cc.same_bits(Sg[~ms], np.broadcast_to(pre, ((~ms).sum(),))), "Sg was written outside the profile's lower tiles"
    assert cc.same_bits(Z[~mz], np.broadcast_to(pre, ((~mz).sum(),))), "Z was written outside (i, k), k < i <= prof[k]"
    for k in range(m["Tc"]):
        t = cc.tile(out["Sg"], ld, k, k)
        assert cc.same_bits(t, t.T), ("diagonal tile not symmetric bit for bit", k)


@pytest.mark.parametrize("padded", [True, False], ids=["ld_padded", "ld_minimal"])
@pytest.mark.parametrize("name", cc.PROFILE_CASES)
def test_profile_case(gpu, name, padded):
    m = cc.profile_model(name)
    ld = cc.lds_of(m["Tc"], padded)
    prep, full = _run(gpu.api, m, ld, 0), _run(gpu.api, m, ld, 1)
    _check_writes(m, ld, prep, 0)
    _check_writes(m, ld, full, 1)
    assert cc.same_bits(prep["Z"], full["Z"]), "Z differs between the prep launch alone and the full pass"
    rz, rp = cc.check_b(m, ld, prep["Sg"], prep["Z"])
    ra = cc.check_a(m, ld, full["Sg"], full["Z"], prep["Sg"])
    rc = cc.check_c_sigma(m, ld, full["Sg"])
    _report(f"{name} ld {ld}", b_Z=rz, b_P=rp, a=ra, c=rc)
    assert rz <= 1 and rp <= 1, "bound (b): k_sinv_prep"
    assert ra <= 1, "bound (a): a tile is not the product of what the device read"
    assert rc <= 1, "bound (c): Sigma against the long-double reference"
    if name in ("one", "diag3"):                      # no column has rows below it: no tile launch, stage 1 = stage 0
        assert cc.same_bits(prep["Sg"], full["Sg"])


def test_dense_profile_null_or_explicit(gpu):
    """prof = NULL and the explicit [4] * 5 give the same bits."""
    m = cc.profile_model("dense5")
    ld = cc.lds_of(5, True)
    a, b = _run(gpu.api, m, ld, 1, explicit_prof=False), _run(gpu.api, m, ld, 1, explicit_prof=True)
    assert cc.same_bits(a["Sg"], b["Sg"]) and cc.same_bits(a["Z"], b["Z"])


@pytest.mark.parametrize("c0,c1", [(0, 4), (4, 8)])
def test_decoupled_halves_alone(gpu, c0, c1):
    """Block column 3 couples to nothing below it: each half equals, bit for bit, the same four columns run as a system of their own — a
    workgroup that read beyond i1 would show."""
    m = cc.profile_model("decoupled")
    sub = cc.sub_model(m, c0, c1)
    ld, lds = cc.lds_of(8, True), cc.lds_of(4, False)
    whole, alone = _run(gpu.api, m, ld, 1), _run(gpu.api, sub, lds, 1)
    for k in range(4):
        for i in [k] + sub["rows"][k]:
            assert cc.same_bits(cc.tile(whole["Sg"], ld, c0 + i, c0 + k), cc.tile(alone["Sg"], lds, i, k)), ("Sg", i, k)
            if i > k:
                assert cc.same_bits(cc.tile(whole["Z"], ld, c0 + i, c0 + k), cc.tile(alone["Z"], lds, i, k)), ("Z", i, k)


def test_refusals_launch_nothing(gpu):
    """What the launcher does not define is refused with the buffers untouched; a defined case still runs afterwards."""
    api = gpu.api
    m = cc.profile_model("two")
    ld = cc.lds_of(2, True)
    f = cc.factor_layout(m, ld)
    pre = np.full(ld * 2 * NB, cc.OUT_NAN)
    bad = [dict(f, prof=[1, 0]), dict(f, prof=[0, 2]), dict(f, prof=[-1, 1]), dict(f, ld=ld - 1, S=f["S"][:(ld - 1) * 2 * NB]),
           dict(f, ld=NB, S=f["S"][:NB * 2 * NB])]
    for g in bad:
        with pytest.raises(api.SlideError) as e:
            api.debug_selected_inverse(g, pre[:g["ld"] * 2 * NB], pre[:g["ld"] * 2 * NB])
        assert e.value.code == -1
    with pytest.raises(api.SlideError) as e:
        api.debug_selected_inverse(f, pre, pre, stage=2)
    assert e.value.code == -1
    with pytest.raises(api.SlideError) as e:
        api.debug_selected_inverse(dict(S=np.zeros(0), ld=ld, T=0, Ld=np.zeros(0), Winv=np.zeros(0), prof=None), np.zeros(0), np.zeros(0))
    assert e.value.code == -1
    out = _run(api, m, ld, 1)
    assert cc.check_c_sigma(m, ld, out["Sg"]) <= 1
