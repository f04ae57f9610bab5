"""The numpy robust step the GPU tests compare against (tests/robust_cases.py), on its own: the four weight functions at their
edges, and the planted-closure scenario, where the reference alone has to tell six true closures from two gross false ones.  No
product code runs here."""
import numpy as np
import pytest

import robust_cases as rc

C = rc.DEFAULT


def test_weights_at_zero():
    for kind in rc.KINDS.values():
        assert rc.weight(kind, 0.0, 0.0) == 1.0


def test_weights_at_the_kink_from_both_sides():
    k = C[rc.HUBER]
    below, above = np.nextafter(k, 0.0), np.nextafter(k, np.inf)
    assert rc.weight(rc.HUBER, 0.0, below) == 1.0 and rc.weight(rc.HUBER, 0.0, k) == 1.0
    assert rc.weight(rc.HUBER, 0.0, above) == k / above < 1.0
    assert rc.weight(rc.HUBER, 0.0, 2 * k) == 0.5
    phi = 4.0                                           # (s = 2 exactly: s^2 = Phi has no rounding of its own)
    assert rc.weight(rc.DCS, phi, 2.0) == 1.0 and rc.weight(rc.DCS, phi, np.nextafter(2.0, 0.0)) == 1.0
    s = np.nextafter(2.0, np.inf)
    assert rc.weight(rc.DCS, phi, s) == (2 * phi / (phi + s * s)) ** 2 < 1.0
    assert np.isclose(rc.weight(rc.DCS, phi, s), 1.0, rtol=0, atol=1e-15)      # (continuous at the kink)
    assert rc.weight(rc.DCS, 0.0, np.sqrt(3.0)) == pytest.approx(0.25, rel=1e-15)
    # the two smooth losses at s = their parameter
    assert rc.weight(rc.CAUCHY, 0.0, C[rc.CAUCHY]) == 0.5
    assert rc.weight(rc.GEMAN_MCCLURE, 0.0, C[rc.GEMAN_MCCLURE]) == 0.25


def test_weights_far_out_and_the_clamp():
    s = 1e6
    assert rc.weight(rc.HUBER, 0.0, s) == C[rc.HUBER] / s                      # 1.345e-6: above the floor
    assert rc.weight(rc.CAUCHY, 0.0, s) == rc.W_MIN                            # 1e-14 unclamped
    assert rc.weight(rc.GEMAN_MCCLURE, 0.0, s) == rc.W_MIN                     # 1e-24 unclamped
    assert rc.weight(rc.DCS, 0.0, s) == rc.W_MIN                               # 4e-24 unclamped
    assert rc.weight(rc.HUBER, 0.0, np.inf) == rc.W_MIN
    assert (rc.weight(rc.CAUCHY, 0.0, np.array([0.0, 0.1, 1e6])) == [1.0, 0.5, rc.W_MIN]).all()


# Measured once (this file, seed 21, 8 steps, chart 0): RMS position error against the ground truth 6.1 mm under Geman-McClure and
# 6.3 mm under DCS (the odometry's and the closures' own noise), 1.49 m without a loss — 240 times as much.
ROBUST_ERR_MAX = 0.02
PLAIN_RATIO_MIN = 50.0


@pytest.fixture(scope="module")
def plain():
    r = rc.planted_reference(0)
    return rc.pose_error(r["ref"], r["values"], r["T"])


@pytest.mark.parametrize("kind", [rc.GEMAN_MCCLURE, rc.DCS], ids=["geman_mcclure", "dcs"])
def test_planted_closures(kind, plain):
    """40 poses, two laps of a circle, odometry noise, 6 true closures and 2 false ones (3.6 m and 1 rad off): after 8 reweighted
    steps of the numpy reference the false closures have weight < 0.1 and the true ones > 0.9.  RMS position error against the
    ground truth: 6.1 mm (Geman-McClure, c = 30) and 6.3 mm (DCS, Phi = 900); the same graph without a loss, same steps: 1.49 m.
    Asserted: robust <= 20 mm, and the plain solve at least 50 times worse."""
    r = rc.planted_reference(kind)
    nt = len(rc.TRUE_CLOSURES)
    w = r["w"]
    assert len(w) == nt + len(rc.FALSE_CLOSURES)
    s0 = np.sqrt(rc.whitened_norms2(r["ref"])[r["sel"]])
    assert (s0[:nt] < 10).all() and (s0[nt:] > 3000).all()        # (a few sigmas of drift; gross)
    assert (w[:nt] > 0.9).all() and (w[nt:] < 0.1).all(), w
    err = rc.pose_error(r["ref"], r["values"], r["T"])
    print(f"[robust-reference] kind {kind}: weights {np.round(w, 6)}, pose error {err:.4e} m, plain {plain:.4e} m")
    assert err <= ROBUST_ERR_MAX
    assert plain >= PLAIN_RATIO_MIN * err
