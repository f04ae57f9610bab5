"""k_border_apply (chol_kernels.hip): yv -= W x_loc before the band's backward substitution, column by column.

slide_debug_border_apply hands caller-built systems (border_cases.py) to launch_border_apply: the full walk over every border row (one
system; three systems of T = 1, 3, 2 in one grid, whose shorter members' workgroups leave early; a view whose border starts further
down than T), the walk over the per-column 64-bit masks behind the segments' table (34 tile rows: the high word is in use; W non-zero
inside the masks only, x_loc non-zero everywhere), the same with 1e30 in W outside the masks (a wrongly decoded bit adds 1e30 x), and a
table without masks (65 tile rows, msk[0] == 0: the full walk).  Every element against the long-double reference under the a-priori
bound (K + 1 + 4) 2^-53 (|yv| + sum |w| |x|), K = 64 x the column's active tile rows."""
import numpy as np
import pytest

import border_cases as bc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", bc.APPLY_CASES)
def test_border_apply(gpu, name):
    systems = bc.apply_case(name)
    out = gpu.api.debug_border_apply(systems)
    assert len(out) == len(systems)
    worst = 0.0
    for i, (d, got) in enumerate(zip(systems, out)):
        ref, bound = bc.apply_reference(d)
        assert got.shape == (d["T"] * bc.NB,)
        ratio = np.abs(got.astype(bc.LD) - ref).astype(np.float64) / bound
        col = int(np.argmax(ratio))
        assert np.all(np.isfinite(got)) and ratio[col] <= 1.0, (f"system {i} (T {d['T']}, nbr {d['nbr']}), column {col}: |err| "
                                                               f"{float(abs(got[col] - ref[col])):.3e}, bound {bound[col]:.3e}")
        worst = max(worst, float(ratio[col]))
    print(f"[border-apply] {name}: worst |err| / bound {worst:.3e}")


def test_border_apply_refuses(gpu):
    """An ld the kernel would read beyond, a mask bit at or above nbr (a tile row that is not there): SLIDE_ERR_INVALID."""
    rng = np.random.default_rng(5)
    d = bc.make_apply_system(rng, 2, 3)
    short = dict(d, ld=d["ld"] - 64, S=np.zeros((d["ld"] - 64) * 2 * bc.NB))
    tab = bc.make_segtab(2, 3, [2], [[0, 0, 0, 0]])
    tab[-2] |= 1 << 3
    for bad in (short, dict(d, segtab=tab)):
        with pytest.raises(gpu.api.SlideError) as e:
            gpu.api.debug_border_apply([bad])
        assert e.value.code == -1
