"""Caller-built FACTORS for the tests of the kernels that read the factor (test_gpu_selected_inverse.py, test_gpu_multi_solve.py,
test_gpu_joint_selected_inverse.py, test_cov_cases_reference.py): k_sinv_prep / k_sinv_tile, k_jsinv_prep / k_jsinv_tile, k_sub_fwd /
k_sub_bwd, k_gram, k_cov_fwd / k_cov_gram.  The operation is the one the reference project delegates to GTSAM (isam->marginalCovariance,
backend/sloam/src/factorgraph/graph.cpp:314-323): entries of (L D L^T)^-1 and solves with L.

A factor is chol_cases._system's L0 (diagonals in [1, 2], off-diagonal entries about 0.03) written into the layout check_system documents:
S column-major with L(i, k) in tile (i, k) for k < i <= prof[k], Ld with the sub-diagonal 16x16 blocks of L_kk, Winv with the long-double
inverses of its diagonal 16x16 blocks rounded to double.  Every place the kernels must never read holds a quiet NaN of a fixed payload
(IN_NAN): S's diagonal tiles, its tiles outside the profile (zero instead for k_cov_fwd, which walks the dense column), the upper tiles,
the rows between T*64 and ld, the diagonal and upper 16x16 blocks of Ld.  Output buffers are pre-filled with a second payload (OUT_NAN).

The model every function here works on ("m") is the joint form, of which the one-store factor is the special case Tb = Tc = Trow, neg0 =
Tc, rows[k] = k+1 .. prof[k]: Tc factor columns, Trow >= Tc tile rows, rows[c] the tile rows of column c, tiles[(R, C)] the 64x64 blocks
of L, D = -I on the columns >= neg0, given[(i, j)] the caller's Sigma of the rows past the columns.

Reference: np.longdouble, no np.linalg.  X = L^-1 by forward substitution row by row, Sigma = X^T D X, the solves from X.

Bounds (u = 2^-53; nothing in them comes from a kernel's output):
 (a) pure products of what the device itself read: Sigma(i, k) = -sum_{j in I} Sigma(i, j) Z(j, k) from the device's final Sg and Z under
     (64 |I| + 4) u sum |Sg| |Z| (border_cases.py's form); the diagonal tile from the stage-0 Sg(k, k), the final Sigma(I, k) and Z,
     symmetrised: two more roundings.  k_gram likewise with K = nrows.
 (b) the prep kernels, E = |L_kk^-1| |L_kk| |L_kk^-1|: |Z - L_ik L_kk^-1| <= 64 u |L_ik| E, |P - L_kk^-T D L_kk^-1| <= 64 u (|X|^T E + E^T |X|)
     (Higham, Accuracy and Stability, ch. 14, componentwise, constant n).
 (c) whole results: 8 times the worst error of the float64 restatement below (block substitution through the rounded Winv, numpy
     products: no code shared with the kernels) against the long-double reference, floor 4 u max|ref|; for Sigma never above
     0.99 n u kappa_2 max|ref| / 16 (which cuts the one-tile case's tolerance below the margin of 8)."""
import functools
import zlib

import numpy as np

import chol_cases

NB = 64
U = 2.0 ** -53
LD = np.longdouble
IN_NAN = np.array([0x7FF80000C0DE0001], np.uint64).view(np.float64)[0]
OUT_NAN = np.array([0x7FF80000F1110002], np.uint64).view(np.float64)[0]
C_MARGIN = 8.0


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def view(flat, ld):
    """[col, row] view of a column-major buffer."""
    return flat.reshape(-1, ld)


def tile(flat, ld, i, k):
    """Tile (i, k) as a (row, col) view."""
    return view(flat, ld)[k * NB:(k + 1) * NB, i * NB:(i + 1) * NB].T


def put(flat, ld, i, k, t):
    view(flat, ld)[k * NB:(k + 1) * NB, i * NB:(i + 1) * NB] = np.asarray(t, np.float64).T


# ---- models --------------------------------------------------------------------------------------------------------------------------

PROFILES = {
    "one": (1, None), "two": (2, [1, 1]), "dense5": (5, [4] * 5), "diag3": (3, [0, 1, 2]),
    "band2": (11, [min(c + 2, 10) for c in range(11)]), "band3": (12, [min(c + 3, 11) for c in range(12)]),
    "decoupled": (8, [2, 3, 3, 3, 6, 7, 7, 7]), "stairs": (7, [1, 4, 4, 4, 6, 6, 6]),
}
PROFILE_CASES = list(PROFILES)


def lds_of(T, padded):
    """chol_cases' padded leading dimension (one tile row behind the band) or the minimal one."""
    return (T + 1) * NB if padded else T * NB


def _tiles_from_L0(L0, T, rows):
    tl = {}
    for c in range(T):
        for r in [c] + list(rows[c]):
            tl[(r, c)] = L0[r * NB:(r + 1) * NB, c * NB:(c + 1) * NB].copy()
    return tl


@functools.lru_cache(maxsize=None)
def profile_model(name):
    T, prof = PROFILES[name]
    pf = [T - 1] * T if prof is None else list(prof)
    _, _, L0, _, _ = chol_cases._system(_rng("cov:" + name), T, 0, pf)
    rows = [list(range(c + 1, pf[c] + 1)) for c in range(T)]
    return dict(name=name, Tc=T, Trow=T, Tb=T, neg0=T, rows=rows, prof=pf, tiles=_tiles_from_L0(L0, T, rows), given={})


def sub_model(m, c0, c1):
    """Columns c0 .. c1 - 1 of a one-store model as a system of their own (they must couple to nothing outside)."""
    T = c1 - c0
    rows = [[r - c0 for r in m["rows"][c]] for c in range(c0, c1)]
    assert all(0 < r < T for rr in rows for r in rr)
    tiles = {(r - c0, c - c0): t for (r, c), t in m["tiles"].items() if c0 <= c < c1}
    return dict(name=f"{m['name']}[{c0}:{c1}]", Tc=T, Trow=T, Tb=T, neg0=T, rows=rows, prof=[m["prof"][c] - c0 for c in range(c0, c1)],
                tiles=tiles, given={})


def _joint(name, Tc, Tb, Trow, rows, neg0):
    rng = _rng("jcov:" + name)
    tiles = {}
    for c in range(Tc):
        for r in [c] + list(rows[c]):
            blk = rng.normal(size=(NB, NB)) * (0.25 / np.sqrt(NB))
            if r == c:
                blk = np.tril(blk)
                blk[np.diag_indices(NB)] = 1.0 + rng.uniform(0, 1, NB)
            tiles[(r, c)] = blk
    given = {}
    if Trow > Tc:                                   # the caller's Sigma of the rows past the columns: symmetric, positive definite, random
        g = (Trow - Tc) * NB
        Q = rng.normal(size=(g, g)) / np.sqrt(g)
        G = Q @ Q.T + 0.5 * np.eye(g)
        G = 0.5 * (G + G.T)
        for i in range(Tc, Trow):
            for j in range(Tc, i + 1):
                given[(i, j)] = G[(i - Tc) * NB:(i - Tc + 1) * NB, (j - Tc) * NB:(j - Tc + 1) * NB].copy()
    return dict(name=name, Tc=Tc, Trow=Trow, Tb=Tb, neg0=neg0, rows=[list(r) for r in rows], prof=None, tiles=tiles, given=given)


# name -> (Tc, Tb, Trow, rows, neg0, ld pad, ldb pad, lds pad) in doubles beyond the minimum
JOINT = {
    "two_store": (5, 3, 5, [[1, 2, 3, 4], [2, 3, 4], [3, 4], [4], []], 5, 2, 66, 0),
    # lists that skip tiles and reach two tile rows past the columns; closed under elimination: i < j in rows[k] -> j in rows[i] or given
    "gaps": (4, 2, 6, [[2, 4, 5], [3, 5], [4, 5], [5]], 4, 64, 2, 6),
    "lambda": (4, 2, 4, [[1, 2, 3], [2, 3], [3], []], 3, 0, 64, 2),
    # three columns that couple to the rows past the columns only: independent of each other, one step
    "uneven_step": (3, 3, 6, [[3, 4, 5], [4], []], 3, 0, 0, 64),
}


@functools.lru_cache(maxsize=None)
def joint_model(name):
    if name == "as_one_store":
        m = dict(profile_model("band3"))
        m["name"] = name
        return m
    Tc, Tb, Trow, rows, neg0 = JOINT[name][:5]
    return _joint(name, Tc, Tb, Trow, rows, neg0)


def joint_dims(name, m):
    """(ld, ldb, lds) of a joint case."""
    pads = JOINT[name][5:] if name in JOINT else (0, 0, 0)
    return m["Trow"] * NB + pads[0], max(m["Trow"] - m["Tb"], 1) * NB + pads[1], m["Trow"] * NB + pads[2]


def sequential_steps(m, sysi=0):
    """One job per step, last column first."""
    return [[(sysi, k)] for k in range(m["Tc"] - 1, -1, -1)]


def row_lists(models):
    """(rp, rows, col0 per system) of the systems' lists, one after the other."""
    rp, rows, col0 = [0], [], []
    for m in models:
        col0.append(len(rp) - 1)
        for c in range(m["Tc"]):
            rows += m["rows"][c]
            rp.append(len(rows))
    return rp, rows, col0


# ---- long-double pieces ---------------------------------------------------------------------------------------------------------------

def tri_inv_ld(L):
    """L^-1 of a lower triangular matrix by forward substitution, row by row, vectorised over the columns."""
    L = np.asarray(L).astype(LD)
    n = L.shape[0]
    X = np.zeros((n, n), LD)
    for i in range(n):
        if i:
            X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
        X[i, i] = LD(1) / L[i, i]
    return X


def winv_blocks(m):
    """Per column the four inverses of the diagonal 16x16 blocks, long double rounded to double: [k][b] = (L_bb^-1) as (row, col)."""
    out = []
    for k in range(m["Tc"]):
        D = m["tiles"][(k, k)]
        out.append([tri_inv_ld(D[16 * b:16 * b + 16, 16 * b:16 * b + 16]).astype(np.float64) for b in range(4)])
    return out


def dense_L(m):
    """The factor as one lower triangular matrix (every row must be an own column)."""
    assert m["Trow"] == m["Tc"]
    n = m["Tc"] * NB
    L = np.zeros((n, n))
    for (r, c), t in m["tiles"].items():
        L[r * NB:(r + 1) * NB, c * NB:(c + 1) * NB] = t
    return L


def dvec(m):
    d = np.ones(m["Tc"] * NB)
    d[m["neg0"] * NB:] = -1.0
    return d


@functools.lru_cache(maxsize=None)
def _reference(kind, name):
    m = profile_model(name) if kind == "profile" else joint_model(name)
    ref = dict(X={}, E={}, Z={}, P={}, B_Z={}, B_P={})
    for k in range(m["Tc"]):
        Lkk = m["tiles"][(k, k)].astype(LD)
        X = tri_inv_ld(Lkk)
        E = np.abs(X) @ np.abs(Lkk) @ np.abs(X)
        sg = LD(-1) if k >= m["neg0"] else LD(1)
        ref["X"][k], ref["E"][k] = X, E
        ref["P"][k] = sg * (X.T @ X)
        ref["B_P"][k] = (64 * U * (np.abs(X).T @ E + E.T @ np.abs(X))).astype(np.float64)
        for i in m["rows"][k]:
            Lik = m["tiles"][(i, k)].astype(LD)
            ref["Z"][(i, k)] = Lik @ X
            ref["B_Z"][(i, k)] = (64 * U * (np.abs(Lik) @ E)).astype(np.float64)
    if m["Trow"] == m["Tc"]:                        # the whole result: Sigma = X^T D X on the lists' tiles
        Xf = tri_inv_ld(dense_L(m))
        d = dvec(m).astype(LD)
        ref["Xfull"] = Xf
        sig = {}
        for k in range(m["Tc"]):
            for i in [k] + m["rows"][k]:
                A = Xf[i * NB:, i * NB:(i + 1) * NB]
                sig[(i, k)] = (A * d[i * NB:, None]).T @ Xf[i * NB:, k * NB:(k + 1) * NB]
        ref["Sigma"] = sig
    return ref


def reference(m):
    return _reference("profile" if m["name"] in PROFILES else "joint", m["name"])


# ---- device layouts -------------------------------------------------------------------------------------------------------------------

def _ld_winv(m, cols):
    """Ld ([k][col][row]) and Winv ([k][b][j][r]) of the columns `cols`."""
    wb = winv_blocks(m)
    Ld = np.full((len(cols), NB, NB), IN_NAN)
    Wi = np.zeros((len(cols), 4, 16, 16))
    for q, k in enumerate(cols):
        D = m["tiles"][(k, k)]
        for I in range(4):
            for J in range(I):
                Ld[q, 16 * J:16 * J + 16, 16 * I:16 * I + 16] = D[16 * I:16 * I + 16, 16 * J:16 * J + 16].T
            Wi[q, I] = wb[k][I].T
    return Ld.ravel(), Wi.ravel()


def factor_layout(m, ld, zero_outside=False, explicit_prof=True):
    """A one-store model in the device's layout: dict(S, ld, T, Ld, Winv, prof) for api.debug_*.  zero_outside: the lower tiles outside
    the profile hold zero (k_cov_fwd's contract), else IN_NAN."""
    T = m["Tc"]
    S = np.full(ld * T * NB, IN_NAN)
    for c in range(T):
        for r in range(c + 1, T):
            if r in m["rows"][c]:
                put(S, ld, r, c, m["tiles"][(r, c)])
            elif zero_outside:
                put(S, ld, r, c, np.zeros((NB, NB)))
    Ld, Wi = _ld_winv(m, range(T))
    return dict(S=S, ld=ld, T=T, Ld=Ld, Winv=Wi, prof=list(m["prof"]) if explicit_prof else None)


def joint_layout(m, ld, ldb, lds, col0):
    """A model in the joint hook's form, Sg / Z pre-filled with OUT_NAN and the caller's Sigma of the rows past the columns."""
    Tc, Tb, Trow = m["Tc"], m["Tb"], m["Trow"]
    S = np.full(ld * Tb * NB, IN_NAN)
    B = np.full(ldb * (Tc - Tb) * NB, IN_NAN)
    for (r, c), t in m["tiles"].items():
        if r == c:
            continue
        if c < Tb:
            put(S, ld, r, c, t)
        else:
            put(B, ldb, r - Tb, c - Tb, t)
    Ld, Wi = _ld_winv(m, range(Tc))
    Sg = np.full(lds * Trow * NB, OUT_NAN)
    for (i, j), t in m["given"].items():
        put(Sg, lds, i, j, t)
        if i == j:
            assert np.array_equal(t, t.T)
    return dict(S=S, ld=ld, Tb=Tb, B=B, ldb=ldb, Tc=Tc, Ld=Ld, Winv=Wi, neg0=m["neg0"], col0=col0, lds=lds, Trow=Trow, Sg=Sg,
                Z=np.full(lds * Trow * NB, OUT_NAN))


def written_masks(m, lds):
    """(Sg mask, Z mask) over [col, row]: True where the passes must write (the lists' tiles; Sg's diagonal tiles too)."""
    shape = (m["Trow"] * NB, lds)
    ms, mz = np.zeros(shape, bool), np.zeros(shape, bool)
    for k in range(m["Tc"]):
        ms[k * NB:(k + 1) * NB, k * NB:(k + 1) * NB] = True
        for i in m["rows"][k]:
            ms[k * NB:(k + 1) * NB, i * NB:(i + 1) * NB] = True
            mz[k * NB:(k + 1) * NB, i * NB:(i + 1) * NB] = True
    return ms, mz


# ---- the float64 restatement -----------------------------------------------------------------------------------------------------------

def linv64(Lkk, wk):
    """L_kk^-1 through the rounded inverses of the 16-blocks: block forward substitution on the identity."""
    X, Y = np.zeros((NB, NB)), np.eye(NB)
    for b in range(4):
        s = slice(16 * b, 16 * b + 16)
        X[s] = wk[b] @ Y[s]
        Y[16 * b + 16:] -= Lkk[16 * b + 16:, s] @ X[s]
    return X


def restate(m, lds, Sg0, Z0, stage=1, plant=None, steps=None):
    """The selected inverse in float64 into copies of Sg0 / Z0 (the device's layout, leading dimension lds).  Returns (Sg, Z, Xhat).
    plant (the test of the tests): ("drop", i, k) one k-step of four left out of tile (i, k)'s product; ("untransposed", i, k) Sigma(j, i)
    used as it lies where its transpose was meant; ("skip_row", i, k) the first row of I left out; ("sign", k) D ignored on column k."""
    Sg, Z = Sg0.copy(), Z0.copy()
    wb = winv_blocks(m)
    Xh = {}
    for k in range(m["Tc"]):
        Xh[k] = X = linv64(m["tiles"][(k, k)], wb[k])
        sg = -1.0 if (k >= m["neg0"] and plant != ("sign", k)) else 1.0
        put(Sg, lds, k, k, sg * (X.T @ X))
        for i in m["rows"][k]:
            put(Z, lds, i, k, m["tiles"][(i, k)] @ X)
    if stage == 0:
        return Sg, Z, Xh
    order = [k for st in (steps or sequential_steps(m)) for _, k in st]
    for k in order:
        I = m["rows"][k]
        if not I:
            continue
        for i in I:
            acc = np.zeros((NB, NB))
            for q, j in enumerate(I):
                if plant == ("skip_row", i, k) and q == 0:
                    continue
                if j <= i:
                    A = tile(Sg, lds, i, j)
                else:
                    A = tile(Sg, lds, j, i) if plant == ("untransposed", i, k) else tile(Sg, lds, j, i).T
                Bm = tile(Z, lds, j, k)
                if plant == ("drop", i, k) and q == len(I) - 1:
                    keep = np.ones(NB, bool)
                    keep[20:24] = False
                    A, Bm = A[:, keep], Bm[keep]
                acc += A @ Bm
            put(Sg, lds, i, k, -acc)
        acc = np.zeros((NB, NB))
        for i in I:
            acc += tile(Sg, lds, i, k).T @ tile(Z, lds, i, k)
        A = tile(Sg, lds, k, k) - acc
        put(Sg, lds, k, k, 0.5 * (A + A.T))
    return Sg, Z, Xh


# ---- the checks ---------------------------------------------------------------------------------------------------------------------------

def _ratio(got, ref, bound):
    err = np.abs(np.asarray(got).astype(LD) - ref).astype(np.float64)
    if not np.all(np.isfinite(err)):
        return np.inf
    return float((err / bound).max())


def check_a(m, lds, Sg, Z, Sg_prep):
    """Bound (a): every tile of the lists as the product of what the device itself read.  Sg, Z: the final buffers; Sg_prep: stage 0's.
    Returns the worst |err| / bound (inf for a NaN)."""
    worst = 0.0
    for k in range(m["Tc"]):
        I = m["rows"][k]
        if not I:
            continue
        K = NB * len(I)
        Zk = [tile(Z, lds, j, k).astype(LD) for j in I]
        for i in I:
            ref, mag = np.zeros((NB, NB), LD), np.zeros((NB, NB), LD)
            for j, Zj in zip(I, Zk):
                A = (tile(Sg, lds, i, j) if j <= i else tile(Sg, lds, j, i).T).astype(LD)
                ref -= A @ Zj
                mag += np.abs(A) @ np.abs(Zj)
            worst = max(worst, _ratio(tile(Sg, lds, i, k), ref, ((K + 4) * U * mag).astype(np.float64)))
        acc = tile(Sg_prep, lds, k, k).astype(LD)
        mag = np.abs(acc)
        for i, Zi in zip(I, Zk):
            A = tile(Sg, lds, i, k).T.astype(LD)
            acc = acc - A @ Zi
            mag = mag + np.abs(A) @ np.abs(Zi)
        ref, mag = (acc + acc.T) / 2, (mag + mag.T) / 2
        worst = max(worst, _ratio(tile(Sg, lds, k, k), ref, ((K + 6) * U * mag).astype(np.float64)))
    return worst


def check_b(m, lds, Sg_prep, Z_prep):
    """Bound (b) on stage 0's buffers: (worst ratio of Z, worst ratio of P)."""
    ref = reference(m)
    wz = wp = 0.0
    for k in range(m["Tc"]):
        wp = max(wp, _ratio(tile(Sg_prep, lds, k, k), ref["P"][k], ref["B_P"][k]))
        for i in m["rows"][k]:
            wz = max(wz, _ratio(tile(Z_prep, lds, i, k), ref["Z"][(i, k)], ref["B_Z"][(i, k)]))
    return wz, wp


def check_xhat(m, Xh):
    """The restatement's own L_kk^-1 under |Xhat - X| <= 64 u E."""
    ref = reference(m)
    lo = np.tril_indices(NB)
    worst = 0.0
    for k in range(m["Tc"]):
        assert not np.triu(Xh[k], 1).any()
        worst = max(worst, _ratio(Xh[k][lo], ref["X"][k][lo], (64 * U * ref["E"][k][lo]).astype(np.float64)))
    return worst


def sigma_error(m, lds, Sg):
    """(max |Sg - Sigma_ref| over the lists' tiles, max |Sigma_ref|)."""
    sig = reference(m)["Sigma"]
    err = mx = 0.0
    for (i, k), r in sig.items():
        e = np.abs(tile(Sg, lds, i, k).astype(LD) - r).astype(np.float64)
        err = max(err, float(e.max()) if np.all(np.isfinite(e)) else np.inf)
        mx = max(mx, float(np.abs(r).max()))
    return err, mx


def c_tolerance(restated_err, ref_max):
    return max(C_MARGIN * restated_err, 4 * U * ref_max)


@functools.lru_cache(maxsize=None)
def _sigma_tol(kind, name):
    m = profile_model(name) if kind == "profile" else joint_model(name)
    lds = m["Trow"] * NB
    buf = np.full(lds * m["Trow"] * NB, OUT_NAN)
    Sg, _, _ = restate(m, lds, buf, buf)
    err, mx = sigma_error(m, lds, Sg)
    # never above what conditioning alone would excuse: on `one` (n = 64, kappa_2 = 4.5) 8 x the restatement's 2.5 u max|ref| is 1.1
    # times n u kappa_2 max|ref| / 16, so the tolerance is cut to that guard there — tighter than the margin of 8, never wider
    guard = m["Tc"] * NB * U * kappa2(m) * mx / 16
    return min(c_tolerance(err, mx), 0.99 * guard), err, mx


def sigma_tolerance(m):
    """(tolerance of check (c) on Sigma, the restatement's own worst error, max |Sigma_ref|)."""
    return _sigma_tol("profile" if m["name"] in PROFILES else "joint", m["name"])


def check_c_sigma(m, lds, Sg):
    err, _ = sigma_error(m, lds, Sg)
    return err / sigma_tolerance(m)[0]


# ---- many right-hand sides ------------------------------------------------------------------------------------------------------------------

NCOL = 33


def rhs(m, kind, k0=0):
    """(NCOL, n) right-hand sides, a row per column of the device's buffer: "dense" normal(0, 1), "unit" unit columns as the gates build
    them (runs of six consecutive rows, tile edges included); zero above row 64 k0."""
    n = m["Tc"] * NB
    rng = _rng(f"rhs:{m['name']}:{kind}:{k0}")
    B = np.zeros((NCOL, n))
    lo = NB * k0
    if kind == "dense":
        B[:, lo:] = rng.normal(size=(NCOL, n - lo))
    else:
        starts = [lo, max(lo, min(60, n - 6)), n - 6, max(lo, n - NB), max(lo, (n // 2) // 6 * 6)]
        c = 0
        while c < NCOL:
            for s0 in starts:
                for a in range(6):
                    if c < NCOL:
                        B[c, s0 + a] = 1.0
                        c += 1
            starts = [int(x) for x in rng.integers(lo, n - 5, 3)]
    return B


def _solve16(Lkk, wk, y):
    x, y = np.zeros_like(y), y.copy()
    for b in range(4):
        s = slice(16 * b, 16 * b + 16)
        x[s] = wk[b] @ y[s]
        y[16 * b + 16:] -= Lkk[16 * b + 16:, s] @ x[s]
    return x


def _solve16_t(Lkk, wk, t):
    t = t.copy()
    for b in range(3, -1, -1):
        s = slice(16 * b, 16 * b + 16)
        t[s] = wk[b].T @ t[s]
        t[:16 * b] -= Lkk[s, :16 * b].T @ t[s]
    return t


def restate_solve(m, B):
    """(W = L^-1 B, X = L^-T W) in float64 by block substitution through the rounded Winv; B: (ncol, n)."""
    wb = winv_blocks(m)
    T = m["Tc"]
    Y, W = B.T.copy(), np.zeros_like(B.T)
    blk = lambda k: slice(k * NB, (k + 1) * NB)
    for k in range(T):
        W[blk(k)] = _solve16(m["tiles"][(k, k)], wb[k], Y[blk(k)])
        for i in m["rows"][k]:
            Y[blk(i)] -= m["tiles"][(i, k)] @ W[blk(k)]
    X = W.copy()
    for k in range(T - 1, -1, -1):
        t = X[blk(k)].copy()
        for i in m["rows"][k]:
            t -= m["tiles"][(i, k)].T @ X[blk(i)]
        X[blk(k)] = _solve16_t(m["tiles"][(k, k)], wb[k], t)
    return W.T.copy(), X.T.copy()


@functools.lru_cache(maxsize=None)
def solve_reference(name, kind):
    """dict(B, W, X: long double (NCOL, n); tol_W, tol_X: check (c)'s tolerances; err_W, err_X: the restatement's own errors)."""
    m = profile_model(name)
    B = rhs(m, kind)
    Xf = reference(m)["Xfull"]
    W = (Xf @ B.T.astype(LD))
    X = (Xf.T @ W)
    Wr, Xr = restate_solve(m, B)
    eW = float(np.abs(Wr.T.astype(LD) - W).max())
    eX = float(np.abs(Xr.T.astype(LD) - X).max())
    return dict(B=B, W=W.T, X=X.T, err_W=eW, err_X=eX, tol_W=c_tolerance(eW, float(np.abs(W).max())),
                tol_X=c_tolerance(eX, float(np.abs(X).max())))


@functools.lru_cache(maxsize=None)
def pose_cov_reference(name, row0):
    """(cov long double (6, 6), tolerance of check (c), the restatement's own error) of the pose whose first row is row0."""
    m = profile_model(name)
    Xf = reference(m)["Xfull"]
    A = Xf[:, row0:row0 + 6]
    cov = A.T @ A
    E = np.zeros((6, m["Tc"] * NB))
    E[np.arange(6), row0 + np.arange(6)] = 1.0
    Wr, _ = restate_solve(m, E)
    err = float(np.abs((Wr @ Wr.T).astype(LD) - cov).max())
    return cov, c_tolerance(err, float(np.abs(cov).max())), err


def kappa2(m):
    """kappa_2(L D L^T) = (sigma_max(L) / sigma_min(L))^2 (for the host test's guard on the tolerances only)."""
    s = np.linalg.svd(dense_L(m), compute_uv=False)
    return float((s[0] / s[-1]) ** 2)


# ---- gram ---------------------------------------------------------------------------------------------------------------------------------

GRAM_NCOL = [1, 16, 17, 33]
GRAM_NROWS = [1, 63, 64, 65, 130]
GRAM_LISTS = ["null", "identity", "scattered"]


def gram_case(ncol, nrows, lst):
    """(X (ncol, ldx), rows or None, M pre-filled (ncol + 1, ncol), ref long double, bound): "scattered": an ascending list inside a
    longer column (ldx > nrows), IN_NAN in the rows the list leaves out."""
    rng = _rng(f"gram:{ncol}:{nrows}:{lst}")
    if lst == "scattered":
        ldx = 2 * nrows + 7
        rows = np.sort(rng.choice(ldx, nrows, replace=False)).astype(np.int32)
        X = np.full((ncol, ldx), IN_NAN)
        X[:, rows] = rng.normal(size=(ncol, nrows))
    else:
        ldx = nrows
        rows = None if lst == "null" else np.arange(nrows, dtype=np.int32)
        X = rng.normal(size=(ncol, ldx))
    used = X[:, rows] if rows is not None else X
    ref = used.astype(LD) @ used.astype(LD).T
    bound = ((nrows + 4) * U * (np.abs(used).astype(LD) @ np.abs(used).astype(LD).T)).astype(np.float64)
    return X, rows, np.full((ncol + 1, ncol), OUT_NAN), ref, bound
