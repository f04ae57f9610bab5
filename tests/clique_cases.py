"""Cases for the CLIPPER clique solver (clq_solve_body and its three kernels): each a small dict with the CSR of the symmetric
affinity matrix, u0, the parameters and the edge it exists for.  Everything is seeded with np.random.default_rng.

Noise(n, density, lo, hi): every upper-triangular entry is present with probability `density` and takes a value from U(lo, hi);
u0 from U(0, 1).

PROBE cases (maxoliters = maxiniters = maxlsiters = 1: two gradient evaluations, one projected step) show the sparse product row
by row instead of through a converged solve, whose u has a handful of non-zero entries:
  M-probe  eps = 10: no constraint is ever active, d = 0, nothing is clamped, u1 ~ 2 u + M u with u = normalise(M u0 + u0) — every
           row's sum is visible in u1;
  C-probe  default eps: d > 0 and the C u term enters every entry that is not clamped.
Their matrices: Noise with the first eight rows rebuilt to hold exactly 0, 1, 63, 64, 65, 128, 129 and 200 non-zeros (the lanes of
a wave stride a row by 64) at n = 257, 1025 and 2049; the small sizes 1, 2 (with and without an edge), 3, 63, 64, 65; and one start
vector with exact zeros and rescale_u0 = 0.

FULL-SOLVE cases each name the branch they must reach ("must": (quantity of clique_reference.summary, comparison, value));
test_clique_reference.py asserts that the reference reaches it.

A case is ADMISSIBLE only if the reference's float64, permuted float64 and long-double runs (long double dropped from n = 1023 on,
where it is slow) give the same decision trace, and the smallest decision distance is at least 100 times the largest difference
in F between them.  reference(name) runs them once per process and keeps the result; the GPU tests reuse it."""
import functools

import numpy as np

import clique_reference as ref

SPECIAL_LENGTHS = (0, 1, 63, 64, 65, 128, 129, 200)
PROBE = dict(maxoliters=1, maxiniters=1, maxlsiters=1)


def noise(n, density, lo, hi, seed):
    """(S symmetric dense, u0, rng — the generator, for what a case draws after)."""
    rng = np.random.default_rng(seed)
    S = np.zeros((n, n))
    iu = np.triu_indices(n, 1)
    mask = rng.uniform(0, 1, len(iu[0])) < density
    S[iu[0][mask], iu[1][mask]] = rng.uniform(lo, hi, int(mask.sum()))
    S = S + S.T
    return S, rng.uniform(0, 1, n), rng


def special_rows(S, rng, lo=0.2, hi=1.0):
    """Rows 0 .. 7 rebuilt to hold exactly SPECIAL_LENGTHS non-zeros, all in columns >= 8 (symmetric)."""
    n, k = len(S), len(SPECIAL_LENGTHS)
    S[:k, :] = 0
    S[:, :k] = 0
    for r, length in enumerate(SPECIAL_LENGTHS):
        cols = rng.permutation(np.arange(k, n))[:length]
        v = rng.uniform(lo, hi, length)
        S[r, cols] = v
        S[cols, r] = v
    assert [int((S[r] != 0).sum()) for r in range(k)] == list(SPECIAL_LENGTHS)
    return S


def planted(n, k, density, seed, lo=0.2, hi=0.9, clo=0.5, chi=1.0):
    S, u0, rng = noise(n, density, lo, hi, seed)
    members = np.sort(rng.permutation(n)[:k])
    for a in range(k):
        for b in range(a + 1, k):
            S[members[a], members[b]] = S[members[b], members[a]] = rng.uniform(clo, chi)
    return S, u0, members


def chunk_boundary_matrix(n, seed):
    """For the dense-to-CSR kernel (one wave per row, the columns in chunks of 64): sparse noise plus, in every row, entries on
    both sides of every 64-column chunk boundary (columns 63 | 64, 127 | 128, ...) and in the last column."""
    S, u0, rng = noise(n, 0.05, 0.2, 1.0, seed)
    edge = [c for b in range(64, n + 64, 64) for c in (b - 1, b) if c < n] + [n - 1]
    for i in range(n):
        for c in edge:
            if c != i:
                S[i, c] = S[c, i] = rng.uniform(0.2, 1.0)
    return S, u0


def _case(name, kind, S, u0, params, edge, must=(), special=False):
    rowptr, col, val = ref.dense_to_csr(S)
    n = len(S)
    return dict(name=name, kind=kind, n=n, rowptr=rowptr, col=col, val=val, u0=np.ascontiguousarray(u0, np.float64), params=dict(params),
                edge=edge, must=tuple(must), special=tuple(enumerate(SPECIAL_LENGTHS)) if special else (), long_double=n < 1023)


def _probe_pair(out, stem, S, u0, extra, edge, special=False):
    out.append(_case(stem + "-M", "M-probe", S, u0, dict(PROBE, eps=10.0, **extra), edge + "; M-probe", special=special))
    out.append(_case(stem + "-C", "C-probe", S, u0, dict(PROBE, **extra), edge + "; C-probe", special=special))


# the seeds were chosen so that every case is admissible and reaches its branch (test_clique_reference.py checks both)
SEEDS = dict(rows257=5, rows1025=6, rows2049=7, small=20, hard130=1, u0zeros=33, weak257=13, n1023=10, n1024=11, n1025=12, k64=3, iso65=4)
# The second density keeps a typical row near 40 entries at every size: in a denser matrix the special rows of 63 to 129 entries
# lie below the typical row, the C-probe's step clamps them to zero and their sums would not show.
PROBE_DENSITIES = {257: (0.02, 0.15), 1025: (0.02, 0.04), 2049: (0.01, 0.02)}


@functools.lru_cache(maxsize=None)
def _rows_matrix(n, density):
    S, u0, rng = noise(n, density, 0.2, 1.0, SEEDS[f"rows{n}"] + int(round(100 * density)))
    return special_rows(S, rng), u0, rng


@functools.lru_cache(maxsize=None)
def _build():
    out = []
    # ---- probes -------------------------------------------------------------------------------------------------------------------
    for n, densities in PROBE_DENSITIES.items():
        for density in densities:
            S, u0, _ = _rows_matrix(n, density)
            _probe_pair(out, f"probe{n}-d{density}", S, u0, {}, f"row lengths {SPECIAL_LENGTHS} at n = {n}, density {density}", special=True)
    S, u0, _ = _rows_matrix(1025, 0.02)
    u0z = np.random.default_rng(SEEDS["u0zeros"]).uniform(0, 1, 1025)
    u0z[::3] = 0.0
    _probe_pair(out, "probe1025-d0.02-u0zeros", S, u0z, dict(rescale_u0=0), "exact zeros in a third of u0, rescale_u0 = 0", special=True)
    small = {"n1": (1, 0.0), "n2-edge": (2, 1.0), "n2-noedge": (2, 0.0), "n3": (3, 1.0), "n63": (63, 0.5), "n64": (64, 0.5), "n65": (65, 0.5)}
    for k, (stem, (n, density)) in enumerate(small.items()):
        S, u0, _ = noise(n, density, 0.2, 1.0, SEEDS["small"] + k)
        _probe_pair(out, "probe-" + stem, S, u0, {}, f"small size {stem}")
    # ---- full solves --------------------------------------------------------------------------------------------------------------
    S, u0, _ = noise(130, 0.8, 0.2, 1.0, SEEDS["hard130"])
    u0z = np.random.default_rng(SEEDS["u0zeros"]).uniform(0, 1, 130)
    u0z[::3] = 0.0
    full = lambda name, S, u0, params, edge, must=(): out.append(_case(name, "full", S, u0, params, edge, must))
    full("hard130", S, u0, {}, "backtracking, deep line searches, d growing several times",
         [("backtracks", ">=", 10), ("deepest", ">=", 2), ("d_updates", ">=", 3), ("d_grows", ">=", 2)])
    full("hard130-beta0.9", S, u0, dict(beta=0.9), "one line search at least 20 backtracks deep", [("deepest", ">=", 20)])
    full("hard130-caps", S, u0, dict(maxlsiters=2, maxiniters=20, maxoliters=3), "maxls, maxin and maxol all end their loops; F < 0: no nodes",
         [("maxls", ">=", 1), ("maxin", ">=", 1), ("maxol", "==", True), ("F", "<", 0.0), ("n_nodes", "==", 0)])
    full("hard130-norescale", S, u0, dict(rescale_u0=0), "the un-rescaled start", [("backtracks", ">=", 1)])
    full("hard130-norescale-u0zeros", S, u0z, dict(rescale_u0=0), "the un-rescaled start with exact zeros in u0", [("backtracks", ">=", 1)])
    full("hard130-maxol1", S, u0, dict(maxoliters=1), "outer cap at the first pass", [("maxol", "==", True), ("outer", "==", 1)])
    full("hard130-tolF", S, u0, dict(tol_F=1e-3), "the |deltaF| < tol_F exit", [("left_by_dF", ">=", 1)])
    full("hard130-eps", S, u0, dict(eps=1e-3), "moved active-set and line-search threshold (on this matrix the path of the default eps)")
    full("hard130-eps0.01", S, u0, dict(eps=1e-2), "a threshold moved far enough to change the path", [("decisions_differ_from_hard130", "==", True)])
    S, u0, _ = planted(257, 10, 0.2, SEEDS["weak257"])
    full("weak257", S, u0, {}, "backtracking on a problem with an answer (weak planted clique)", [("backtracks", ">=", 1), ("n_nodes", ">=", 2)])
    S, u0, _ = _rows_matrix(257, 0.15)
    out.append(_case("rows257", "full", S, u0, {}, "row shapes inside a long solve", [("backtracks", ">=", 1), ("evals", ">=", 100)], special=True))
    rng = np.random.default_rng(SEEDS["k64"])
    K = np.triu(rng.uniform(0.5, 1.0, (64, 64)), 1)
    full("complete64", K + K.T, rng.uniform(0, 1, 64), {}, "complete graph: no constraint active, d stays 0, the outer loop leaves at its first d update",
         [("active", "==", (0, 0)), ("d", "==", 0.0), ("outer", "==", 1), ("maxol", "==", False)])
    full("isolated65", np.zeros((65, 65)), np.random.default_rng(SEEDS["iso65"]).uniform(0, 1, 65), {}, "65 isolated nodes: nnz = 0, empty col / val",
         [("nnz", "==", 0), ("evals", ">=", 10)])
    for n in (1023, 1024, 1025):
        S, u0, _ = noise(n, 0.05, 0.2, 1.0, SEEDS[f"n{n}"])
        full(f"noise{n}", S, u0, {}, "the threads' second round / the cooperative threshold; hundreds of barriers with backtracking and several d updates",
             [("evals", ">=", 200), ("backtracks", ">=", 1), ("d_grows", ">=", 2)])
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return {c["name"]: c for c in out}


def names(kind=None, n=None):
    return [k for k, c in _build().items() if (kind is None or c["kind"] in kind) and (n is None or c["n"] in n)]


def case(name):
    return _build()[name]


def csr(c):
    return c["rowptr"], c["col"], c["val"]


def dense_upper(c):
    M, _ = ref.csr_to_dense(*csr(c))
    return np.ascontiguousarray(np.triu(M, 1))


def fixed_perm(n):
    return np.random.default_rng(977 + n).permutation(n)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference's runs of a case (float64, float64 under fixed_perm, long double where c["long_double"]), made once:
    dict(run = the float64 run, runs, same_trace, spread_u, spread_F, min_dist, min_dist_kind)."""
    c = case(name)
    runs = [ref.solve(csr(c), c["u0"], c["params"]), ref.solve(csr(c), c["u0"], c["params"], perm=fixed_perm(c["n"]))]
    if c["long_double"]:
        runs.append(ref.solve(csr(c), c["u0"], c["params"], dtype=np.longdouble))
    base = runs[0]
    same = all(r["trace"]["decisions"] == base["trace"]["decisions"] and r["nodes"] == base["nodes"] for r in runs[1:])
    spread_u = max(float(np.abs(np.asarray(r["u_raw"], np.longdouble) - base["u_raw"]).max()) for r in runs[1:])
    spread_F = max(abs(float(np.longdouble(r["F_raw"]) - np.longdouble(base["F_raw"]))) for r in runs[1:])
    k = int(np.argmin([r["trace"]["min_dist"] for r in runs]))
    return dict(run=base, runs=runs, same_trace=same, spread_u=spread_u, spread_F=spread_F, min_dist=runs[k]["trace"]["min_dist"],
                min_dist_kind=runs[k]["trace"]["min_dist_kind"])


def quantities(name):
    """What a case's "must" tuples speak of: clique_reference.summary of the float64 run plus F, d, active, the node count, nnz, the
    number of inner loops left by |deltaF| < tol_F alone, and whether the decisions differ from hard130's."""
    c, r = case(name), reference(name)["run"]
    q = ref.summary(r["trace"])
    q.update(F=r["F"], d=r["d"], active=r["trace"]["active"], n_nodes=len(r["nodes"]), nnz=int(c["rowptr"][-1]),
             left_by_dF=sum(1 for o in r["trace"]["outer"] if o[3] == "dF"),
             decisions_differ_from_hard130=r["trace"]["decisions"] != reference("hard130")["run"]["trace"]["decisions"])
    return q


def tolerances(name):
    """(tol on u: per entry or one number, tol on F) — probes: twice the forward error bound of clique_reference.probe_error_bound
    (the reference and the implementation each lie within it); full solves: 1000 times the reference's own spread over its float64,
    permuted and long-double runs, floored at 1e-12."""
    c = case(name)
    if c["kind"] != "full":
        eu, eF = ref.probe_error_bound(csr(c), c["u0"], c["params"])
        return 2.0 * eu, 2.0 * eF
    R = reference(name)
    return max(1000.0 * R["spread_u"], 1e-12), max(1000.0 * R["spread_F"], 1e-12)
