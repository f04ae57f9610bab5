"""A plain numpy restatement of CLIPPER's dense-clique solve (clipper.cpp:172-323, rounding DSD_HEU :302-310 with the bounded
min-heap scan of utils.cpp:33-55), written from the reference's text and independent of the product and of the C++ oracle.

solve() takes what oracle/clipper.hpp::clipper_dense_clique takes — the symmetric affinity matrix without its diagonal (dense, or
as CSR), a start vector and the parameters — and returns u, F, the nodes and a DECISION TRACE: every branch the solve took (the
line searches' backtracks and caps, the inner and outer loops' lengths and caps, the active-constraint count of every update of the
penalty d) and the smallest distance of any decision's operand from its threshold.  Two runs with the same trace took the same
path; the smallest distance says how far a perturbation of the arithmetic is from changing it.

dtype selects float64 or np.longdouble; perm solves the relabelled problem (M[perm][:, perm], u0[perm]) and maps the result back,
which changes the order of every sum.  probe_error_bound() is the forward error bound of the one-step probe cases
(clique_cases.py), derived in its docstring."""
import heapq

import numpy as np

DEFAULTS = dict(tol_u=1e-8, tol_F=1e-9, maxiniters=200, maxoliters=1000, beta=0.25, maxlsiters=99, eps=1e-9, rescale_u0=1)   # clipper.h:27-60


def csr_to_dense(rowptr, col, val, dtype=np.float64):
    """(M, C): the values and the pattern (the STORED entries, zero-valued ones included) as dense n x n matrices."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    M, Cm = np.zeros((n, n), dtype), np.zeros((n, n), dtype)
    M[rows, col] = np.asarray(val, dtype)
    Cm[rows, col] = 1
    return M, Cm


def dense_to_csr(S):
    """CSR (int32 rowptr, int32 col, float64 val) of a symmetric matrix's non-zeros off the diagonal, columns ascending."""
    S = np.asarray(S, np.float64)
    n = len(S)
    mask = S != 0
    np.fill_diagonal(mask, False)
    r, c = np.nonzero(mask)                       # row-major: rows ascending, columns ascending within a row
    rowptr = np.zeros(n + 1, np.int32)
    rowptr[1:] = np.cumsum(np.bincount(r, minlength=n))
    return rowptr, c.astype(np.int32), np.ascontiguousarray(S[r, c])


def round_half_away(x):
    """std::round."""
    x = float(x)
    return int(np.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def k_largest(x, k):
    """utils.cpp:33-55: a min-heap of (value, index) bounded at k; a later entry replaces the top only if its VALUE is strictly
    larger; the indices come out largest pair first."""
    if k < 1:
        return []
    q = []
    for i, v in enumerate(x):
        if len(q) < k:
            heapq.heappush(q, (v, i))
        elif q[0][0] < v:
            heapq.heapreplace(q, (v, i))
    return [i for _, i in sorted(q, reverse=True)]


def solve(matrix, u0, params=None, dtype=np.float64, perm=None):
    """matrix: a dense symmetric (or upper-filled) n x n array, or (rowptr, col, val).  Returns a dict:
      u (n, float64 rounded from dtype), u_raw (dtype), F (float), nodes (list), omega, d, clamped_last (entries the last accepted
      step cut off at zero), trace.
    trace: evals; active (the active-constraint count of every d update, the first one — before the loops — included); outer: one
    (inner iterations, maxin ended it, ((backtracks, maxls ended it) per inner iteration), how the inner loop left: "cap", "du",
    "dF" or "du+dF") per outer iteration; maxol: the outer
    loop ran out; decisions: all of that as one tuple; min_dist / min_dist_kind: the smallest |operand - threshold| over
    deltaF + eps, du - tol_u, |deltaF| - tol_F, every Cbu_i - eps and u_i - eps of every d update, F's distance from the next
    half-integer (omega = round(F)) and the gap between the last selected and the best unselected entry of u."""
    P = dict(DEFAULTS)
    P.update(params or {})
    dt = dtype
    if isinstance(matrix, tuple):
        M, Cm = csr_to_dense(*matrix, dtype=dt)
    else:
        M = np.array(matrix, dt)
        M = np.triu(M, 1)
        M = M + M.T
        Cm = (M != 0).astype(dt)
    n = len(M)
    u0 = np.asarray(u0, dt)
    inv = None
    if perm is not None:
        perm = np.asarray(perm)
        M, Cm, u0 = M[np.ix_(perm, perm)], Cm[np.ix_(perm, perm)], u0[perm]
        inv = np.empty(n, np.int64)
        inv[perm] = np.arange(n)
    M, Cm = np.ascontiguousarray(M), np.ascontiguousarray(Cm)
    eps, beta, tol_u, tol_F = dt(P["eps"]), dt(P["beta"]), dt(P["tol_u"]), dt(P["tol_F"])
    mind = [np.inf, ""]

    def near(x, kind):
        x = float(np.min(np.abs(x))) if np.size(x) else np.inf
        if x < mind[0]:
            mind[0], mind[1] = x, kind

    evals = 0
    active = []

    def d_terms(v, absval):                          # clipper.cpp:201-216, 283-295
        cbu = v.sum() - Cm @ v - v
        near(cbu - eps, "Cbu - eps")
        near(v - eps, "u - eps")
        act = (cbu > eps) & (v > eps)
        cnt = int(act.sum())
        active.append(cnt)
        if cnt == 0:
            return 0, dt(0)
        q = (M @ v + v)[act] / cbu[act]
        return cnt, (np.abs(q) if absval else q).sum() / dt(cnt)

    def grad(v, d):                                  # clipper.cpp:224-226, 246-248
        nonlocal evals
        evals += 1
        return (1 + d) * v - d * v.sum() + M @ v + (Cm @ v) * d

    u = M @ u0 + u0 if P["rescale_u0"] else u0.copy()    # clipper.cpp:186-199
    u = u / np.sqrt((u * u).sum())
    d = dt(0)
    c, t = d_terms(u, False)
    if c > 0:
        d = t
    F = dt(0)
    outer, maxol_hit, clamped_last = [], True, 0
    for _ in range(P["maxoliters"]):
        g = grad(u, d)
        F = u @ g
        searches, maxin_hit = [], True
        for _ in range(P["maxiniters"]):
            alpha, Fnew, dF, bt, capped = dt(1), dt(0), dt(0), 0, True
            unew, gnew = u, g
            for _ in range(P["maxlsiters"]):
                y = u + alpha * g
                x = np.maximum(y, 0)
                clamped_last = int((y < 0).sum())
                unew = x / np.sqrt((x * x).sum())
                gnew = grad(unew, d)
                Fnew = unew @ gnew
                dF = Fnew - F
                near(dF + eps, "deltaF + eps")
                if dF < -eps:
                    alpha = alpha * beta
                    bt += 1
                else:
                    capped = False
                    break
            searches.append((bt, capped))
            e = unew - u
            du = np.sqrt((e * e).sum())
            F, u, g = Fnew, unew, gnew
            near(du - tol_u, "du - tol_u")
            near(abs(dF) - tol_F, "|deltaF| - tol_F")
            if du < tol_u or abs(dF) < tol_F:
                maxin_hit = False
                left = "+".join(k for k, hit in (("du", du < tol_u), ("dF", abs(dF) < tol_F)) if hit)
                break
        outer.append((len(searches), maxin_hit, tuple(searches), "cap" if maxin_hit else left))
        c, dd = d_terms(u, True)
        if c > 0:
            d = d + dd
        else:
            maxol_hit = False
            break
    if inv is not None:
        u = u[inv]
    u64 = np.asarray(u, np.float64)
    omega = round_half_away(F)
    frac = abs(float(F)) + 0.5 - np.floor(abs(float(F)) + 0.5)           # 0 on a half-integer, where round() jumps
    near(min(frac, 1.0 - frac), "F - half-integer")
    nodes = k_largest(u64.tolist(), omega)
    if 0 < len(nodes) < n:
        rest = np.ones(n, bool)
        rest[nodes] = False
        near(u64[nodes].min() - u64[rest].max(), "selection gap")
    trace = dict(evals=evals, active=tuple(active), outer=tuple(outer), maxol=maxol_hit, min_dist=mind[0], min_dist_kind=mind[1])
    trace["decisions"] = (evals, trace["active"], trace["outer"], maxol_hit, omega)
    return dict(u=u64, u_raw=u, F=float(F), F_raw=F, nodes=nodes, omega=omega, d=float(d), clamped_last=clamped_last, trace=trace)


def summary(trace):
    """The counts the branch assertions speak of."""
    ls = [s for o in trace["outer"] for s in o[2]]
    return dict(evals=trace["evals"], backtracks=sum(b for b, _ in ls), deepest=max([b for b, _ in ls], default=0),
                maxls=sum(1 for _, c in ls if c), maxin=sum(1 for o in trace["outer"] if o[1]), maxol=trace["maxol"],
                d_updates=len(trace["active"]), d_grows=sum(1 for a in trace["active"][1:] if a > 0), outer=len(trace["outer"]))


def probe_error_bound(matrix, u0, params=None):
    """Forward error bound of a PROBE solve (maxoliters = maxiniters = maxlsiters = 1: two gradient evaluations, one projected
    step), for ANY order of summation in IEEE double: returns (bound on |u1 - exact| per entry, bound on |F - exact|).  An
    implementation and this module's solve() each lie within the bound of the exact result, so they differ by at most twice it.

    First order in e = 2^-53, with the standard bound for a sum of k terms in any order, |fl(sum) - sum| <= (k - 1) e sum|terms|
    (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2); every product, quotient and square root adds one e.
      w = M u0 + u0      row i: L_i + 1 non-negative terms of one product each      rel. error (L_i + 2) e        [rescale only]
      u = w / |w|        n squares summed, a root, a quotient                        r_i = rel(w_i) + max rel(w) + (n/2 + 2) e
      su, Cu_i, Mu_i     sums of n, L_i, L_i non-negative terms                      rel. max r + (n, L_i, L_i + 1) e
      Cbu_i = su - Cu_i - u_i     cancels: ABSOLUTE error from the three operands + 2 e (su + Cu_i + u_i)
      d = mean over the active i of (Mu_i + u_i) / Cbu_i     rel. error of a quotient rel(num) + abs(Cbu_i) / Cbu_i + e, the mean
                         adds (cnt + 1) e; no active constraint (the M-probe): d = 0 exactly
      g_i = (1 + d) u_i - d su + Mu_i + d Cu_i     absolute: |u_i - su + Cu_i| err(d) + every term's magnitude times its relative
                         error + 4 e (sum of the magnitudes)
      x_i = max(u_i + g_i, 0)      1-Lipschitz: err(u_i) + err(g_i) + e |x_i|
      u1 = x / |x|       err(|x|) <= sum x_i err(x_i) / |x| + (n/2 + 2) e |x|;  err(u1_i) = err(x_i) / |x| + u1_i err(|x|) / |x| + e u1_i
      g1 = gradient at u1 (same d): as g, the products' input errors being M err(u1), C err(u1), sum err(u1)
      F = u1 . g1        sum (u1_i err(g1_i) + err(u1_i) |g1_i|) + (n + 1) e sum |u1_i g1_i|
    The bound assumes both sides take the same decisions (active set, accepted step, clamps away from zero by more than the bound
    on x): clique_cases.py admits a case only if the decisions' distances from their thresholds say so."""
    P = dict(DEFAULTS)
    P.update(params or {})
    assert P["maxoliters"] == P["maxiniters"] == P["maxlsiters"] == 1
    e = 2.0 ** -53
    if isinstance(matrix, tuple):
        M, Cm = csr_to_dense(*matrix)
    else:
        M = np.triu(np.asarray(matrix, np.float64), 1)
        M = M + M.T
        Cm = (M != 0).astype(np.float64)
    n = len(M)
    L = Cm.sum(1)
    u0 = np.asarray(u0, np.float64)
    if P["rescale_u0"]:
        w, rw = M @ u0 + u0, (L + 2) * e
    else:
        w, rw = u0.copy(), np.zeros(n)
    u = w / np.sqrt((w * w).sum())
    r = rw + rw.max() + (n / 2 + 2) * e                       # relative error of u, per entry
    eu = r * u

    def products(v, ev):
        """su, Cu, Mu at v and their absolute error bounds, ev the bound on v's."""
        su, Cu, Mu = v.sum(), Cm @ v, M @ v
        return su, Cu, Mu, ev.sum() + n * e * su, Cm @ ev + L * e * Cu, M @ ev + (L + 1) * e * Mu

    su, Cu, Mu, esu, eCu, eMu = products(u, eu)
    cbu = su - Cu - u
    ecbu = esu + eCu + eu + 2 * e * (su + Cu + u)
    act = (cbu > P["eps"]) & (u > P["eps"])
    d, ed = 0.0, 0.0
    if act.any():
        q = (Mu + u)[act] / cbu[act]
        relq = (eMu + eu)[act] / (Mu + u)[act] + ecbu[act] / cbu[act] + 2 * e
        d = q.mean()
        ed = (q * relq).mean() + (act.sum() + 1) * e * d

    def grad(v, ev, su, Cu, Mu, esu, eCu, eMu):
        g = (1 + d) * v - d * su + Mu + Cu * d
        mag = (1 + d) * v + d * su + Mu + d * Cu
        eg = ed * np.abs(v - su + Cu) + (1 + d) * ev + d * esu + eMu + d * eCu + 4 * e * mag
        return g, eg

    g, eg = grad(u, eu, su, Cu, Mu, esu, eCu, eMu)
    x = np.maximum(u + g, 0.0)
    ex = eu + eg + e * np.abs(u + g)
    nn = np.sqrt((x * x).sum())
    enn = (x * ex).sum() / nn + (n / 2 + 2) * e * nn
    u1 = x / nn
    eu1 = ex / nn + u1 * enn / nn + e * u1
    g1, eg1 = grad(u1, eu1, *products(u1, eu1))
    eF = (u1 * eg1 + eu1 * np.abs(g1)).sum() + (n + 1) * e * np.abs(u1 * g1).sum()
    return eu1, eF
