"""Cases and plain references for the inter-robot map matchers (csrc/place_kernels.hip): SlideMatch sweep, SlideGraph triangle
matching, CLIPPER affinity.  No GPU, no product import, no oracle import: numpy float64 written from the reference's loops
(place_recognition.cpp:98-387, semantic_clipper.cpp:49-118, clipper.cpp:21-65), one elementary operation per numpy call in source
order, so nothing is contracted or re-associated.  Every builder returns its inputs plus a dict `edges` of the kernel edges it claims
to reach; tests/test_place_reference.py asserts each claim on the REFERENCE's results, tests/test_gpu_place_edges.py then holds the
kernels against the reference."""
import math

import numpy as np

PLACE_DEFAULTS = dict(dilation_factor=1.2, search_xy_step_size=0.5, match_yaw_half_range=180. * math.pi / 180.,
                      search_yaw_step_size=2.0 * math.pi / 180., match_threshold_position=0.5, match_threshold_dimension=1.0,
                      disable_yaw_search=0, ignore_dimension=0, min_num_inliers=5, use_nonlinear_least_squares=1,
                      min_num_map_objects_to_start=1, max_rings=-1)


def place_params(**kw):
    p = dict(PLACE_DEFAULTS)
    assert not set(kw) - set(p), kw
    p.update(kw)
    return p


# ---- SlideMatch: lattice, counts, arg-max, pairs ------------------------------------------------------------------------------------
def lattice(ref7, qry7, params):
    """Half ranges (findTransformation :768-787), rings and yaws (:136-241) by the same repeated additions in plain Python floats.
    Candidates in loop order: ring, x, y, then yaw.  cos / sin: math.cos / math.sin, i.e. the C library's, which is what the host code
    that fills the kernels' tables calls (numpy's own vectorised cos may differ in the last bit)."""
    P = params
    mx = my = 0.0
    for m in (ref7, qry7):
        for row in m:
            mx = max(mx, abs(float(row[1])))
            my = max(my, abs(float(row[2])))
    if not P["disable_yaw_search"]:
        mx = my = max(mx, my)
    x_half, y_half = mx * P["dilation_factor"], my * P["dilation_factor"]
    yaws = []
    if P["disable_yaw_search"]:
        yaws.append(0.0)
    else:
        y = -P["match_yaw_half_range"]
        while y < P["match_yaw_half_range"]:
            yaws.append(y)
            y += P["search_yaw_step_size"]
    step = P["search_xy_step_size"]
    outer = 10 * step
    cx, cy = [], []
    steps = int(math.ceil(min(x_half, y_half) / outer))
    if steps > 0:
        sx, sy = x_half / float(steps), y_half / float(steps)
        if not (sx < step or sy < step):
            nrings = min(P["max_rings"], steps) if P["max_rings"] >= 0 else steps
            for cur in range(nrings):
                cs = float(cur)
                x_pe, x_ns, x_lb, x_rb = (cs + 1) * sx, -(cs + 1) * sx, -cs * sx, cs * sx
                y_pe, y_ns, y_lb, y_rb = (cs + 1) * sy, -(cs + 1) * sy, -cs * sy, cs * sy
                ys = []
                y = y_ns
                while y <= y_pe:
                    ys.append(y)
                    y += step
                x = x_ns
                while x <= x_pe:
                    for y in ys:
                        if not ((x >= x_lb and x <= x_rb) and (y >= y_lb and y <= y_rb)):
                            cx.append(x)
                            cy.append(y)
                    x += step
    ny, ncell = len(yaws), len(cx)
    if ncell == 0 or ny == 0 or len(qry7) == 0:
        ncell = 0
        cx, cy = [], []
    ya = np.array(yaws, np.float64)
    return dict(n_yaw=ny, n_cells=ncell, n=ncell * ny,
                x=np.repeat(np.array(cx, np.float64), ny), y=np.repeat(np.array(cy, np.float64), ny), yaw=np.tile(ya, ncell),
                cos=np.tile(np.array([math.cos(v) for v in yaws], np.float64), ncell),
                sin=np.tile(np.array([math.sin(v) for v in yaws], np.float64), ncell))


def cand_xyyaw(lat):
    return np.stack([lat["x"], lat["y"], lat["yaw"]], axis=1) if lat["n"] else np.zeros((0, 3))


def _pair_gate(ref7, qry7, params):
    """(nq, nr) label and dimension gate of :281-357 — everything of a pair test that does not depend on the candidate."""
    label = np.equal(ref7[None, :, 0], qry7[:, None, 0])
    if params["ignore_dimension"]:
        return label
    a4 = np.abs(np.subtract(ref7[None, :, 4], qry7[:, None, 4]))
    a5 = np.abs(np.subtract(ref7[None, :, 5], qry7[:, None, 5]))
    a6 = np.abs(np.subtract(ref7[None, :, 6], qry7[:, None, 6]))
    avg3 = np.divide(np.add(np.add(a4, a5), a6), 3.0)
    only_d1 = np.logical_and(ref7[:, 5] == 0, ref7[:, 6] == 0)[None, :]
    avg = np.where(only_d1, a4, avg3)
    return np.logical_and(label, np.less(avg, params["match_threshold_dimension"]))


def first_hits(ref7, qry7, lat, params, sel=None, budget=3_000_000):
    """(len(sel), nq) index of the first reference object each query object matches under each candidate, -1 for none: the
    un-optimised rule (label test, square root, `<`), chunked over candidates."""
    ref7, qry7 = np.asarray(ref7, np.float64), np.asarray(qry7, np.float64)
    nr, nq = len(ref7), len(qry7)
    sel = np.arange(lat["n"]) if sel is None else np.asarray(sel, np.int64)
    out = np.full((len(sel), nq), -1, np.int64)
    if nr == 0 or nq == 0 or len(sel) == 0:
        return out
    gate = _pair_gate(ref7, qry7, params)
    q1, q2 = qry7[None, :, 1], qry7[None, :, 2]
    tw = np.add(np.add(np.multiply(0.0, q1), np.multiply(0.0, q2)), 1.0 * 1.0)
    thr = params["match_threshold_position"]
    chunk = max(1, budget // (nr * nq))
    for a in range(0, len(sel), chunk):
        s_ = sel[a:a + chunk]
        c, s, x, y = lat["cos"][s_, None], lat["sin"][s_, None], lat["x"][s_, None], lat["y"][s_, None]
        tx = np.add(np.add(np.multiply(c, q1), np.multiply(np.negative(s), q2)), np.multiply(x, 1.0))
        ty = np.add(np.add(np.multiply(s, q1), np.multiply(c, q2)), np.multiply(y, 1.0))
        tx, ty = np.divide(tx, tw), np.divide(ty, tw)
        xd = np.subtract(ref7[None, None, :, 1], tx[:, :, None])
        yd = np.subtract(ref7[None, None, :, 2], ty[:, :, None])
        d = np.sqrt(np.add(np.multiply(xd, xd), np.multiply(yd, yd)))
        ok = np.logical_and(np.less(d, thr), gate[None, :, :])
        first = np.argmax(ok, axis=2)
        out[a:a + chunk] = np.where(np.any(ok, axis=2), first, -1)
    return out


def sweep_counts(ref7, qry7, lat, params, sel=None):
    return (first_hits(ref7, qry7, lat, params, sel) >= 0).sum(axis=1).astype(np.int32)


def first_argmax(counts):
    """The reference keeps a candidate only when it has STRICTLY more inliers: the first index of the maximum; -1 for no candidate."""
    best, bi = -10000, -1
    for i, c in enumerate(np.asarray(counts).tolist()):
        if c > best:
            best, bi = c, i
    return bi


def pairs_at(ref7, qry7, lat, params, index):
    fh = first_hits(ref7, qry7, lat, params, [index])[0]
    q = np.nonzero(fh >= 0)[0]
    return fh[q].astype(np.int32), q.astype(np.int32)


def v_crit(thr):
    """The smallest double whose correctly rounded square root is >= thr (what k_place_sweep_b compares dx^2 + dy^2 with)."""
    v = thr * thr
    while math.sqrt(v) >= thr:
        v = math.nextafter(v, -math.inf)
    while math.sqrt(v) < thr:
        v = math.nextafter(v, math.inf)
    return v


def bucket_layout(ref7, qry7):
    """How the bucketed kernel sees the two maps, re-derived here from its description: buckets = distinct reference labels in order of
    first appearance, query objects sorted stably by bucket (labels the reference lacks last, with an empty range), wavefront chunks of
    64 query objects.  Returns dict(sizes: bucket sizes, qbucket: bucket per SORTED query object (-1 = absent), chunks: per chunk the
    list of distinct non-empty buckets in it, rank: position of every reference object inside its bucket)."""
    labels, rb = [], []
    for l in ref7[:, 0].tolist():
        if l not in labels:
            labels.append(l)
        rb.append(labels.index(l))
    sizes = [rb.count(b) for b in range(len(labels))]
    seen = [0] * len(labels)
    rank = []
    for b in rb:
        rank.append(seen[b])
        seen[b] += 1
    qb = [labels.index(l) if l in labels else len(labels) for l in qry7[:, 0].tolist()]
    order = sorted(range(len(qb)), key=lambda j: qb[j])          # (Python's sort is stable)
    qs = [qb[j] if qb[j] < len(labels) else -1 for j in order]
    chunks = []
    for j0 in range(0, len(qs), 64):
        ch = []
        for b in qs[j0:j0 + 64]:
            if b >= 0 and b not in ch:
                ch.append(b)
        chunks.append(ch)
    return dict(sizes=sizes, qbucket=np.array(qs), order=np.array(order), chunks=chunks, rank=np.array(rank), rbucket=np.array(rb),
                n_absent_query=sum(1 for b in qs if b < 0), unused_ref_buckets=sorted(set(range(len(labels))) - set(qs)))


def sweep_edges(case, lat, fh):
    """The edges a sweep case reaches, measured on the reference's first hits `fh` (all candidates): what the builders' claims are
    checked against."""
    ref7, qry7 = case["ref7"], case["qry7"]
    L = bucket_layout(ref7, qry7)
    nq = len(qry7)
    e = dict(nq=nq, chunks=len(L["chunks"]), last_chunk_fill=nq - 64 * (len(L["chunks"]) - 1) if nq else 0,
             bucket_sizes=sorted(set(L["sizes"])), n_labels_ref=len(L["sizes"]),
             max_buckets_in_later_chunk=max([len(c) for c in L["chunks"][1:]] or [0]),
             query_label_absent_from_ref=L["n_absent_query"] > 0, ref_label_absent_from_query=len(L["unused_ref_buckets"]) > 0,
             candidates=lat["n"], n_yaw=lat["n_yaw"])
    counts = (fh >= 0).sum(axis=1)
    e["max_count"] = int(counts.max()) if len(counts) else -1
    e["distinct_counts"] = int(len(np.unique(counts)))
    # per (candidate, chunk, bucket) group of lanes: all closed before the bucket's 16th object (the early exit fires at the next
    # multiple of 16), and groups in which some lanes close while others stay open to the end
    early = mixed = False
    if len(fh) and nq:
        hit_sorted = fh[:, L["order"]]                                   # (C, nq) in the kernel's lane order
        pos = np.where(hit_sorted >= 0, L["rank"][np.maximum(hit_sorted, 0)], -1)
        for ci, ch in enumerate(L["chunks"]):
            lanes = np.arange(64 * ci, min(64 * ci + 64, nq))
            for b in ch:
                mine = lanes[L["qbucket"][lanes] == b]
                p = pos[:, mine]
                allhit = (p >= 0).all(axis=1)
                if L["sizes"][b] > 16 and (allhit & (p.max(axis=1) < 16)).any():
                    early = True
                if ((p >= 0).any(axis=1) & (p < 0).any(axis=1)).any():
                    mixed = True
    e["early_exit"] = early
    e["closed_and_open_lanes_in_one_bucket"] = mixed
    return e


def _forest(rng, ref_buckets, qry_buckets, extent, dims="mixed", yaw=math.pi / 4, shift=(1.0, -0.5), noise=0.05):
    """A reference map with the given {label: count}, shuffled so that the buckets interleave, and a query map with {label: count}
    whose objects are, as far as the reference has that label, reference objects seen from a frame rotated by `yaw` and shifted."""
    rows = []
    for l, n in ref_buckets.items():
        for _ in range(n):
            rows.append(l)
    lab = np.array(rows, np.float64)[rng.permutation(len(rows))]
    n = len(lab)
    ref = np.zeros((n, 7))
    ref[:, 0] = lab
    ref[:, 1:3] = rng.uniform(-extent, extent, (n, 2))
    ref[:, 3] = rng.normal(0, 0.2, n)
    ref[:, 4:7] = rng.uniform(0.3, 2.0, (n, 3))
    if dims == "mixed":                      # d2 / d3 patterns: (0, 0) takes the one-dimension branch, the other three the average
        pat = rng.integers(0, 4, n)
        ref[pat == 0, 5:7] = 0.0
        ref[pat == 1, 5] = 0.0
        ref[pat == 2, 6] = 0.0
    elif dims == "zero":
        ref[:, 4:7] = 0.0
    q = []
    c, s = math.cos(-yaw), math.sin(-yaw)
    for l, k in qry_buckets.items():
        have = np.nonzero(lab == l)[0]
        take = have[rng.permutation(len(have))[:k]]
        for i in take:
            r = ref[i].copy()
            xy = r[1:3] - np.array(shift)
            r[1], r[2] = c * xy[0] - s * xy[1], s * xy[0] + c * xy[1]
            r[1:3] += rng.normal(0, noise, 2)
            r[4:7] += rng.normal(0, 0.2, 3) * (r[4:7] != 0)
            q.append(r)
        for _ in range(k - len(take)):
            r = np.zeros(7)
            r[0] = l
            r[1:3] = rng.uniform(-0.7 * extent, 0.7 * extent, 2)
            r[4:7] = rng.uniform(0.3, 2.0, 3)
            q.append(r)
    q = np.array(q)[rng.permutation(len(q))]
    return np.ascontiguousarray(ref), np.ascontiguousarray(q)


def sweep_cases():
    """name -> dict(ref7, qry7, params, edges).  Lattices are kept to a few thousand candidates (1 m cells, 45 deg yaw steps) so that
    the numpy reference of every candidate stays affordable; the kernels do not care how a lattice came about."""
    out = {}
    base = dict(search_xy_step_size=1.0, search_yaw_step_size=math.pi / 4, match_threshold_position=1.0)

    def add(name, seed, rb, qb, extent=9.0, dims="mixed", edges=None, **kw):
        rng = np.random.default_rng(seed)
        ref, q = _forest(rng, rb, qb, extent, dims)
        p = dict(base)
        p.update(kw)
        out[name] = dict(ref7=ref, qry7=q, params=place_params(**p), edges=edges or {})

    add("q63_one_label_bucket33", 1, {2.0: 33}, {2.0: 63}, ignore_dimension=1,
        edges=dict(nq=63, chunks=1, last_chunk_fill=63, bucket_sizes=[33], n_labels_ref=1, closed_and_open_lanes_in_one_bucket=True))
    add("q64_three_labels_15_16_17", 2, {1.0: 16, 2.0: 17, 3.0: 15}, {1.0: 20, 2.0: 24, 3.0: 20}, ignore_dimension=1,
        edges=dict(nq=64, chunks=1, last_chunk_fill=64, bucket_sizes=[15, 16, 17], n_labels_ref=3))
    add("q65_dims_3_4_5_absent_labels", 3, {1.0: 4, 2.0: 5, 3.0: 3, 9.0: 6}, {1.0: 30, 2.0: 20, 3.0: 10, 7.0: 5}, extent=4.0,
        ignore_dimension=0, match_threshold_position=2.0, match_threshold_dimension=0.6,
        edges=dict(nq=65, chunks=2, last_chunk_fill=1, bucket_sizes=[3, 4, 5, 6], query_label_absent_from_ref=True,
                   ref_label_absent_from_query=True, closed_and_open_lanes_in_one_bucket=True))
    sizes = [1, 3, 4, 5, 15, 16, 17, 33]
    labs = [(-1) ** i * (0.25 + 0.5 * i) for i in range(40)]                 # negative and fractional labels
    add("q128_forty_labels", 4, {l: sizes[i % 8] for i, l in enumerate(labs)}, {l: (4 if i < 8 else 3) for i, l in enumerate(labs)},
        ignore_dimension=1, match_threshold_position=2.5, max_rings=1,
        edges=dict(nq=128, chunks=2, last_chunk_fill=64, bucket_sizes=sizes, n_labels_ref=40, early_exit=True,
                   max_buckets_in_later_chunk=20, closed_and_open_lanes_in_one_bucket=True))
    add("q130_buckets_1_33_400", 5, {1.0: 1, 2.0: 400, 3.0: 33}, {1.0: 10, 2.0: 70, 3.0: 50}, ignore_dimension=1, max_rings=1,
        edges=dict(nq=130, chunks=3, last_chunk_fill=2, bucket_sizes=[1, 33, 400], max_buckets_in_later_chunk=3,
                   closed_and_open_lanes_in_one_bucket=True))
    add("q200_dims_three_labels", 6, {1.0: 63, 2.0: 64, 3.0: 65}, {1.0: 60, 2.0: 70, 3.0: 70}, ignore_dimension=0,
        match_threshold_dimension=0.5, max_rings=1,
        edges=dict(nq=200, chunks=4, last_chunk_fill=8, bucket_sizes=[63, 64, 65], max_buckets_in_later_chunk=2,
                   closed_and_open_lanes_in_one_bucket=True))
    add("q128_zero_dims_no_yaw", 7, {1.0: 40, 2.0: 50}, {1.0: 60, 2.0: 68}, dims="zero", ignore_dimension=0, disable_yaw_search=1,
        search_xy_step_size=0.5, edges=dict(nq=128, chunks=2, n_yaw=1, max_buckets_in_later_chunk=2))
    add("q70_all_rings", 8, {1.0: 20, 2.0: 21, 3.0: 22}, {1.0: 24, 2.0: 23, 3.0: 23}, extent=12.0, ignore_dimension=1, max_rings=-1,
        search_yaw_step_size=math.pi / 2, edges=dict(nq=70, chunks=2, last_chunk_fill=6, max_buckets_in_later_chunk=1))
    add("max_rings_0", 9, {1.0: 5}, {1.0: 5}, ignore_dimension=1, max_rings=0, edges=dict(candidates=0))
    add("empty_lattice_sx_below_step", 10, {1.0: 5}, {1.0: 5}, extent=0.3, ignore_dimension=1, search_xy_step_size=0.5,
        edges=dict(candidates=0))
    for m in (out["empty_lattice_sx_below_step"]["ref7"], out["empty_lattice_sx_below_step"]["qry7"]):
        m[:, 1:3] = np.clip(m[:, 1:3], -0.3, 0.3)           # half range 0.36 -> one ring of 0.36 < the 0.5 step: no candidate at all
    # few query objects per label against large dense buckets: every lane closes within a bucket's first 16 objects, so the scan of
    # that bucket ends early (`k = bhi` in the four-wide loop without dimensions, `break` in the one-by-one loop with them)
    add("early_exit_four_wide", 11, {1.0: 200, 2.0: 100, 3.0: 35}, {1.0: 2, 2.0: 3, 3.0: 2}, ignore_dimension=1,
        match_threshold_position=2.5, max_rings=1, edges=dict(early_exit=True, bucket_sizes=[35, 100, 200]))
    add("early_exit_with_dims", 12, {1.0: 200, 2.0: 100, 3.0: 35}, {1.0: 2, 2.0: 3, 3.0: 2}, ignore_dimension=0,
        match_threshold_position=2.5, match_threshold_dimension=2.0, max_rings=1, edges=dict(early_exit=True))
    out.update(threshold_cases())
    out["argmax_ties"] = argmax_tie_case()
    return out


def _scan(f, lo=0, hi=64):
    for k in range(lo, hi):
        r = f(k)
        if r is not None:
            return r
    raise AssertionError("no exact case within the scan")


def _step(v, k):
    """v moved by k units in the last place (k < 0: towards zero)."""
    for _ in range(abs(k)):
        v = math.nextafter(v, math.inf if k > 0 else 0.0)
    return v


def threshold_cases():
    """Pairs exactly at the decision thresholds.  dilation 1, no yaw search, step 0.5 and extent 8: every lattice value is exact;
    query object j sits at minus a lattice point, so at that candidate its transformed position is exactly (0, 0) and dx, dy are the
    reference object's coordinates themselves.  thr = 0.625 with the 3-4-5 pair (0.375, 0.5)."""
    thr = 0.625
    vc = v_crit(thr)
    targets = [(1.0, 0.5), (-1.5, 2.0), (2.5, -1.0), (0.5, 3.0), (-2.0, -2.5)]

    def v_of(xd, yd):
        return xd * xd + yd * yd

    def grid(cond, sign):
        """the first (xd, yd) around (0.375, 0.5), a few units in the last place away (sign < 0: towards zero), that meets cond"""
        return _scan(lambda n: next(((_step(0.375, sign * k), _step(0.5, sign * (n - k))) for k in range(n + 1)
                                     if cond(v_of(_step(0.375, sign * k), _step(0.5, sign * (n - k))))), None))
    # (a) v exactly v_crit: its root rounds to thr, it must NOT match, and `v <= v_crit` would match it; (b) the double below v_crit:
    # the first match; (c) above 0.375 / 0.5 with a root above thr
    p_eq = (0.375, 0.5)
    p_crit = grid(lambda v: v == vc, -1)
    p_in = grid(lambda v: v == math.nextafter(vc, 0.0), -1)
    p_out = grid(lambda v: math.sqrt(v) > thr, 1)
    assert math.sqrt(v_of(*p_eq)) == thr and math.sqrt(v_of(*p_crit)) == thr and v_of(*p_crit) == vc < v_of(*p_eq)
    assert math.sqrt(v_of(*p_in)) < thr and math.sqrt(v_of(*p_out)) > thr
    xs = [p_eq, p_crit, p_in, p_out, (-p_in[0], -p_in[1])]
    ref = np.zeros((len(xs) + 1, 7))
    qry = np.zeros((len(xs), 7))
    for j, (xd, t) in enumerate(zip(xs, targets)):
        ref[j, :3] = (10.0 + j, xd[0], xd[1])
        qry[j, :3] = (10.0 + j, -t[0], -t[1])
    ref[-1, :3] = (99.0, 8.0, 8.0)                                   # fixes the extent (a label no query object has)
    pos = dict(ref7=ref, qry7=qry, targets=targets, expect_hit=[False, False, True, False, True],
               params=place_params(dilation_factor=1.0, disable_yaw_search=1, search_xy_step_size=0.5, ignore_dimension=1,
                                   match_threshold_position=thr),
               edges=dict(pair_at_threshold=True, pair_at_v_crit=True, pair_one_below_v_crit=True, pair_above_threshold=True))
    # dimension threshold, both branches of (d2 == 0 && d3 == 0); positions coincide exactly at the target candidate
    td = 1.0
    one = lambda q4: abs(1.5 - q4)                                     # noqa: E731
    three = lambda q4: ((abs(1.5 - q4) + abs(0.5 - 1.5)) + abs(0.25 - 1.25)) / 3     # noqa: E731
    rows = []
    for f, d23 in ((one, (0.0, 0.0)), (three, (0.5, 0.25))):
        q_eq = 0.5
        q_in = _scan(lambda k: _step(0.5, k) if f(_step(0.5, k)) < td else None, 1)
        q_out = _scan(lambda k: _step(0.5, -k) if f(_step(0.5, -k)) > td else None, 1)
        assert f(q_eq) == td and f(q_in) < td and f(q_out) > td
        rows += [(d23, q_eq, False), (d23, q_in, True), (d23, q_out, False)]
    targets = [(1.0, 0.5), (-1.5, 2.0), (2.5, -1.0), (0.5, 3.0), (-2.0, -2.5), (3.0, 3.5)]
    ref = np.zeros((len(rows) + 1, 7))
    qry = np.zeros((len(rows), 7))
    for j, ((d23, q4, _), t) in enumerate(zip(rows, targets)):
        ref[j] = (20.0 + j, 0.0, 0.0, 0.0, 1.5, d23[0], d23[1])
        qry[j] = (20.0 + j, -t[0], -t[1], 0.0, q4, 1.5, 1.25)
    ref[-1, :3] = (99.0, 8.0, 8.0)
    dim = dict(ref7=ref, qry7=qry, targets=targets, expect_hit=[r[2] for r in rows],
               params=place_params(dilation_factor=1.0, disable_yaw_search=1, search_xy_step_size=0.5, ignore_dimension=0,
                                   match_threshold_position=thr, match_threshold_dimension=td),
               edges=dict(dim_at_threshold_one_branch=True, dim_at_threshold_avg_branch=True))
    return {"threshold_position": pos, "threshold_dimension": dim}


def threshold_targets_hit(case, lat, fh):
    """Per query object of a threshold case: whether the reference matches it at ITS target candidate."""
    got = []
    for j, t in enumerate(case["targets"]):
        idx = np.nonzero((lat["x"] == t[0]) & (lat["y"] == t[1]))[0]
        assert len(idx) == 1, (t, idx)
        got.append(bool(fh[idx[0], j] >= 0))
    return got


def argmax_tie_case():
    """One query object at the origin: every candidate (x, y, any yaw) within thr of a reference object counts 1.  The reference map
    holds that object twice, in ring 1 and in ring 3 of a 0.5 m / 5 deg lattice of ~470 k candidates: the equal maxima lie more than
    256 * 256 candidates apart (a later grid-stride trip of k_place_argmax), in other workgroups, and neighbouring yaws tie inside one
    workgroup."""
    ref = np.zeros((2, 7))
    ref[0, :3] = (1.0, -6.25, 0.25)
    ref[1, :3] = (1.0, 17.25, 12.25)
    qry = np.zeros((1, 7))
    qry[0, 0] = 1.0
    return dict(ref7=ref, qry7=qry,
                params=place_params(dilation_factor=1.0, search_xy_step_size=0.5, search_yaw_step_size=math.radians(5.0),
                                    ignore_dimension=1, match_threshold_position=0.5),
                edges=dict(nq=1, max_count=1, ties_further_than_a_grid_stride=True, ties_in_other_workgroups=True,
                           ties_inside_one_workgroup=True))


def argmax_tie_edges(counts):
    tied = np.nonzero(counts == counts.max())[0]
    first = int(tied[0])
    far = tied[tied - first > 256 * 256]
    return dict(ties_further_than_a_grid_stride=len(far) > 0,
                ties_in_other_workgroups=bool(len(far) and ((far // 256) % 256 != (first // 256) % 256).any()),
                ties_inside_one_workgroup=bool(((tied[1:] - tied[:-1] == 1) & (tied[1:] // 256 == tied[:-1] // 256)).any()),
                first_tie_not_in_first_trip=first >= 256 * 256, n_tied=int(len(tied)), first=first)


def full_size_pair(rings):
    """The 792 / 554-object pair of the benchmark's synthetic_forest_792 leg (the same generator and seed, restated as test data) at
    the forest parameters, over the first `rings` rings."""
    rng = np.random.default_rng(792)
    n = 792
    big = np.zeros((n, 7))
    big[:, 0] = rng.integers(1, 4, n)
    big[:, 1:3] = rng.uniform(-105.0, 105.0, (n, 2))
    big[:, 3] = rng.normal(0, 0.3, n)
    big[:, 4:7] = rng.uniform(0.3, 2.0, (n, 3))
    keep = rng.permutation(n)[: int(0.7 * n)]
    q = big[keep].copy()
    yaw, shift = 0.6, np.array([7.5, -4.0])
    c, sn = np.cos(-yaw), np.sin(-yaw)
    xy = q[:, 1:3] - shift
    q[:, 1] = c * xy[:, 0] - sn * xy[:, 1]
    q[:, 2] = sn * xy[:, 0] + c * xy[:, 1]
    q[:, 1:3] += rng.normal(0, 0.05, q[:, 1:3].shape)
    for m in (big, q):
        m[:, 1:3] -= m[:, 1:3].mean(axis=0)
    return dict(ref7=np.ascontiguousarray(big), qry7=np.ascontiguousarray(q),
                params=place_params(ignore_dimension=1, search_yaw_step_size=np.deg2rad(5.0), search_xy_step_size=0.5, max_rings=rings),
                edges=dict(nq=554, chunks=9, last_chunk_fill=42))


FULL_SIZE_RINGS = 1


# On-chip capacity of the two sweep kernels (150 KiB of LDS): bucketed kernel 16 B per object of either map with ignore_dimension,
# 40 B without, + 8 B per query object + 16; plain kernel (SLIDE_PLACE_PLAIN=1) 48 B per reference object.
LDS_BYTES = 150 * 1024


def bucketed_max_nr(nq, ignore_dimension):
    per = 16 if ignore_dimension else 40
    return (LDS_BYTES - 16 - 8 * nq) // per - nq


def plain_max_nr():
    return LDS_BYTES // 48


def capacity_case(nr, ignore_dimension, seed=0):
    """nr reference objects of ONE label (a single bucket of several thousand) against three query objects on a 49-cell lattice."""
    rng = np.random.default_rng(100 + seed)
    ref = np.zeros((nr, 7))
    ref[:, 0] = 1.0
    ref[:, 1:3] = rng.uniform(-6.0, 6.0, (nr, 2))
    ref[:, 4:7] = rng.uniform(0.3, 2.0, (nr, 3))
    ref[::2, 5:7] = 0.0
    qry = np.zeros((3, 7))
    qry[:, 0] = 1.0
    qry[:, 1:3] = rng.uniform(-3.0, 3.0, (3, 2))
    qry[:, 4:7] = rng.uniform(0.3, 2.0, (3, 3))
    return dict(ref7=ref, qry7=qry, edges={},
                params=place_params(dilation_factor=1.0, disable_yaw_search=1, search_xy_step_size=2.0, ignore_dimension=ignore_dimension,
                                    match_threshold_position=0.06, match_threshold_dimension=0.3))


# ---- SlideGraph triangle matching ----------------------------------------------------------------------------------------------------
def triangle_sorted(tri):
    """(n, 3, 2) -> sorted centroid distances (n, 3) and the vertices re-ordered by a STABLE ascending sort of them."""
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 2)
    cx = np.divide(np.add(np.add(tri[:, 0, 0], tri[:, 1, 0]), tri[:, 2, 0]), 3.0)
    cy = np.divide(np.add(np.add(tri[:, 0, 1], tri[:, 1, 1]), tri[:, 2, 1]), 3.0)
    dx, dy = np.subtract(tri[:, :, 0], cx[:, None]), np.subtract(tri[:, :, 1], cy[:, None])
    d = np.sqrt(np.add(np.multiply(dx, dx), np.multiply(dy, dy)))
    o = np.argsort(d, axis=1, kind="stable")
    return np.take_along_axis(d, o, axis=1), np.take_along_axis(tri, o[:, :, None], axis=1), d


def triangle_rows(tm, td, thr):
    """pts (n_pairs, 3, 4) rows [model x, model y, data x, data y] and diffs, pairs in model-major order."""
    dm, xm, _ = triangle_sorted(tm)
    dd, xd, _ = triangle_sorted(td)
    if len(dm) == 0 or len(dd) == 0:
        return np.zeros((0, 3, 4)), np.zeros(0), np.zeros((len(dm), len(dd)))
    e = np.subtract(dm[:, None, :], dd[None, :, :])
    sq = np.multiply(e, e)
    diff = np.sqrt(np.add(np.add(np.add(0.0, sq[:, :, 0]), sq[:, :, 1]), sq[:, :, 2]))
    i, j = np.nonzero(np.less(diff, thr))                                 # row-major = model-major, data-minor
    pts = np.concatenate([xm[i], xd[j]], axis=2)
    return pts, diff[i, j], diff


_SPECIAL_TRIANGLES = [
    [(0.0, 0.0), (4.0, 0.0), (2.0, 3.0)],        # isosceles: d0 == d1 exactly (sqrt(5)), d2 = 2
    [(2.0, 3.0), (0.0, 0.0), (4.0, 0.0)],        # the same, rotated vertex order
    [(4.0, 0.0), (2.0, 3.0), (0.0, 0.0)],
    [(-1.0, 0.0), (0.0, 0.0), (1.0, 0.0)],       # collinear: d = 1, 0, 1
    [(1.0, 0.0), (-1.0, 0.0), (0.0, 0.0)],
    [(2.5, -1.5), (2.5, -1.5), (2.5, -1.5)],     # degenerate: three equal distances (0, 0, 0)
    [(0.0, 5.0), (0.0, -5.0), (0.0, 0.0)],       # collinear, two equal
]


def _random_triangles(rng, n):
    return rng.uniform(-30, 30, (n, 1, 2)) + rng.uniform(-4, 4, (n, 3, 2))


def triangle_cases():
    """name -> dict(tm, td, thr, edges)."""
    out = {}
    rng = np.random.default_rng(21)
    special = np.array(_SPECIAL_TRIANGLES)

    def moved(tri, rng, noise):
        """rigidly moved, vertex-permuted copies: the same sorted distances up to `noise`"""
        res = []
        for t in tri:
            a = rng.uniform(-np.pi, np.pi)
            R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
            res.append((t @ R.T + rng.uniform(-5, 5, 2) + rng.normal(0, noise, (3, 2)))[rng.permutation(3)])
        return np.array(res)
    for ntm, ntd in ((0, 5), (5, 0), (1, 1), (3, 63), (4, 64), (5, 65), (7, 129), (9, 200)):
        tm = _random_triangles(rng, ntm)
        td = _random_triangles(rng, ntd)
        if ntm and ntd:                       # every data triangle a moved copy of a model triangle, except model triangle 1 of >= 3
            src = np.array([i for i in range(ntm) if not (ntm >= 3 and i == 1)])
            td = moved(tm[src[rng.integers(0, len(src), ntd)]], rng, 0.004)
        out[f"tm{ntm}_td{ntd}"] = dict(tm=tm, td=td, thr=0.02, edges=dict(ntm=ntm, ntd=ntd, unmatched_model_between_matched=ntm >= 3 and ntd > 0,
                                                    rank_carries_across_rounds=ntm > 0 and ntd > 64))
    tm = np.concatenate([special, _random_triangles(rng, 6)])
    td = np.concatenate([special[::-1], moved(tm, rng, 0.0), special])
    out["special_shapes"] = dict(tm=tm, td=td, thr=0.05, edges=dict(two_equal_distances=True, three_equal_distances=True))
    tm, td = _random_triangles(rng, 6), _random_triangles(rng, 130)
    out["every_pair_matches"] = dict(tm=tm, td=td, thr=1e6, edges=dict(all_pairs=True, ntm=6, ntd=130, rows=780, rank_carries_across_rounds=True))
    # diff == thr exactly: thr is the float64 diff of one pair (that pair must NOT be emitted), and one unit in the last place above it
    tm = _random_triangles(rng, 5)
    td = moved(tm[[0, 1, 2, 3, 4] * 15], rng, 0.02)
    _, _, diff = triangle_rows(tm, td, 1.0)
    cand = np.argwhere((diff > 0.01) & (diff < 0.05))
    i, j = cand[len(cand) // 2]
    out["diff_equals_thr"] = dict(tm=tm, td=td, thr=float(diff[i, j]), pair=(int(i), int(j)), edges=dict(pair_at_thr_excluded=True))
    out["diff_one_ulp_below_thr"] = dict(tm=tm, td=td, thr=math.nextafter(float(diff[i, j]), math.inf), pair=(int(i), int(j)),
                                         edges=dict(pair_below_thr_included=True))
    return out


def triangle_edges(case):
    tm, td, thr = case["tm"], case["td"], case["thr"]
    pts, diffs, diff = triangle_rows(tm, td, thr)
    e = dict(ntm=len(tm), ntd=len(td), rows=len(diffs))
    hit = diff < thr if diff.size else np.zeros((len(tm), len(td)), bool)
    per = hit.sum(axis=1)
    e["unmatched_model_between_matched"] = bool(any(per[i] == 0 and per[:i].any() and per[i + 1:].any() for i in range(len(per))))
    e["all_pairs"] = bool(hit.size and hit.all())
    e["rank_carries_across_rounds"] = bool(len(td) > 64 and any(hit[i, :64].any() and hit[i, 64:].any() for i in range(len(tm))))
    d = np.concatenate([triangle_sorted(tm)[2], triangle_sorted(td)[2]]) if len(tm) + len(td) else np.zeros((0, 3))
    eq = (d[:, 0] == d[:, 1]).astype(int) + (d[:, 1] == d[:, 2]) + (d[:, 0] == d[:, 2])
    e["two_equal_distances"] = bool((eq == 1).any())
    e["three_equal_distances"] = bool((eq == 3).any())
    if "pair" in case:
        i, j = case["pair"]
        e["pair_at_thr_excluded"] = bool(diff[i, j] == thr and not hit[i, j])
        e["pair_below_thr_included"] = bool(diff[i, j] < thr and math.nextafter(diff[i, j], math.inf) == thr and hit[i, j])
    return e


# ---- CLIPPER affinity ---------------------------------------------------------------------------------------------------------------
def _hp_exp(args):
    """exp of float64 arguments in higher precision, rounded once to float64 (mpmath when present, else numpy.longdouble)."""
    try:
        import mpmath
        mpmath.mp.prec = 200
        return np.array([float(mpmath.exp(mpmath.mpf(float(a)))) for a in args], np.float64), "mpmath"
    except ImportError:
        return np.exp(np.asarray(args, np.longdouble)).astype(np.float64), "longdouble"


def affinity(D1, D2, A, sigma, eps, mindist, affinityeps):
    """scorePairwiseConsistency (clipper.cpp:21-65 with euclidean_distance.cpp:13-31): upper triangle, decisions (`c < eps`,
    `scr > affinityeps`, `mindist`) in float64 as the reference takes them.  Returns dict(M: float64 values with numpy's exp,
    M_hp: the same entries with exp evaluated in higher precision, margin: the smallest relative distance of a higher-precision
    score from affinityeps over all pairs that reach the exp)."""
    D1, D2, A = np.asarray(D1, np.float64), np.asarray(D2, np.float64), np.asarray(A, np.int64)
    m, dim = len(A), D1.shape[1]
    M, Mhp = np.zeros((m, m)), np.zeros((m, m))
    if m < 2:
        return dict(M=M, M_hp=Mhp, margin=np.inf, exp="none")
    i, j = np.triu_indices(m, 1)
    keep = np.logical_and(A[i, 0] != A[j, 0], A[i, 1] != A[j, 1])
    i, j = i[keep], j[keep]
    s1, s2 = np.zeros(len(i)), np.zeros(len(i))
    for k in range(dim):
        a = np.subtract(D1[A[i, 0], k], D1[A[j, 0], k])
        b = np.subtract(D2[A[i, 1], k], D2[A[j, 1], k])
        s1 = np.add(s1, np.multiply(a, a))
        s2 = np.add(s2, np.multiply(b, b))
    l1, l2 = np.sqrt(s1), np.sqrt(s2)
    alive = np.ones(len(i), bool)
    if mindist > 0:
        alive = np.logical_not(np.logical_or(l1 < mindist, l2 < mindist))
    c = np.abs(np.subtract(l1, l2))
    alive = np.logical_and(alive, c < eps)
    i, j, c = i[alive], j[alive], c[alive]
    arg = np.divide(np.multiply(np.multiply(-0.5, c), c), sigma * sigma)
    scr = np.exp(arg)
    hp, how = _hp_exp(arg)
    margin = float(np.min(np.abs(hp - affinityeps) / affinityeps)) if len(hp) else np.inf
    on = scr > affinityeps
    M[i[on], j[on]] = scr[on]
    Mhp[i[on], j[on]] = hp[on]
    return dict(M=M, M_hp=Mhp, margin=margin, exp=how, n_exp=int(len(c)), n_below_affinityeps=int((~on).sum()))


def affinity_cases():
    """name -> dict(D1, D2, A, kw, edges).  The first associations are planted pairs with exact distances (points on the x axis, so a
    length is one correctly rounded sqrt of an exact square); the rest are random putative associations of a noisy sub-map."""
    out = {}
    for m, dim, mindist in ((1, 2, 0.0), (2, 3, 0.0), (127, 2, 0.0), (128, 3, 1.0), (129, 2, 1.0), (257, 3, 0.0)):
        rng = np.random.default_rng(300 + m)
        sigma, eps, aeps = 0.25, 0.5, 1e-4
        # planted: model points on the x axis at 0 and 3 (and 0 / 1 for mindist); data points so that |l1 - l2| is eps exactly, just
        # below, just above; a pair whose score is far below affinityeps needs eps > 4.3 sigma, so one case widens eps
        if m == 257:
            eps = 2.0
        P1 = [(0.0,), (3.0,), (1.0,), (math.nextafter(1.0, 0.0),), (1.25,)]
        P2 = [(0.0,), (2.5,), (math.nextafter(2.5, 3.0),), (math.nextafter(2.5, 0.0),), (1.0,), (1.0,), (0.0,)]
        pad = lambda pts: [tuple(p) + (0.0,) * (dim - 1) for p in pts]     # noqa: E731
        n1r, n2r = 30, 24
        R1 = rng.uniform(-10, 10, (n1r, dim))
        R2 = R1[rng.permutation(n1r)[:n2r]] + rng.normal(0, 0.05, (n2r, dim))
        D1 = np.concatenate([np.array(pad(P1)), R1])
        D2 = np.concatenate([np.array(pad(P2)), R2])
        # (model, data): 0-0 is the anchor.  1-1: c == eps (0 when eps = 0.5); 1-2: just inside; 1-3: just outside;
        # 2-4: l1 == mindist == 1 exactly (kept); 3-5: l1 one unit below 1 (dropped when mindist = 1); 4-6: shares nothing, c = 1.25
        planted = [(0, 0), (1, 1), (1, 2), (1, 3), (2, 4), (3, 5), (4, 6), (0, 1), (1, 0)]
        allr = [(len(P1) + a, len(P2) + b) for a in range(n1r) for b in range(n2r)]
        pick = [allr[k] for k in rng.permutation(len(allr))[:max(m - len(planted), 0)]]
        A = np.array((planted + pick)[:m], np.int32).reshape(-1, 2)
        out[f"m{m}_dim{dim}_mindist{mindist:g}"] = dict(
            D1=D1, D2=D2, A=A, kw=dict(sigma=sigma, epsilon=eps, mindist=mindist, affinityeps=aeps),
            edges=dict(m=m, dim=dim, shared_points=m >= 9, c_equals_eps=m >= 9 and eps == 0.5, below_affinityeps=m == 257,
                       at_mindist=m >= 9 and mindist > 0))
    return out


def affinity_edges(case, ref):
    D1, D2, A, kw = case["D1"], case["D2"], np.asarray(case["A"], np.int64), case["kw"]
    m = len(A)
    e = dict(m=m, dim=D1.shape[1])
    i, j = np.triu_indices(m, 1)
    e["shared_points"] = bool(((A[i, 0] == A[j, 0]) | (A[i, 1] == A[j, 1])).any())
    M = ref["M"]
    e["c_equals_eps"] = e["at_mindist"] = False
    if m >= 9:
        l1 = abs(D1[A[0, 0], 0] - D1[A[1, 0], 0])
        c = [abs(l1 - abs(D2[A[0, 1], 0] - D2[A[k, 1], 0])) for k in (1, 2, 3)]
        e["c_equals_eps"] = bool(c[0] == kw["epsilon"] and c[1] < kw["epsilon"] < c[2] and M[0, 1] == 0 and M[0, 2] > 0 and M[0, 3] == 0)
        e["at_mindist"] = bool(kw["mindist"] > 0 and D1[A[4, 0], 0] == kw["mindist"] and D1[A[5, 0], 0] < kw["mindist"]
                               and M[0, 4] > 0 and M[0, 5] == 0)
    e["below_affinityeps"] = bool(ref.get("n_below_affinityeps", 0) > 0)
    return e
