# Per-launch device time of named kernels over the last exact joint passes of a rocprofv3 kernel trace (csv): median (min .. max) in
# microseconds, one line per kernel — the figures of the keep-or-revert tables under profiles/ (assembly_kernels_timing.txt,
# global_addressing_timing.txt).  Passes are delimited as in trace_exact.py (k_status_clear before a k_sep_gather).  A kernel launched
# several times per pass is listed by its position in the pass (k_border_syrk#0 = the robots' launch).
# usage: trace_launches.py <dir> [n passes] [kernel ...]        (default kernels: the ones that take the graphs as a table, + the yardsticks)
import collections
import csv
import glob
import sys

DEFAULT = ["k_schur_lb", "k_landmark_b<3>", "k_lin_lf_b", "k_pose_b", "k_backsub_sep_b", "k_border_clear_b", "k_sep_extract_b", "k_relin_b",
           "k_ghost_refresh_local", "k_estimate_b", "k_sep_pose_scatter_b", "k_border_syrk"]

rows = []
for f in glob.glob(sys.argv[1] + '/**/*kernel_trace.csv', recursive=True):
    rows += list(csv.DictReader(open(f)))
n = int(sys.argv[2]) if len(sys.argv) > 2 else 15
want = sys.argv[3:] or DEFAULT
rows.sort(key=lambda r: int(r['Start_Timestamp']))
name = lambda r: r['Kernel_Name'].split('(')[0].replace('void ', '').replace('sl::', '')
marks = [i for i, r in enumerate(rows) if name(r) == 'k_status_clear']
gathers = [i for i, r in enumerate(rows) if name(r) == 'k_sep_gather']
if len(gathers) < n + 1:
    print("not enough passes in the trace:", len(gathers)); sys.exit(1)
starts = [max(m for m in marks if m < g) for g in gathers]
sel = starts[-(n + 1):]
per = collections.defaultdict(list)       # (kernel, position in the pass) -> durations
grid = {}
for a, b in zip(sel[:-1], sel[1:]):
    seen = collections.Counter()
    for r in rows[a:b]:
        k = name(r)
        if k in want:
            per[(k, seen[k])].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
            grid[(k, seen[k])] = "x".join(str(r.get(g, "?")) for g in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"))
            seen[k] += 1
total = [0.0] * n
print(f"{n} exact joint passes; per-launch device time, us: median (min .. max), spread = max - min")
for k in want:
    pos = sorted(p for kk, p in per if kk == k)
    for p in pos:
        v = per[(k, p)]
        if len(v) != n:
            continue        # (not launched in every pass)
        s = sorted(v)
        label = k if len(pos) == 1 else f"{k}#{p}"
        print(f"{label:26s} {s[len(s) // 2]:8.2f} ({s[0]:.2f} .. {s[-1]:.2f})   spread {s[-1] - s[0]:5.2f}   grid {grid[(k, p)]}")
        if len(pos) == 1:
            total = [t + x for t, x in zip(total, v)]
s = sorted(total)
print(f"{'sum of the single launches':26s} {s[len(s) // 2]:8.2f} ({s[0]:.2f} .. {s[-1]:.2f})")
