#!/usr/bin/env python3
"""How the kernels address memory, read from their gfx950 assembly (CPU only: hipcc cross-compiles).

    python tools/isa_addressing.py [file.hip ...] [--all] [--csrc DIR]

Compiles the named files of slide_slam_amd/csrc (default: solver_kernels.hip, pcg_kernels.hip, obs_gate_kernels.hip) with build.py's
flags plus `--cuda-device-only -S` and prints, per kernel: flat_* and global_* instructions, the vector-memory waits — full
(`s_waitcnt vmcnt(0) lgkmcnt(0)`: what every use of a flat load's value needs), `vmcnt(0)` alone, and partial (`vmcnt(N)`, N > 0:
later loads stay in flight) —, ds_* instructions, VGPRs, scratch bytes per lane and waves per SIMD.  Without --all only the kernels
that take a pointer to GraphDev are listed (the batched pass's kernels).

A struct of pointers that a kernel reads from memory gives generic pointers, and every access through one is a flat_* instruction;
graph_dev.hpp therefore declares the members as global pointers for the device.  tests/test_isa_addressing.py asserts the outcome.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from slide_slam_amd import build as B  # noqa: E402

DEFAULT_FILES = ["solver_kernels.hip", "pcg_kernels.hip", "obs_gate_kernels.hip"]
GRAPH_ARG = re.compile(r"\bGraphDev const\*")      # in a demangled kernel name: takes the graphs as a table in memory

_LABEL = re.compile(r"^([A-Za-z_][\w$.]*):")
_WAIT = re.compile(r"^s_waitcnt\b(.*)")
_VM = re.compile(r"vmcnt\((\d+)\)")
_LGKM = re.compile(r"lgkmcnt\((\d+)\)")


def hipcc_available() -> bool:
    return os.path.exists(B.HIPCC) or shutil.which(B.HIPCC) is not None


def compile_asm(name: str, csrc: str = B.CSRC, out_dir: str | None = None) -> str:
    """Assembly text of one csrc file, built with build.py's flags for that file."""
    extra = dict(B.SOURCES)[name]
    tmp = out_dir or tempfile.mkdtemp(prefix="isa_")
    out = os.path.join(tmp, name.replace(".hip", ".s"))
    try:
        p = subprocess.run([B.HIPCC, *B.COMMON, *extra, "--cuda-device-only", "-S", os.path.join(csrc, name), "-o", out],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {name}:\n{p.stdout}")
        with open(out) as f:
            return f.read()
    finally:
        if out_dir is None:
            shutil.rmtree(tmp, ignore_errors=True)


def demangle(names: list[str]) -> dict[str, str]:
    filt = os.path.join(os.path.dirname(os.path.realpath(B.HIPCC)), "..", "llvm", "bin", "llvm-cxxfilt")
    if not os.path.exists(filt):
        filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not filt or not names:
        return {n: n for n in names}
    out = subprocess.run([filt, *names], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    return dict(zip(names, out))


def parse(asm: str) -> dict[str, dict]:
    """mangled kernel name -> counts.  A kernel's text runs from its label to .Lfunc_end; its resources follow as comments."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    res: dict[str, dict] = {}
    cur = None
    tail = None      # the kernel whose resource comments are being read
    for raw in asm.splitlines():
        line = raw.strip()
        m = _LABEL.match(raw)
        if m and m.group(1) in kernels and m.group(1) not in res:
            cur = res[m.group(1)] = dict(flat=0, flat_load=0, flat_store=0, flat_atomic=0, glob=0, wait_full=0, wait_vm0=0,
                                         wait_partial=0, ds=0, vgprs=None, scratch=None, waves=None)
            tail = None
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                tail, cur = cur, None
                continue
            op = line.split(None, 1)[0] if line else ""
            if op.startswith("flat_"):
                cur["flat"] += 1
                for k in ("flat_load", "flat_store", "flat_atomic"):
                    if op.startswith(k):
                        cur[k] += 1
            elif op.startswith("global_"):
                cur["glob"] += 1
            elif op.startswith("ds_"):
                cur["ds"] += 1
            else:
                w = _WAIT.match(line)
                if w:
                    vm, lg = _VM.search(w.group(1)), _LGKM.search(w.group(1))
                    if vm and int(vm.group(1)) > 0:
                        cur["wait_partial"] += 1
                    elif vm and lg and int(lg.group(1)) == 0:
                        cur["wait_full"] += 1
                    elif vm:
                        cur["wait_vm0"] += 1
        elif tail is not None:
            for key, pat in (("vgprs", r";\s*NumVgprs:\s*(\d+)"), ("scratch", r";\s*ScratchSize:\s*(\d+)"), ("waves", r";\s*Occupancy:\s*(\d+)")):
                mm = re.match(pat, line)
                if mm:
                    tail[key] = int(mm.group(1))
            if line.startswith(".amdhsa_kernel") or (m and not line.startswith(";")):
                tail = None
    return res


def table(files: list[str], csrc: str = B.CSRC, only_graph_tables: bool = True) -> list[dict]:
    rows = []
    for name in files:
        res = parse(compile_asm(name, csrc))
        dm = demangle(list(res))
        for k, c in res.items():
            if only_graph_tables and not GRAPH_ARG.search(dm[k]):
                continue
            rows.append(dict(file=name, kernel=dm[k], **c))
    return rows


def short(name: str) -> str:
    """sl::k_landmark_b<3>(sl::GraphDev const*) -> k_landmark_b<3>"""
    head = name.split("(", 1)[0].replace("sl::", "")
    return head.split(" ")[-1]


def main(argv: list[str]) -> int:
    csrc = B.CSRC
    if "--csrc" in argv:
        i = argv.index("--csrc")
        csrc = argv[i + 1]
        del argv[i:i + 2]
    everything = "--all" in argv
    files = [a for a in argv if not a.startswith("--")] or DEFAULT_FILES
    rows = table([os.path.basename(f) for f in files], csrc, not everything)
    print(f"{'kernel':38s} {'flat_*':>6s} {'global_*':>8s} {'full':>5s} {'vm0':>4s} {'partial':>7s} {'ds_*':>5s} {'VGPRs':>5s} {'scratch':>7s} {'waves':>5s}")
    last = None
    for r in rows:
        if r["file"] != last:
            print(f"-- {r['file']}")
            last = r["file"]
        print(f"{short(r['kernel']):38s} {r['flat']:6d} {r['glob']:8d} {r['wait_full']:5d} {r['wait_vm0']:4d} {r['wait_partial']:7d} {r['ds']:5d} "
              f"{r['vgprs']!s:>5s} {r['scratch']!s:>7s} {r['waves']!s:>5s}")
    print(f"{len(rows)} kernels, {sum(r['flat'] for r in rows)} flat_* instructions, {sum(1 for r in rows if r['flat'])} kernels with at least one")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
