"""Child process of tests/test_gpu_place_edges.py: sweeps the named cases with whatever sweep kernel the environment selects
(SLIDE_PLACE_PLAIN is read once per process) and writes what the kernels returned to an .npz; the parent compares.
usage: place_plain_child.py <out.npz> <case> [<case> ...]   (case = a name of place_cases.sweep_cases() or capacity:<nr>:<ignore_dim>)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    torch.zeros(1, device="cuda:0")          # torch first (tests/conftest.py)
    import slide_slam_amd as s
    import place_cases as pc
    s.device_check()
    cases = pc.sweep_cases()
    out = {}
    for name in sys.argv[2:]:
        if name.startswith("capacity:"):
            _, nr, ign = name.split(":")
            case = pc.capacity_case(int(nr), int(ign))
        else:
            case = cases[name]
        gp = s.place_default_params(**case["params"])
        r = s.match_maps_sweep(case["ref7"], case["qry7"], gp)
        key = name.replace(":", "_")
        out[key + "/status"] = np.array(r["status"])
        out[key + "/candidates"] = np.array(r["candidates"])
        out[key + "/best_index"] = np.array(r["best_index"])
        out[key + "/xyyaw"] = r["xyyaw"]
        out[key + "/inliers"] = r["inliers"]
        print(name, r["status"], r["candidates"], file=sys.stderr, flush=True)
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
