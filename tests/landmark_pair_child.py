"""Child process of test_gpu_landmark_pairs.py (not a test): builds dup40 under the chart given, runs every planted pair of both classes
through SlideGraph.landmark_pair_mahalanobis and .get_landmark_pair_covariances with whatever SLIDE_LM_PAIR_SUBSTITUTE the parent put
into the environment, and writes the results to the .npz named.  Usage: landmark_pair_child.py <chart> <out.npz>"""
import os
import sys

import torch  # noqa: F401  (before the product library, as tests/conftest.py does)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np  # noqa: E402

import slide_slam_amd as s  # noqa: E402

import landmark_pair_cases as lp  # noqa: E402


def main(chart, path):
    s.device_check()
    G, W = lp.device_graph(s, "dup40", chart)
    out = {}
    for kind in ("point", "cylinder"):
        pairs = np.array([(a, b) for a, b, _ in W.pairs[kind]], np.uint64)
        res = G.landmark_pair_mahalanobis(lp.CLS[kind], pairs, lp.SIGMA[kind])
        cov, st, route = G.get_landmark_pair_covariances(lp.CLS[kind], pairs)
        for f in ("d2", "C", "r", "route", "status"):
            out[f"{kind}_{f}"] = res[f]
        out[f"{kind}_cov"], out[f"{kind}_cov_route"], out[f"{kind}_cov_status"] = cov, route, st
        out[f"{kind}_lm"] = np.array([np.concatenate([G.get_landmark(lp.CLS[kind], int(a))[1], G.get_landmark(lp.CLS[kind], int(b))[1]]) for a, b in pairs])
    np.savez(path, **out)


if __name__ == "__main__":
    main(int(sys.argv[1]), sys.argv[2])
