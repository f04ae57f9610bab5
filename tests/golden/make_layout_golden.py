"""Records the layout tables of a set of graphs into tests/golden/layout_parent.npz: the outputs of SlideGraph.tile_profile,
border_profile, segments and segment_table (int32) and, for shards of a batch, stats()["chol_dim"].

The file was recorded once, on the GPU, at the commit BEFORE the layout planning moved into csrc/host_layout.hpp (its hash is stored
under "parent"); test_gpu_layout_tables.py rebuilds the same graphs case by case (cases()) and requires every array to match.  The graphs come
from the existing generators (joint_graphs, stream_graphs, landmark_merge_cases); each takes seconds.

    python tests/golden/make_layout_golden.py <commit hash> [output.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

BORDERS = {63: (9, 0, 0), 64: (1, 5, 4), 65: (2, 5, 2), 128: (5, 10, 1), 129: (3, 10, 6)}      # test_gpu_joint_step.BORDERS
STREAM_P = 50              # T = 1 .. 5: S is allocated for 4 block columns first, so the last updates re-allocate it


def _i32(v):
    return np.asarray(v, np.int32).reshape(-1)


def tables(G):
    """The four getters of one graph as int32 arrays."""
    segs, n_sep = G.segments()
    tab = G.segment_table()
    out = {"prof": _i32(G.tile_profile()), "bfirst": _i32(G.border_profile()), "segs": _i32([v for s in segs for v in s] + [n_sep])}
    out["seg_ends"] = _i32(tab[0] if tab else [])
    out["seg_first"] = _i32(tab[1] if tab else [])
    return out


def joint_tables(s, J, segments=None):
    """The shards of J in one CholBatch, set up for exact joint passes as test_gpu_joint_step.Run does; segments: SLIDE_SEGMENTS."""
    import torch
    import joint_graphs as jg
    from slide_slam_amd.distributed import PassDriver, setup_local_shards
    dev = torch.device("cuda", 0)
    old = os.environ.get("SLIDE_SEGMENTS")
    if segments is None:
        os.environ.pop("SLIDE_SEGMENTS", None)
    else:
        os.environ["SLIDE_SEGMENTS"] = str(segments)
    shards, assoc = jg.build(J, lambda: s.SlideGraph(s.default_params(pose_chart=0)))
    batch = s.CholBatch(J.R)
    out = {}
    try:
        for t, sh in enumerate(shards):
            sh.graph.join_chol_batch(batch, t)
        bufs, info = setup_local_shards(shards, None, device=dev, assoc=assoc)
        drv = PassDriver(shards, bufs, info["n_slots"], batch=batch, device=dev, arrow=True, sep_dim=info["sep_dim"],
                         sep_prof=info.get("sep_prof"))
        if J.relmeas:
            assert drv.setup_ghosts(J.relmeas) > 0
        for t, sh in enumerate(shards):
            for k, v in tables(sh.graph).items():
                out[f"r{t}/{k}"] = v
            out[f"r{t}/chol_dim"] = _i32([sh.graph.stats()["chol_dim"]])
    finally:
        for sh in shards:
            sh.graph.join_chol_batch(None)
        if old is None:
            os.environ.pop("SLIDE_SEGMENTS", None)
        else:
            os.environ["SLIDE_SEGMENTS"] = old
    return out


def stream_tables(s):
    """A single-robot stream of STREAM_P frames, solved after each: the tile profile after every update, end to end."""
    import stream_graphs as sg
    G = s.SlideGraph(s.default_params(pose_chart=0))
    S = sg.Stream([G], STREAM_P, seed=0)
    profs = []
    for k in range(STREAM_P):
        S.frame(k)
        assert G.solve() == 0
        profs.append(_i32(G.tile_profile()))
    out = {"prof_len": _i32([len(p) for p in profs]), "prof_flat": np.concatenate(profs)}
    out.update({"end/" + k: v for k, v in tables(G).items()})
    return out


def merge_tables(s):
    """landmark_merge_cases' count graph (two point landmarks, 32 factors each, on disjoint halves of 64 poses) before and after
    merge_landmarks joins them: the merged landmark couples the first pose to the last."""
    import landmark_merge_cases as lm
    G, _ = lm.device_graph(s, ("count", 2, 32, 32), 0)
    out = {"before/" + k: v for k, v in tables(G).items()}
    res = G.merge_landmarks(2, [(0, 1)], False)
    assert res["status"].tolist() == [0]
    out.update({"after/" + k: v for k, v in tables(G).items()})
    return out


def cases(s):
    """{case name: a function that builds the case's graphs -> {table name: int32 array}}"""
    import joint_graphs as jg
    out = {"sizes": lambda: joint_tables(s, jg.sizes_case([10, 33, 65, 150])),
           "sizes_private": lambda: joint_tables(s, jg.sizes_case([150, 10, 65, 33], private_only=(1,))),
           "shared_mix4": lambda: joint_tables(s, jg.shared_mix_case(4, sizes=[12] * 4)),
           "relmeas": lambda: joint_tables(s, jg.relmeas_case(R=2, n_rel=3)),
           "walk": lambda: joint_tables(s, jg.walk_case()),
           "column_cap": lambda: joint_tables(s, jg.column_cap_case()),
           "stream": lambda: stream_tables(s),
           "merge": lambda: merge_tables(s)}
    for n in (1, 2, 3, 4):
        out[f"segments{n}"] = lambda n=n: joint_tables(s, jg.segments_case(R=2, P=150), segments=n)
    for coords, mix in sorted(BORDERS.items()):
        out[f"border{coords}"] = lambda mix=mix: joint_tables(s, jg.border_case(mix))
    return out


CASE_NAMES = ["sizes", "sizes_private", "shared_mix4", "relmeas", "walk", "column_cap", "stream", "merge"] + \
             [f"segments{n}" for n in (1, 2, 3, 4)] + [f"border{c}" for c in sorted(BORDERS)]


def record(s):
    """{case name/table name: int32 array} over every case."""
    return {f"{name}/{k}": v for name, fn in cases(s).items() for k, v in fn().items()}


if __name__ == "__main__":
    import torch  # noqa: F401   (torch before the product library: tests/conftest.py)
    torch.zeros(1, device="cuda:0")
    import slide_slam_amd as s
    s.device_check()
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "layout_parent.npz")
    arrays = record(s)
    np.savez_compressed(path, parent=np.array(sys.argv[1]), **arrays)
    print(f"{len(arrays)} arrays, {sum(a.size for a in arrays.values())} words -> {path}")
