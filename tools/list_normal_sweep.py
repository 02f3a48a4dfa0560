"""Spec S2l's parameter sweep: point-to-plane ICP on voxelised point lists with ball normals, for a grid of
radius x min_points / min_inliers, against svd on the same lists.  CPU only -- the numpy restatement of tests/test_list_normals.py
(the HIP path computes the same iterates, tests/test_list_normals.py checks that on the GPU).

Cases: the reference's Kinect voxel clouds as perturbed self-alignments (synth.pose_from_seed(77, 2.0, 0.03), against the identity),
synth.make_pair pairs voxelised like readimage (against T_gt; BASELINE.md section 4's workload and the low-noise one), and Kinect
dep1 -> dep2 (no ground truth: the distance to svd's pose is printed).  Usage: python tools/list_normal_sweep.py [workers]"""
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import oracle_lib as O                                  # noqa: E402
import test_list_normals as L                           # noqa: E402
from slam3d_gx_amd import synth                         # noqa: E402

RADII = (0.06, 0.08, 0.10, 0.12, 0.15)
COUNTS = ((5, 4), (10, 8), (20, 15))
INLIER_DIST = 0.01


def cases():
    v1, v2 = L.kinect_voxel_clouds()
    Ti = synth.pose_from_seed(77, 2.0, 0.03)
    out = [("dep1->dep1", L.as_list(v1), L.as_list(v1), Ti, np.eye(4)), ("dep2->dep2", L.as_list(v2), L.as_list(v2), Ti, np.eye(4))]
    for wl, tag in (("baseline_md", "BASELINE.md"), ("low_noise", "low-noise")):
        for seed in (1000, 1001):
            s, t, Tg = L.synthetic_voxel_pair(seed, wl)
            out.append((f"{tag} {seed}", L.as_list(s), L.as_list(t), None, Tg))
    out.append(("dep1->dep2", L.as_list(v1), L.as_list(v2), None, None))
    return out


def run(cfg):
    CASES = cases()
    res = []
    svd12 = None
    for name, s, t, Ti, Tg in CASES:
        if name == "dep1->dep2":
            svd12 = L.icp_list_numpy(s, t, None, None, estimator=1)[-1]
        if cfg is None:
            T = L.icp_list_numpy(s, t, None, Ti, estimator=1)[-1]
        else:
            nrm = L.list_normals_numpy(t, radius=cfg[0], min_points=cfg[1], min_inliers=cfg[2], inlier_dist=INLIER_DIST)
            T = L.icp_list_numpy(s, t, nrm, Ti, estimator=0)[-1]
        ref = Tg if Tg is not None else svd12
        rot, tr = O.pose_error(ref, T)
        res.append((rot * 1e3, tr * 1e3))
    return cfg, res


def main():
    workers = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    cfgs = [None] + [(r, mp, mi) for r in RADII for mp, mi in COUNTS]
    names = [c[0] for c in cases()]
    with Pool(workers) as pool:
        rows = pool.map(run, cfgs)
    print("| radius / min_points / min_inliers | " + " | ".join(names) + " | Σ trans (no dep1->dep2) |")
    print("|---" * (len(names) + 2) + "|")
    for cfg, res in rows:
        label = "svd" if cfg is None else f"{cfg[0]:.2f} / {cfg[1]} / {cfg[2]}"
        tot = sum(tr for (_, tr), n in zip(res, names) if n != "dep1->dep2")
        print(f"| {label} | " + " | ".join(f"{r:.2f} / {t:.2f}" for r, t in res) + f" | {tot:.1f} |")


if __name__ == "__main__":
    main()
