"""`icp_cloud_estimator` (parameters.yaml): the estimator of the point lists `icp_cloud: voxel` aligns -- svd (the default), point2plane
or plane, whose normals come from metric balls (DESIGN.md spec S2l, keys icp_list_normal_*)."""
import os
import subprocess

import numpy as np
import pytest

import test_host_frontend as HF
from slam3d_gx_amd import synth


def _voxel_sequence(tmp_path, n_steps=4):
    step = synth.pose_from_seed(4242, max_angle_deg=1.0, max_trans=0.02)
    poses = [np.eye(4)]
    for _ in range(n_steps):
        poses.append(step @ poses[-1])
    intr, data = HF._sequence(tmp_path, poses)
    (data / "pcd").mkdir()
    head = ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgba\nSIZE 4 4 4 4\nTYPE F F F U\nCOUNT 1 1 1 1\n"
            "WIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n")
    from PIL import Image
    for k in range(len(poses)):
        d = np.array(Image.open(str(data / "dep_index" / f"{k + 1}.png"))).astype(np.uint16)
        c = synth.backproject_numpy(d, intr, z_filter=1e9).reshape(-1, 4)
        c = c[np.isfinite(c[:, 2])].copy()
        c[:, 3] = np.float32(0)
        (data / "pcd" / f"{k + 1}.pcd").write_bytes(head.format(n=c.shape[0]).encode() + c.tobytes())
    return poses, intr, data


def _params(tmp_path, intr, data, extra):
    (tmp_path / "parameters.yaml").write_text(
        HF.PARAMS.format(src=str(data), mpc=10.0, fx=intr.fx, fy=intr.fy, cx=intr.cx, cy=intr.cy, w=320, h=240, lc="no", planes="no",
                         pcd="yes", extra="icp_cloud: voxel\n" + extra))


def test_unknown_cloud_estimator_is_a_fatal_configuration_error(tmp_path):
    HF._build_host()
    poses, intr, data = _voxel_sequence(tmp_path, 1)
    _params(tmp_path, intr, data, "icp_cloud_estimator: kabsch\n")
    bad = subprocess.run([os.path.join(HF.HOST, "run_SLAM"), "1"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert bad.returncode != 0 and "icp_cloud_estimator" in bad.stderr, bad.stderr[-2000:]


@pytest.mark.gpu
@pytest.mark.parametrize("estimator", ["point2plane", "plane"])
def test_run_slam_tracks_voxel_lists_with_ball_normals(gpu_lib, tmp_path, estimator):
    """run_SLAM on PCD input with `icp_cloud: voxel` and `icp_cloud_estimator: point2plane` (or plane with its window fallback) tracks
    the synthetic sequence: the robot position within 2 cm of the ground truth at quarter resolution (the S2l sweep: 1-15 mm per
    full-resolution alignment), every alignment a real one (inliers > 1000 of the voxel list).  The svd default run of the same
    sequence gives other numbers, so the key reaches the device; the icp_list_normal_* keys do too."""
    HF._build_host()
    poses, intr, data = _voxel_sequence(tmp_path)
    n = len(poses) - 1
    logs = {}
    for name, extra in (("svd", ""), (estimator, f"icp_cloud_estimator: {estimator}\n"),
                        ("r12", f"icp_cloud_estimator: {estimator}\nicp_list_normal_radius: 0.12\n")):
        _params(tmp_path, intr, data, extra)
        out = subprocess.run([os.path.join(HF.HOST, "run_SLAM"), str(n)], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        logs[name] = (tmp_path / "data" / "error_of_transform.log").read_text().split()
        if name == estimator:
            got = [int(t.split()[2]) for t in out.stdout.splitlines() if t.startswith("multiICP::inliers")]
            assert got and all(a > 1000 for a in got), got
            traj = np.loadtxt(str(tmp_path / "data" / "trajectory_icp.txt"))
            assert traj.shape == (n + 1, 8)
            for k in range(1, n + 1):
                cam_to_world = np.linalg.inv(poses[k])
                assert np.abs(traj[k, 1:4] - cam_to_world[:3, 3]).max() < 2e-2, (k, traj[k, 1:4], cam_to_world[:3, 3])
    assert logs[estimator] != logs["svd"] and logs["r12"] != logs[estimator]
