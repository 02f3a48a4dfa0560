"""Oracle and HIP path against the committed golden vectors (tests/golden/*.json)."""
import hashlib
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from slam3d_gx_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "synthetic_golden.json")))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def unhx(v):
    return np.array([float.fromhex(x) for x in v])


def _inputs(c):
    pr = synth.make_pair(c["seed"], c["width"], c["height"])
    assert pr.sha256() == c["depth_sha256"], "synthetic generator drifted: depth images differ from the golden inputs"
    return pr, synth.backproject_numpy(pr.depth_src, pr.intr), synth.backproject_numpy(pr.depth_tgt, pr.intr)


def _check(c, n_src, n_tgt, inliers, status, norm, T_final, sums_last, idx, d2):
    assert (n_src, n_tgt, inliers, status) == (c["n_src"], c["n_tgt"], c["inliers"], c["status"])
    assert sha(idx) == c["idx_sha256"], "correspondence indices differ from the golden vector"
    assert sha(d2) == c["d2_sha256"]
    for i, j in c["idx_first64"] + c["idx_last64"]:
        assert idx[i] == j
    Tg = unhx(c["T_final"]).reshape(4, 4)
    rot, tr = O.pose_error(Tg, T_final)
    assert rot <= 1e-4 and tr <= 1e-4                      # the contractual bar
    assert np.array_equal(T_final.reshape(-1), Tg.reshape(-1))   # and bit-identical by design
    assert np.array_equal(sums_last, unhx(c["sums_last"]))
    assert norm == float.fromhex(c["norm"])


SMALL = [c for c in GOLD["cases"] if c["width"] == 160]
FULL = [c for c in GOLD["cases"] if c["width"] == 640]


@pytest.mark.parametrize("c", SMALL, ids=lambda c: f"{c['seed']}-est{c['estimator']}")
def test_oracle_reproduces_golden_small(c):
    pr, s4, t4 = _inputs(c)
    for method in (0, 1):
        r = O.icp(s4, t4, O.params(pr.intr, estimator=c["estimator"], iterations=c["iterations"], nn_method=method))
        _check(c, r["n_src"], r["n_tgt"], r["inliers"], r["status"], r["norm"], r["T_trace"][-1], r["sums_trace"][-1], r["idx"], r["d2"])
    if c["estimator"] == 0:
        assert sha(O.normals(t4, O.params(pr.intr))) == c["normals_sha256"]


@pytest.mark.parametrize("c", FULL, ids=lambda c: f"{c['seed']}-est{c['estimator']}")
def test_oracle_reproduces_golden_full_size(c):
    pr, s4, t4 = _inputs(c)
    r = O.icp(s4, t4, O.params(pr.intr, estimator=c["estimator"], iterations=c["iterations"], nn_method=1))
    _check(c, r["n_src"], r["n_tgt"], r["inliers"], r["status"], r["norm"], r["T_trace"][-1], r["sums_trace"][-1], r["idx"], r["d2"])


@pytest.mark.gpu
@pytest.mark.parametrize("c", GOLD["cases"], ids=lambda c: f"{c['width']}-{c['seed']}-est{c['estimator']}")
def test_hip_path_reproduces_golden(gpu_lib, c):
    """GPU vs committed vectors only -- no oracle call in the loop."""
    from slam3d_gx_amd import capi
    pr, s4, t4 = _inputs(c)
    with capi.IcpHandle(capi.default_params(pr.intr, estimator=c["estimator"], iterations=c["iterations"])) as h:
        r = h.align(s4, t4)
        idx, d2 = h.get_correspondences(0)
        Tt, St = h.get_trace(0)
        if c["estimator"] == 0:
            nrm = h.get_clouds(0, normals=True)[2]
            assert sha(nrm) == c["normals_sha256"]
    _check(c, r["n_src"], r["n_tgt"], r["inliers"], r["status"], r["norm"], Tt[-1], St[-1], idx, d2)


# ---------------------------------------------------------------- reference fixtures (committed copies under golden/kinect)
KINECT = os.path.join(HERE, "golden", "kinect")


def _read_png16(path):
    from PIL import Image
    return np.array(Image.open(path)).astype(np.uint16)


def _read_pcd_xyz(path):
    """binary PCD v0.7 'x y z rgba' 16-byte records (written by the reference's src/convert2PCD.cpp:72-78), xz-compressed."""
    import lzma
    raw = lzma.open(path).read()
    head_end = raw.index(b"DATA binary\n") + len(b"DATA binary\n")
    header = raw[:head_end].decode("ascii", "replace")
    n = int([l for l in header.splitlines() if l.startswith("POINTS")][0].split()[1])
    assert "FIELDS x y z rgba" in header and "SIZE 4 4 4 4" in header
    rec = np.frombuffer(raw, dtype=np.float32, count=n * 4, offset=head_end).reshape(n, 4)
    return rec[:, :3]


@pytest.mark.parametrize("k", [1, 2])
def test_backprojection_pinned_by_reference_pcd(k):
    """S1 is the one stage a reference artefact pins: data/exp1/pcd/k.pcd was produced by the reference's
    convert2PCD from data/exp1/dep/k.png (raster order, zero depth dropped, src/convert2PCD.cpp:54-72)."""
    d = _read_png16(os.path.join(KINECT, f"exp1_dep_{k}.png"))
    p = O.params(synth.Intrinsics(), z_filter=1e9)          # the PCD has no PassThrough applied
    cloud = O.backproject(d, p).reshape(-1, 4)
    ours = cloud[d.reshape(-1) > 0, :3]
    ref = _read_pcd_xyz(os.path.join(KINECT, f"exp1_pcd_{k}.pcd.xz"))
    assert ours.shape == ref.shape
    assert np.abs(ours - ref).max() <= 1e-6


def test_oracle_reproduces_reference_golden():
    G = json.load(open(os.path.join(HERE, "golden", "reference_golden.json")))
    intr = synth.Intrinsics()
    d1, d2, db = _kinect()
    assert int((d1 > 0).sum()) == G["inputs"]["dep1"]["nonzero"] == 221202
    assert int((d2 > 0).sum()) == G["inputs"]["dep2"]["nonzero"] == 236128
    assert int((db > 0).sum()) == G["inputs"]["bin_dep_1"]["nonzero"] == 201063
    p = O.params(intr)
    c1, c2, cb = (O.backproject(d, p) for d in (d1, d2, db))
    assert sha(c1) == G["backproject_sha256"]["dep1"] and sha(c2) == G["backproject_sha256"]["dep2"]
    nb = O.normals(cb, p)
    assert int((nb[..., 3] > 0).sum()) == G["config1_bin_dep_1"]["planar_pixels"]
    assert sha(nb) == G["config1_bin_dep_1"]["normals_sha256"]
    c = G["real_pair_dep1_to_dep2"]["0"]
    r = O.icp(c1, c2, O.params(intr, estimator=0, iterations=c["iterations"], nn_method=1))
    _check(c, r["n_src"], r["n_tgt"], r["inliers"], r["status"], r["norm"], r["T_trace"][-1], r["sums_trace"][-1], r["idx"], r["d2"])


def _kinect():
    return (_read_png16(os.path.join(KINECT, "exp1_dep_1.png")), _read_png16(os.path.join(KINECT, "exp1_dep_2.png")),
            _read_png16(os.path.join(KINECT, "bin_dep_1.png")))


def test_oracle_on_committed_kinect_frames_reproduces_reference_golden():
    """The same check as above on the committed copies of the reference's three depth images (runs everywhere)."""
    G = json.load(open(os.path.join(HERE, "golden", "reference_golden.json")))
    d1, d2, db = _kinect()
    assert int((d1 > 0).sum()) == 221202 and int((d2 > 0).sum()) == 236128 and int((db > 0).sum()) == 201063
    p = O.params(synth.Intrinsics())
    c1, c2, cb = (O.backproject(d, p) for d in (d1, d2, db))
    assert sha(c1) == G["backproject_sha256"]["dep1"] and sha(c2) == G["backproject_sha256"]["dep2"]
    nb = O.normals(cb, p)
    assert sha(nb) == G["config1_bin_dep_1"]["normals_sha256"]


@pytest.mark.gpu
def test_hip_path_on_real_kinect_frames(gpu_lib):
    """SURVEY.md 8(c) golden (3): the HIP path on REAL sensor frames.  dep/1 -> dep/2 is a wide-baseline pair (plain ICP
    from identity does not converge to a unique answer there), so this is an EQUALITY test, not an
    accuracy test: every iterate, the 29 sums of every iteration and the last correspondences bit-identical to the
    oracle, for both estimators; the target normals of BASELINE config 1's frame (bin/dep_1.png) through k_normals
    bit-identical too."""
    from slam3d_gx_amd import capi
    G = json.load(open(os.path.join(HERE, "golden", "reference_golden.json")))
    d1, d2, db = _kinect()
    intr = synth.Intrinsics()
    for est in (0, 1):
        c = G["real_pair_dep1_to_dep2"][str(est)] if str(est) in G["real_pair_dep1_to_dep2"] else None
        iters = c["iterations"] if c else 12
        with capi.IcpHandle(capi.default_params(intr, estimator=est, iterations=iters)) as h:
            r = h.align_depth_batch([d1], [d2])[0]
            Tt, St = h.get_trace(0)
            idx, d2c = h.get_correspondences(0)
            s_dev, t_dev, n_dev = h.get_clouds(0, normals=(est == 0))
        p = O.params(intr, estimator=est, iterations=iters, nn_method=1)
        c1, c2 = O.backproject(d1, p), O.backproject(d2, p)
        assert np.array_equal(s_dev.view(np.uint32), c1.view(np.uint32)) and np.array_equal(t_dev.view(np.uint32), c2.view(np.uint32))
        ro = O.icp(c1, c2, p)
        assert np.array_equal(ro["T_trace"], Tt) and np.array_equal(ro["sums_trace"], St)
        assert np.array_equal(ro["idx"], idx) and np.array_equal(ro["d2"].view(np.uint32), d2c.view(np.uint32))
        assert r["inliers"] == ro["inliers"] and r["status"] == ro["status"] and r["n_src"] == ro["n_src"] and r["n_tgt"] == ro["n_tgt"]
        if est == 0:
            assert sha(n_dev) == sha(O.normals(c2, p))
        if c:
            _check(c, r["n_src"], r["n_tgt"], r["inliers"], r["status"], r["norm"], Tt[-1], St[-1], idx, d2c)
    # config 1's frame: normals of bin/dep_1.png on the device == the golden hash the oracle produced
    with capi.IcpHandle(capi.default_params(intr, iterations=1)) as h:
        h.align_depth_batch([db], [db])
        _, _, nb = h.get_clouds(0)
    assert sha(nb) == G["config1_bin_dep_1"]["normals_sha256"]
    assert int((nb[..., 3] > 0).sum()) == G["config1_bin_dep_1"]["planar_pixels"]


@pytest.mark.gpu
def test_hip_path_reproduces_the_scipy_only_goldens(gpu_lib):
    """HIP == scipy with no oracle ANYWHERE in the chain: tests/golden/independent_golden.json was written by the numpy / scipy
    restatement ALONE (make_independent_golden.py: whole-frame numpy.linalg.eigh normals -- round 4 --, cKDTree + canonical
    re-evaluation, lstsq / SVD), and the HIP path starts from the same depth-derived clouds with its own k_normals.  The full
    BASELINE config-2 loop -- 640x480, 20 iterations, seeds 1000..1003 --, the reference's Kinect pair for 20 iterations and
    one iterate at config 5's 1280x960: the HIP path must produce the same index array (hash) and the same pose (lstsq vs
    fixed-point LDL^T: 1e-7), from clouds and (the projective window search taking part) from the depth images."""
    from slam3d_gx_amd import capi
    import test_oracle_independent as R
    G = json.load(open(os.path.join(HERE, "golden", "independent_golden.json")))
    n = 0
    for c in G["cases"]:
        if c["width"] < 640:
            continue
        pr, s4, t4 = R._case(c["seed"], c["width"], c["height"], c.get("workload"))
        with capi.IcpHandle(capi.default_params(pr.intr, estimator=c["estimator"], iterations=c["iterations"], plane_flags=c.get("plane_flags", 0))) as h:
            for depth in (False, True):
                r = h.align_depth_batch([pr.depth_src], [pr.depth_tgt])[0] if depth else h.align(s4, t4)
                idx, _ = h.get_correspondences(0)
                assert hashlib.sha256(idx.astype("<i4").tobytes()).hexdigest() == c["idx_sha256"], (c["seed"], c["width"], depth)
                assert np.allclose(r["T_raw"], np.array(c["T_final"]), rtol=0, atol=1e-7) and r["inliers"] == c["inliers"]
        n += 1
    assert n >= 12 and sum(1 for c in G["cases"] if c["estimator"] == 2 and c["width"] >= 640) >= 4      # round 5: + SLAM3D_EST_PLANE
