"""Spec S2l: normals of POINT LISTS from metric balls, and point-to-plane ICP on them.

A list (height == 1 handle: readimage's PassThrough + VoxelGrid cloud, src/GraphicEnd.cpp:279-295) has no 7x7 image windows, so a
point's normal is spec S2 on its ball N(i) = { valid j of the same list : canonical d2(x_i, x_j) <= (float)(radius^2) }.  The checks
here use no oracle code (oracle/ knows no S2l): the restatement below is written against the spec with other algorithms --

  ball membership   scipy cKDTree.query_ball_point at a slightly larger radius, re-filtered with the canonical float d2
                    (the kernel: tile boxes of the Morton sort, every candidate tile scanned)
  moments / normal  int64 sums, numpy.linalg.eigh of C' = n S2 - S1 S1^T, the dominance rule of
                    tests/test_oracle_independent.py::normals_numpy_full   (the kernel: adjugate power iteration)

and the ICP loop is checked with that module's nn_scipy / row_vectors / gram_sums / update_from_rows.
"""
import itertools
import os

import numpy as np
import pytest
from scipy.spatial import cKDTree

import oracle_lib as O
import test_oracle_independent as TI
from slam3d_gx_amd import synth
from test_unorganized import kinect_voxel_clouds, pad

HERE = os.path.dirname(os.path.abspath(__file__))
NMAX = 2048                  # spec S2l's cap on |N(i)|
DEFAULTS = dict(radius=0.06, min_points=10, min_inliers=8, inlier_dist=0.01)      # slam3d_list_normal_default_params


# ------------------------------------------------------------------------------------------------ the restatement
def ball_members(P, radius):
    """(query, member) index pairs of N(i) over the rows of P (float32 (n, 3), all valid), grouped by query in ascending order"""
    r2 = np.float32(np.float64(np.float32(radius)) ** 2)
    tree = cKDTree(P.astype(np.float64))
    lists = tree.query_ball_point(P.astype(np.float64), float(np.float32(radius)) * 1.001 + 1e-6)
    cnt = np.fromiter(map(len, lists), np.int64, len(lists))
    qi = np.repeat(np.arange(len(P), dtype=np.int64), cnt)
    mj = np.fromiter(itertools.chain.from_iterable(lists), np.int64, int(cnt.sum()))
    keep = TI.canon_d2(P[qi], P[mj]) <= r2
    return qi[keep], mj[keep]


def list_normals_numpy(c4, radius=0.10, min_points=10, min_inliers=8, inlier_dist=0.01, zmax=7.0, want_n=False):
    """spec S2l for a whole list: (N, 4) float32 normals, planar flag in .w (and |N(i)| per record with want_n)"""
    c = np.ascontiguousarray(c4, dtype=np.float32).reshape(-1, 4)
    ok = TI.valid_mask(c, zmax)
    vi = np.flatnonzero(ok)
    out = np.zeros((len(c), 4), dtype=np.float32)
    nrec = np.zeros(len(c), dtype=np.int64)
    if len(vi) == 0:
        return (out, nrec) if want_n else out
    P = c[vi, :3]
    qi, mj = ball_members(P, radius)
    Xq = np.rint(P * np.float32(65536.0)).astype(np.float32).astype(np.int64)
    n = np.bincount(qi, minlength=len(P)).astype(np.int64)              # >= 1: every point is its own member
    starts = np.concatenate([[0], np.cumsum(n)[:-1]])
    Xm = Xq[mj]
    S1 = np.add.reduceat(Xm, starts, axis=0)
    S2 = np.add.reduceat(Xm[:, :, None] * Xm[:, None, :], starts, axis=0)
    capped = n <= NMAX
    nn = np.where(capped, n, 1)
    C = (nn[:, None, None] * np.where(capped[:, None, None], S2, 0) - np.where(capped[:, None], S1, 0)[:, :, None] * np.where(capped[:, None], S1, 0)[:, None, :])
    C = C.astype(np.float64)                                              # exact: every entry below 2^53 (the radius bound)
    evals, evecs = np.linalg.eigh(C)
    l0, l1, l2 = np.abs(evals[:, 0]), evals[:, 1], evals[:, 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        r1 = np.where(l1 > 0, (l0 / l1) ** 128, np.inf)
        r2 = np.where(l2 > 0, (l0 / l2) ** 128, np.inf)
        dominant = 2.0 * (r1 + r2 + r1 * r2) / (1.0 + r1 + r2) ** 2 <= 2.0 ** -40
    nv = evecs[:, :, 0]
    flip = (nv * Xq.astype(np.float64)).sum(-1) > 0                      # toward the camera, on the quantised point
    nv = np.where(flip[:, None], -nv, nv)
    mean = S1.astype(np.float64) * (1.0 / nn.astype(np.float64))[:, None]
    dqf = ((nv[:, 0] * mean[:, 0] + nv[:, 1] * mean[:, 1]) + nv[:, 2] * mean[:, 2]).astype(np.float32)
    nf = nv.astype(np.float32)
    Xf = Xm.astype(np.float32)
    e = TI.fma32(nf[qi, 2], Xf[:, 2], TI.fma32(nf[qi, 1], Xf[:, 1], nf[qi, 0] * Xf[:, 0])) - dqf[qi]
    cnt = np.bincount(qi, weights=(np.abs(e) <= np.float32(np.float64(np.float32(inlier_dist)) * 65536.0)), minlength=len(P))
    good = (n >= min_points) & capped & dominant & (cnt >= min_inliers)
    out[vi, :3] = np.where(good[:, None], nf, np.float32(0))
    out[vi, 3] = good
    nrec[vi] = n
    return (out, nrec) if want_n else out


def icp_list_numpy(src, tgt, nrm, T0=None, iterations=20, gate=0.10, estimator=0, coarse_iterations=3):
    """the HIP point-list loop restated (spec S4 / S4c / S5 through test_oracle_independent's pieces): the iterates T_0 .. T_iterations"""
    s4 = np.ascontiguousarray(src, dtype=np.float32).reshape(1, -1, 4)
    t4 = np.ascontiguousarray(tgt, dtype=np.float32).reshape(1, -1, 4)
    n4 = None if nrm is None else np.ascontiguousarray(nrm, dtype=np.float32).reshape(1, -1, 4)
    tgt_ok = TI.valid_mask(t4) & ((n4[..., 3] > 0.5) if estimator == 0 else True)
    T = np.eye(4) if T0 is None else np.asarray(T0, dtype=np.float64)
    trace = [T]
    for k in range(iterations):
        idx, ps, sv = TI.nn_scipy(s4, t4, tgt_ok, T, gate, coarse=TI.is_coarse(k, iterations, coarse_iterations))
        V = TI.row_vectors(ps, sv, idx, t4, n4, estimator, gate)
        T = TI.update_from_rows(V, estimator, gate, T)
        trace.append(T)
    return trace


def synthetic_voxel_pair(seed, workload):
    """synth.make_pair's frames back-projected and voxelised as readimage does (leaf 0.03, z <= 7 m)"""
    kw = TI.BASELINE_MD if workload == "baseline_md" else {}
    pr = synth.make_pair(seed, 640, 480, **kw)
    out = []
    for d in (pr.depth_src, pr.depth_tgt):
        c = synth.backproject_numpy(d, pr.intr).reshape(-1, 4)
        c = c[np.isfinite(c[:, 2])].copy()
        c[:, 3] = np.float32(0)
        out.append(O.voxel_grid(c, 0.03, 7.0))
    return out[0], out[1], pr.T_gt


def as_list(v):
    return pad(v, len(v))[0]


# ------------------------------------------------------------------------------------------------ CPU: the restatement itself
def _voxel_plane(n_hat, d, half=0.6, step=0.004, seed=0):
    """points of the plane n.x = d (n toward the camera: d < 0), dense, voxelised at 0.03 m"""
    n_hat = np.asarray(n_hat, np.float64) / np.linalg.norm(n_hat)
    a = np.cross(n_hat, [0.0, 1.0, 0.0]); a /= np.linalg.norm(a)
    b = np.cross(n_hat, a)
    u, v = np.meshgrid(np.arange(-half, half, step), np.arange(-half, half, step))
    P = (d * n_hat)[None, :] + u.reshape(-1, 1) * a[None, :] + v.reshape(-1, 1) * b[None, :]
    rec = np.zeros((len(P), 4), np.float32)
    rec[:, :3] = P
    return O.voxel_grid(rec, 0.03, 7.0), n_hat


@pytest.mark.parametrize("n_hat", [(0.0, 0.0, -1.0), (0.3, -0.2, -1.0)])
def test_restatement_gives_the_plane_normal_on_a_noiseless_voxelised_plane(n_hat):
    v, nh = _voxel_plane(n_hat, -2.0)
    got = list_normals_numpy(as_list(v), **DEFAULTS)
    m = got[:, 3] > 0.5
    assert m.mean() > 0.8                                       # (the rim of the patch has fewer than min_points neighbours)
    dots = got[m, :3].astype(np.float64) @ nh
    assert dots.min() > 1 - 1e-6                                 # the plane's normal, toward the camera
    if n_hat == (0.0, 0.0, -1.0):
        assert np.all(got[m, :3] == np.float32([0, 0, -1]) + np.float32(0))


def test_restatement_does_not_depend_on_the_order_of_the_points():
    v1, _ = kinect_voxel_clouds()
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(v1))
    a = list_normals_numpy(as_list(v1), **DEFAULTS)
    b = list_normals_numpy(as_list(v1)[perm], **DEFAULTS)
    assert np.array_equal(a[perm].view(np.uint32), b.view(np.uint32))
    assert (a[:, 3] > 0.5).mean() > 0.5


def test_cap_and_min_points():
    """|N(i)| > 2048: no normal; |N(i)| = 2048 on a plane: a normal; |N(i)| < min_points: no normal"""
    u, v = np.meshgrid(np.arange(64) * 0.0006, np.arange(32) * 0.0012)           # 2,048 points, 0.038 x 0.037 m: all within 0.06 m of each other
    patch = np.zeros((2048, 4), np.float32)
    patch[:, 0] = u.ravel(); patch[:, 1] = v.ravel(); patch[:, 2] = 2.0; patch[:, 3] = 1.0
    lone = np.array([[1.0, 1.0, 3.0, 1.0], [1.05, 1.0, 3.0, 1.0], [-1.0, 0.5, 2.5, 1.0]], np.float32)     # a pair and a single point, far away
    got, n = list_normals_numpy(np.concatenate([patch, lone]), **DEFAULTS, want_n=True)
    assert np.all(n[:2048] == 2048) and np.all(got[:2048, 3] == 1) and np.all(got[:2048, :3] == np.float32([0, 0, -1]))
    assert np.all(n[2048:] == [2, 2, 1]) and np.all(got[2048:] == 0)
    extra = np.array([[0.02, 0.02, 2.0, 1.0]], np.float32)
    got, n = list_normals_numpy(np.concatenate([patch, extra]), **DEFAULTS, want_n=True)
    assert np.all(n == 2049) and np.all(got == 0)
    got = list_normals_numpy(np.concatenate([patch, extra]), **dict(DEFAULTS, min_points=2050))
    assert np.all(got == 0)


# the DESIGN.md section 3 S2l table: the chosen defaults' rows (pose error after 20 iterations, mrad / mm, rounded to 0.01)
DESIGN_SELF = {"dep1->dep1": (0.50, 1.41), "dep2->dep2": (0.39, 0.90)}


@pytest.mark.parametrize("case", ["dep1->dep1", "dep2->dep2"])
def test_sweep_defaults_reproduce_the_design_table(case):
    v1, v2 = kinect_voxel_clouds()
    v = v1 if case == "dep1->dep1" else v2
    L = as_list(v)
    nrm = list_normals_numpy(L, **DEFAULTS)
    T = icp_list_numpy(L, L, nrm, synth.pose_from_seed(77, 2.0, 0.03))[-1]
    rot, tr = O.pose_error(np.eye(4), T)
    assert (round(rot * 1e3, 2), round(tr * 1e3, 2)) == DESIGN_SELF[case], (rot * 1e3, tr * 1e3)


# ------------------------------------------------------------------------------------------------ GPU
def _holes(v, extra, rng):
    """the list v with `extra` invalid records scattered among its points (positions drawn by rng)"""
    W = len(v) + extra
    out = np.full((1, W, 4), np.nan, np.float32)
    out[0, np.sort(rng.choice(W, len(v), replace=False))] = as_list(v)
    return out


def _gpu_normals(h, cloud):
    """the handle's normals of `cloud` as the target of a run (self-alignment: source = target)"""
    h.align(cloud, cloud)
    return h.get_clouds(0)[2].reshape(-1, 4)


def _same_bits(a, b):
    return np.array_equal((a + np.float32(0)).view(np.uint32), (b + np.float32(0)).view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["dep1", "dep2", "synthetic"])
def test_hip_list_normals_equal_the_restatement(gpu_lib, case):
    """k_list_normals against the restatement: ragged views (handle width > view width) with 500 invalid records interspersed --
    planar flags equal on every record, float components differ on at most 3 (the precedent of
    test_whole_frame_normals_vs_numpy_eigh); a shuffled list gives every point the same normal bits."""
    from slam3d_gx_amd import capi
    v1, v2 = kinect_voxel_clouds()
    v = v1 if case == "dep1" else (v2 if case == "dep2" else synthetic_voxel_pair(1000, "low_noise")[1])
    rng = np.random.default_rng(11)
    c = _holes(v, 500, rng)
    W = c.shape[1] + 300
    intr = synth.Intrinsics(width=W, height=1)
    want = np.zeros((W, 4), np.float32)
    want[: c.shape[1]] = list_normals_numpy(c, **DEFAULTS)
    perm = rng.permutation(c.shape[1])
    with capi.IcpHandle(capi.default_params(intr, normal_window=0, iterations=2, estimator=capi.EST_POINT2PLANE)) as h:
        got = _gpu_normals(h, c)
        got_p = _gpu_normals(h, np.ascontiguousarray(c[:, perm]))
    fo, fn = got[:, 3] > 0.5, want[:, 3] > 0.5
    assert fn.sum() > 0.4 * len(v)
    assert np.array_equal(fo, fn), f"{(fo != fn).sum()} planar flags differ"
    assert np.all(got[~fo] == 0) and np.all(got[fo, 3] == 1)
    diff = ((got[:, :3] + np.float32(0)).view(np.uint32) != (want[:, :3] + np.float32(0)).view(np.uint32)) & fo[:, None]
    assert diff.sum() <= 3, f"{diff.sum()} float components differ"
    assert (got[fo, :3].astype(np.float64) * want[fo, :3].astype(np.float64)).sum(-1).min() > 1 - 1e-6
    assert _same_bits(got_p[: c.shape[1]], got[perm])


def _pair_case(case):
    v1, v2 = kinect_voxel_clouds()
    if case == "1->2":
        return as_list(v1), as_list(v2), None
    return as_list(v1), as_list(v1), synth.pose_from_seed(77, 2.0, 0.03)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["1->2", "1->1 perturbed"])
def test_hip_list_point2plane_every_iteration(gpu_lib, case, monkeypatch):
    """20 iterations of point-to-plane ICP on Kinect voxel lists: at every HIP iterate T_k the restatement's NN gives the same indices,
    gram_sums of its integer rows equals the HIP sums exactly and update_from_rows gives T_{k+1} to 1e-9.  AUTO (the persistent
    kernel), NN_TILES and NN_BRUTE_VALU give the same bits, and so does SLAM3D_LIST_ICP=0."""
    from slam3d_gx_amd import capi
    s, t, Ti = _pair_case(case)
    W = max(len(s), len(t))
    intr = synth.Intrinsics(width=W, height=1)
    iters, gate = 20, 0.10
    sv, tv = s[None], t[None]
    runs = {}
    for name, mode, env in (("auto", capi.NN_AUTO, None), ("tiles", capi.NN_TILES, None), ("valu", capi.NN_BRUTE_VALU, None),
                            ("auto, SLAM3D_LIST_ICP=0", capi.NN_AUTO, "0")):
        if env is not None:
            monkeypatch.setenv("SLAM3D_LIST_ICP", env)
        with capi.IcpHandle(capi.default_params(intr, normal_window=0, iterations=iters, nn_mode=mode, estimator=capi.EST_POINT2PLANE)) as h:
            h.set_corr_trace(True)
            r = h.align(np.ascontiguousarray(sv), np.ascontiguousarray(tv), Ti)
            Tt, St = h.get_trace(0)
            per_it = [h.get_correspondences_at(k) for k in range(iters)]
            nrm = h.get_clouds(0)[2].reshape(-1, 4)
        if env is not None:
            monkeypatch.delenv("SLAM3D_LIST_ICP")
        runs[name] = (r, Tt, St, per_it, nrm)
    r, Tt, St, per_it, nrm = runs["auto"]
    for name, (r2, Tt2, St2, per2, nrm2) in runs.items():
        assert _same_bits(nrm2, nrm), name
        assert np.array_equal(Tt2, Tt) and np.array_equal(St2, St), name
        assert all(np.array_equal(a[: len(s)], b[: len(s)]) for a, b in zip(per2, per_it)), name
        assert r2["status"] == r["status"] and r2["inliers"] == r["inliers"] and np.array_equal(r2["T_raw"], r["T_raw"]), name
    assert np.array_equal(nrm[: len(t), 3] > 0.5, list_normals_numpy(t, **DEFAULTS)[:, 3] > 0.5) and np.all(nrm[len(t):] == 0)
    s4, t4, n4 = s.reshape(1, -1, 4), t.reshape(1, -1, 4), nrm[: len(t)].reshape(1, -1, 4)
    tgt_ok = TI.valid_mask(t4) & (n4[..., 3] > 0.5)
    for k in range(iters):
        idx, ps, svi = TI.nn_scipy(s4, t4, tgt_ok, Tt[k], gate, coarse=TI.is_coarse(k, iters))
        assert np.array_equal(idx, per_it[k][: len(s)]), f"iteration {k}: {(idx != per_it[k][: len(s)]).sum()} indices differ"
        V = TI.row_vectors(ps, svi, idx, t4, n4, 0, gate)
        assert np.array_equal(St[k], TI.gram_sums(V, 0, gate)), k
        T_next = TI.update_from_rows(V, 0, gate, Tt[k])
        assert np.allclose(T_next, Tt[k + 1], rtol=0, atol=1e-9), (k, np.abs(T_next - Tt[k + 1]).max())
    if Ti is not None:          # (dep1 -> dep2 from the identity: point-to-plane leaves the basin on these lists, DESIGN.md section 3's S2l sweep)
        assert r["status"] == 0
        rot, tr = O.pose_error(np.eye(4), r["T_raw"])
        assert rot < 3e-3 and tr < 5e-3, (rot, tr)


@pytest.mark.gpu
def test_hip_list_plane_estimator_falls_back_to_ball_normals(gpu_lib):
    """SLAM3D_EST_PLANE with flags 0 on a list: a point on a plane takes the PLANE_ONLY handle's normal (w = 1 + r), every other point
    the POINT2PLANE handle's ball normal with w = 0.75.  The pair gate and the normal-angle gate run on lists, the same bits in
    every search mode."""
    from slam3d_gx_amd import capi
    v1, _ = kinect_voxel_clouds()
    L = as_list(v1)[None]
    intr = synth.Intrinsics(width=L.shape[1], height=1)
    got = {}
    for name, kw in (("plane", dict(estimator=capi.EST_PLANE)), ("only", dict(estimator=capi.EST_PLANE, plane_flags=capi.PLANE_ONLY)),
                     ("p2p", dict(estimator=capi.EST_POINT2PLANE))):
        with capi.IcpHandle(capi.default_params(intr, normal_window=0, iterations=2, **kw)) as h:
            got[name] = _gpu_normals(h, L)
    pl, only, p2p = got["plane"], got["only"], got["p2p"]
    on = pl[:, 3] >= 1
    assert on.sum() > 1000 and (~on & (pl[:, 3] > 0)).sum() > 1000
    assert _same_bits(pl[on], only[on]) and np.all(only[~on] == 0)
    fb = np.where((p2p[:, 3] > 0.5)[:, None], np.concatenate([p2p[:, :3], np.full((len(p2p), 1), 0.75, np.float32)], 1), np.float32(0))
    assert _same_bits(pl[~on], fb[~on])
    Ti = synth.pose_from_seed(77, 2.0, 0.03)
    for kw in (dict(plane_flags=capi.PLANE_PAIR_GATE), dict(min_normal_cos=0.9), dict(plane_flags=capi.PLANE_PAIR_GATE, min_normal_cos=0.9)):
        res = []
        for mode in (capi.NN_AUTO, capi.NN_TILES, capi.NN_BRUTE_VALU):
            with capi.IcpHandle(capi.default_params(intr, normal_window=0, iterations=20, nn_mode=mode, estimator=capi.EST_PLANE, **kw)) as h:
                r = h.align(L, L, Ti)
                res.append((r, h.get_trace(0)))
        for r, (Tt, St) in res[1:]:
            assert np.array_equal(Tt, res[0][1][0]) and np.array_equal(St, res[0][1][1]) and r["status"] == res[0][0]["status"], kw
        assert res[0][0]["status"] == 0 and res[0][0]["inliers"] > 1000, kw


@pytest.mark.gpu
def test_hip_list_normal_params_and_seg_params_between_runs(gpu_lib):
    """slam3d_icp_set_list_normal_params / slam3d_icp_set_seg_params between two runs on the SAME resident frames give what a fresh
    handle created with the new parameters gives (the frames' normals and target lists are rebuilt); the setter refuses an organized
    handle (E_STATE) and values out of range (E_INVALID)."""
    from slam3d_gx_amd import capi
    v1, v2 = kinect_voxel_clouds()
    W = max(len(v1), len(v2))
    intr = synth.Intrinsics(width=W, height=1)
    a, b = as_list(v1)[None], as_list(v2)[None]

    def run(h):
        h.run(1)
        r = h.fetch_results(1)[0]
        Tt, St = h.get_trace(0)
        return r, Tt, St, h.get_clouds(0)[2]

    def frames(h):
        h.frame_set_cloud_host(0, a); h.frame_set_cloud_host(1, b); h.set_pair(0, 0, 1)

    def same(x, y):
        return np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) and _same_bits(x[3], y[3])

    for est, change, fresh in (
            (capi.EST_POINT2PLANE, lambda h: h.set_list_normal_params(radius=0.08, min_inliers=6), lambda h: h.set_list_normal_params(radius=0.08, min_inliers=6)),
            (capi.EST_PLANE, lambda h: h.set_seg_params(h.seg_params(distance_threshold=0.06)), lambda h: h.set_seg_params(h.seg_params(distance_threshold=0.06))),
            (capi.EST_PLANE, lambda h: h.set_list_normal_params(radius=0.12), lambda h: h.set_list_normal_params(radius=0.12))):
        with capi.IcpHandle(capi.default_params(intr, normal_window=0, iterations=20, estimator=est)) as h:
            frames(h)
            r0 = run(h)
            change(h)
            r1 = run(h)
        with capi.IcpHandle(capi.default_params(intr, normal_window=0, iterations=20, estimator=est)) as h:
            fresh(h)
            frames(h)
            r2 = run(h)
        assert same(r1, r2) and not same(r0, r1)
    with capi.IcpHandle(capi.default_params(synth.Intrinsics.scaled(160, 120), iterations=2)) as h:
        with pytest.raises(capi.Slam3dError) as e:
            h.set_list_normal_params()
        assert e.value.code == -5
    with capi.IcpHandle(capi.default_params(intr, normal_window=0, iterations=2, estimator=capi.EST_POINT2PLANE)) as h:
        for bad in (dict(radius=0.0), dict(radius=0.46), dict(min_points=2), dict(min_points=2049), dict(min_inliers=0), dict(inlier_dist=0.0)):
            with pytest.raises(capi.Slam3dError) as e:
                h.set_list_normal_params(**bad)
            assert e.value.code == -1, bad
        h.set_list_normal_params(radius=0.45, min_points=2048, min_inliers=2048)


@pytest.mark.gpu
def test_unorganized_handles_take_ball_normals_with_no_window(gpu_lib):
    """A list has no image window: POINT2PLANE and PLANE without PLANE_ONLY (any pair gate) are refused with a window, as before spec
    S2l, and accepted with normal_window = 0 (ball normals); every estimator takes normal_window = 0 on a list, an organized handle
    never.  A view wider than the handle is refused; empty clouds give no inliers and the Identity."""
    from slam3d_gx_amd import capi
    intr = synth.Intrinsics(width=5000, height=1)
    need = (dict(estimator=capi.EST_POINT2PLANE), dict(estimator=capi.EST_PLANE, plane_flags=0), dict(estimator=capi.EST_PLANE, plane_flags=capi.PLANE_PAIR_GATE))
    for kw in need:
        for w in (7, 3, 1):
            with pytest.raises(capi.Slam3dError) as e:
                capi.IcpHandle(capi.default_params(intr, normal_window=w, **kw))
            assert e.value.code == -1
    for ok in need + (dict(estimator=capi.EST_PLANE, plane_flags=capi.PLANE_ONLY), dict(estimator=capi.EST_SVD)):
        with capi.IcpHandle(capi.default_params(intr, normal_window=0, **ok)) as h:
            with pytest.raises(AssertionError):
                h.align(np.zeros((1, 5001, 4), np.float32), np.zeros((1, 10, 4), np.float32))
            r = h.align(np.full((1, 0, 4), np.nan, np.float32), np.full((1, 7, 4), np.nan, np.float32))      # empty clouds: no inliers, Identity
            assert r["status"] == 1 and np.array_equal(r["T"], np.eye(4)), ok
    with pytest.raises(capi.Slam3dError) as e:
        capi.IcpHandle(capi.default_params(synth.Intrinsics.scaled(160, 120), normal_window=0))
    assert e.value.code == -1
    p = capi.default_params(intr, normal_window=0, estimator=capi.EST_POINT2PLANE, z_filter=9.3)          # 3 z^2 >= 256: ball moments could leave int64 exactness
    with pytest.raises(capi.Slam3dError) as e:
        capi.IcpHandle(p)
    assert e.value.code == -1
