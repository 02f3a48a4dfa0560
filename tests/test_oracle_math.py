"""Property tests of the oracle's small solvers against numpy/scipy."""
import math

import numpy as np
from hypothesis import given, settings, strategies as st

import oracle_lib as O

rng = np.random.default_rng(7)


def _sym6(M):
    return np.array([M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]])


def test_eig3_vs_numpy_100_cases():
    for k in range(100):
        A = rng.normal(size=(3, 3)) * 10.0 ** rng.integers(-6, 3)
        S = A @ A.T if k % 2 == 0 else (A + A.T)
        ev, V = O.eig3(_sym6(S))
        w = np.linalg.eigvalsh(S)
        scale = max(1e-300, np.abs(w).max())
        assert np.allclose(np.sort(ev), w, atol=1e-12 * scale)
        assert np.allclose(V.T @ V, np.eye(3), atol=1e-12)
        assert np.allclose(S @ V, V * ev[None, :], atol=1e-11 * scale)


def test_eig3_degenerate_inputs():
    ev, V = O.eig3(np.zeros(6))
    assert np.array_equal(ev, np.zeros(3)) and np.array_equal(V, np.eye(3))
    ev, V = O.eig3(np.array([2.0, 0, 0, 2.0, 0, 2.0]))
    assert np.array_equal(ev, [2, 2, 2])
    ev, V = O.eig3(np.array([1.0, 1e-300, 0, 1.0, 0, 3.0]))   # huge theta -> no NaN
    assert np.all(np.isfinite(ev)) and np.all(np.isfinite(V))


def test_smallest_evec3_vs_numpy_eigh():
    """Spec S2's direction of least variance (power iteration on the adjugate, seven squarings + dominance test, round 4):
    against numpy's eigh on covariances with a prescribed spectrum.  A spectrum with l1 / l0 >= 1.27 passes the dominance
    test and the direction is eigh's to 1e-12 (error angle (l0 / l1)^128); one with l1 / l0 <= 1.23 has NO direction (the
    test's threshold sits at ~1.25: ||M||_F^2 >= (1 - 2^-40) tr(M)^2 of the squared adjugate); scales from (0.1 mm)^2 to (1 m)^2."""
    worst = 0.0
    for k in range(400):
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        l0 = 10.0 ** rng.uniform(-9, -1)
        r = 10.0 ** rng.uniform(np.log10(1.27), 3.5)
        l1 = l0 * r
        l2 = l1 * 10.0 ** rng.uniform(0, 2)
        S = Q @ np.diag([l0, l1, l2]) @ Q.T
        ok, n = O.smallest_evec3(_sym6(S))
        assert ok and abs(np.linalg.norm(n) - 1.0) < 1e-15
        w, V = np.linalg.eigh(S)
        err = 1.0 - abs(float(n @ V[:, 0]))
        assert err <= 1e-13, (k, r, err)
        worst = max(worst, err)
        S2 = Q @ np.diag([l0, l0 * rng.uniform(1.0, 1.23), l2]) @ Q.T           # the two smallest too close: no normal
        assert not O.smallest_evec3(_sym6(S2))[0], k
    assert worst < 1e-13


def test_smallest_evec3_degenerate_inputs():
    assert not O.smallest_evec3(np.zeros(6))[0]                                   # no spread at all
    assert not O.smallest_evec3(np.array([1.0, 0, 0, 0.0, 0, 0.0]))[0]            # a line: two zero eigenvalues, adj = 0
    ok, n = O.smallest_evec3(np.array([2.0, 0, 0, 3.0, 0, 0.0]))                  # an exact plane z = const
    assert ok and np.array_equal(np.abs(n), [0, 0, 1])
    assert not O.smallest_evec3(np.array([1.0, 0, 0, 1.0, 0, 1.0]))[0]            # isotropic: no direction of least variance (round 4: dominance test)
    ok, n = O.smallest_evec3(np.array([1e-300, 0, 0, 1e-300, 0, 1e-300]))         # adj underflows: no direction, no NaN
    assert not ok


def test_solve6_vs_numpy_100_cases():
    for _ in range(100):
        J = rng.normal(size=(40, 6))
        A = J.T @ J
        b = rng.normal(size=6)
        U = np.array([A[r, c] for r in range(6) for c in range(r, 6)])
        rc, x = O.solve6(U, b)
        assert rc == 1
        assert np.allclose(x, np.linalg.solve(A, b), rtol=1e-9, atol=1e-12)


def test_solve6_rank_deficient_is_damped_or_fails():
    J = rng.normal(size=(40, 6)); J[:, 5] = J[:, 4]          # two identical columns -> singular
    A = J.T @ J
    U = np.array([A[r, c] for r in range(6) for c in range(r, 6)])
    rc, x = O.solve6(U, rng.normal(size=6))
    assert rc in (0, 2)
    assert O.solve6(np.zeros(21), np.zeros(6))[0] == 0


def test_svd3_rotation_vs_numpy_kabsch():
    for k in range(100):
        P = rng.normal(size=(50, 3))
        ang = rng.uniform(0, math.pi)
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        Rt = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * K @ K
        if k % 3 == 0:
            P[:, 2] = 0.0                                      # planar data: rank-2 H, reflection fix must hold
        Q = P @ Rt.T + 0.01 * rng.normal(size=P.shape)
        Pc, Qc = P - P.mean(0), Q - Q.mean(0)
        H = Pc.T @ Qc
        R = O.svd3_rotation(H)
        U, S, Vt = np.linalg.svd(H)
        D = np.diag([1, 1, np.sign(np.linalg.det(Vt.T @ U.T))])
        Rn = Vt.T @ D @ U.T
        assert abs(np.linalg.det(R) - 1) < 1e-12
        assert np.allclose(R, Rn, atol=1e-9)


def test_svd3_rank_deficient_returns_identity():
    assert np.array_equal(O.svd3_rotation(np.zeros(9)), np.eye(3))
    H = np.outer([1.0, 2, 3], [3.0, 2, 1])                     # rank 1
    assert np.array_equal(O.svd3_rotation(H), np.eye(3))


@settings(max_examples=200, deadline=None)
@given(st.floats(min_value=-50.0, max_value=50.0, allow_nan=False))
def test_spec_sincos_matches_libm(x):
    s, c = O.sincos(x)
    assert abs(s - math.sin(x)) < 2e-15 and abs(c - math.cos(x)) < 2e-15


def test_pose_error_metric():
    T = np.eye(4); T[:3, 3] = [0.3, 0.0, 0.4]
    r, t = O.pose_error(np.eye(4), T)
    assert abs(t - 0.5) < 1e-15 and r == 0.0
    a = 0.3
    T = np.eye(4); T[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
    r, t = O.pose_error(np.eye(4), T)
    assert abs(r - a) < 1e-12 and t == 0.0
    r, t = O.pose_error(T, T)
    assert r < 1e-7 and t == 0.0


def _bf16_rne(v):
    """the bf16 nearest to each float32 (round to nearest even), returned as float32 -- csrc/icp_kernels.hpp::bf16_rne"""
    u = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def test_bf16_three_way_split_is_exact_and_its_cross_terms_are_bounded():
    """What the bf16 matrix-core scan (k_nn_mfma16) rests on: a float is EXACTLY h + m + l with h = bf16(v), m = bf16(v - h),
    l = bf16(v - h - m) (bf16: 8 significand bits, so |m| <= 2^-8 |v|, |l| <= 2^-16 |v|); and the six products the kernel keeps
    of (a_h + a_m + a_l)(b_h + b_m + b_l) miss a b by less than 2^-23 |a b| (a_m b_l + a_l b_m + a_l b_l: the bound its eps uses).  Checked in exact (float64) arithmetic on magnitudes the clouds have."""
    rng = np.random.default_rng(7)
    v = np.concatenate([rng.uniform(-8, 8, 200000), rng.normal(0, 1e-3, 50000), rng.uniform(0, 70, 50000)]).astype(np.float32)
    h = _bf16_rne(v)
    r1 = (v - h).astype(np.float32)
    assert np.array_equal(r1.astype(np.float64), v.astype(np.float64) - h.astype(np.float64))          # v - h is exact in float
    m = _bf16_rne(r1)
    r2 = (r1 - m).astype(np.float32)
    assert np.array_equal(r2.astype(np.float64), r1.astype(np.float64) - m.astype(np.float64))
    l = _bf16_rne(r2)
    assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), v.astype(np.float64))   # three terms: exact
    a, b = v[:150000].astype(np.float64), v[150000:300000].astype(np.float64)
    ah, am, al = (x[:150000].astype(np.float64) for x in (h, m, l))
    bh, bm, bl = (x[150000:300000].astype(np.float64) for x in (h, m, l))
    kept = ah * bh + ah * bm + ah * bl + al * bh + am * bh + am * bm
    err = np.abs(a * b - kept)
    assert np.all(err <= 2.0 ** -23 * np.abs(a * b) + 1e-300)
    assert np.all(np.abs(m) <= 2.0 ** -8 * np.abs(v)) and np.all(np.abs(l) <= 2.0 ** -16 * np.abs(v))


def test_pose_error_matches_the_reference_tool():
    """Row a14, pinned by the reference itself: orc_pose_error (the metric every parity test and bench leg reports) against the
    numbers the reference's tools/evaluate_rpe.py functions (ominus, compute_angle, compute_distance) returned for 96 seeded
    pose pairs -- tests/golden/pose_error_golden.json, made by tests/golden/make_pose_error_golden.py, which executes those
    functions where they lie in the reference repository.  The two differ only in how the relative pose is formed (numpy.linalg.inv
    there, the analytic inverse here): 1e-9 on the angle away from 0, 5e-8 where acos meets a trace rounded next to 3."""
    import json, os
    g = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_error_golden.json")))
    assert len(g["cases"]) >= 90
    worst_a = worst_d = 0.0
    for c in g["cases"]:
        rot, tr = O.pose_error(np.array(c["A"]).reshape(4, 4), np.array(c["B"]).reshape(4, 4))
        tol = 1e-9 if c["angle"] > 1e-3 else 5e-8
        assert abs(rot - c["angle"]) <= tol, (rot, c["angle"])
        assert abs(tr - c["distance"]) <= 1e-12 * max(1.0, c["distance"]), (tr, c["distance"])
        if c["angle"] > 1e-3:
            worst_a = max(worst_a, abs(rot - c["angle"]))
        worst_d = max(worst_d, abs(tr - c["distance"]))
    assert worst_a <= 1e-9 and worst_d <= 1e-12
