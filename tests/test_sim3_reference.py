"""tests/sim3_reference.py against itself (no GPU): Horn's closed form recovers a noise-free similarity, the selection rule on
hand-made count vectors, the OptimizeSim3 restatement reduces chi2 and recovers the truth, and its numeric Jacobian agrees
with the closed form."""
import numpy as np
import pytest

import sim3_reference as ref


def _rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _triples(rs, H, R, t, s):
    P2 = rs.uniform(-3, 3, (H, 3, 3)) + np.array([0, 0, 6.0])
    P1 = s * np.einsum("ij,hkj->hki", R, P2) + t
    return P1, P2


@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("negate", [False, True])
def test_horn_recovers_ground_truth(fix_scale, negate):
    rs = np.random.RandomState(11)
    for angle in (0.05, 0.7, 2.5, np.pi - 1e-3):
        R = _rodrigues(rs.normal(size=3) / np.sqrt(3) * angle)
        t = rs.uniform(-1, 1, 3)
        s = 1.0 if fix_scale else rs.uniform(0.5, 2.0)
        P1, P2 = _triples(rs, 50, R, t, s)
        R1, t1, s1, gap = ref.horn(P1, P2, fix_scale, np.float64, negate=negate)
        ok = gap >= 1e-3                                # a nearly collinear triple is ill-posed in any arithmetic
        assert ok.mean() >= 0.9
        assert np.abs(R1[ok] - R).max() < 1e-9 and np.abs(t1[ok] - t).max() < 1e-9 and np.abs(s1[ok] - s).max() < 1e-9


def test_selection_rule():
    assert ref.select([3, 20, 7, 30], 15) == (1, 1)                 # the first above the minimum, not the largest
    assert ref.select([3, 16, 16], 15) == (1, 1)
    assert ref.select([3, 15, 7, 15, 2], 15) == (0, 3)              # none above: the last one that attains the maximum
    assert ref.select([0, 0, 0], 15) == (0, 2)                      # >= also with zero inliers
    assert ref.select([15, 16], 15) == (1, 1)                       # strictly greater
    assert ref.select([], 15) == (0, -1)


def test_too_few_correspondences_are_not_scored():
    rs = np.random.RandomState(3)
    n = 10
    prob = dict(X1c=rs.uniform(1, 5, (n, 3)).astype(np.float32), X2c=rs.uniform(1, 5, (n, 3)).astype(np.float32),
                max_err1=np.full(n, 9, np.float32), max_err2=np.full(n, 9, np.float32), K1=np.array([450, 450, 320, 240], np.float32),
                K2=np.array([450, 450, 320, 240], np.float32), fix_scale=0, min_inliers=15, triples=np.array([[0, 1, 2]] * 5))
    r = ref.ransac(prob)
    assert (r["scored"], r["converged"], r["index"]) == (0, 0, -1) and not r["count"].any() and not r["mask"].any()


def test_mask_packing_round_trip():
    rs = np.random.RandomState(5)
    for n in (1, 63, 64, 65, 130):
        inl = rs.uniform(size=(7, n)) < 0.5
        m = ref.pack_mask(inl)
        assert m.shape == (7, (n + 63) // 64) and np.array_equal(ref.unpack_mask(m, n), inl)
        assert ((int(m[2, 0]) >> 0) & 1) == int(inl[2, 0])


def _clean_problem(seed, fix_scale, n=40):
    rs = np.random.RandomState(seed)
    K = np.array([458.654, 457.296, 367.215, 248.375])
    X1 = np.stack([rs.uniform(-3, 3, n), rs.uniform(-2, 2, n), rs.uniform(2, 10, n)], 1)
    R = _rodrigues(rs.normal(size=3) * 0.1)
    s = 1.0 if fix_scale else 1.2
    t = rs.uniform(-0.5, 0.5, 3)
    X2 = ((X1 - t) @ R) / s
    obs1 = ref.project(X1, K)
    obs2 = ref.project(X2, K)
    dR = _rodrigues(rs.normal(size=3) * 0.01)
    S0 = ref.sim3_from_Rts(dR @ R, t + rs.normal(0, 0.01, 3), s if fix_scale else s * 1.01)
    pr = dict(q=S0[0], t=S0[1], s=S0[2], X1c=X1, X2c=X2, obs1=obs1, obs2=obs2, inv_sigma2_1=np.ones(n), inv_sigma2_2=np.ones(n),
              K1=K, K2=K, th2=10.0, huber_delta=float(np.sqrt(np.float32(10.0))), fix_scale=int(fix_scale))
    return pr, R, t, s


@pytest.mark.parametrize("fix_scale", [False, True])
def test_optimize_recovers_ground_truth(fix_scale):
    pr, R, t, s = _clean_problem(21, fix_scale)
    p = ref._prepare(pr, np.float64)
    S0 = (np.asarray(pr["q"]), np.asarray(pr["t"]), np.float64(pr["s"]))
    chi0 = ref.edge_chi2(ref.edge_errors(S0, ref.sim3_inv(S0, np.float64), p, np.float64), p).sum()
    r = ref.optimize_sim3(pr)
    assert r["n_in"] == 40 and r["n_bad"] == 0 and r["keep"].all()
    assert r["chi2"][1] < 1e-6 * chi0 and chi0 > 1.0
    assert np.abs(ref.quat_xyzw_to_R(r["q"]) - R).max() < 1e-6 and np.abs(r["t"] - t).max() < 1e-6 and abs(r["s"] - s) < 1e-6
    assert r["iterations"][0] >= 1 and r["iterations"][1] >= 1 and r["trials"][0] >= r["iterations"][0]


def test_optimize_with_few_pairs_returns_zero():
    pr, R, t, s = _clean_problem(22, False, n=9)
    r = ref.optimize_sim3(pr)
    assert r["n_in"] == 0 and np.array_equal(r["q"], pr["q"]) and np.array_equal(r["t"], pr["t"]) and r["s"] == pr["s"]
    pr["X1c"] = pr["X1c"][:0]; pr["X2c"] = pr["X2c"][:0]; pr["obs1"] = pr["obs1"][:0]; pr["obs2"] = pr["obs2"][:0]
    pr["inv_sigma2_1"] = pr["inv_sigma2_1"][:0]; pr["inv_sigma2_2"] = pr["inv_sigma2_2"][:0]
    r = ref.optimize_sim3(pr)
    assert r["n_in"] == 0 and r["iterations"] == [0, 0] and len(r["keep"]) == 0


@pytest.mark.parametrize("fix_scale", [False, True])
def test_numeric_jacobian_matches_closed_form(fix_scale):
    pr, R, t, s = _clean_problem(23, fix_scale)
    p = ref._prepare(pr, np.float64)
    S = (np.asarray(pr["q"]), np.asarray(pr["t"]), np.float64(pr["s"]))
    Jn = ref.numeric_jacobians(S, p, np.float64)
    Ja = ref.analytic_jacobians(S, p)
    assert np.abs(Jn - Ja).max() <= 1e-5 * np.abs(Ja).max()
    if fix_scale:
        assert not Jn[:, :, 6].any()


def test_sim3_group_operations():
    rs = np.random.RandomState(9)
    for _ in range(20):
        u = rs.normal(0, 0.3, 7)
        v = rs.normal(0, 0.3, 7)
        A, B = ref.sim3_exp(u, np.float64), ref.sim3_exp(v, np.float64)
        AB = ref.sim3_mul(A, B, np.float64)
        X = rs.normal(size=(5, 3))
        lhs = np.stack(ref.sim3_map(AB, X), 1)
        rhs = np.stack(ref.sim3_map(A, np.stack(ref.sim3_map(B, X), 1)), 1)
        assert np.abs(lhs - rhs).max() < 1e-12
        back = np.stack(ref.sim3_map(ref.sim3_inv(A, np.float64), np.stack(ref.sim3_map(A, X), 1)), 1)
        assert np.abs(back - X).max() < 1e-12
        assert abs(A[2] - np.exp(u[6])) < 1e-15
