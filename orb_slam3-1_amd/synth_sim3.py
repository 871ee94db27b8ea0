"""Seeded scenes for the loop-closing geometry: two key frames that see the same points, a ground-truth similarity S12
(X1 = s R X2 + t), pixel-level noise, gross outliers and octaves.  They produce both problem kinds of include/orbslam3_hip.h:
Sim3RansacProblem (Sim3Solver, reference src/Sim3Solver.cc) and Sim3OptProblem (Optimizer::OptimizeSim3,
src/Optimizer.cc:2115-2381).  Pure numpy apart from the index triples, which come from the library's sim3_draw_triples."""
import numpy as np

from .capi import sim3_draw_triples
from .synth import _quat_from_R, _rodrigues

K_EUROC = (458.654, 457.296, 367.215, 248.375)
K_OTHER = (435.2047, 435.2047, 367.4517, 252.2008)      # a second client with another camera


def _f32(a):
    return np.asarray(a, np.float32)


def _scene(rs, n, inlier, noise_px, fix_scale):
    X1 = np.stack([rs.uniform(-3, 3, n), rs.uniform(-2, 2, n), rs.uniform(2, 10, n)], 1)
    R = _rodrigues(rs.normal(0, 1, 3) * rs.uniform(0, 0.3) / np.sqrt(3))
    s = 1.0 if fix_scale else rs.uniform(0.7, 1.4)
    t = rs.uniform(-0.5, 0.5, 3)
    X2 = ((X1 - t) @ R) / s                              # X1 = s R X2 + t
    X2 = X2 + rs.normal(0, noise_px, X2.shape) * X2[:, 2:3] / K_EUROC[0]        # about noise_px of reprojection error
    out = rs.uniform(size=n) > inlier
    k = int(out.sum())
    X2[out] = np.stack([rs.uniform(-3, 3, k), rs.uniform(-2, 2, k), rs.uniform(2, 10, k)], 1)
    octv = rs.randint(0, 8, (2, n))
    return X1, X2, R, t, s, out, octv


def make_ransac_problem(seed, n=120, inlier=0.5, noise_px=1.0, fix_scale=False, n_hyp=300, min_inliers=15, two_cameras=False):
    """One Sim3RansacProblem as the Sim3Solver constructor derives it (:35-121): camera-frame points of both key frames in float,
    max_err = 9.210 * level sigma^2 truncated like the reference's vector<size_t> (:99-100), and n_hyp index triples."""
    rs = np.random.RandomState(7331 + 104729 * seed)
    X1, X2, R, t, s, out, octv = _scene(rs, n, inlier, noise_px, fix_scale)
    sig2 = _f32(1.2) ** (2 * octv)
    max_err = np.floor(9.210 * sig2.astype(np.float64)).astype(np.float32)
    tri = sim3_draw_triples(seed, n, n_hyp) if n >= 3 else np.zeros((n_hyp, 3), np.int32)
    return dict(X1c=np.ascontiguousarray(_f32(X1)), X2c=np.ascontiguousarray(_f32(X2)), max_err1=max_err[0].copy(), max_err2=max_err[1].copy(),
                K1=_f32(K_EUROC), K2=_f32(K_OTHER if two_cameras else K_EUROC), fix_scale=int(fix_scale), min_inliers=int(min_inliers),
                triples=tri, true_R=R, true_t=t, true_s=s, is_outlier=out)


def make_opt_problem(seed, n=100, outlier_frac=0.1, noise_px=0.7, fix_scale=False, n_unobserved=0, th2=10.0, two_cameras=False, init_off=1.0):
    """One Sim3OptProblem as Optimizer::OptimizeSim3 builds its graph (:2167-2304): n edge pairs, observations with pixel noise
    by octave, a share of gross outliers, the initial S12 a little off the truth (what the RANSAC hands over).  The last
    n_unobserved pairs are matches whose point is not observed in key frame 2 (i2 < 0 with bAllPoints): obs2 is the float
    (x/z, y/z) of P3D2c, as the reference sets it (:2273-2283).  init_off scales how far the initial S12 starts from the truth
    (1.0: one degree, two centimetres; the random draws do not depend on it)."""
    rs = np.random.RandomState(9973 + 15485863 * seed % (2 ** 31 - 1))
    X1 = np.stack([rs.uniform(-3, 3, n), rs.uniform(-2, 2, n), rs.uniform(2, 10, n)], 1)
    R = _rodrigues(rs.normal(0, 1, 3) * rs.uniform(0.02, 0.3) / np.sqrt(3))
    s = 1.0 if fix_scale else rs.uniform(0.7, 1.4)
    t = rs.uniform(-0.5, 0.5, 3)
    X2 = ((X1 - t) @ R) / s
    K1, K2 = np.array(_f32(K_EUROC), np.float64), np.array(_f32(K_OTHER if two_cameras else K_EUROC), np.float64)
    scale2 = 1.2 ** (2 * np.arange(8))
    octv = rs.randint(0, 8, (2, n))
    sig = np.sqrt(scale2[octv])
    X1f, X2f = _f32(X1).astype(np.float64), _f32(X2).astype(np.float64)
    obs1 = np.stack([K1[0] * X1f[:, 0] / X1f[:, 2] + K1[2], K1[1] * X1f[:, 1] / X1f[:, 2] + K1[3]], 1) + rs.normal(0, 1, (n, 2)) * sig[0][:, None] * noise_px
    obs2 = np.stack([K2[0] * X2f[:, 0] / X2f[:, 2] + K2[2], K2[1] * X2f[:, 1] / X2f[:, 2] + K2[3]], 1) + rs.normal(0, 1, (n, 2)) * sig[1][:, None] * noise_px
    out = rs.uniform(size=n) < outlier_frac
    obs1[out] += np.stack([rs.choice([-40.0, 40.0], out.sum()), rs.choice([-25.0, 25.0], out.sum())], 1)
    if n_unobserved:
        f = _f32(X2)[n - n_unobserved:]
        invz = np.float32(1) / f[:, 2]
        obs2[n - n_unobserved:] = np.stack([f[:, 0] * invz, f[:, 1] * invz], 1)
    dR = _rodrigues(rs.normal(0, np.deg2rad(1.0) / np.sqrt(3), 3) * init_off)
    q0 = _quat_from_R(dR @ R)
    t0 = dR @ t + rs.normal(0, 0.02 / np.sqrt(3), 3) * init_off
    s0 = 1.0 if fix_scale else s * (1 + rs.normal(0, 0.01))
    return dict(q=np.asarray(q0, np.float64), t=np.asarray(t0, np.float64), s=float(s0), X1c=np.ascontiguousarray(X1f), X2c=np.ascontiguousarray(X2f),
                obs1=np.ascontiguousarray(_f32(obs1).astype(np.float64)), obs2=np.ascontiguousarray(_f32(obs2).astype(np.float64)),
                inv_sigma2_1=_f32(1.0 / scale2[octv[0]]).astype(np.float64), inv_sigma2_2=_f32(1.0 / scale2[octv[1]]).astype(np.float64),
                K1=K1, K2=K2, th2=float(np.float32(th2)), huber_delta=float(np.sqrt(np.float32(th2))), fix_scale=int(fix_scale),
                true_R=R, true_t=t, true_s=s, is_outlier=out)
