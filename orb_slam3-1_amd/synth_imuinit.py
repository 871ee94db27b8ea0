"""Synthetic IMU-initialisation problems (Optimizer::InertialOptimization, reference src/Optimizer.cc:3042, :3227, :3389) for the
tests, the timing tool and the golden file.  Plain numpy; nothing here touches the library."""
import numpy as np

from .synth import _so3_exp

GRAVITY = float(np.float32(9.81))           # const float IMU::GRAVITY_VALUE (include/ImuTypes.h:43), as the edge reads it

# variant -> what is free, the priors, the algorithm (the table of include/orbslam3_hip_imu_init.h)
VARIANTS = dict(
    mono=dict(free_vel=1, free_bias=1, free_gdir=1, free_scale=1, prior_g=1e2, prior_a=1e10, lambda_init=1e3, max_iters=200),
    mono_noprior=dict(free_vel=1, free_bias=1, free_gdir=1, free_scale=1, prior_g=0.0, prior_a=0.0, lambda_init=0.0, max_iters=200),
    stereo=dict(free_vel=1, free_bias=1, free_gdir=1, free_scale=0, prior_g=1e2, prior_a=1e10, lambda_init=1e3, max_iters=200),
    bias=dict(free_vel=1, free_bias=1, free_gdir=0, free_scale=0, prior_g=1e2, prior_a=1e10, lambda_init=1e3, max_iters=200),
    scale_refine=dict(free_vel=0, free_bias=0, free_gdir=1, free_scale=1, prior_g=0.0, prior_a=0.0, lambda_init=0.0, max_iters=10,
                      gauss_newton=1, huber_delta=1.0),
    fixed_vel=dict(free_vel=0, free_bias=0, free_gdir=1, free_scale=1, prior_g=0.0, prior_a=0.0, lambda_init=0.0, max_iters=200),
)


def make_imu_init(seed, n, variant="mono", n_paths=1, n_isolated=0, shuffle=False, dt=0.25, noise=0.2, bias_offset=1.0, float_inputs=True,
                  **overrides):
    """An IMU-initialisation problem of n key frames: n - n_isolated of them on n_paths chains of pre-integrated links (the recipe of
    synth.make_inertial_window), the rest in no link.

    A metric, gravity-aligned trajectory (accelerations of about 1 m/s^2 standard deviation: scale and accelerometer bias are
    unobservable without excitation) is pre-integrated at a bias that differs from the true one by bias_offset standard deviations,
    then handed over rotated by a random Rwg and divided by a scale, so that (Rwg, scale, true bias, true velocities) is the minimum
    of a noise-free problem.  The initial guesses are InitializeIMU's (src/LocalMapping.cc:1230-1262): gravity direction from the
    summed dV, finite-difference velocities, zero biases, scale 1; the variants that keep velocities and biases fixed get the true
    ones and a perturbed gravity direction and scale.  noise: standard deviation of the link noise in units of a fifth of sigma, 0
    for none; in the scale_refine variant every fifth link gets ten times as much, which the Huber kernel then weights down.
    Returns (problem dict, ground truth dict)."""
    rs = np.random.RandomState(seed)
    cfg = dict(VARIANTS[variant])
    cfg.update(overrides)
    n_chain = n - n_isolated
    if n_chain < 2 * n_paths:
        raise ValueError("a path needs two key frames")
    g = np.array([0.0, 0.0, -GRAVITY])
    Rgb = [np.eye(3)]; pgb = [np.zeros(3)]; vgb = [np.array([0.6, 0.1, 0.0])]
    acc = rs.normal(0, 1.0, (n, 3)); omg = rs.normal(0, 0.3, (n, 3))
    for i in range(1, n):
        Rgb.append(Rgb[-1] @ _so3_exp(omg[i] * dt))
        pgb.append(pgb[-1] + vgb[-1] * dt + 0.5 * acc[i] * dt * dt)
        vgb.append(vgb[-1] + acc[i] * dt)
    Rgb, pgb, vgb = np.array(Rgb), np.array(pgb), np.array(vgb)
    bg_true = rs.normal(0, 0.01, 3).astype(np.float32).astype(np.float64); ba_true = rs.normal(0, 0.05, 3).astype(np.float32).astype(np.float64)
    fixed_states = not cfg["free_bias"]
    bg0 = bg_true if fixed_states else (bg_true + bias_offset * rs.normal(0, 0.01, 3)).astype(np.float32).astype(np.float64)
    ba0 = ba_true if fixed_states else (ba_true + bias_offset * rs.normal(0, 0.05, 3)).astype(np.float32).astype(np.float64)
    # the paths: consecutive key frames of the trajectory, cut at n_paths - 1 places
    cuts = sorted(rs.choice(np.arange(2, n_chain - 1), n_paths - 1, replace=False).tolist()) if n_paths > 1 else []
    while any(b - a < 2 for a, b in zip([0] + cuts, cuts + [n_chain])):
        cuts = sorted(rs.choice(np.arange(2, n_chain - 1), n_paths - 1, replace=False).tolist())
    starts = set([0] + cuts)
    sig_r, sig_v, sig_p = 2e-3, 1e-2, 5e-3
    links = []
    for i in range(1, n_chain):
        if i in starts:
            continue
        R1 = Rgb[i - 1]
        dR = R1.T @ Rgb[i]
        dV = R1.T @ (vgb[i] - vgb[i - 1] - g * dt)
        dP = R1.T @ (pgb[i] - pgb[i - 1] - vgb[i - 1] * dt - 0.5 * g * dt * dt)
        JRg = -dt * np.eye(3); JVg = rs.normal(0, 0.01, (3, 3)); JVa = -dt * dR; JPg = rs.normal(0, 0.003, (3, 3)); JPa = -0.5 * dt * dt * dR
        f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
        JRg, JVg, JVa, JPg, JPa = map(f32, (JRg, JVg, JVa, JPg, JPa))
        # what an IMU with the bias (bg0, ba0) subtracted would have integrated: the getters add J (b - b0) back
        dbg, dba = bg_true - bg0, ba_true - ba0
        dR = dR @ _so3_exp(JRg @ dbg).T
        dV = dV - JVg @ dbg - JVa @ dba
        dP = dP - JPg @ dbg - JPa @ dba
        k = noise * (10.0 if variant == "scale_refine" and len(links) % 5 == 2 else 1.0)
        if noise:
            dR = dR @ _so3_exp(rs.normal(0, sig_r * k, 3)); dV = dV + rs.normal(0, sig_v * k, 3); dP = dP + rs.normal(0, sig_p * k, 3)
        info9 = np.diag([1 / sig_r ** 2] * 3 + [1 / sig_v ** 2] * 3 + [1 / sig_p ** 2] * 3)
        links.append(dict(kf1=i - 1, kf2=i, dR=dR.astype(np.float32), dV=dV.astype(np.float32), dP=dP.astype(np.float32),
                          JRg=JRg.astype(np.float32), JVg=JVg.astype(np.float32), JVa=JVa.astype(np.float32), JPg=JPg.astype(np.float32),
                          JPa=JPa.astype(np.float32), dT=np.float32(dt), bias0=np.concatenate([ba0, bg0]).astype(np.float32),
                          info9=info9, info_gyro=np.zeros((3, 3)), info_acc=np.zeros((3, 3)), robust=np.uint8(cfg.get("huber_delta", 0.0) > 0)))
    # the solver's world: rotated by Rwg, divided by the scale
    mono = bool(cfg["free_scale"])
    aligned = not cfg["free_gdir"]
    Rwg_true = np.eye(3) if aligned else _so3_exp(rs.normal(0, 0.8, 3))
    # (ScaleRefinement runs on a map that is metric already: its Gauss-Newton steps, whose scale column lacks the factor s, overshoot
    # by that factor and diverge from a scale above 2)
    s_true = (float(rs.uniform(0.9, 1.1)) if cfg.get("gauss_newton", 0) else float(rs.uniform(1.5, 4.0))) if mono else 1.0
    Rwb = Rwg_true @ Rgb
    twb = pgb @ Rwg_true.T / s_true
    vel_true = vgb @ Rwg_true.T / s_true
    if float_inputs:                        # key-frame members are floats (GetImuRotation / GetImuPosition / GetVelocity)
        Rwb, twb = Rwb.astype(np.float32).astype(np.float64), twb.astype(np.float32).astype(np.float64)
    # initial guesses
    vel0 = vel_true.copy()
    if cfg["free_vel"]:
        for L in links:
            v = (twb[L["kf2"]] - twb[L["kf1"]]) / dt
            vel0[L["kf2"]] = v; vel0[L["kf1"]] = v
    if aligned:
        Rwg0 = np.eye(3)
    elif cfg["free_vel"]:
        dirG = np.zeros(3)
        for L in links:
            dirG -= Rwb[L["kf1"]] @ L["dV"].astype(np.float64)
        dirG /= np.linalg.norm(dirG)
        gI = np.array([0.0, 0.0, -1.0])
        v = np.cross(gI, dirG)
        Rwg0 = _so3_exp(v * np.arccos(gI @ dirG) / np.linalg.norm(v))
    else:
        Rwg0 = Rwg_true @ _so3_exp(np.array([0.05, -0.04, 0.0]))
    scale0 = 1.0 if cfg["free_vel"] or not mono or cfg.get("gauss_newton", 0) else s_true * 1.05
    if float_inputs:
        vel0 = vel0.astype(np.float32).astype(np.float64)
    bg_in, ba_in = (bg_true, ba_true) if fixed_states else (np.zeros(3), np.zeros(3))
    if shuffle:                             # key frames and links in no particular order
        perm = rs.permutation(n)            # old index -> new index
        inv = np.argsort(perm)
        Rwb, twb, vel0, vel_true = Rwb[inv], twb[inv], vel0[inv], vel_true[inv]
        for L in links:
            L["kf1"], L["kf2"] = int(perm[L["kf1"]]), int(perm[L["kf2"]])
        links = [links[i] for i in rs.permutation(len(links))]
    pr = dict(Rwb=Rwb, twb=twb, vel=vel0, bg=bg_in.copy(), ba=ba_in.copy(), Rwg=Rwg0, scale=scale0, links=links,
              huber_delta=0.0, gauss_newton=0)
    pr.update(cfg)
    gt = dict(vel=vel_true, bg=bg_true, ba=ba_true, Rwg=Rwg_true, scale=s_true)
    return pr, gt
