/* Part of the C ABI of orbslam3_hip.h, which includes this file at its end: include that header, not this one.
 *
 * ---- IMU initialisation: the three Optimizer::InertialOptimization overloads (src/Optimizer.cc:3042, :3227, :3389) ----
 * LocalMapping::InitializeIMU and ScaleRefinement (src/LocalMapping.cc:1271, :1465) and the inertial map merge
 * (src/LoopClosing.cc:1867) call them to estimate the gravity direction, the metric scale, the IMU biases and the key-frame
 * velocities of a map whose poses stay fixed.  All three are built from EdgeInertialGS (src/G2oTypes.cc:596-718), VertexGDir and
 * VertexScale (include/G2oTypes.h:257-317) and are three settings of ONE problem:
 *
 *   overload                                   free                                   priors  algorithm            its  Huber
 *   (Rwg, scale, bg, ba, bMono, .., bFixedVel,  vel + bias unless bFixedVel; gravity   yes     Levenberg, lambda_0  200  none
 *    .., priorG, priorA)               :3042    direction; scale iff bMono                     1e3 iff priorG != 0
 *   (bg, ba, priorG, priorA)           :3227    vel + bias; Rwg = I, scale = 1 fixed   yes     Levenberg, 1e3       200  none
 *   (Rwg, scale)                       :3389    gravity direction, scale; the key      none    Gauss-Newton         10   delta 1 on
 *                                               frames' common bias in bg / ba                                          every link
 *
 *   - key frame k: Rwb / twb / vel = GetImuRotation() / GetImuPosition() / GetVelocity(), floats cast to double.  Every pose is fixed;
 *   - link l: kf1 = mPrevKF, kf2 = the key frame; info9 as EdgeInertialGS forms it (:604-612, no factor 1e-2); info_gyro and
 *     info_acc are not read.  Each key frame is kf1 of at most one link and kf2 of at most one, and the links form no cycle: they
 *     are disjoint paths, which is what mPrevKF produces.  A key frame in no link has no active edge: its velocity comes back
 *     bit-identical.  With n_links == 0 the call returns its inputs and stats.iterations == 0;
 *   - the error is computeError (:617-640) with the float GetDelta* arithmetic on the shared bias, the Jacobians the analytic ones
 *     of linearizeOplus (:642-718) AS WRITTEN: the scale column is Rbw1 (v2 - v1) and Rbw1 (p2 - p1 - v1 dt), without the factor
 *     s that the update s <- s exp(u) would call for.  Updates: Rwg <- Rwg ExpSO3(u0, u1, 0), s <- s exp(u), velocities and
 *     biases by addition.  A robust link weights H and b by rho1;
 *   - prior_g / prior_a: EdgePriorGyro / EdgePriorAcc, information prior x I, prior value 0.  Inactive when free_bias == 0
 *     (g2o drops an edge whose vertices are all fixed);
 *   - gauss_newton != 0: OptimizationAlgorithmGaussNewton, exactly max_iters iterations, no lambda, no chi2 stop (stop_reason 4
 *     ends it when the linear system cannot be solved);
 *   - lambda_init == 0: 1e-5 * max diag H over the free unknowns (computeLambdaInit); > 0: setUserLambdaInit.
 * A fixed scale, Rwg or bias comes back bit-identical.  chi2_initial / chi2_final: the active robust chi2 (priors included) at
 * the first and at the returned estimate.  stats.stop_reason as everywhere: 0 iteration cap, 1 ten trials or rho == 0, 2 three
 * iterations below 1e-3 relative gain, 4 solver failure.
 * Argument checks (imu_init_check; ORBX_ERR_ARG, ORBX_ERR_CAPACITY for n_kf > IMU_INIT_MAX_KF) are made before anything touches
 * a device: NULL pointers, an index out of range, kf1 == kf2, links that are not disjoint paths, a value that is not finite (of a
 * key frame, bg, ba, Rwg, any member of a link that is read, the priors, huber_delta), a scale that is not positive,
 * lambda_init < 0, max_iters outside 0 .. 1000, a negative prior, huber_delta <= 0 with a robust link.
 * imu_init_optimize_batch solves n_problems <= IMU_INIT_MAX_BATCH independent problems in one launch (one workgroup each), every
 * one exactly as a call of its own would (bit-identical).  A handle serves ONE call at a time. */
#ifndef ORBSLAM3_HIP_IMU_INIT_H
#define ORBSLAM3_HIP_IMU_INIT_H

#define IMU_INIT_MAX_KF 256
#define IMU_INIT_MAX_BATCH 64

typedef struct ImuInitProblem {
    int32_t n_kf;                   /* <= IMU_INIT_MAX_KF */
    const double* Rwb;              /* [n_kf][9] row-major */
    const double* twb;              /* [n_kf][3] */
    const double* vel;              /* [n_kf][3] */
    double bg[3], ba[3];            /* VertexGyroBias / VertexAccBias(vpKFs.front()) */
    double Rwg[9], scale;
    int32_t n_links;
    const LibaLink* links;
    uint8_t free_vel, free_bias, free_gdir, free_scale;
    double prior_g, prior_a;
    double huber_delta;             /* applied to links with robust != 0 */
    int32_t gauss_newton;           /* 0: Levenberg; 1: OptimizationAlgorithmGaussNewton */
    double lambda_init;             /* 0: 1e-5 * max diag H */
    int32_t max_iters;              /* 0 .. 1000 */
} ImuInitProblem;

typedef struct ImuInitResult {
    double* vel_out;                /* [n_kf][3] */
    double bg_out[3], ba_out[3], Rwg_out[9], scale_out, chi2_initial, chi2_final;
    LbaStats stats;
} ImuInitResult;

typedef struct imu_init_solver imu_init_solver;
int  imu_init_create(int device, imu_init_solver** out);
void imu_init_destroy(imu_init_solver* s);
int  imu_init_check(const ImuInitProblem* problem, const ImuInitResult* result);     /* host only */
int  imu_init_optimize_batch(imu_init_solver* s, const ImuInitProblem* problems, int n_problems, ImuInitResult* results);
double imu_init_last_device_ms(const imu_init_solver* s);   /* HIP-event time of the last call's launch, milliseconds */

#endif /* ORBSLAM3_HIP_IMU_INIT_H */
