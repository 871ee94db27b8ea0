/* Part of the C ABI of orbslam3_hip.h, which includes this file at its end: include that header, not this one.
 *
 * ---- Optimizer::FullInertialBA (src/Optimizer.cc:392-811): visual-inertial bundle adjustment of a whole map ----
 * LocalMapping::InitializeIMU calls it after InertialOptimization (100 iterations, bInit with priorG / priorA or not,
 * src/LocalMapping.cc:1311,1313) and LoopClosing::RunGlobalBundleAdjustment for every inertial map (7 iterations and a stop flag,
 * src/LoopClosing.cc:2290).  The vertices and edges are those of LocalInertialBA (LibaProblem, LibaLink); what differs:
 *
 *   - every key frame of the map is a vertex and every map point a marginalised one; n_links is not bounded;
 *   - shared_bias != 0 (bInit): ONE gyro-bias and ONE accelerometer-bias vertex for the whole map (:456-466), started at
 *     shared_bg / shared_ba (the bias of the last key frame visited).  Every EdgeInertial uses them as G1 / A1: columns 9-14 of
 *     a link address the 6 shared rows, which come last in the reduced system.  There are no random-walk edges (info_gyro /
 *     info_acc are not read) and one EdgePriorGyro / EdgePriorAcc with prior value 0 and information prior_g I / prior_a I
 *     (:570-590).  The inputs bg / ba are only handed back (key frames without IMU states; a raised stop flag); every key frame
 *     with IMU states gets the shared values back;
 *   - shared_bias == 0: per-key-frame biases with EdgeGyroRW / EdgeAccRW as in LocalInertialBA; prior_g / prior_a are not read;
 *   - a Huber kernel of huber_inertial (sqrt(16.92)) on EVERY inertial edge (:540-542): LibaLink::robust is not read;
 *   - Levenberg started at lambda_init (> 0: setUserLambdaInit(1e-5)), max_iters iterations, stop_flag as in lba_solve and
 *     essg_optimize: polled (never written) before every iteration and after every trial, and once before the first
 *     (:721-723): raised there, the call returns 0 iterations, stop_reason 3 and its inputs;
 *   - no outlier pass: no per-edge chi2 or depth sign comes back.
 * The prior edges: EdgePriorAcc / EdgePriorGyro compute prior - estimate (include/G2oTypes.h:778-781,802-805) while
 * linearizeOplus writes +I (src/G2oTypes.cc:762-774).  As imu_init_optimize_batch, this solver reads the edge as
 * estimate - prior, whose gradient points toward the prior.
 * g2o activates only vertices that have an edge.  The host therefore drops from the unknowns, and returns bit for bit: the
 * velocity / bias of a key frame in no link; the pose of a key frame with neither an observation nor a link; a point none of
 * whose observers has a free pose (bAllFixed, :714-718) together with its edges.
 * Capacity: one map per call, at most FIBA_MAX_UNKNOWNS reduced unknowns (6 per free pose; 9 per free velocity + biases, or 3 per
 * free velocity + 6 with shared_bias): the substitution kernel keeps the solution in the LDS of one compute unit; and at most
 * FIBA_MAX_KF key frames, fixed ones included.  The reduced system is dense ((n + 1) n doubles on the device and as many pinned on
 * the host); the largest system the tests run has 495 unknowns.  Up to 480
 * unknowns the factorisation is one launch, beyond that a diag / panel / update launch per block column of 60.
 * Errors: ORBX_ERR_ARG for an index out of range, a link to a key frame without IMU states, nothing to optimise, shared_bias
 * without a link, lambda_init <= 0, max_iters < 0, a negative prior; ORBX_ERR_CAPACITY beyond the limit.  All of them are made
 * by fiba_check before anything touches a device, and the handle stays usable after either.
 * Two calls with the same inputs return the same bits.  A handle serves ONE call at a time. */
#ifndef ORBSLAM3_HIP_FULLBA_H
#define ORBSLAM3_HIP_FULLBA_H

#define FIBA_MAX_UNKNOWNS 15732
#define FIBA_MAX_KF 4096           /* fixed key frames included: the host's pair-count tables have n_kf x n_kf entries (2 x 64 MiB here) */

typedef struct FibaProblem {
    int32_t n_kf;
    const double* Rwb;              /* [n_kf][9] GetImuRotation() */
    const double* twb;              /* [n_kf][3] GetImuPosition() */
    const double* vel;              /* [n_kf][3] */
    const double* bg;               /* [n_kf][3]; with shared_bias only handed back */
    const double* ba;               /* [n_kf][3] */
    const uint8_t* pose_fixed;      /* bFixLocal && mnId < nNonFixed-window rule (:431-447) */
    const uint8_t* has_imu;         /* pKFi->bImu */
    const uint8_t* imu_fixed;       /* velocity (and, without shared_bias, biases) fixed with the pose */
    double Rcb[9], tcb[3], tbc[3];
    double fx, fy, cx, cy, bf;
    int32_t n_points;
    const double* points;
    int32_t n_edges;                /* in addEdge order */
    const int32_t* edge_kf;
    const int32_t* edge_point;
    const double* edge_obs;         /* [n_edges][3] */
    const double* edge_inv_sigma2;
    const uint8_t* edge_stereo;
    int32_t n_links;                /* unbounded */
    const LibaLink* links;          /* robust, and with shared_bias info_gyro / info_acc, are not read */
    double huber_mono, huber_stereo, huber_inertial;    /* (float)sqrt(5.991), (float)sqrt(7.815), sqrt(16.92) */
    double lambda_init;             /* > 0; the reference sets 1e-5 */
    int32_t max_iters;              /* 100 (InitializeIMU) or 7 (RunGlobalBundleAdjustment) */
    uint8_t shared_bias;            /* bInit */
    double shared_bg[3], shared_ba[3];
    double prior_g, prior_a;
    const volatile uint8_t* stop_flag;      /* NULL: never raised */
} FibaProblem;

typedef struct FibaOutputs {        /* any pointer may be NULL */
    double* Rwb;                    /* [n_kf][9] */
    double* twb;                    /* [n_kf][3] */
    double* vel;
    double* bg;
    double* ba;
    double* points;                 /* [n_points][3] */
} FibaOutputs;

typedef struct fiba_solver fiba_solver;
int  fiba_create(int device, fiba_solver** out);
void fiba_destroy(fiba_solver* s);
int  fiba_check(const FibaProblem* problem);                /* host only: the argument and capacity checks of fiba_solve */
int  fiba_solve(fiba_solver* s, const FibaProblem* problem, const FibaOutputs* outputs, LbaStats* stats);
double fiba_last_device_ms(const fiba_solver* s);   /* HIP-event time of the last call's Levenberg rounds, milliseconds */

#endif /* ORBSLAM3_HIP_FULLBA_H */
