/* Part of the C ABI of orbslam3_hip.h, which includes this file at its end: include that header, not this one.
 *
 * ---- the KannalaBrandt8 fisheye camera (src/CameraModels/KannalaBrandt8.cpp) for PoseOptimization and LocalBundleAdjustment ----
 * ORB-SLAM3 uses this camera for every fisheye lens (all TUM-VI sequences).  A handle on which a KB8 camera is set runs the
 * monocular edges EdgeSE3ProjectXYZOnlyPose / EdgeSE3ProjectXYZ with pCamera = KannalaBrandt8: the error is
 * obs - project(Xc) with project(Vector3d) of :46-65 (theta and psi through float arctangents, the polynomial in double), the
 * Jacobians are -projectJac(Xc) (:145-175, all double) times the SE3 derivative rows of the pinhole edges.  Huber kernels,
 * Levenberg, the four outlier rounds of PoseOptimization and isDepthPositive do not depend on the camera.
 * The device's theta and psi differ from the host libm's by at most one float ulp (csrc/camera_kb8.h says why), so results are
 * close to, not bit-identical with, a CPU build of the reference; DESIGN.md 4g gives the measured spread.
 *
 * While a KB8 camera is set on a handle:
 *   - pose_optimize, pose_optimize_batch, lba_solve and lba_solve_batch use it; fx, fy, cx, cy and bf of the problem are not read;
 *   - a stereo edge is ORBX_ERR_ARG (such a frame is monocular; a two-camera rig is set with *_set_rig_kb8);
 *   - pose_optimize_batch_device returns ORBX_ERR_ARG (it has no KB8 path and must not project as a pinhole);
 *   - fx <= 0 or fy <= 0 in a setter is ORBX_ERR_ARG and leaves the handle's camera as it was.
 * These checks are made before anything touches a device, and the handle stays usable.  A setter with cam == NULL returns the
 * handle to the pinhole camera of the problems; results are then bit-identical to those of a fresh handle.
 * lba_solve_batch keeps its contract: window i equals lba_solve of that window bit for bit.
 * The stereo step of a two-camera rig, Frame::ComputeStereoFishEyeMatches, is built: orbslam3_hip_fisheye.h.  The right-camera edges
 * of such a rig, EdgeSE3ProjectXYZOnlyPoseToBody / EdgeSE3ProjectXYZToBody with mpCamera2, are built: OrbxKB8Rig below.
 * Not built: the Nleft != -1 branches of the matchers, KeyFrame::UnprojectStereoFishEye, the matcher's device-side projections,
 * the KB8 camera (one or two) in the inertial solvers, in the sharded global BA (lba_shard_*) and in the pose graphs. */
typedef struct OrbxKB8 { double fx, fy, cx, cy, k[4]; } OrbxKB8;   /* mvParameters[0..7], floats promoted to double */

int pose_set_camera_kb8(pose_solver* s, const OrbxKB8* cam);        /* NULL: back to pinhole */
int lba_set_camera_kb8(lba_solver* s, const OrbxKB8* cam);
int lba_batch_set_camera_kb8(lba_batch* b, const OrbxKB8* cam);     /* one camera for every window of a call */
/* diagnostic: project (and, if jac != NULL, projectJac, 2 x 3 row-major) of n camera-frame points with the device functions
 * the solvers use */
int orbx_kb8_project(int device, const OrbxKB8* cam, const double* Xc, int n, double* uv /*[n][2]*/, double* jac /*[n][6], may be NULL*/);

/* ---- a rig of two KannalaBrandt8 cameras (mpCamera, mpCamera2) in PoseOptimization and LocalBundleAdjustment ----
 * While a rig is set on a handle, the per-edge byte PoseProblem::stereo[i] / LbaProblem::edge_stereo[e] names the camera of the edge:
 *   0                a left-camera edge: the monocular KB8 edge above with rig.left, bit for bit;
 *   ORBX_EDGE_RIGHT  a right-camera edge, EdgeSE3ProjectXYZOnlyPoseToBody / EdgeSE3ProjectXYZToBody (src/OptimizableTypes.cpp:91-107,
 *                    192-213): error obs - right.project(X_r) with X_r = Trl X_l, obs[0..1] the key point of mvKeysRight; pose Jacobian
 *                    -right.projectJac(X_r) R_rl SE3deriv(X_l), point Jacobian -right.projectJac(X_r) R_rl R_lw; isDepthPositive is
 *                    X_r.z > 0.  Huber delta, information, the 5.991 threshold and the four outlier rounds are those of a mono edge;
 *   anything else    (1 = rectified stereo, or > 2) is ORBX_ERR_ARG.
 * Edges are summed in the order given, left and right interleaved, as g2o sums them in addEdge order.
 * pose_optimize_batch_device returns ORBX_ERR_ARG.  A setter rejects fx <= 0 or fy <= 0 in either camera and a quaternion of zero or
 * non-finite norm with ORBX_ERR_ARG and leaves the handle as it was.  All these checks are made before anything touches a device, and
 * the handle stays usable.  The last setter wins, *_set_camera_kb8 or *_set_rig_kb8; NULL to either returns the handle to the pinhole
 * camera of the problems, with the bits of a fresh handle.  lba_solve_batch keeps its contract: window i equals lba_solve of that
 * window bit for bit. */
typedef struct OrbxKB8Rig {
    OrbxKB8 left, right;      /* mpCamera, mpCamera2 */
    double q_rl[4], t_rl[3];  /* GetRelativePoseTrl() as g2o::SE3Quat: qx qy qz qw (normalised on entry like the SE3Quat ctor), t; floats cast to double */
} OrbxKB8Rig;
#define ORBX_EDGE_RIGHT 2     /* value of PoseProblem::stereo[i] / LbaProblem::edge_stereo[e] for a right-camera edge */
int pose_set_rig_kb8(pose_solver* s, const OrbxKB8Rig* rig);       /* NULL: back to pinhole */
int lba_set_rig_kb8(lba_solver* s, const OrbxKB8Rig* rig);
int lba_batch_set_rig_kb8(lba_batch* b, const OrbxKB8Rig* rig);    /* one rig for every window of a call */
