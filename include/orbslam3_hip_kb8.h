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
 *   - a stereo edge is ORBX_ERR_ARG (KB8 frames are monocular, or a two-camera rig, whose edges are not built);
 *   - pose_optimize_batch_device returns ORBX_ERR_ARG (it has no KB8 path and must not project as a pinhole);
 *   - fx <= 0 or fy <= 0 in a setter is ORBX_ERR_ARG and leaves the handle's camera as it was.
 * These checks are made before anything touches a device, and the handle stays usable.  A setter with cam == NULL returns the
 * handle to the pinhole camera of the problems; results are then bit-identical to those of a fresh handle.
 * lba_solve_batch keeps its contract: window i equals lba_solve of that window bit for bit.
 * The stereo step of a two-camera rig, Frame::ComputeStereoFishEyeMatches, is built: orbslam3_hip_fisheye.h.
 * Not built: what reads its outputs (the Nleft != -1 branches of the matchers, the EdgeSE3ProjectXYZToBody edges with mpCamera2,
 * KeyFrame::UnprojectStereoFishEye), the matcher's device-side projections, the inertial solvers, the sharded global BA
 * (lba_shard_*) and the pose graphs. */
typedef struct OrbxKB8 { double fx, fy, cx, cy, k[4]; } OrbxKB8;   /* mvParameters[0..7], floats promoted to double */

int pose_set_camera_kb8(pose_solver* s, const OrbxKB8* cam);        /* NULL: back to pinhole */
int lba_set_camera_kb8(lba_solver* s, const OrbxKB8* cam);
int lba_batch_set_camera_kb8(lba_batch* b, const OrbxKB8* cam);     /* one camera for every window of a call */
/* diagnostic: project (and, if jac != NULL, projectJac, 2 x 3 row-major) of n camera-frame points with the device functions
 * the solvers use */
int orbx_kb8_project(int device, const OrbxKB8* cam, const double* Xc, int n, double* uv /*[n][2]*/, double* jac /*[n][6], may be NULL*/);
