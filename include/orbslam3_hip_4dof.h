/* Part of the C ABI of orbslam3_hip.h, which includes this file at its end: include that header, not this one.
 *
 * ---- pose graph of an inertial map: Optimizer::OptimizeEssentialGraph4DoF (src/Optimizer.cc:5292-5588) ----
 * LoopClosing::CorrectLoop calls it instead of OptimizeEssentialGraph once the map's IMU is initialised (src/LoopClosing.cc:1182):
 * roll, pitch and scale are observable there, so a key frame keeps them and moves in yaw and translation only.
 * essg_optimize_4dof is what the function does between building the graph and writing the map back: VertexPose4DoF vertices
 * (include/G2oTypes.h:155-189; oplusImpl = ImuCamPose::UpdateW with ur = (0, 0, u0), ut = (u1, u2, u3), including the clean-up of
 * DR on every fifth accepted update), Edge4DoF edges (:817-843) with ONE information matrix for all of them and no robust
 * kernel, g2o's numeric Jacobians (central differences, delta = 1e-9, through oplusImpl, the columns of a fixed vertex
 * skipped), Levenberg and optimize(max_iters), all in double; then the pose recovery and the map-point correction of
 * :5548-5586.  Every vertex is a pose, so there is no Schur complement: the 4 x 4-block system over the free vertices is
 * assembled densely and factored by the Cholesky kernels of the global BA.
 * The caller flattens the graph (include/orbslam3_shim_loop.hpp does it for the reference's types):
 *   - vertex k: rcw / tcw = Rcw[0], tcw[0], rwb / twb = Rwb (= Rwb0), twb, rcb / tcb = Rcb[0], tcb[0] of the ImuCamPose as its
 *     constructor leaves them (src/G2oTypes.cc:25-71 for a key frame's float pose, :121-146 for a corrected Sim3), rotations
 *     row-major.  The camera pose and the body pose of the first constructor are read from different float members and need not
 *     agree to the last bit: rcw / tcw are used as given until the vertex is first updated (and in the unperturbed side of a
 *     Jacobian column), afterwards Rcw = Rcb Rwb^T, tcw = Rcb (-Rwb^T twb) + tcb.  fixed[k] != 0 for setFixed(true);
 *   - edge e: edge_vertices[2e] = vertex 0 (i), [2e + 1] = vertex 1 (j), edge_rot / edge_trans = dRij, dtij (rotation and
 *     translation of Sij = Siw * Sjw^-1; the scale of a Sim3 product stays inside its translation).  The error is
 *     (LogSO3(Ri Rj^T dRij^T), Ri (-Rj^T tj) + ti - dtij).  An edge between two fixed vertices stays in the graph (it counts in
 *     chi2), and the same pair may appear more than once;
 *   - information: the 6 x 6 matrix of every edge, row-major; the reference's is diag(1e3, 1e3, 1, 1, 1, 1) (:5363-5366);
 *   - lambda_init <= 0: lambda_0 = 1e-5 * max diag H over the free unknowns (computeLambdaInit; the reference sets no user
 *     lambda here); > 0: used as given;
 *   - point p (optional): points[3p..] = GetWorldPos() (float), point_ref[p] = vertex of GetReferenceKeyFrame(); the result is
 *     Sim3(Ri, ti, 1).inverse().map(vScw[ref].map(P)) with scw[8 ref..] = vScw as q x y z w, t, s -- the INPUT Sim3 of that vertex,
 *     scale included (a corrected key frame's is not 1) -- computed in double and cast to float.  scw is read by this correction
 *     only and is NULL iff n_points == 0.
 * rcw_out / tcw_out: Rcw[0], tcw[0] of the optimised estimate in double; fixed vertices come back bit-identical to rcw / tcw.
 * pose_q / pose_t (may be NULL): what SetPose receives, SE3d(Quaterniond(Ri), ti).cast<float>(): x y z w normalised in double
 * and, after the cast, in float (Sophus::SO3's constructors), and the translation cast to float.
 * The handle is essg_optimize's (essg_create / essg_destroy / essg_last_device_ms): its stream and scratch serve either kind of
 * graph, ONE call at a time.  Capacity: ESSG_MAX_FREE_VERTICES free vertices (any number of fixed ones); above it
 * ORBX_ERR_CAPACITY, and the adapter falls back to the reference.  The dense factorisation grows with the cube of the number of
 * free vertices.
 * Argument checks (ORBX_ERR_ARG) are made before anything touches a device: NULL pointers, negative sizes, an index out of
 * range, an edge from a vertex to itself, no free vertex, a value that is not finite, a scale in scw that is not positive, an
 * information matrix that is not symmetric or has a diagonal entry that is not positive.
 * stop_flag (may be NULL): polled, never written, before every iteration and after every Levenberg trial (stop reason 3).
 * stats.stop_reason: 0 iteration cap, 1 ten trials or rho == 0, 2 three iterations below 1e-3 relative gain, 3 stop flag. */
#ifndef ORBSLAM3_HIP_4DOF_H
#define ORBSLAM3_HIP_4DOF_H

typedef struct Essg4DofProblem {
    int32_t n_vertices;
    const double* rcw;  const double* tcw;      /* [n][9] row-major, [n][3]: Rcw[0], tcw[0] as the constructor leaves them */
    const double* rwb;  const double* twb;      /* [n][9], [n][3]: Rwb (= Rwb0), twb */
    const double* rcb;  const double* tcb;      /* [n][9], [n][3]: mImuCalib.mTcb of that key frame */
    const uint8_t* fixed;                       /* [n] */
    int32_t n_edges;
    const int32_t* edge_vertices;               /* [n_edges][2]: vertex 0 (i), vertex 1 (j) */
    const double* edge_rot; const double* edge_trans;   /* [n_edges][9], [n_edges][3]: dRij, dtij */
    double information[36];                     /* one symmetric 6x6 for every edge, row-major */
    int32_t max_iters;                          /* 20 */
    double lambda_init;                         /* <= 0: 1e-5 * max diag H (what the reference does); > 0: used as given */
    int32_t n_points; const float* points; const int32_t* point_ref;
    const double* scw;                          /* [n][8] q x y z w, t, s: vScw, read by the point correction only; NULL iff n_points == 0 */
} Essg4DofProblem;
typedef struct Essg4DofResult { double* rcw_out; double* tcw_out; float* pose_q; float* pose_t; float* points_out; LbaStats stats; } Essg4DofResult;
int essg_optimize_4dof(essg_solver* s, const Essg4DofProblem*, Essg4DofResult*, const volatile uint8_t* stop_flag);
int essg_check_4dof(const Essg4DofProblem*, const Essg4DofResult*);   /* host only */

#endif /* ORBSLAM3_HIP_4DOF_H */
