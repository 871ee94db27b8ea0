// pose_opt_body.inc -- the body of the kernel template k_pose_opt (pose_solver.hip): the text of a kernel, not a function.
// Expects: problems (const ProblemDev*), cam (a camera policy: Pinhole, Fisheye or RigCam), STEREO (bool constant), kRegEdges (int constant).
// (As a __device__ function template called by the kernels the same statements compiled to other code for the pinhole kernels:
// other register allocation throughout, DESIGN.md 4f / 4g.  As the text of one templated kernel every instantiation is what it was, 4j.1.)
    __shared__ double s_acc[28][kAccRow];       // per-thread partials of H (21), b (6), chi2 (1), transposed
    __shared__ double s_out[28];
    __shared__ double s_red[4];
    const ProblemDev P = problems[blockIdx.x];
    const int tid = threadIdx.x;
    const int n = P.n;
    const int e_rest = tid + kRegEdges * 256;   // first edge of this thread that lives in global memory

    double T0[7] = {P.q[0], P.q[1], P.q[2], P.q[3], P.t[0], P.t[1], P.t[2]};
    quat_normalize(T0);                                 // SE3Quat(Quaterniond, Vector3d) (:829)
    double T[7];
    for (int k = 0; k < 7; k++) T[k] = T0[k];
    __shared__ int s_iters[4], s_trials[4];             // statistics only (thread 0)
    __shared__ double s_chi[4];
    if (tid < 4) { s_iters[tid] = 0; s_trials[tid] = 0; s_chi[tid] = 0; }
    // register-resident edges: data, level (active), outlier flag, last computed error
    Edge ce[kRegEdges];
    double cerr[kRegEdges][3];
    bool cvalid[kRegEdges], cact[kRegEdges], cout_[kRegEdges];
#pragma unroll
    for (int j = 0; j < kRegEdges; j++) {
        const int e = tid + j * 256;
        cvalid[j] = e < n;
        if (cvalid[j]) ce[j] = load_edge<STEREO>(cam, P, e);
        else { ce[j].X[0] = 0; ce[j].X[1] = 0; ce[j].X[2] = 1; ce[j].o[0] = 0; ce[j].o[1] = 0; ce[j].o[2] = 0; ce[j].w = 0; ce[j].st = 0; }
        cact[j] = cvalid[j]; cout_[j] = false;
        cerr[j][0] = 0; cerr[j][1] = 0; cerr[j][2] = 0;
    }
    for (int e = e_rest; e < n; e += 256) { P.active[e] = 1; P.outlier[e] = 0; P.err[3 * (size_t)e] = 0; P.err[3 * (size_t)e + 1] = 0; P.err[3 * (size_t)e + 2] = 0; }
    Robust rb;
    rb.on = true;
    rb.delta_m = P.huber_mono; rb.delta_s = P.huber_stereo;
    rb.dsq_m = P.huber_mono * P.huber_mono; rb.dsq_s = P.huber_stereo * P.huber_stereo;
    int nBad = 0;
#ifdef POSE_TIMING
    long long tm[6] = {0, 0, 0, 0, 0, 0}, t_prev = clock64();
#define POSE_TICK(k) { const long long t_now = clock64(); tm[k] += t_now - t_prev; t_prev = t_now; }
#else
#define POSE_TICK(k)
#endif
    const int rounds = (n >= 3) ? 4 : 0;                // nInitialCorrespondences < 3 -> return 0 (:998-999)
#pragma unroll 1
    for (int round = 0; round < rounds; round++) {
        for (int k = 0; k < 7; k++) T[k] = T0[k];       // every round restarts from the frame pose (:1007-1008)
        // ---- optimizer.initializeOptimization(0); optimizer.optimize(10) ----
        double cnt = 0;
#pragma unroll
        for (int j = 0; j < kRegEdges; j++) cnt += cact[j] ? 1.0 : 0.0;
        for (int e = e_rest; e < n; e += 256) cnt += P.active[e];
        const int n_active = (int)dlm::block_sum(cnt, s_red);
        if (n_active > 0) {
            double lambda = 0, ni = 2;
            int nbad_lm = 0;
#pragma unroll 1
            for (int it = 0; it < 10; it++) {
                // computeActiveErrors + activeRobustChi2 + buildSystem on the current estimate
                double acc[28];
                for (int k = 0; k < 28; k++) acc[k] = 0;
#pragma unroll
                for (int j = 0; j < kRegEdges; j++)
                    if (cact[j]) edge_build<STEREO>(cam, P, T, ce[j], rb, cerr[j], acc);
                for (int e = e_rest; e < n; e += 256) {
                    if (!P.active[e]) continue;
                    const Edge d = load_edge<STEREO>(cam, P, e);
                    double r[3];
                    edge_build<STEREO>(cam, P, T, d, rb, r, acc);
                    P.err[3 * (size_t)e] = r[0]; P.err[3 * (size_t)e + 1] = r[1]; P.err[3 * (size_t)e + 2] = r[2];
                }
                POSE_TICK(0)
                // two-stage ordered reduction through LDS: 28 values x 256 partials -> 8 partials of 32 -> 1
#pragma unroll
                for (int k = 0; k < 28; k++) s_acc[k][tid + (tid >> 5)] = acc[k];
                __syncthreads();
                if (tid < 224) {
                    const int k = tid >> 3, part = tid & 7;
                    const double* src = &s_acc[k][part * 33];
                    double v = 0;
#pragma unroll 8
                    for (int i = 0; i < 32; i++) v += src[i];
                    v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
                    if (part == 0) s_out[k] = v;
                }
                __syncthreads();
                double Hu[21], b[6];
#pragma unroll
                for (int k = 0; k < 21; k++) Hu[k] = s_out[k];
#pragma unroll
                for (int k = 0; k < 6; k++) b[k] = s_out[21 + k];
                double cur = s_out[27];
                const double ini = cur;
                if (it == 0) { lambda = dlm::lambda_init<6>(Hu); ni = 2; nbad_lm = 0; }
                POSE_TICK(1)
                // ---- LM trial loop (levenberg.cpp:102-149) ----
                int qmax = 0;
                double rho = 0;
#pragma unroll 1
                do {
                    double x[6], Tt[7];
                    const bool ok2 = dlm::ldlt_solve<6, true>(Hu, lambda, b, x);
                    if (ok2) pose_oplus<true>(T, x, Tt);
                    else {
                        for (int k = 0; k < 7; k++) Tt[k] = T[k];
                        for (int k = 0; k < 6; k++) x[k] = 0;
                    }
                    POSE_TICK(2)
                    double tchi = 0;
#pragma unroll
                    for (int j = 0; j < kRegEdges; j++)
                        if (cact[j]) tchi += edge_trial<STEREO>(cam, P, Tt, ce[j], rb, cerr[j]);
                    for (int e = e_rest; e < n; e += 256) {
                        if (!P.active[e]) continue;
                        const Edge d = load_edge<STEREO>(cam, P, e);
                        double r[3];
                        tchi += edge_trial<STEREO>(cam, P, Tt, d, rb, r);
                        P.err[3 * (size_t)e] = r[0]; P.err[3 * (size_t)e + 1] = r[1]; P.err[3 * (size_t)e + 2] = r[2];
                    }
                    POSE_TICK(3)
                    const double tempChi = dlm::block_sum(tchi, s_red);
                    double scale = 0;
#pragma unroll
                    for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + b[j]);
                    if (dlm::trial(ok2, tempChi, scale, lambda, ni, cur, rho))
                        for (int k = 0; k < 7; k++) T[k] = Tt[k];     // discardTop(); after pop() the estimate stays
                    qmax++;
                    POSE_TICK(4)
                } while (dlm::more_trials(rho, qmax));
                if (tid == 0) { s_iters[round]++; s_trials[round] += qmax; s_chi[round] = cur; }
                if (dlm::stop_reason(qmax, rho, ini, cur, nbad_lm)) break;      // stop rules (:151-166)
            }
        }
        // ---- inlier / outlier classification with float chi2 (:1016-1100) ----
        double bad = 0;
#pragma unroll
        for (int j = 0; j < kRegEdges; j++) {
            if (!cvalid[j]) continue;
            double Xc[3];
            if (cout_[j]) edge_eval<STEREO>(cam, P, T, ce[j], Xc, cerr[j]);      // inactive edges did not follow the estimate: e->computeError()
            const bool o = edge_is_outlier<STEREO>(ce[j], cerr[j]);
            cout_[j] = o; cact[j] = !o; bad += o ? 1.0 : 0.0;
        }
        for (int e = e_rest; e < n; e += 256) {
            const Edge d = load_edge<STEREO>(cam, P, e);
            double r[3];
            if (P.outlier[e]) {
                double Xc[3];
                edge_eval<STEREO>(cam, P, T, d, Xc, r);
                P.err[3 * (size_t)e] = r[0]; P.err[3 * (size_t)e + 1] = r[1]; P.err[3 * (size_t)e + 2] = r[2];
            } else {
                r[0] = P.err[3 * (size_t)e]; r[1] = P.err[3 * (size_t)e + 1]; r[2] = P.err[3 * (size_t)e + 2];
            }
            const bool o = edge_is_outlier<STEREO>(d, r);
            P.outlier[e] = o ? 1 : 0; P.active[e] = o ? 0 : 1; bad += o ? 1.0 : 0.0;
        }
        nBad = (int)dlm::block_sum(bad, s_red);
        POSE_TICK(5)
        if (round == 2) rb.on = false;      // setRobustKernel(0) after the third round
        if (n < 10) break;                  // optimizer.edges().size() < 10
    }
#pragma unroll
    for (int j = 0; j < kRegEdges; j++)
        if (cvalid[j]) P.outlier[tid + j * 256] = cout_[j] ? 1 : 0;
    if (tid == 0) {
        PoseResult R;
        for (int k = 0; k < 4; k++) R.q[k] = T[k];
        for (int k = 0; k < 3; k++) R.t[k] = T[4 + k];
        R.n_bad = nBad;
        R.inliers = (n < 3) ? 0 : n - nBad;
        for (int k = 0; k < 4; k++) { R.iterations[k] = s_iters[k]; R.trials[k] = s_trials[k]; R.chi2[k] = s_chi[k]; }
#ifdef POSE_TIMING
        for (int k = 0; k < 4; k++) R.chi2[k] = (double)tm[k];
        R.t[0] = (double)tm[4]; R.t[1] = (double)tm[5];
#endif
        *P.result = R;
    }
