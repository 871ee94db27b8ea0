// The arithmetic of IMU pre-integration, one function per unit of work (a job, a measurement of a frame, a link, a prediction), for
// the device (imu_preintegrate.hip: one lane each) and for a host compiler (tools/preint_cpu.cpp, the single-core yardstick of
// tools/preint_timing.py, and the stand-alone checks of tests/test_imu_preint_reference.py).  Plain C++: no HIP call, no LDS, nothing
// shared between units.  Build with -ffp-contract=off: the float state must not depend on FMA contraction.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/orbslam3_hip.h"

#ifdef __HIPCC__
#define PREINT_HD __host__ __device__ __forceinline__
#define PREINT_UNROLL _Pragma("unroll")
#else
#define PREINT_HD inline
#define PREINT_UNROLL
#endif

namespace preint {

// ---- 3 x 3 helpers (row major, float unless the name says otherwise; -ffp-contract=off: no FMA) ----
PREINT_HD void mul33(const float* A, const float* B, float* R)         // R = A B
{
PREINT_UNROLL
    for (int r = 0; r < 3; r++)
PREINT_UNROLL
        for (int c = 0; c < 3; c++) R[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
PREINT_HD void mul33t(const float* A, const float* B, float* R)        // R = A B^T
{
PREINT_UNROLL
    for (int r = 0; r < 3; r++)
PREINT_UNROLL
        for (int c = 0; c < 3; c++) R[3 * r + c] = A[3 * r] * B[3 * c] + A[3 * r + 1] * B[3 * c + 1] + A[3 * r + 2] * B[3 * c + 2];
}
PREINT_HD void mult33(const float* A, const float* B, float* R)        // R = A^T B
{
PREINT_UNROLL
    for (int r = 0; r < 3; r++)
PREINT_UNROLL
        for (int c = 0; c < 3; c++) R[3 * r + c] = A[r] * B[c] + A[3 + r] * B[3 + c] + A[6 + r] * B[6 + c];
}
PREINT_HD void mulv3(const float* A, const float* v, float* r)
{
PREINT_UNROLL
    for (int k = 0; k < 3; k++) r[k] = A[3 * k] * v[0] + A[3 * k + 1] * v[1] + A[3 * k + 2] * v[2];
}
PREINT_HD void hat(const float* v, float* W)
{
    W[0] = 0.f; W[1] = -v[2]; W[2] = v[1];
    W[3] = v[2]; W[4] = 0.f; W[5] = -v[0];
    W[6] = -v[1]; W[7] = v[0]; W[8] = 0.f;
}

// The polar factor U V^T of a nearly orthogonal X (NormalizeRotation), in double: Newton's X <- (X + X^-T) / 2, which converges
// quadratically from a matrix that is orthogonal to float rounding; the loop ends when the next step would be below double rounding.
PREINT_HD void polar3(double* X)
{
    for (int it = 0; it < 24; it++) {
        const double c00 = X[4] * X[8] - X[5] * X[7], c01 = X[5] * X[6] - X[3] * X[8], c02 = X[3] * X[7] - X[4] * X[6];
        const double c10 = X[2] * X[7] - X[1] * X[8], c11 = X[0] * X[8] - X[2] * X[6], c12 = X[1] * X[6] - X[0] * X[7];
        const double c20 = X[1] * X[5] - X[2] * X[4], c21 = X[2] * X[3] - X[0] * X[5], c22 = X[0] * X[4] - X[1] * X[3];
        const double inv = 1.0 / (X[0] * c00 + X[1] * c01 + X[2] * c02);
        const double cof[9] = {c00, c01, c02, c10, c11, c12, c20, c21, c22};        // X^-T = cofactor matrix / det
        double move = 0.0;
PREINT_UNROLL
        for (int k = 0; k < 9; k++) {
            const double n = 0.5 * (X[k] + cof[k] * inv);
            move = fmax(move, fabs(n - X[k]));
            X[k] = n;
        }
        if (!(move > 1e-8)) break;          // quadratic: what is left is the square of the last step (also ends on NaN)
    }
}
PREINT_HD void normalize_product(const float* A, const double* B, float* R)   // R = polar(A B)
{
    double X[9];
PREINT_UNROLL
    for (int r = 0; r < 3; r++)
PREINT_UNROLL
        for (int c = 0; c < 3; c++) X[3 * r + c] = (double)A[3 * r] * B[c] + (double)A[3 * r + 1] * B[3 + c] + (double)A[3 * r + 2] * B[6 + c];
    polar3(X);
PREINT_UNROLL
    for (int k = 0; k < 9; k++) R[k] = (float)X[k];
}

// exp and right Jacobian of the rotation vector v (IntegratedRotation, :84-105).  The branch is the reference's, on the float angle;
// the coefficients are taken in double: (1 - cos d) and (d - sin d) cancel to a few bits in float at the angles of one IMU sample.
PREINT_HD void rotation_increment(const float* v, double* dRi, double* rJ)
{
    const float d2f = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    const float df = std::sqrt(d2f);
    const double x = v[0], y = v[1], z = v[2];
    const double W[9] = {0, -z, y, z, 0, -x, -y, x, 0};
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (df < 1e-4f) {
PREINT_UNROLL
        for (int k = 0; k < 9; k++) { dRi[k] = I[k] + W[k]; rJ[k] = I[k]; }
        return;
    }
    const double d2 = x * x + y * y + z * z;
    double ka, kb, kc;                                      // sin d / d, (1 - cos d) / d^2, (d - sin d) / d^3
    if (d2 < 0.0625) {
        // their series in d^2 (Horner): below d = 0.25 the ninth term is under 1e-19 of the first, and nothing cancels
        ka = 1.0 + d2 * (-1.0 / 6 + d2 * (1.0 / 120 + d2 * (-1.0 / 5040 + d2 * (1.0 / 362880 + d2 * (-1.0 / 39916800 + d2 * (1.0 / 6227020800.0 + d2 * (-1.0 / 1307674368000.0)))))));
        kb = 0.5 + d2 * (-1.0 / 24 + d2 * (1.0 / 720 + d2 * (-1.0 / 40320 + d2 * (1.0 / 3628800 + d2 * (-1.0 / 479001600 + d2 * (1.0 / 87178291200.0 + d2 * (-1.0 / 20922789888000.0)))))));
        kc = 1.0 / 6 + d2 * (-1.0 / 120 + d2 * (1.0 / 5040 + d2 * (-1.0 / 362880 + d2 * (1.0 / 39916800 + d2 * (-1.0 / 6227020800.0 + d2 * (1.0 / 1307674368000.0 + d2 * (-1.0 / 355687428096000.0)))))));
    } else {
        const double d = sqrt(d2), s = sin(d), h = sin(0.5 * d);
        ka = s / d; kb = 2.0 * h * h / d2; kc = (d - s) / (d2 * d);         // 1 - cos d = 2 sin^2(d / 2)
    }
    double WW[9];
PREINT_UNROLL
    for (int r = 0; r < 3; r++)
PREINT_UNROLL
        for (int q = 0; q < 3; q++) WW[3 * r + q] = W[3 * r] * W[q] + W[3 * r + 1] * W[3 + q] + W[3 * r + 2] * W[6 + q];
PREINT_UNROLL
    for (int k = 0; k < 9; k++) { dRi[k] = I[k] + W[k] * ka + WW[k] * kb; rJ[k] = I[k] - W[k] * kb + WW[k] * kc; }
}

PREINT_HD bool finite_measurement(const ImuMeasurement& m)
{
    bool ok = m.dt > 0.f && std::isfinite(m.dt);
PREINT_UNROLL
    for (int k = 0; k < 3; k++) ok = ok && std::isfinite(m.a[k]) && std::isfinite(m.w[k]);
    return ok;
}

// ---- Initialize + IntegrateNewMeasurement: one lane per job ----
PREINT_HD void preintegrate_job(ImuPreintState* states, int n_states, const ImuPreintJob* jobs, int n_jobs, const ImuMeasurement* meas, int n_meas,
                                int32_t* status, int j, bool trusted)
{
    const ImuPreintJob job = jobs[j];
    // contents: the ranges, one writer per state, every measurement of the job.  Nothing is written before all of them hold.
    // trusted: the host entry has made these very checks (check_preintegrate) before it staged the call.
    bool ok = trusted || (job.state >= 0 && job.state < n_states && job.count >= 0 && job.first >= 0 && job.first <= n_meas && job.count <= n_meas - job.first);
    if (ok && !trusted) {
PREINT_UNROLL
        for (int k = 0; k < 6; k++) ok = ok && (!job.reset || std::isfinite(job.bias[k]));
        int writers = 0;                            // (every lane reads the same words: the loads are uniform and independent)
        for (int k = 0; k < n_jobs; k++) writers += jobs[k].state == job.state ? 1 : 0;
        ok = ok && writers == 1;
    }
    if (ok && !trusted)
        for (int i = 0; i < job.count; i++) ok = ok && finite_measurement(meas[job.first + i]);
    if (!ok) { status[j] = ORBX_ERR_ARG; return; }
    status[j] = ORBX_OK;

    ImuPreintState* const S = states + job.state;
    float dT, b[6], nga[6], walk[6], dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], avgA[3], avgW[3], C[81], Cw[6];
    int32_t n_done;
PREINT_UNROLL
    for (int k = 0; k < 6; k++) { nga[k] = S->nga[k]; walk[k] = S->nga_walk[k]; }
    if (job.reset) {
        dT = 0.f; n_done = 0;
PREINT_UNROLL
        for (int k = 0; k < 6; k++) { b[k] = job.bias[k]; Cw[k] = 0.f; }
PREINT_UNROLL
        for (int k = 0; k < 9; k++) { dR[k] = (k % 4 == 0) ? 1.f : 0.f; JRg[k] = JVg[k] = JVa[k] = JPg[k] = JPa[k] = 0.f; }
PREINT_UNROLL
        for (int k = 0; k < 3; k++) dV[k] = dP[k] = avgA[k] = avgW[k] = 0.f;
PREINT_UNROLL
        for (int k = 0; k < 81; k++) C[k] = 0.f;
        for (int k = 0; k < 225; k++) S->C[k] = 0.f;
PREINT_UNROLL
        for (int k = 0; k < 6; k++) { S->b[k] = job.bias[k]; S->bu[k] = job.bias[k]; }
    } else {
        dT = S->dT; n_done = S->n_meas;
PREINT_UNROLL
        for (int k = 0; k < 6; k++) { b[k] = S->b[k]; Cw[k] = S->C[15 * (9 + k) + 9 + k]; }
PREINT_UNROLL
        for (int k = 0; k < 9; k++) { dR[k] = S->dR[k]; JRg[k] = S->JRg[k]; JVg[k] = S->JVg[k]; JVa[k] = S->JVa[k]; JPg[k] = S->JPg[k]; JPa[k] = S->JPa[k]; }
PREINT_UNROLL
        for (int k = 0; k < 3; k++) { dV[k] = S->dV[k]; dP[k] = S->dP[k]; avgA[k] = S->avgA[k]; avgW[k] = S->avgW[k]; }
PREINT_UNROLL
        for (int r = 0; r < 9; r++)
PREINT_UNROLL
            for (int c = 0; c < 9; c++) C[9 * r + c] = S->C[15 * r + c];
    }

    ImuMeasurement next;
    if (job.count > 0) next = meas[job.first];
    for (int i = 0; i < job.count; i++) {
        const ImuMeasurement m = next;
        if (i + 1 < job.count) next = meas[job.first + i + 1];          // loaded ahead of its use
        const float dt = m.dt;
        float acc[3], accW[3], Ra[3];
PREINT_UNROLL
        for (int k = 0; k < 3; k++) { acc[k] = m.a[k] - b[k]; accW[k] = m.w[k] - b[3 + k]; }
        mulv3(dR, acc, Ra);
        const float tsum = dT + dt;
PREINT_UNROLL
        for (int k = 0; k < 3; k++) {
            avgA[k] = (dT * avgA[k] + Ra[k] * dt) / tsum;
            avgW[k] = (dT * avgW[k] + accW[k] * dt) / tsum;
            dP[k] = dP[k] + dV[k] * dt + 0.5f * Ra[k] * dt * dt;
            dV[k] = dV[k] + Ra[k] * dt;
        }
        // the velocity and position rows of A and B, with the rotation before this measurement
        float Wacc[9], Rdt[9], Rh[9], A10[9], A20[9], T[9];
        hat(acc, Wacc);
PREINT_UNROLL
        for (int k = 0; k < 9; k++) { Rdt[k] = dR[k] * dt; Rh[k] = 0.5f * dR[k] * dt * dt; }
        mul33(Rdt, Wacc, A10);
        mul33(Rh, Wacc, A20);
PREINT_UNROLL
        for (int k = 0; k < 9; k++) { A10[k] = -A10[k]; A20[k] = -A20[k]; }
        // the Jacobians of position and velocity with respect to the biases
        mul33(A20, JRg, T);
PREINT_UNROLL
        for (int k = 0; k < 9; k++) { JPa[k] = JPa[k] + JVa[k] * dt - Rh[k]; JPg[k] = JPg[k] + JVg[k] * dt + T[k]; }
        mul33(A10, JRg, T);
PREINT_UNROLL
        for (int k = 0; k < 9; k++) { JVa[k] = JVa[k] - Rdt[k]; JVg[k] = JVg[k] + T[k]; }
        // the rotation
        float v[3];
PREINT_UNROLL
        for (int k = 0; k < 3; k++) v[k] = accW[k] * dt;
        double dRi_d[9], rJ_d[9];
        rotation_increment(v, dRi_d, rJ_d);
        float dRi[9], B00[9];
PREINT_UNROLL
        for (int k = 0; k < 9; k++) { dRi[k] = (float)dRi_d[k]; B00[k] = (float)rJ_d[k] * dt; }
        normalize_product(dR, dRi_d, dR);
        // C <- A C A^T + B N B^T in 3 x 3 blocks.  A = [E 0 0; A10 I 0; A20 dt I I] with E = dRi^T, so M = A C has the block rows
        //   M0j = E C0j,   M1j = A10 C0j + C1j,   M2j = A20 C0j + dt C1j + C2j
        // and C' = M A^T the block columns   C'i0 = Mi0 E^T,   C'i1 = Mi0 A10^T + Mi1,   C'i2 = Mi0 A20^T + dt Mi1 + Mi2.
        float M[81];
PREINT_UNROLL
        for (int jb = 0; jb < 3; jb++) {
            float C0[9], C1[9], C2[9], P[9], Q[9];
PREINT_UNROLL
            for (int r = 0; r < 3; r++)
PREINT_UNROLL
                for (int c = 0; c < 3; c++) { C0[3 * r + c] = C[9 * r + 3 * jb + c]; C1[3 * r + c] = C[9 * (3 + r) + 3 * jb + c]; C2[3 * r + c] = C[9 * (6 + r) + 3 * jb + c]; }
            mult33(dRi, C0, P);
PREINT_UNROLL
            for (int r = 0; r < 3; r++)
PREINT_UNROLL
                for (int c = 0; c < 3; c++) M[9 * r + 3 * jb + c] = P[3 * r + c];
            mul33(A10, C0, P);
            mul33(A20, C0, Q);
PREINT_UNROLL
            for (int r = 0; r < 3; r++)
PREINT_UNROLL
                for (int c = 0; c < 3; c++) {
                    M[9 * (3 + r) + 3 * jb + c] = P[3 * r + c] + C1[3 * r + c];
                    M[9 * (6 + r) + 3 * jb + c] = Q[3 * r + c] + C1[3 * r + c] * dt + C2[3 * r + c];
                }
        }
PREINT_UNROLL
        for (int ib = 0; ib < 3; ib++) {
            float M0[9], M1[9], M2[9], P[9], Q[9], R0[9];
PREINT_UNROLL
            for (int r = 0; r < 3; r++)
PREINT_UNROLL
                for (int c = 0; c < 3; c++) { M0[3 * r + c] = M[9 * (3 * ib + r) + c]; M1[3 * r + c] = M[9 * (3 * ib + r) + 3 + c]; M2[3 * r + c] = M[9 * (3 * ib + r) + 6 + c]; }
            mul33(M0, dRi, R0);                 // Mi0 E^T = Mi0 dRi
            mul33t(M0, A10, P);
            mul33t(M0, A20, Q);
PREINT_UNROLL
            for (int r = 0; r < 3; r++)
PREINT_UNROLL
                for (int c = 0; c < 3; c++) {
                    C[9 * (3 * ib + r) + c] = R0[3 * r + c];
                    C[9 * (3 * ib + r) + 3 + c] = P[3 * r + c] + M1[3 * r + c];
                    C[9 * (3 * ib + r) + 6 + c] = Q[3 * r + c] + M1[3 * r + c] * dt + M2[3 * r + c];
                }
        }
        // B N B^T: B = [B00 0; 0 Rdt; 0 Rh], N = diag(gyro x3, acc x3)
        {
            float Bg[9], Ba1[9], Ba2[9], P[9];
PREINT_UNROLL
            for (int r = 0; r < 3; r++)
PREINT_UNROLL
                for (int c = 0; c < 3; c++) { Bg[3 * r + c] = B00[3 * r + c] * nga[c]; Ba1[3 * r + c] = Rdt[3 * r + c] * nga[3 + c]; Ba2[3 * r + c] = Rh[3 * r + c] * nga[3 + c]; }
            mul33t(Bg, B00, P);
PREINT_UNROLL
            for (int r = 0; r < 3; r++)
PREINT_UNROLL
                for (int c = 0; c < 3; c++) C[9 * r + c] += P[3 * r + c];
            mul33t(Ba1, Rdt, P);
PREINT_UNROLL
            for (int r = 0; r < 3; r++)
PREINT_UNROLL
                for (int c = 0; c < 3; c++) C[9 * (3 + r) + 3 + c] += P[3 * r + c];
            mul33t(Ba1, Rh, P);
PREINT_UNROLL
            for (int r = 0; r < 3; r++)
PREINT_UNROLL
                for (int c = 0; c < 3; c++) C[9 * (3 + r) + 6 + c] += P[3 * r + c];
            mul33t(Ba2, Rdt, P);
PREINT_UNROLL
            for (int r = 0; r < 3; r++)
PREINT_UNROLL
                for (int c = 0; c < 3; c++) C[9 * (6 + r) + 3 + c] += P[3 * r + c];
            mul33t(Ba2, Rh, P);
PREINT_UNROLL
            for (int r = 0; r < 3; r++)
PREINT_UNROLL
                for (int c = 0; c < 3; c++) C[9 * (6 + r) + 6 + c] += P[3 * r + c];
        }
PREINT_UNROLL
        for (int k = 0; k < 6; k++) Cw[k] += walk[k];
        // the Jacobian of the rotation
        mult33(dRi, JRg, T);
PREINT_UNROLL
        for (int k = 0; k < 9; k++) JRg[k] = T[k] - B00[k];
        dT = tsum;
        n_done++;
    }

    S->dT = dT; S->n_meas = n_done;
PREINT_UNROLL
    for (int k = 0; k < 9; k++) { S->dR[k] = dR[k]; S->JRg[k] = JRg[k]; S->JVg[k] = JVg[k]; S->JVa[k] = JVa[k]; S->JPg[k] = JPg[k]; S->JPa[k] = JPa[k]; }
PREINT_UNROLL
    for (int k = 0; k < 3; k++) { S->dV[k] = dV[k]; S->dP[k] = dP[k]; S->avgA[k] = avgA[k]; S->avgW[k] = avgW[k]; }
PREINT_UNROLL
    for (int r = 0; r < 9; r++)
PREINT_UNROLL
        for (int c = 0; c < 9; c++) S->C[15 * r + c] = C[9 * r + c];
PREINT_UNROLL
    for (int k = 0; k < 6; k++) S->C[15 * (9 + k) + 9 + k] = Cw[k];
}

// ---- the interpolation loop of Tracking::PreintegrateIMU: one lane per (stream, measurement) ----
PREINT_HD void frame_measurement(const OrbeImuSample* samples, const int32_t* n_imu, const int64_t* t_prev_ns, const int64_t* t_cur_ns, int imu_cap,
                                 ImuMeasurement* meas_out, int32_t* count_out, int bq, int i)
{
    const int ni = n_imu[bq];
    const int n = (ni >= 1 && ni <= imu_cap) ? ni - 1 : 0;
    if (i == 0) count_out[bq] = n;
    if (i >= n) return;
    const OrbeImuSample s0 = samples[(size_t)bq * imu_cap + i], s1 = samples[(size_t)bq * imu_cap + i + 1];
    const double t0 = (double)s0.ts / 1e9, t1 = (double)s1.ts / 1e9, tp = (double)t_prev_ns[bq] / 1e9, tc = (double)t_cur_ns[bq] / 1e9;
    ImuMeasurement m;
    if (i == 0 && i < n - 1) {                      // the first of several: back to the previous frame's time
        const float tab = (float)(t1 - t0), tini = (float)(t0 - tp), f = tini / tab;
PREINT_UNROLL
        for (int k = 0; k < 3; k++) {
            m.a[k] = (s0.acce[k] + s1.acce[k] - (s1.acce[k] - s0.acce[k]) * f) * 0.5f;
            m.w[k] = (s0.gyro[k] + s1.gyro[k] - (s1.gyro[k] - s0.gyro[k]) * f) * 0.5f;
        }
        m.dt = (float)(t1 - tp);
    } else if (i < n - 1) {                         // in the middle
PREINT_UNROLL
        for (int k = 0; k < 3; k++) { m.a[k] = (s0.acce[k] + s1.acce[k]) * 0.5f; m.w[k] = (s0.gyro[k] + s1.gyro[k]) * 0.5f; }
        m.dt = (float)(t1 - t0);
    } else if (i > 0) {                             // the last of several: up to this frame's time
        const float tab = (float)(t1 - t0), tend = (float)(t1 - tc), f = tend / tab;
PREINT_UNROLL
        for (int k = 0; k < 3; k++) {
            m.a[k] = (s0.acce[k] + s1.acce[k] - (s1.acce[k] - s0.acce[k]) * f) * 0.5f;
            m.w[k] = (s0.gyro[k] + s1.gyro[k] - (s1.gyro[k] - s0.gyro[k]) * f) * 0.5f;
        }
        m.dt = (float)(tc - t0);
    } else {                                        // the only one
PREINT_UNROLL
        for (int k = 0; k < 3; k++) { m.a[k] = s0.acce[k]; m.w[k] = s0.gyro[k]; }
        m.dt = (float)(tc - tp);
    }
    meas_out[(size_t)bq * imu_cap + i] = m;
}

// ---- the informations of a link, in double: one lane per link ----
// A^-1 by Gauss-Jordan with partial pivoting, in place on [A | I]; false when a pivot is zero or the result is not finite
template <int N>
PREINT_HD bool invert(double* A, double* Inv)
{
    for (int r = 0; r < N; r++)
        for (int c = 0; c < N; c++) Inv[N * r + c] = r == c ? 1.0 : 0.0;
    for (int k = 0; k < N; k++) {
        int p = k;
        double best = fabs(A[N * k + k]);
        for (int r = k + 1; r < N; r++)
            if (fabs(A[N * r + k]) > best) { best = fabs(A[N * r + k]); p = r; }
        if (!(best > 0.0) || !std::isfinite(best)) return false;
        if (p != k)
            for (int c = 0; c < N; c++) {
                double t = A[N * k + c]; A[N * k + c] = A[N * p + c]; A[N * p + c] = t;
                t = Inv[N * k + c]; Inv[N * k + c] = Inv[N * p + c]; Inv[N * p + c] = t;
            }
        const double piv = A[N * k + k];
        for (int c = 0; c < N; c++) { A[N * k + c] /= piv; Inv[N * k + c] /= piv; }
        for (int r = 0; r < N; r++) {
            if (r == k) continue;
            const double f = A[N * r + k];
            if (f == 0.0) continue;
            for (int c = 0; c < N; c++) { A[N * r + c] -= f * A[N * k + c]; Inv[N * r + c] -= f * Inv[N * k + c]; }
        }
    }
    bool ok = true;
    for (int k = 0; k < N * N; k++) ok = ok && std::isfinite(Inv[k]);
    return ok;
}

// S (symmetric 9 x 9) <- V max(L, clamp) V^T with eigenvalues below 1e-12 set to 0: cyclic Jacobi.  A rotation whose off-diagonal
// entry is exactly zero is skipped, so a row and column that are decoupled stay decoupled to the bit.
PREINT_HD void clamp_eigenvalues9(double* S, double* V)
{
    constexpr int N = 9;
    for (int r = 0; r < N; r++)
        for (int c = 0; c < N; c++) V[N * r + c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int r = 0; r < N; r++)
            for (int c = 0; c < N; c++) { if (r != c) off += S[N * r + c] * S[N * r + c]; else diag += S[N * r + c] * S[N * r + c]; }
        if (!(off > 1e-34 * diag)) break;
        for (int p = 0; p < N - 1; p++)
            for (int q = p + 1; q < N; q++) {
                const double apq = S[N * p + q];
                if (apq == 0.0) continue;
                const double app = S[N * p + p], aqq = S[N * q + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < N; k++) {           // columns p, q
                    const double skp = S[N * k + p], skq = S[N * k + q];
                    S[N * k + p] = c * skp - s * skq; S[N * k + q] = s * skp + c * skq;
                }
                for (int k = 0; k < N; k++) {           // rows p, q
                    const double spk = S[N * p + k], sqk = S[N * q + k];
                    S[N * p + k] = c * spk - s * sqk; S[N * q + k] = s * spk + c * sqk;
                }
                S[N * p + q] = S[N * q + p] = 0.0;
                for (int k = 0; k < N; k++) {
                    const double vkp = V[N * k + p], vkq = V[N * k + q];
                    V[N * k + p] = c * vkp - s * vkq; V[N * k + q] = s * vkp + c * vkq;
                }
            }
    }
    double L[N];
    for (int k = 0; k < N; k++) L[k] = S[N * k + k] < 1e-12 ? 0.0 : S[N * k + k];
    for (int r = 0; r < N; r++)
        for (int c = r; c < N; c++) {
            double a = 0.0;
            for (int k = 0; k < N; k++) a += V[N * r + k] * L[k] * V[N * c + k];
            S[N * r + c] = a; S[N * c + r] = a;
        }
}

PREINT_HD void build_link(const ImuPreintState* states, int n_states, const ImuLinkSpec* specs, LibaLink* links, int32_t* status, int l)
{
    const ImuLinkSpec sp = specs[l];
    if (sp.state < 0 || sp.state >= n_states || sp.walk_state < -1 || sp.walk_state >= n_states) { status[l] = ORBX_ERR_ARG; return; }
    const ImuPreintState* const S = states + sp.state;
    LibaLink* const L = links + l;
    L->kf1 = sp.kf1; L->kf2 = sp.kf2; L->robust = sp.robust; L->dT = S->dT;
    for (int k = 0; k < 9; k++) { L->dR[k] = S->dR[k]; L->JRg[k] = S->JRg[k]; L->JVg[k] = S->JVg[k]; L->JVa[k] = S->JVa[k]; L->JPg[k] = S->JPg[k]; L->JPa[k] = S->JPa[k]; }
    for (int k = 0; k < 3; k++) { L->dV[k] = S->dV[k]; L->dP[k] = S->dP[k]; }
    for (int k = 0; k < 6; k++) L->bias0[k] = S->b[k];
    double A[81], Inv[81];
    for (int r = 0; r < 9; r++)
        for (int c = 0; c < 9; c++) A[9 * r + c] = (double)S->C[15 * r + c];
    bool ok = invert<9>(A, Inv);
    double G[9], Gi[9], Ac[9], Ai[9];
    for (int k = 0; k < 9; k++) Gi[k] = Ai[k] = 0.0;
    if (sp.walk_state >= 0) {
        const ImuPreintState* const Wk = states + sp.walk_state;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) { G[3 * r + c] = (double)Wk->C[15 * (9 + r) + 9 + c]; Ac[3 * r + c] = (double)Wk->C[15 * (12 + r) + 12 + c]; }
        ok = invert<3>(G, Gi) && ok;
        ok = invert<3>(Ac, Ai) && ok;
    }
    if (ok) {
        for (int r = 0; r < 9; r++)
            for (int c = r; c < 9; c++) { const double m = (Inv[9 * r + c] + Inv[9 * c + r]) / 2; A[9 * r + c] = m; A[9 * c + r] = m; }
        clamp_eigenvalues9(A, Inv);
        for (int k = 0; k < 81; k++) { A[k] *= sp.info_scale; ok = ok && std::isfinite(A[k]); }
    }
    if (!ok) {
        for (int k = 0; k < 81; k++) A[k] = 0.0;
        for (int k = 0; k < 9; k++) Gi[k] = Ai[k] = 0.0;
    }
    for (int k = 0; k < 81; k++) L->info9[k] = A[k];
    for (int k = 0; k < 9; k++) { L->info_gyro[k] = Gi[k]; L->info_acc[k] = Ai[k]; }
    status[l] = ok ? ORBX_OK : ORBX_ERR_ARG;
}

// ---- the arithmetic of Tracking::PredictStateIMU: one lane per job ----
PREINT_HD void predict_job(const ImuPreintState* states, int n_states, const ImuPredictJob* jobs, ImuPredictOut* out, int32_t* status, int j)
{
    const ImuPredictJob job = jobs[j];
    if (job.state < 0 || job.state >= n_states) { status[j] = ORBX_ERR_ARG; return; }
    const ImuPreintState* const S = states + job.state;
    float dba[3], dbg[3], dR[9], JRg[9], J[9], v[3], r3[3], q3[3];
PREINT_UNROLL
    for (int k = 0; k < 3; k++) { dba[k] = job.bias[k] - S->b[k]; dbg[k] = job.bias[3 + k] - S->b[3 + k]; }
PREINT_UNROLL
    for (int k = 0; k < 9; k++) { dR[k] = S->dR[k]; JRg[k] = S->JRg[k]; }
    // GetDeltaRotation: Normalize(dR Exp(JRg dbg)); the exponential in double (Sophus::SO3f::exp has no first-order branch)
    mulv3(JRg, dbg, v);
    double E[9];
    {
        const double x = v[0], y = v[1], z = v[2], d2 = x * x + y * y + z * z, d = sqrt(d2);
        double ka, kb;
        if (d2 < 1e-10) { ka = 1.0 - d2 / 6.0; kb = 0.5 - d2 / 24.0; }
        else { const double h = sin(0.5 * d); ka = sin(d) / d; kb = 2.0 * h * h / d2; }
        const double W[9] = {0, -z, y, z, 0, -x, -y, x, 0};
PREINT_UNROLL
        for (int r = 0; r < 3; r++)
PREINT_UNROLL
            for (int c = 0; c < 3; c++)
                E[3 * r + c] = (r == c ? 1.0 : 0.0) + W[3 * r + c] * ka + (W[3 * r] * W[c] + W[3 * r + 1] * W[3 + c] + W[3 * r + 2] * W[6 + c]) * kb;
    }
    float dRb[9], Rwb2[9];
    normalize_product(dR, E, dRb);
    double dRb_d[9];
PREINT_UNROLL
    for (int k = 0; k < 9; k++) dRb_d[k] = dRb[k];
    normalize_product(job.Rwb1, dRb_d, Rwb2);
    // GetDeltaVelocity / GetDeltaPosition
    float dVb[3], dPb[3];
PREINT_UNROLL
    for (int k = 0; k < 9; k++) J[k] = S->JVg[k];
    mulv3(J, dbg, r3);
PREINT_UNROLL
    for (int k = 0; k < 9; k++) J[k] = S->JVa[k];
    mulv3(J, dba, q3);
PREINT_UNROLL
    for (int k = 0; k < 3; k++) dVb[k] = S->dV[k] + r3[k] + q3[k];
PREINT_UNROLL
    for (int k = 0; k < 9; k++) J[k] = S->JPg[k];
    mulv3(J, dbg, r3);
PREINT_UNROLL
    for (int k = 0; k < 9; k++) J[k] = S->JPa[k];
    mulv3(J, dba, q3);
PREINT_UNROLL
    for (int k = 0; k < 3; k++) dPb[k] = S->dP[k] + r3[k] + q3[k];
    const float t12 = S->dT;
    const float Gz[3] = {0.f, 0.f, -9.81f};
    mulv3(job.Rwb1, dPb, r3);
    mulv3(job.Rwb1, dVb, q3);
    ImuPredictOut o;
PREINT_UNROLL
    for (int k = 0; k < 9; k++) o.Rwb2[k] = Rwb2[k];
PREINT_UNROLL
    for (int k = 0; k < 3; k++) {
        o.twb2[k] = job.twb1[k] + job.Vwb1[k] * t12 + 0.5f * t12 * t12 * Gz[k] + r3[k];
        o.Vwb2[k] = job.Vwb1[k] + t12 * Gz[k] + q3[k];
    }
    out[j] = o;
    status[j] = ORBX_OK;
}

}  // namespace preint
