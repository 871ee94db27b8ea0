// Shared pieces of the solvers that run a whole dense Levenberg optimisation in ONE 256-thread workgroup (k_pose_opt,
// k_sim3_optimize): the packed LDL^T solve, the ordered block sum, the Huber kernel and g2o's Levenberg policy
// (OptimizationAlgorithmLevenberg::solve, optimization_algorithm_levenberg.cpp:61-185) in the kernels' replicated-in-every-thread
// form.  lm_control.h is the same policy for the host-driven solvers; tests/test_lm_control.py replays both on the same scripts.
// The solve and the policy are plain C++ behind DLM_FN, so that g++ compiles them without HIP for the CPU tests.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define DLM_FN __device__ __forceinline__
#define DLM_UNROLL _Pragma("unroll")
#else
#include <cmath>
#define DLM_FN inline
#define DLM_UNROLL
#endif

namespace dlm {

#ifndef __HIPCC__
using std::fabs; using std::fmax; using std::fmin; using std::isfinite; using std::sqrt;
#endif

// N x N LDL^T solve (LinearSolverDense, solvers/linear_solver_dense.h:55-110) of (H + lambda I) x = b; Hu = packed upper
// triangle (row a, column c >= a at a*N - a(a-1)/2 + c - a).  Returns false for a non-positive pivot.  Everything is
// indexed at compile time (registers only).  RECIP: one reciprocal per pivot instead of a division per entry.
template <int N, bool RECIP>
DLM_FN bool ldlt_solve(const double* Hu, double lambda, const double* b, double* x)
{
    double A[N * N], D[N], P[N];        // P: what the entries are scaled by, 1 / D (RECIP) or D itself
    DLM_UNROLL
    for (int r = 0; r < N; r++)
        DLM_UNROLL
        for (int c = r; c < N; c++) { const double v = Hu[r * N - (r * (r - 1)) / 2 + (c - r)]; A[r * N + c] = v; A[c * N + r] = v; }
    DLM_UNROLL
    for (int i = 0; i < N; i++) A[i * (N + 1)] += lambda;
    bool ok = true;
    DLM_UNROLL
    for (int j = 0; j < N; j++) {
        double d = A[j * N + j];
        DLM_UNROLL
        for (int k = 0; k < j; k++) d -= A[j * N + k] * A[j * N + k] * D[k];
        ok = ok && (d > 0.0) && isfinite(d);
        D[j] = d;
        P[j] = RECIP ? 1.0 / d : d;
        DLM_UNROLL
        for (int i = j + 1; i < N; i++) {
            double sv = A[i * N + j];
            DLM_UNROLL
            for (int k = 0; k < j; k++) sv -= A[i * N + k] * A[j * N + k] * D[k];
            A[i * N + j] = RECIP ? sv * P[j] : sv / P[j];
        }
    }
    DLM_UNROLL
    for (int i = 0; i < N; i++) {
        double sv = b[i];
        DLM_UNROLL
        for (int k = 0; k < i; k++) sv -= A[i * N + k] * x[k];
        x[i] = sv;
    }
    DLM_UNROLL
    for (int i = 0; i < N; i++) x[i] = RECIP ? x[i] * P[i] : x[i] / P[i];
    DLM_UNROLL
    for (int i = N - 1; i >= 0; i--) {
        double sv = x[i];
        DLM_UNROLL
        for (int k = i + 1; k < N; k++) sv -= A[k * N + i] * x[k];
        x[i] = sv;
    }
    return ok;
}

// RobustKernelHuber::robustify (robust_kernel_impl.cpp): rho0 and rho1 of a squared error; dsq = delta * delta
DLM_FN void huber(bool on, double chi, double delta, double dsq, double& rho0, double& rho1)
{
    rho0 = chi; rho1 = 1.0;
    if (on && !(chi <= dsq)) { const double sq = sqrt(chi); rho0 = 2 * sq * delta - dsq; rho1 = delta / sq; }
}

// computeLambdaInit (levenberg.cpp:171-185): tau * max(diag H) with tau = 1e-5
template <int N>
DLM_FN double lambda_init(const double* Hu)
{
    double m = 0;
    DLM_UNROLL
    for (int j = 0; j < N; j++) m = fmax(fabs(Hu[j * N - (j * (j - 1)) / 2]), m);
    return 1e-5 * m;
}

// One trial of the loop levenberg.cpp:102-149, arguments as lm::Levenberg::trial: chi_new is the trial's chi2, scale is
// dx^T (lambda dx + b), solved says whether the system was.  Updates lambda, ni, cur (the accepted chi2) and rho; returns true
// when the trial state is accepted (discardTop: the caller takes the trial estimate over), false when the estimate stays (pop).
DLM_FN bool trial(bool solved, double chi_new, double scale, double& lambda, double& ni, double& cur, double& rho)
{
    const double tempChi = solved ? chi_new : 1.7976931348623157e308;
    rho = (cur - tempChi) / (scale + 1e-3);
    const bool accepted = rho > 0 && isfinite(tempChi);
    if (accepted) {
        const double c1 = 2 * rho - 1;
        double alpha = 1. - c1 * c1 * c1;      // pow(2 rho - 1, 3) (levenberg.cpp:129), <= 2 ulp apart
        alpha = fmin(alpha, 2. / 3.);
        lambda *= fmax(1. / 3., alpha);
        ni = 2;
        cur = tempChi;
    } else {
        lambda *= ni; ni *= 2;
    }
    return accepted;
}

// another trial in this iteration?  (the while of levenberg.cpp:149)
DLM_FN bool more_trials(double rho, int qmax) { return rho < 0 && qmax < 10; }

// Stop rules at the end of an iteration (levenberg.cpp:151-166) that ran qmax trials from chi2 ini to cur: 0 continue,
// 1 ten trials or rho == 0, 2 three iterations in a row (counted in nbad) below 1e-3 relative gain.
DLM_FN int stop_reason(int qmax, double rho, double ini, double cur, int& nbad)
{
    if (qmax == 10 || rho == 0) return 1;
    if ((ini - cur) * 1e3 < ini) nbad++; else nbad = 0;
    return nbad >= 3 ? 2 : 0;
}

#ifdef __HIPCC__
// ordered block sum of K values per thread (256 threads): wave butterfly, then the four wave partials in a fixed order;
// the result is replicated in every thread
template <int K>
__device__ __forceinline__ void block_sum(double* v, double (*s_part)[4])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; k++) {
        double a = v[k];
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        v[k] = a;
    }
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; k++) s_part[k][wave] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = ((s_part[k][0] + s_part[k][1]) + s_part[k][2]) + s_part[k][3];
}

__device__ __forceinline__ double block_sum(double v, double (&s_part)[4])
{
    block_sum<1>(&v, &s_part);
    return v;
}
#endif

}  // namespace dlm
