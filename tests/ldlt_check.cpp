// dlm::ldlt_solve (orb_slam3-1_amd/csrc/dense_lm_device.h) on the CPU against Gaussian elimination in long double:
// symmetric positive-definite H = Q diag(e) Q^T with e log-spaced over [1, 1e3], lambda = 0.25, 2000 systems per variant.
// stdout per variant: "<N> <recip> <all solved> <worst component error / max|x|> <non-positive first pivot rejected>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <utility>

#include "dense_lm_device.h"

namespace {

uint64_t g_state = 20261017;
double uniform()        // splitmix64 -> (-1, 1)
{
    g_state += 0x9E3779B97F4A7C15ull;
    uint64_t z = g_state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (double)(z >> 11) / 4503599627370496.0 - 1.0;
}

template <int N, bool RECIP>
void check()
{
    const double lambda = 0.25;
    bool all_ok = true;
    double worst = 0;
    for (int trial = 0; trial < 2000; trial++) {
        long double Q[N][N];                        // Gram-Schmidt of a random matrix: rows orthonormal
        for (int i = 0; i < N; i++) {
            for (int k = 0; k < N; k++) Q[i][k] = uniform();
            for (int j = 0; j < i; j++) {
                long double d = 0;
                for (int k = 0; k < N; k++) d += Q[i][k] * Q[j][k];
                for (int k = 0; k < N; k++) Q[i][k] -= d * Q[j][k];
            }
            long double nn = 0;
            for (int k = 0; k < N; k++) nn += Q[i][k] * Q[i][k];
            for (int k = 0; k < N; k++) Q[i][k] /= std::sqrt(nn);
        }
        double Hu[N * (N + 1) / 2], b[N], x[N];
        long double A[N][N + 1];
        for (int r = 0; r < N; r++)
            for (int c = r; c < N; c++) {
                long double v = 0;
                for (int k = 0; k < N; k++) v += Q[k][r] * std::pow(1e3L, (long double)k / (N - 1)) * Q[k][c];
                const double h = (double)v;         // the system is the one of the rounded entries
                Hu[r * N - (r * (r - 1)) / 2 + (c - r)] = h;
                A[r][c] = A[c][r] = h;
            }
        for (int i = 0; i < N; i++) { A[i][i] += lambda; b[i] = 10.0 * uniform(); A[i][N] = b[i]; }
        all_ok = dlm::ldlt_solve<N, RECIP>(Hu, lambda, b, x) && all_ok;
        for (int j = 0; j < N; j++) {               // elimination with partial pivoting
            int p = j;
            for (int i = j + 1; i < N; i++) if (std::fabs(A[i][j]) > std::fabs(A[p][j])) p = i;
            for (int k = 0; k <= N; k++) std::swap(A[j][k], A[p][k]);
            for (int i = j + 1; i < N; i++) {
                const long double f = A[i][j] / A[j][j];
                for (int k = j; k <= N; k++) A[i][k] -= f * A[j][k];
            }
        }
        long double xr[N], xmax = 0, err = 0;
        for (int i = N - 1; i >= 0; i--) {
            long double v = A[i][N];
            for (int k = i + 1; k < N; k++) v -= A[i][k] * xr[k];
            xr[i] = v / A[i][i];
        }
        for (int i = 0; i < N; i++) { xmax = std::fmax(xmax, std::fabs(xr[i])); err = std::fmax(err, std::fabs((long double)x[i] - xr[i])); }
        worst = std::fmax(worst, (double)(err / xmax));
    }
    double Hu[N * (N + 1) / 2], b[N], x[N];
    for (int r = 0; r < N; r++)
        for (int c = r; c < N; c++) Hu[r * N - (r * (r - 1)) / 2 + (c - r)] = (r == c) ? 2.0 : 0.0;
    for (int i = 0; i < N; i++) b[i] = 1.0;
    Hu[0] = -1.0;                                   // first pivot -1 + lambda <= 0
    const bool rejected = !dlm::ldlt_solve<N, RECIP>(Hu, lambda, b, x);
    Hu[0] = -lambda;                                // first pivot exactly 0
    const bool rejected0 = !dlm::ldlt_solve<N, RECIP>(Hu, lambda, b, x);
    std::printf("%d %d %d %.3e %d\n", N, RECIP ? 1 : 0, all_ok ? 1 : 0, worst, (rejected && rejected0) ? 1 : 0);
}

}  // namespace

int main()
{
    check<6, true>();
    check<7, false>();
    return 0;
}
