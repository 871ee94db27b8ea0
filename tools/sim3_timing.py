#!/usr/bin/env python3
"""Timing of the loop-closing geometry (needs a HIP device): sim3_ransac_batch for 1 / 16 / 64 problems at N = 100 and 300 (H = 300)
and sim3_optimize_batch for 1 / 16 / 64 problems at 100 and 300 pairs.  Per row: kernel ms (sim3_last_kernel_ms, HIP events),
call ms (host clock around the C call, which ends in a stream synchronise; median of the timed repetitions after warm-up) and
the time of a single-threaded C++ restatement of the same work that this tool compiles with g++ -O3 (the numpy reference is
no fair baseline).  Writes profiles/sim3_timing.json.  No speed threshold is attached to these numbers."""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CPU_SRC = r'''
// single-threaded restatement of Sim3Solver's hypothesis loop and of Optimizer::OptimizeSim3 (same formulas as the kernels)
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
static void jacobi4(double A[4][4], double V[4][4])
{
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) V[i][j] = i == j;
    for (int sweep = 0; sweep < 8; sweep++)
        for (int p = 0; p < 4; p++) for (int q = p + 1; q < 4; q++) {
            const double apq = A[p][q];
            if (apq == 0) continue;
            const double th = (A[q][q] - A[p][p]) / (2 * apq), t = (th >= 0 ? 1 : -1) / (std::fabs(th) + std::sqrt(th * th + 1));
            const double c = 1 / std::sqrt(t * t + 1), s = t * c;
            A[p][p] -= t * apq; A[q][q] += t * apq; A[p][q] = A[q][p] = 0;
            for (int r = 0; r < 4; r++) {
                if (r != p && r != q) { const double a = A[r][p], b = A[r][q]; A[r][p] = A[p][r] = c * a - s * b; A[r][q] = A[q][r] = s * a + c * b; }
                const double a = V[r][p], b = V[r][q]; V[r][p] = c * a - s * b; V[r][q] = s * a + c * b;
            }
        }
}
extern "C" void ransac_cpu(int n, const float* X1, const float* X2, const float* e1, const float* e2, const float* K1, const float* K2,
                           int fix, int H, const int32_t* tri, int32_t* count)
{
    std::vector<float> p1(2 * n), p2(2 * n);
    for (int i = 0; i < n; i++) {
        p1[2 * i] = K1[0] * X1[3 * i] / X1[3 * i + 2] + K1[2]; p1[2 * i + 1] = K1[1] * X1[3 * i + 1] / X1[3 * i + 2] + K1[3];
        p2[2 * i] = K2[0] * X2[3 * i] / X2[3 * i + 2] + K2[2]; p2[2 * i + 1] = K2[1] * X2[3 * i + 1] / X2[3 * i + 2] + K2[3];
    }
    for (int h = 0; h < H; h++) {
        double O1[3] = {0, 0, 0}, O2[3] = {0, 0, 0}, a[3][3], b[3][3], M[3][3], N[4][4], V[4][4];
        for (int p = 0; p < 3; p++) for (int k = 0; k < 3; k++) { O1[k] += X1[3 * tri[3 * h + p] + k] / 3.0; O2[k] += X2[3 * tri[3 * h + p] + k] / 3.0; }
        for (int p = 0; p < 3; p++) for (int k = 0; k < 3; k++) { a[p][k] = X1[3 * tri[3 * h + p] + k] - O1[k]; b[p][k] = X2[3 * tri[3 * h + p] + k] - O2[k]; }
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) M[i][j] = b[0][i] * a[0][j] + b[1][i] * a[1][j] + b[2][i] * a[2][j];
        N[0][0] = M[0][0] + M[1][1] + M[2][2]; N[0][1] = M[1][2] - M[2][1]; N[0][2] = M[2][0] - M[0][2]; N[0][3] = M[0][1] - M[1][0];
        N[1][1] = M[0][0] - M[1][1] - M[2][2]; N[1][2] = M[0][1] + M[1][0]; N[1][3] = M[2][0] + M[0][2];
        N[2][2] = -M[0][0] + M[1][1] - M[2][2]; N[2][3] = M[1][2] + M[2][1]; N[3][3] = -M[0][0] - M[1][1] + M[2][2];
        for (int i = 0; i < 4; i++) for (int j = 0; j < i; j++) N[i][j] = N[j][i];
        jacobi4(N, V);
        int m = 0;
        for (int k = 1; k < 4; k++) if (N[k][k] > N[m][m]) m = k;
        double q[4] = {V[0][m], V[1][m], V[2][m], V[3][m]};
        const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        const double w = q[0] / qn, x = q[1] / qn, y = q[2] / qn, z = q[3] / qn;
        const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                             2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
        double s = 1;
        if (!fix) {
            double nom = 0, den = 0;
            for (int p = 0; p < 3; p++) for (int i = 0; i < 3; i++) { const double p3 = R[3 * i] * b[p][0] + R[3 * i + 1] * b[p][1] + R[3 * i + 2] * b[p][2]; nom += a[p][i] * p3; den += p3 * p3; }
            s = nom / den;
        }
        float sR[9], sRi[9], t[3], ti[3];
        const float sf = (float)s, is = 1.0f / sf;
        for (int i = 0; i < 3; i++) {
            t[i] = (float)(O1[i] - s * (R[3 * i] * O2[0] + R[3 * i + 1] * O2[1] + R[3 * i + 2] * O2[2]));
            for (int j = 0; j < 3; j++) { sR[3 * i + j] = sf * (float)R[3 * i + j]; sRi[3 * i + j] = is * (float)R[3 * j + i]; }
        }
        for (int i = 0; i < 3; i++) ti[i] = -(sRi[3 * i] * t[0] + sRi[3 * i + 1] * t[1] + sRi[3 * i + 2] * t[2]);
        int c = 0;
        for (int i = 0; i < n; i++) {
            float Y[3], Z[3];
            for (int r = 0; r < 3; r++) {
                Y[r] = sR[3 * r] * X2[3 * i] + sR[3 * r + 1] * X2[3 * i + 1] + sR[3 * r + 2] * X2[3 * i + 2] + t[r];
                Z[r] = sRi[3 * r] * X1[3 * i] + sRi[3 * r + 1] * X1[3 * i + 1] + sRi[3 * r + 2] * X1[3 * i + 2] + ti[r];
            }
            const float dx1 = p1[2 * i] - (K1[0] * Y[0] / Y[2] + K1[2]), dy1 = p1[2 * i + 1] - (K1[1] * Y[1] / Y[2] + K1[3]);
            const float dx2 = (K2[0] * Z[0] / Z[2] + K2[2]) - p2[2 * i], dy2 = (K2[1] * Z[1] / Z[2] + K2[3]) - p2[2 * i + 1];
            c += (dx1 * dx1 + dy1 * dy1 < e1[i]) && (dx2 * dx2 + dy2 * dy2 < e2[i]);
        }
        count[h] = c;
    }
}

// ---- OptimizeSim3: a similarity is qx qy qz qw tx ty tz s ----
static void qrot(const double* q, const double* v, double* o)
{
    double ux = q[1] * v[2] - q[2] * v[1], uy = q[2] * v[0] - q[0] * v[2], uz = q[0] * v[1] - q[1] * v[0];
    ux += ux; uy += uy; uz += uz;
    o[0] = v[0] + q[3] * ux + (q[1] * uz - q[2] * uy); o[1] = v[1] + q[3] * uy + (q[2] * ux - q[0] * uz); o[2] = v[2] + q[3] * uz + (q[0] * uy - q[1] * ux);
}
static void qfromR(const double* R, double* q)
{
    double t = R[0] + R[4] + R[8];
    if (t > 0) { t = std::sqrt(t + 1); q[3] = 0.5 * t; t = 0.5 / t; q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t; return; }
    int i = 0; if (R[4] > R[0]) i = 1; if (R[8] > R[i * 4]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(R[i * 4] - R[j * 4] - R[k * 4] + 1); q[i] = 0.5 * t; t = 0.5 / t;
    q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t; q[j] = (R[j * 3 + i] + R[i * 3 + j]) * t; q[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
}
static void s_exp(const double* u, double* S)
{
    const double th = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), sg = u[6], s = std::exp(sg), eps = 1e-5;
    const double O[9] = {0, -u[2], u[1], u[2], 0, -u[0], -u[1], u[0], 0};
    double O2[9], R[9], A, B, Cc, sn = 0, cs = 1;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) O2[i * 3 + j] = O[i * 3] * O[j] + O[i * 3 + 1] * O[3 + j] + O[i * 3 + 2] * O[6 + j];
    const bool small = th < eps;
    if (small) for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) + O[i] + O2[i];
    else { sn = std::sin(th); cs = std::cos(th); for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) + sn / th * O[i] + (1 - cs) / (th * th) * O2[i]; }
    if (std::fabs(sg) < eps) { Cc = 1; if (small) { A = 0.5; B = 1. / 6; } else { A = (1 - cs) / (th * th); B = (th - sn) / (th * th * th); } }
    else {
        Cc = (s - 1) / sg;
        if (small) { A = ((sg - 1) * s + 1) / (sg * sg); B = ((0.5 * sg * sg - sg + 1) * s) / (sg * sg * sg); }
        else { const double a = s * sn, b = s * cs, c = th * th + sg * sg; A = (a * sg + (1 - b) * th) / (th * c); B = (Cc - ((b - 1) * sg + a * th) / c) / (th * th); }
    }
    qfromR(R, S);
    for (int i = 0; i < 3; i++) { double v = 0; for (int j = 0; j < 3; j++) v += (A * O[i * 3 + j] + B * O2[i * 3 + j] + (i == j ? Cc : 0)) * u[3 + j]; S[4 + i] = v; }
    S[7] = s;
}
static void s_mul(const double* a, const double* b, double* o)
{
    double rt[3]; qrot(a, b + 4, rt);
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]; o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2]; o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    for (int i = 0; i < 3; i++) o[4 + i] = a[7] * rt[i] + a[4 + i];
    o[7] = a[7] * b[7];
}
static void s_inv(const double* a, double* o)
{
    const double m = -1. / a[7], v[3] = {m * a[4], m * a[5], m * a[6]};
    o[0] = -a[0]; o[1] = -a[1]; o[2] = -a[2]; o[3] = a[3]; qrot(o, v, o + 4); o[7] = 1. / a[7];
}
static void e_err(const double* S, const double* K, const double* X, const double* ob, double* r)
{
    double Y[3]; qrot(S, X, Y);
    for (int i = 0; i < 3; i++) Y[i] = S[7] * Y[i] + S[4 + i];
    r[0] = ob[0] - (K[0] * Y[0] / Y[2] + K[2]); r[1] = ob[1] - (K[1] * Y[1] / Y[2] + K[3]);
}
static bool solve7(const double H[7][7], double lam, const double* b, double* x)
{
    double L[7][7] = {}, D[7]; bool ok = true;
    for (int j = 0; j < 7; j++) {
        double d = H[j][j] + lam; for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k] * D[k];
        ok = ok && d > 0 && std::isfinite(d); D[j] = d;
        for (int i = j + 1; i < 7; i++) { double v = H[i][j]; for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k] * D[k]; L[i][j] = v / d; }
    }
    for (int i = 0; i < 7; i++) { double v = b[i]; for (int k = 0; k < i; k++) v -= L[i][k] * x[k]; x[i] = v; }
    for (int i = 0; i < 7; i++) x[i] /= D[i];
    for (int i = 6; i >= 0; i--) { double v = x[i]; for (int k = i + 1; k < 7; k++) v -= L[k][i] * x[k]; x[i] = v; }
    return ok;
}
struct Pr { int n, fix; const double *X1, *X2, *o1, *o2, *w1, *w2; double K1[4], K2[4], th2, delta; };
static double rchi(const Pr& P, const double* T, const uint8_t* keep, bool robust, double* err)
{
    double Ti[8], tot = 0; s_inv(T, Ti);
    for (int e = 0; e < P.n; e++) {
        if (!keep[e]) continue;
        for (int side = 0; side < 2; side++) {
            double* r = err + 4 * e + 2 * side;
            e_err(side ? Ti : T, side ? P.K2 : P.K1, (side ? P.X1 : P.X2) + 3 * e, (side ? P.o2 : P.o1) + 2 * e, r);
            const double w = side ? P.w2[e] : P.w1[e], c = w * (r[0] * r[0] + r[1] * r[1]), d2 = P.delta * P.delta;
            tot += (robust && c > d2) ? 2 * std::sqrt(c) * P.delta - d2 : c;
        }
    }
    return tot;
}
static void lm(const Pr& P, double* T, uint8_t* keep, bool robust, int max_it, double* err, int* iters)
{
    double lam = 0, ni = 2; int nbad = 0;
    for (int it = 0; it < max_it; it++) {
        double cur = rchi(P, T, keep, robust, err), ini = cur, H[7][7] = {}, b[7] = {}, Sp[14][2][8], Ti[8];
        s_inv(T, Ti);
        for (int k = 0; k < 14; k++) { double u[7] = {}, E[8]; u[k % 7] = k < 7 ? 1e-9 : -1e-9; if (P.fix) u[6] = 0; s_exp(u, E); s_mul(E, T, Sp[k][0]); s_inv(Sp[k][0], Sp[k][1]); }
        for (int e = 0; e < P.n; e++) {
            if (!keep[e]) continue;
            for (int side = 0; side < 2; side++) {
                const double* X = (side ? P.X1 : P.X2) + 3 * e; const double* ob = (side ? P.o2 : P.o1) + 2 * e; const double* K = side ? P.K2 : P.K1;
                const double w = side ? P.w2[e] : P.w1[e]; const double* r = err + 4 * e + 2 * side;
                double J[2][7];
                for (int d = 0; d < 7; d++) { double rp[2], rm[2]; e_err(Sp[d][side], K, X, ob, rp); e_err(Sp[7 + d][side], K, X, ob, rm); J[0][d] = (rp[0] - rm[0]) / 2e-9; J[1][d] = (rp[1] - rm[1]) / 2e-9; }
                const double c = w * (r[0] * r[0] + r[1] * r[1]), rho1 = (robust && c > P.delta * P.delta) ? P.delta / std::sqrt(c) : 1.0;
                for (int a = 0; a < 7; a++) { b[a] -= rho1 * w * (J[0][a] * r[0] + J[1][a] * r[1]); for (int cc = 0; cc < 7; cc++) H[a][cc] += rho1 * w * (J[0][a] * J[0][cc] + J[1][a] * J[1][cc]); }
            }
        }
        if (it == 0) { double m = 0; for (int j = 0; j < 7; j++) m = std::fmax(m, std::fabs(H[j][j])); lam = 1e-5 * m; ni = 2; nbad = 0; }
        int qmax = 0; double rho = 0;
        do {
            double x[7], Tt[8];
            const bool ok = solve7(H, lam, b, x);
            if (ok) { double u[7], E[8]; std::memcpy(u, x, sizeof u); if (P.fix) u[6] = 0; s_exp(u, E); s_mul(E, T, Tt); } else { std::memcpy(Tt, T, sizeof Tt); std::memset(x, 0, sizeof x); }
            double temp = rchi(P, Tt, keep, robust, err);
            if (!ok) temp = 1.7976931348623157e308;
            double scale = 1e-3; for (int j = 0; j < 7; j++) scale += x[j] * (lam * x[j] + b[j]);
            rho = (cur - temp) / scale;
            if (rho > 0 && std::isfinite(temp)) { double al = 1 - std::pow(2 * rho - 1, 3); al = std::fmin(al, 2. / 3); lam *= std::fmax(1. / 3, al); ni = 2; cur = temp; std::memcpy(T, Tt, sizeof Tt); }
            else { lam *= ni; ni *= 2; }
            qmax++;
        } while (rho < 0 && qmax < 10);
        (*iters)++;
        if (qmax == 10 || rho == 0) break;
        if ((ini - cur) * 1e3 < ini) nbad++; else nbad = 0;
        if (nbad >= 3) break;
    }
}
extern "C" int optimize_cpu(int n, int fix, const double* S0, const double* X1, const double* X2, const double* o1, const double* o2, const double* w1,
                            const double* w2, const double* K1, const double* K2, double th2, double delta, double* S, int* iters)
{
    Pr P{n, fix, X1, X2, o1, o2, w1, w2, {K1[0], K1[1], K1[2], K1[3]}, {K2[0], K2[1], K2[2], K2[3]}, th2, delta};
    std::vector<uint8_t> keep(n + 1, 1); std::vector<double> err(4 * n + 4, 0.0);
    double T[8]; std::memcpy(T, S0, sizeof T); std::memcpy(S, S0, sizeof T); *iters = 0;
    if (n > 0) lm(P, T, keep.data(), true, 5, err.data(), iters);
    int nbad = 0;
    for (int e = 0; e < n; e++) { const double* r = &err[4 * e]; if (w1[e] * (r[0] * r[0] + r[1] * r[1]) > th2 || w2[e] * (r[2] * r[2] + r[3] * r[3]) > th2) { keep[e] = 0; nbad++; } }
    if (n - nbad < 10) return 0;
    lm(P, T, keep.data(), false, nbad ? 10 : 5, err.data(), iters);
    rchi(P, T, keep.data(), false, err.data());
    int nin = 0;
    for (int e = 0; e < n; e++) { const double* r = &err[4 * e]; if (keep[e] && !(w1[e] * (r[0] * r[0] + r[1] * r[1]) > th2 || w2[e] * (r[2] * r[2] + r[3] * r[3]) > th2)) nin++; }
    std::memcpy(S, T, sizeof T);
    return nin;
}
'''


def _build_cpu(tmp):
    src, lib = os.path.join(tmp, "sim3_cpu.cpp"), os.path.join(tmp, "libsim3_cpu.so")
    with open(src, "w") as f:
        f.write(CPU_SRC)
    subprocess.check_call(["g++", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", lib, src])
    return C.CDLL(lib)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_timing.json"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401  (one HIP runtime per process: torch first)
    except Exception:
        pass
    pkg = importlib.import_module("orb_slam3-1_amd")
    ss = importlib.import_module("orb_slam3-1_amd.synth_sim3")
    if pkg.device_count() < 1:
        raise SystemExit("sim3_timing needs a HIP device: there is nothing to fall back to")
    try:
        import torch
        device_name = torch.cuda.get_device_name(0)             # what the runtime reports
    except Exception:
        device_name = "unknown (torch not importable)"
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        cpu = _build_cpu(tmp)
        s = pkg.Sim3Solver()
        for n in (100, 300):
            for B in (1, 16, 64):
                probs = [ss.make_ransac_problem(1000 + k, n=n, inlier=0.5, n_hyp=300, min_inliers=15, fix_scale=k % 2) for k in range(B)]
                prep = s.ransac_prepare(probs)
                for _ in range(a.warmup):
                    s.ransac_launch(prep)
                kms = []
                call = _median_ms(lambda: (s.ransac_launch(prep), kms.append(s.last_kernel_ms())), a.reps)
                dev = s.ransac_results(prep)
                counts = [np.zeros(300, np.int32) for _ in probs]

                def run_cpu():
                    for p, c in zip(probs, counts):
                        cpu.ransac_cpu(n, _p(p["X1c"]), _p(p["X2c"]), _p(p["max_err1"]), _p(p["max_err2"]), _p(p["K1"]), _p(p["K2"]), p["fix_scale"],
                                       300, _p(p["triples"]), _p(c))
                run_cpu()
                cpu_ms = _median_ms(run_cpu, max(3, a.reps // 5))
                same = float(np.mean([np.mean(c == d["count"]) for c, d in zip(counts, dev)]))
                rows.append(dict(entry="sim3_ransac_batch", problems=B, n=n, hypotheses=300, kernel_ms=float(np.median(kms)), call_ms=call,
                                 cpu_1thread_ms=cpu_ms, cpu_counts_equal_share=same))
                print(rows[-1], flush=True)
        for n in (100, 300):
            for B in (1, 16, 64):
                probs = [ss.make_opt_problem(2000 + k, n=n, outlier_frac=0.1, fix_scale=k % 2) for k in range(B)]
                prep = s.optimize_prepare(probs)
                for _ in range(a.warmup):
                    s.optimize_launch(prep)
                kms = []
                call = _median_ms(lambda: (s.optimize_launch(prep), kms.append(s.last_kernel_ms())), a.reps)
                dev = s.optimize_results(prep)
                nin = []
                cpu.optimize_cpu.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 9 + [C.c_double, C.c_double, C.c_void_p, C.c_void_p]
                S0s = [np.array(list(p["q"]) + list(p["t"]) + [p["s"]], np.float64) for p in probs]
                S, it = np.zeros(8), C.c_int(0)

                def run_cpu():
                    nin.clear()
                    for p, S0 in zip(probs, S0s):
                        nin.append(cpu.optimize_cpu(n, p["fix_scale"], _p(S0), _p(p["X1c"]), _p(p["X2c"]), _p(p["obs1"]), _p(p["obs2"]), _p(p["inv_sigma2_1"]),
                                                    _p(p["inv_sigma2_2"]), _p(p["K1"]), _p(p["K2"]), p["th2"], p["huber_delta"], _p(S), C.byref(it)))
                run_cpu()
                cpu_ms = _median_ms(run_cpu, max(3, a.reps // 5))
                same = float(np.mean([abs(c - d["n_in"]) <= 1 for c, d in zip(nin, dev)]))
                rows.append(dict(entry="sim3_optimize_batch", problems=B, pairs=n, kernel_ms=float(np.median(kms)), call_ms=call, cpu_1thread_ms=cpu_ms,
                                 cpu_n_in_equal_share=same, lm_iterations=float(np.mean([sum(d["iterations"]) for d in dev])),
                                 lm_trials=float(np.mean([sum(d["trials"]) for d in dev]))))
                print(rows[-1], flush=True)
        s.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=device_name, reps=a.reps, warmup=a.warmup, rows=rows), f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
