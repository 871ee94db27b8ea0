// The per-link arithmetic of the IMU initialisation (imu_init_solver.hip): EdgeInertialGS::computeError and linearizeOplus
// (reference src/G2oTypes.cc:617-718) with the quadratic form of a link, and the 3 x 3 pivot inverse of the chain elimination.
// Plain C++ behind IMI_FN: the kernel compiles it for the device, tools/imuinit_cpu.cpp with g++ for the single-threaded
// CPU side of the timing tool.
#pragma once
#include "dense_lm_device.h"
#include "imu_link_device.h"

#ifdef __HIPCC__
#define IMI_FN __device__ inline
#else
#define IMI_FN inline
#endif

namespace imuinit {

using namespace liba;

constexpr int kSlot = 136;          // a link's quadratic form: packed upper 15 x 15 (120), b (15), rho0 (1)
// columns of a link's Jacobian: v1 0-2, v2 3-5, gyro bias 6-8, accelerometer bias 9-11, gravity direction 12-13, scale 14
constexpr double kGravity = (double)9.81f;      // const float IMU::GRAVITY_VALUE (include/ImuTypes.h:43)

struct Cfg { double huber_delta; uint8_t free_vel, free_bias, free_gdir, free_scale; };
struct Border { double bg[3], ba[3], Rwg[9], s; };
struct Geom { double Rwb1[9], Rwb2[9], twb1[3], twb2[3]; };     // the two fixed poses of a link

IMI_FN int up15(int a, int c) { return a * 15 - (a * (a - 1)) / 2 + (c - a); }      // a <= c
IMI_FN int sym15(int a, int c) { return a <= c ? up15(a, c) : up15(c, a); }

// EdgeInertialGS::computeError (G2oTypes.cc:617-640); also eR, Rbw1 and the float bias difference for the Jacobians
IMI_FN void gs_error(const LibaLink& L, const Geom& G, const double* v1, const double* v2, const Border& x, double* e9, double* eR,
                                double* Rbw1, double* dbg)
{
    double dR[9], dV[3], dP[3];
    link_delta(L, x.bg, x.ba, dR, dV, dP, dbg);
    const double dt = L.dT, gI[3] = {0, 0, -kGravity};
    double g[3], dRt[9], t[9], a[3], b[3];
    mvec(x.Rwg, gI, g);
    mtr(G.Rwb1, Rbw1); mtr(dR, dRt);
    mmul(dRt, Rbw1, t); mmul(t, G.Rwb2, eR);
    log_so3(eR, e9);
    for (int i = 0; i < 3; i++) a[i] = x.s * (v2[i] - v1[i]) - g[i] * dt;
    mvec(Rbw1, a, e9 + 3);
    for (int i = 0; i < 3; i++) e9[3 + i] -= dV[i];
    for (int i = 0; i < 3; i++) b[i] = x.s * (G.twb2[i] - G.twb1[i] - v1[i] * dt) - g[i] * dt * dt / 2;
    mvec(Rbw1, b, e9 + 6);
    for (int i = 0; i < 3; i++) e9[6 + i] -= dP[i];
}

IMI_FN double chi2_of(const LibaLink& L, const double* e)
{
    double c = 0;
    for (int i = 0; i < 9; i++) for (int j = 0; j < 9; j++) c += e[i] * L.info9[9 * i + j] * e[j];
    return c;
}

// robust chi2 of a link at a state
IMI_FN double gs_chi2(const Cfg& d, const LibaLink& L, const Geom& G, const double* v1, const double* v2, const Border& x)
{
    double e[9], eR[9], Rbw1[9], dbg[3], rho0, rho1;
    gs_error(L, G, v1, v2, x, e, eR, Rbw1, dbg);
    dlm::huber(L.robust != 0, chi2_of(L, e), d.huber_delta, d.huber_delta * d.huber_delta, rho0, rho1);
    return rho0;
}

// computeError + robustify + linearizeOplus (:642-718, the analytic Jacobians as written) + constructQuadraticForm of one link
// into its slot; the columns of a fixed unknown are zero
IMI_FN void gs_linearize(const Cfg& d, const LibaLink& L, const Geom& G, const double* v1, const double* v2, const Border& x, double* slot)
{
    double e[9], eR[9], Rbw1[9], dbg[3], J[9 * 15];
    gs_error(L, G, v1, v2, x, e, eR, Rbw1, dbg);
    for (int k = 0; k < 135; k++) J[k] = 0.0;
    const double dt = L.dT, s = x.s;
    if (d.free_vel)
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                J[(3 + i) * 15 + j] = -s * Rbw1[3 * i + j];            // velocity 1
                J[(6 + i) * 15 + j] = -s * Rbw1[3 * i + j] * dt;
                J[(3 + i) * 15 + 3 + j] = s * Rbw1[3 * i + j];         // velocity 2
            }
    if (d.free_bias) {
        double invJr[9], JRg[9], wv[3], rj[9], eRt[9], C[9], Dm[9];
        inv_right_jac(e, invJr);
        for (int k = 0; k < 9; k++) JRg[k] = L.JRg[k];
        mvec(JRg, dbg, wv); right_jac(wv, rj); mtr(eR, eRt);
        mmul(invJr, eRt, C); mmul(C, rj, Dm); mmul(Dm, JRg, C);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                J[i * 15 + 6 + j] = -C[3 * i + j];
                J[(3 + i) * 15 + 6 + j] = -(double)L.JVg[3 * i + j];
                J[(6 + i) * 15 + 6 + j] = -(double)L.JPg[3 * i + j];
                J[(3 + i) * 15 + 9 + j] = -(double)L.JVa[3 * i + j];
                J[(6 + i) * 15 + 9 + j] = -(double)L.JPa[3 * i + j];
            }
    }
    if (d.free_gdir) {
        // dGdTheta = Rwg Gm, Gm(0,1) = -G, Gm(1,0) = G: its columns are G Rwg[:,1] and -G Rwg[:,0]
        double c0[3], c1[3], r0[3], r1[3];
        for (int i = 0; i < 3; i++) { c0[i] = x.Rwg[3 * i + 1] * kGravity; c1[i] = x.Rwg[3 * i] * -kGravity; }
        mvec(Rbw1, c0, r0); mvec(Rbw1, c1, r1);
        for (int i = 0; i < 3; i++) {
            J[(3 + i) * 15 + 12] = -r0[i] * dt; J[(3 + i) * 15 + 13] = -r1[i] * dt;
            J[(6 + i) * 15 + 12] = -0.5 * r0[i] * dt * dt; J[(6 + i) * 15 + 13] = -0.5 * r1[i] * dt * dt;
        }
    }
    if (d.free_scale) {
        // the scale column WITHOUT the factor s of d/du (s exp(u)): G2oTypes.cc:716-717 as written
        double a[3], b[3], ra[3], rb[3];
        for (int i = 0; i < 3; i++) { a[i] = v2[i] - v1[i]; b[i] = G.twb2[i] - G.twb1[i] - v1[i] * dt; }
        mvec(Rbw1, a, ra); mvec(Rbw1, b, rb);
        for (int i = 0; i < 3; i++) { J[(3 + i) * 15 + 14] = ra[i]; J[(6 + i) * 15 + 14] = rb[i]; }
    }
    double rho0, rho1;
    dlm::huber(L.robust != 0, chi2_of(L, e), d.huber_delta, d.huber_delta * d.huber_delta, rho0, rho1);
    slot[135] = rho0;
    for (int c = 0; c < 15; c++) {
        double wj[9];
        for (int r = 0; r < 9; r++) {
            double t = 0;
            for (int q = 0; q < 9; q++) t += L.info9[9 * r + q] * J[q * 15 + c];
            wj[r] = rho1 * t;
        }
        for (int a = 0; a <= c; a++) {
            double h = 0;
            for (int r = 0; r < 9; r++) h += J[r * 15 + a] * wj[r];
            slot[up15(a, c)] = h;
        }
        double sv = 0;
        for (int r = 0; r < 9; r++) sv += wj[r] * e[r];         // J^T (rho1 Omega) e, Omega symmetric
        slot[120 + c] = -sv;
    }
}

// symmetric 3 x 3 (row major, all nine entries): inverse by cofactors; false unless positive definite
IMI_FN bool spd_inv3(const double* A, double* Ai)
{
    const double c00 = A[4] * A[8] - A[5] * A[5], c01 = A[5] * A[2] - A[1] * A[8], c02 = A[1] * A[5] - A[4] * A[2];
    const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
    const double m2 = A[0] * A[4] - A[1] * A[1];
    const bool ok = A[0] > 0.0 && m2 > 0.0 && det > 0.0 && isfinite(det);
    const double id = 1.0 / det;
    Ai[0] = c00 * id; Ai[1] = c01 * id; Ai[2] = c02 * id;
    Ai[3] = Ai[1]; Ai[4] = (A[0] * A[8] - A[2] * A[2]) * id; Ai[5] = (A[1] * A[2] - A[0] * A[5]) * id;
    Ai[6] = Ai[2]; Ai[7] = Ai[5]; Ai[8] = m2 * id;
    return ok;
}

}  // namespace imuinit
