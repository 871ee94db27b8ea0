// Single-threaded CPU side of tools/posegraph_timing.py: the per-edge work of Optimizer::OptimizeEssentialGraph (errors, numeric
// Jacobians, the edge's blocks) and the trial update, from the same plain C++ text the kernels compile (csrc/sim3_group.h).
// The pg4_* functions are the same for Optimizer::OptimizeEssentialGraph4DoF (csrc/pose4dof_group.h).
// The tool assembles the sparse system and factors it with scipy (SuperLU), which is not Eigen's SimplicialLDLT.
#include <cstdint>

#include "../orb_slam3-1_amd/csrc/pose4dof_group.h"
#include "../orb_slam3-1_amd/csrc/sim3_group.h"

extern "C" {

// rec [nE][162]; returns chi2
double pg_linearize(int nE, const double* meas, const int32_t* ev, const double* est, const uint8_t* fixed, int fix_scale, double* rec)
{
    double chi = 0;
    for (int e = 0; e < nE; e++) {
        const int vi = ev[2 * e], vj = ev[2 * e + 1];
        double err[7], J[98];
        sim3g::edge_linearize(meas + 8 * e, est + 8 * vi, est + 8 * vj, fixed[vi] != 0, fixed[vj] != 0, fix_scale != 0, err, J, rec + (long)sim3g::kRec * e);
        chi += rec[(long)sim3g::kRec * e + sim3g::kRecChi];
    }
    return chi;
}

// trial = exp(dx) * est over the free vertices (col[v] >= 0), chi2 of the trial state
double pg_update_errors(int nV, int nE, const double* meas, const int32_t* ev, const double* est, const int32_t* col, const double* x, int fix_scale, double* trial)
{
    for (int v = 0; v < nV; v++) {
        if (col[v] < 0) { for (int k = 0; k < 8; k++) trial[8 * v + k] = est[8 * v + k]; }
        else sim3g::oplus(est + 8 * v, x + 7 * col[v], fix_scale != 0, trial + 8 * v);
    }
    double chi = 0;
    for (int e = 0; e < nE; e++) {
        double err[7];
        sim3g::edge_error(meas + 8 * e, trial + 8 * ev[2 * e], trial + 8 * ev[2 * e + 1], err);
        for (int k = 0; k < 7; k++) chi += err[k] * err[k];
    }
    return chi;
}

// 4-DoF graph: est [nV][18] (p4g::kState), konst [nV][21], meas [nE][12] dRij | dtij, W [36]; rec [nE][57]; returns chi2
double pg4_linearize(int nE, const double* meas, const double* W, const int32_t* ev, const double* est, const double* konst, const uint8_t* fixed, double* rec)
{
    double chi = 0;
    for (int e = 0; e < nE; e++) {
        const int vi = ev[2 * e], vj = ev[2 * e + 1];
        p4g::edge_linearize(meas + 12 * e, W, est + p4g::kState * vi, konst + p4g::kConst * vi, est + p4g::kState * vj, konst + p4g::kConst * vj,
                            fixed[vi] != 0, fixed[vj] != 0, rec + (long)p4g::kRec * e);
        chi += rec[(long)p4g::kRec * e + p4g::kRecChi];
    }
    return chi;
}

// trial = oplusImpl(dx) over the free vertices (col[v] >= 0), chi2 of the trial state
double pg4_update_errors(int nV, int nE, const double* meas, const double* W, const int32_t* ev, const double* est, const double* konst, const int32_t* col,
                         const double* x, double* trial)
{
    for (int v = 0; v < nV; v++) {
        if (col[v] < 0) { for (int k = 0; k < p4g::kState; k++) trial[p4g::kState * v + k] = est[p4g::kState * v + k]; }
        else p4g::oplus(est + p4g::kState * v, konst + p4g::kConst * v, x + 4 * col[v], trial + p4g::kState * v);
    }
    double chi = 0;
    for (int e = 0; e < nE; e++) {
        const double* Ti = trial + p4g::kState * ev[2 * e];
        const double* Tj = trial + p4g::kState * ev[2 * e + 1];
        double err[6];
        p4g::edge_error(meas + 12 * e, Ti + p4g::kRcw, Ti + p4g::kTcw, Tj + p4g::kRcw, Tj + p4g::kTcw, err);
        chi += p4g::chi2(W, err);
    }
    return chi;
}

}
