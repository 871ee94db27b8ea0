// dense_chol.h -- the dense Cholesky of the host-driven Levenberg solvers (LocalBA, LocalInertialBA, the essential-graph pose
// graph): factorisation and substitution kernels of an (n + 1) x n row-major system whose row n is the right-hand side, and the
// host calls that enqueue them.  The kernels have external linkage: ONE translation unit includes this header (lba_solver.hip
// with its two .inc files), so that there is one copy of k_chol_* and of the LBA_STEP_TIMING counters.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hip_check.h"

namespace chol {

constexpr int NB = 60;      // Cholesky block size (10 poses)

// ---- blocked right-looking Cholesky of the (dense, small) reduced camera system, lower triangle ----
// Per 60-column step: k_chol_diag factors the diagonal block AND inverts it (Gauss-Jordan on [L | I]) in LDS with
// O(1)-depth steps; k_chol_panel then gets the rows below as a dense product X = A * Linv^T (no substitution chains);
// k_chol_update applies the trailing update.  The substitutions in k_chol_solve also only need Linv.
// Factor AND invert one diagonal block held in registers.  Thread (ty, tx) of a 16 x 16 grid owns the elements
// (ty + 16a, tx + 16b), a, b < 4, of the 64 x 64-padded block L (identity beyond nb) and of X = L^-1.
// (History: one column per barrier 33.7 us per 60-column block, two columns 27.5 us, four columns 19.1 us.)
// FOUR columns per barrier.  The owners publish the raw columns j0..j0+3 of L and rows j0..j0+3 of X; every thread factors the
// 4 x 4 pivot block P = Lp Lp^T itself and forms M = Lp^-1 (replicated: no broadcast), then
//   U = A[:, j0..j0+3] M^T  (its rows / its columns),   Xn = M X[j0..j0+3][:],
//   rows below the pivot block:  L -= U U^T,  X -= U Xn;   rows of the pivot block: X <- Xn.
// L itself is not an output (only X = L^-1 is), so finished columns are never written back, and garbage above the diagonal of
// the diagonal 16 x 16 tiles is never read (columns are consumed from their diagonal element downwards).
typedef double mfma_d4 __attribute__((ext_vector_type(4)));
struct CholVec4 { double col[2][4][64], row[2][4][64]; };
__device__ __forceinline__ double rsqrt_newton(double d)
{
    double inv = __builtin_amdgcn_rsq(d);
    inv = inv * fma(-0.5 * d * inv, inv, 1.5);
    return inv * fma(-0.5 * d * inv, inv, 1.5);
}
// The rank-4 updates of the step run on the f64 matrix pipe.  A 256-thread workgroup is one wave per SIMD,
// where a v_fma_f64 issues every ~8.5 clocks and v_mfma_f64_16x16x4 (2048 FLOP) every 64 (tools/probes/f64_rates.hip): the
// 128 FMAs per thread of the register-tile update become at most 5 MFMAs, and a lane only prepares the operands the MFMA takes
// from it (one value of U, one of V or Xn per column block: 4 FMAs each on M's row k = lane >> 4) instead of the 48 values
// its 4 x 4 tile would need.  Thread (ty, tx) = lane (ty & 3) * 16 + tx of wave ty >> 2 owns rows ty + 16 a: exactly the rows
// of accumulator component a when the wave feeds the MFMA rows m -> 4 w + (m & 3) + 16 (m >> 2) (as k_chol_step does), so
// Lacc[b][a] / Xacc[b][a] ARE the thread's elements (ty + 16 a, tx + 16 b).
#ifdef LBA_STEP_TIMING       // cycle split of the 4-column groups of chol_tile_mfma (thread 0 of the factoring workgroup)
__device__ unsigned long long d_tile_prof[8];
#define LBA_TTICK(k) if (threadIdx.x == 0) { const long long t_now = clock64(); d_tile_prof[k] += (unsigned long long)(t_now - t_tile); t_tile = t_now; }
#else
#define LBA_TTICK(k)
#endif
__device__ __forceinline__ bool chol_tile_mfma(double (&Lr)[4][4], int nb, double* __restrict__ Li, CholVec4& sv)
{
#ifdef LBA_STEP_TIMING
    long long t_tile = clock64();
#endif
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int lk = ty & 3, wv4 = ty & ~3;                   // MFMA k index of this lane; first row of the wave's row group
    const int r_u = wv4 + (tx & 3) + 16 * (tx >> 2);        // the row whose U value this lane feeds (MFMA row m = tx)
    mfma_d4 Lacc[4], Xacc[4];
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
        for (int a = 0; a < 4; a++) { Lacc[b][a] = Lr[a][b]; Xacc[b][a] = (ty + 16 * a == tx + 16 * b) ? 1.0 : 0.0; }
    bool failed = false;
#pragma unroll
    for (int ja = 0; ja < 4; ja++) {
        for (int jy = 0; jy < 16; jy += 4) {
            const int j0 = 16 * ja + jy;
            if (j0 >= nb || failed) break;                  // a partial last group pairs with the identity padding
            const int p = (jy >> 2) & 1;
            const int ko = tx - jy;                         // 0..3: this thread owns a pivot column
            const bool own_rows = wv4 == jy;                // wave-uniform: this wave owns the pivot rows j0 + (ty & 3)
            LBA_TTICK(0)
            if (ko >= 0 && ko < 4) {
#pragma unroll
                for (int a = 0; a < 4; a++) sv.col[p][ko][ty + 16 * a] = Lacc[ja][a];
            }
            if (own_rows) {
#pragma unroll
                for (int b = 0; b < 4; b++) sv.row[p][lk][tx + 16 * b] = Xacc[b][ja];
            }
            LBA_TTICK(1)
            __syncthreads();
            LBA_TTICK(2)
            // the operand reads go out first: they land while the pivot chain below runs
            // A operand: -U[r_u][lk], zero for the rows of the pivot block and above (they take no update)
            const double c0u = sv.col[p][0][r_u], c1u = sv.col[p][1][r_u], c2u = sv.col[p][2][r_u], c3u = sv.col[p][3][r_u];
            double cv[4][4], rv[4][4];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int c = tx + 16 * b;
                if (b >= ja) {
#pragma unroll
                    for (int k = 0; k < 4; k++) cv[b][k] = sv.col[p][k][c];
                }
                if (b <= ja) {
#pragma unroll
                    for (int k = 0; k < 4; k++) rv[b][k] = sv.row[p][k][c];
                }
            }
            // pivot block (lower triangle): P[k][m] = column m, row j0 + k
            const double P00 = sv.col[p][0][j0], P10 = sv.col[p][0][j0 + 1], P20 = sv.col[p][0][j0 + 2], P30 = sv.col[p][0][j0 + 3];
            const double P11 = sv.col[p][1][j0 + 1], P21 = sv.col[p][1][j0 + 2], P31 = sv.col[p][1][j0 + 3];
            const double P22 = sv.col[p][2][j0 + 2], P32 = sv.col[p][2][j0 + 3], P33 = sv.col[p][3][j0 + 3];
            bool ok = (P00 > 0.0) && isfinite(P00);                                 // (checked once per group: one uniform branch, not four)
            const double i0 = rsqrt_newton(P00);
            const double l10 = P10 * i0, l20 = P20 * i0, l30 = P30 * i0;
            const double d1 = fma(-l10, l10, P11);
            ok = ok && (d1 > 0.0) && isfinite(d1);
            const double i1 = rsqrt_newton(d1);
            const double l21 = fma(-l20, l10, P21) * i1, l31 = fma(-l30, l10, P31) * i1;
            const double d2 = fma(-l21, l21, fma(-l20, l20, P22));
            ok = ok && (d2 > 0.0) && isfinite(d2);
            const double i2 = rsqrt_newton(d2);
            const double l32 = fma(-l31, l21, fma(-l30, l20, P32)) * i2;
            const double d3 = fma(-l32, l32, fma(-l31, l31, fma(-l30, l30, P33)));
            ok = ok && (d3 > 0.0) && isfinite(d3);
            const double i3 = rsqrt_newton(d3);
            if (!ok) { failed = true; break; }          // uniform: same values in every thread
            // M = Lp^-1 (lower triangular); this lane needs row lk of it
            const double M10 = -(l10 * i0) * i1;
            const double M20 = -fma(l21, M10, l20 * i0) * i2, M21 = -(l21 * i1) * i2;
            const double M30 = -fma(l32, M20, fma(l31, M10, l30 * i0)) * i3, M31 = -fma(l32, M21, l31 * i1) * i3, M32 = -(l32 * i2) * i3;
            const double m0 = lk == 0 ? i0 : lk == 1 ? M10 : lk == 2 ? M20 : M30;
            const double m1 = lk == 0 ? 0.0 : lk == 1 ? i1 : lk == 2 ? M21 : M31;
            const double m2 = lk < 2 ? 0.0 : lk == 2 ? i2 : M32;
            const double m3 = lk < 3 ? 0.0 : i3;
#ifdef LBA_STEP_TIMING
            if (threadIdx.x == 0 && m3 == 12345.678) d_tile_prof[7] += 1;      // (keeps the pivot chain ahead of the tick)
#endif
            LBA_TTICK(3)
            // independent FMA trees the scheduler can interleave, the MFMAs back to back after them
            double au = fma(m1, c1u, m0 * c0u) + fma(m3, c3u, m2 * c2u);
            au = (r_u > j0 + 3) ? -au : 0.0;
            double vb[4], xb[4];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int c = tx + 16 * b;
                if (b >= ja) {      // columns right of the pivot group belong to L:  L -= U V^T
                    vb[b] = fma(m1, cv[b][1], m0 * cv[b][0]) + fma(m3, cv[b][3], m2 * cv[b][2]);
                    if (b == ja && c <= j0 + 3) vb[b] = 0.0;
                }
                if (b <= ja)        // the others to X:  X -= U Xn, and the pivot rows of X become Xn
                    xb[b] = fma(m1, rv[b][1], m0 * rv[b][0]) + fma(m3, rv[b][3], m2 * rv[b][2]);
            }
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int c = tx + 16 * b;
                if (b >= ja) Lacc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(au, vb[b], Lacc[b], 0, 0, 0);
                if (b <= ja) {
                    const double xop = (b == ja && c > j0 + 3) ? 0.0 : xb[b];
                    Xacc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(au, xop, Xacc[b], 0, 0, 0);
                    if (own_rows) Xacc[b][ja] = xb[b];      // X[j0 + lk][c] = Xn[lk][c]
                }
            }
        }
    }
    LBA_TTICK(0)
    if (failed) return false;
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int r = ty + 16 * a, c = tx + 16 * b;
            if (r < nb && c < nb) Li[r * NB + c] = (c <= r) ? Xacc[b][a] : 0.0;
        }
    return true;
}

// (Measured, round 2, per 60-column block: register-tile VALU updates with 16 x 16 threads 19.4 us; the same with 32 x 32 threads
// and 2 x 2 tiles 26.1 us; this MFMA form 18.7 us.  The step is bound by its dependent chain -- barrier, pivot loads, four pivots
// of rsqrt + two Newton steps at ~15 clocks per dependent v_fma_f64 (tools/probes/f64_rates.hip) -- not by f64 issue.
// EIGHT columns per barrier (8 x 8 pivot block and its inverse replicated in every thread, two MFMA k-steps per update) was built
// and is bit-compatible, but slower: 29 us per block against 22 -- the replicated pivot algebra grows with the cube of the group
// width and outweighs the publish / barrier / operand rounds it saves.  Per 4-column group (tools/lba_step_timing.py): operands +
// MFMA 1400-1700 cycles, pivot block + M 1000-1300, publish 475, barrier 290.)
__device__ __forceinline__ void chol_diag_body(const double* __restrict__ S, int n, int k0, int nb,
                                                   double* __restrict__ Linv, double* __restrict__ scal, const int bx)
{
    __shared__ CholVec4 sv;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    double Lr[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int r = ty + 16 * a, c = tx + 16 * b;
            Lr[a][b] = (r < nb && c < nb) ? S[(size_t)(k0 + r) * n + k0 + c] : ((r == c) ? 1.0 : 0.0);
        }
    if (!chol_tile_mfma(Lr, nb, Linv + (size_t)(k0 / NB) * NB * NB, sv) && tid == 0) scal[5] = 1.0;
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_chol_diag(const double* __restrict__ S, int n, int k0, int nb,
                                                   double* __restrict__ Linv, double* __restrict__ scal)
{
    chol_diag_body(S, n, k0, nb, Linv, scal, (int)blockIdx.x);
}

// One launch per block column K (instead of panel + update + the next diagonal factorisation): the workgroup of trailing
// tile (bi, bj), K < bj <= bi, recomputes the two panel blocks it needs, X_i = A_iK Linv_K^T and X_j (a 60^3 product each --
// cheaper than a launch), applies T_ij -= X_i X_j^T to its register tile, and the workgroup of tile (K+1, K+1) goes straight
// on to factor and invert it, while the other tiles are still being updated.  The tiles of block column K+1 also store their
// X_i (= L_iK) into a second (n+1) x n buffer Lp, which the substitution kernel then reads.  The right-hand side (row n of the (n+1) x n buffer) rides along as a 61st row of the last block row.
#ifdef LBA_STEP_TIMING       // phase times (wall clock ticks, 100 MHz) of the factoring workgroup of k_chol_step, summed (tools/lba_step_timing.py)
__device__ unsigned long long d_step_prof[8];
#define LBA_STICK(k) if (bi == K + 1 && bj == K + 1 && threadIdx.x == 0) { const unsigned long long t_now = wall_clock64(); d_step_prof[k] += t_now - t_prev; t_prev = t_now; }
#else
#define LBA_STICK(k)
#endif
constexpr int kFusedMaxBlocks = 8;       // up to 480 reduced unknowns (80 key frames); larger systems keep panel / update launches
static_assert(NB + 16 * 28 >= kFusedMaxBlocks * NB, "k_chol_solve<true> prefetches at most 28 rows per row group");
constexpr int kStepLds = (NB * (NB + 1) + 2 * 64 * (NB + 1)) * 8 + (int)sizeof(CholVec4);
// workgroups of one flow-factorisation launch (k_chol_flow_b, ki_chol_flow) that are resident at once: kStepLds (100 KB of LDS)
// allows one per CU, and every workgroup of such a launch may wait on others, so all of them must be resident
constexpr int kMaxFlowGroups = 240;
__device__ __forceinline__ void chol_step_body(double* __restrict__ S, double* __restrict__ Lp, int n, int K, int nblk,
                                                   double* __restrict__ Linv, double* __restrict__ scal, const int bx, double* __restrict__ sm_step)
{
    constexpr int P = NB + 1;
    double* sI = sm_step;
    double* sXi = sI + NB * P;
    double* sXj = sXi + 64 * P;
    CholVec4& sv = *(CholVec4*)(sXj + 64 * P);
    if (scal[5] != 0.0) return;         // an earlier diagonal block was not positive definite
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    int li = 0, t = bx;
    while (t > li) { t -= li + 1; li++; }
    const int bi = K + 1 + li, bj = K + 1 + t;
    const bool diag_tile = bi == bj;
    const int k0 = K * NB;                                              // block K is a full one (it is not the last)
    const int r0 = bi * NB, nri = min(NB, n - r0) + (bi == nblk - 1 ? 1 : 0);       // + the right-hand-side row
    const int c0 = bj * NB, ncj = min(NB, n - c0);
    const double* Lk = Linv + (size_t)K * NB * NB;
#ifdef LBA_STEP_TIMING
    unsigned long long t_prev = wall_clock64();
#endif
    {
        // staging: all loads of a thread are issued before the first LDS store (16-byte loads; n = 6 * poses is even and
        // every row segment starts at an even column, so the double2 accesses are aligned)
        constexpr int H = NB / 2, kIt = (64 * H + 255) / 256;          // 30 double2 per row, 8 rounds
        double2 vI[kIt], vA[kIt], vB[kIt];
#pragma unroll
        for (int it = 0; it < kIt; it++) {
            const int i = tid + 256 * it, r = i / H, q2 = i - r * H;
            vI[it] = make_double2(0.0, 0.0); vA[it] = vI[it]; vB[it] = vI[it];
            if (r < NB) vI[it] = *(const double2*)(Lk + r * NB + 2 * q2);
            if (r < nri) vA[it] = *(const double2*)(S + (size_t)(r0 + r) * n + k0 + 2 * q2);
            if (!diag_tile && r < ncj) vB[it] = *(const double2*)(S + (size_t)(c0 + r) * n + k0 + 2 * q2);
        }
#pragma unroll
        for (int it = 0; it < kIt; it++) {
            const int i = tid + 256 * it, r = i / H, q2 = i - r * H;
            if (r < NB) { sI[r * P + 2 * q2] = vI[it].x; sI[r * P + 2 * q2 + 1] = vI[it].y; }
            if (r < 64) {
                sXi[r * P + 2 * q2] = vA[it].x; sXi[r * P + 2 * q2 + 1] = vA[it].y;
                sXj[r * P + 2 * q2] = vB[it].x; sXj[r * P + 2 * q2 + 1] = vB[it].y;
            }
        }
    }
    __syncthreads();
    LBA_STICK(0)
    // X = A Linv^T, X[r][c] = sum_{q <= c} A[r][q] Linv[c][q], on the f64 matrix pipe (v_mfma_f64_16x16x4: lane l feeds
    // A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15], 1/8 of the LDS bytes of a register-blocked VALU product).  Wave w owns
    // rows 16w .. 16w+15 (it reads and overwrites only those, so the product is done in place); column block C needs the
    // k-steps up to its last column only (Linv is lower triangular).
    {
        const int wv = tid >> 6, ln = tid & 63, lr = ln & 15, lk = ln >> 4;
        mfma_d4 xa[4], xb[4];
#pragma unroll
        for (int C = 0; C < 4; C++) { xa[C] = mfma_d4{0.0, 0.0, 0.0, 0.0}; xb[C] = xa[C]; }
        const double* pa = sXi + (16 * wv + lr) * P + lk;
        const double* pb = sXj + (16 * wv + lr) * P + lk;
#pragma unroll
        for (int ks = 0; ks < NB / 4; ks++) {
            const double av = pa[4 * ks];
            const double bv = diag_tile ? 0.0 : pb[4 * ks];
#pragma unroll
            for (int C = 0; C < 4; C++) {
                if (ks >= 4 * C + 4) continue;              // compile-time: above the diagonal of Linv
                const int c = 16 * C + lr;
                const double lv = (c < NB) ? sI[c * P + 4 * ks + lk] : 0.0;
                xa[C] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, lv, xa[C], 0, 0, 0);
                if (!diag_tile) xb[C] = __builtin_amdgcn_mfma_f64_16x16x4f64(bv, lv, xb[C], 0, 0, 0);
            }
        }
        // results: lane l, component i = row (l >> 4) + 4 i, column l & 15 of the 16 x 16 block
#pragma unroll
        for (int C = 0; C < 4; C++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int c = 16 * C + lr;
                if (c < NB) {
                    sXi[(16 * wv + lk + 4 * i) * P + c] = xa[C][i];
                    if (!diag_tile) sXj[(16 * wv + lk + 4 * i) * P + c] = xb[C][i];
                }
            }
    }
    __syncthreads();
    LBA_STICK(1)
    if (bj == K + 1) {      // this tile's X_i is L_iK: keep it -- in Lp, because the other tiles of this block row still read A_iK from S
        for (int i = tid; i < nri * NB; i += 256) { const int r = i / NB, q = i - r * NB; Lp[(size_t)(r0 + r) * n + k0 + q] = sXi[r * P + q]; }
    }
    LBA_STICK(2)
    const double* sB = diag_tile ? sXi : sXj;
    double Lr[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int r = ty + 16 * a, c = tx + 16 * b;
            Lr[a][b] = (r < nri && c < ncj) ? S[(size_t)(r0 + r) * n + c0 + c] : 0.0;
        }
    LBA_STICK(3)
    {
        // T -= X_i X_j^T on the matrix pipe.  Wave w feeds the 16 rows its threads own (local row m = global row
        // 4w + (m & 3) + 16 (m >> 2)), so component i of column block C of the result IS this thread's element (ty + 16 i, tx + 16 C).
        const int wv = tid >> 6, ln = tid & 63, lr = ln & 15, lk = ln >> 4;
        const double* pa = sXi + (4 * wv + (lr & 3) + 16 * (lr >> 2)) * P + lk;
        const double* pb = sB + lr * P + lk;
        mfma_d4 acc[4];
#pragma unroll
        for (int C = 0; C < 4; C++) acc[C] = mfma_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int ks = 0; ks < NB / 4; ks++) {
            const double av = pa[4 * ks];
#pragma unroll
            for (int C = 0; C < 4; C++) acc[C] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, pb[16 * C * P + 4 * ks], acc[C], 0, 0, 0);
        }
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) Lr[a][b] -= acc[b][a];
    }
    LBA_STICK(4)
    const bool factor_here = diag_tile && bi == K + 1;
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int r = ty + 16 * a, c = tx + 16 * b;
            const bool live = r < nri && c < ncj && (!diag_tile || c <= r);
            // the tile that is factored next stays in registers, except a right-hand-side row riding along with it
            if (live && (!factor_here || r >= ncj)) S[(size_t)(r0 + r) * n + c0 + c] = Lr[a][b];
            if (factor_here && (r >= ncj || c >= ncj)) Lr[a][b] = (r == c) ? 1.0 : 0.0;
        }
    LBA_STICK(5)
    if (factor_here) {
        if (!chol_tile_mfma(Lr, ncj, Linv + (size_t)bi * NB * NB, sv) && tid == 0) scal[5] = 1.0;
    }
    LBA_STICK(6)
#ifdef LBA_STEP_TIMING
    if (bi == K + 1 && bj == K + 1 && threadIdx.x == 0) d_step_prof[7] += 1;
#endif
}

// ---- the whole factorisation in ONE launch (round 3): a workgroup per lower-triangle tile (r, c) of the block matrix ----
// k_chol_diag + k_chol_step x (nblk - 1) is a chain of launches whose critical path is the factoring workgroup of every block
// column; between two of them lie a launch boundary, a tile write-back and a tile load.  Here tile (r, c) is ONE workgroup
// for its whole life: it loads its tile into registers once, and for K = 0 .. c-1 waits until block column K is factored
// (flag fac[K]) and the tiles (r, K), (c, K) are final (flags done[.][K]), recomputes the two panel blocks X_r = A_rK Linv_K^T,
// X_c (as k_chol_step does), applies T -= X_r X_c^T in registers, and at the end either factors and inverts its tile (r == c,
// publishes fac[c]) or writes it back (publishes done[r][c]).  The panel inputs of a step are final long before the pivot block
// they wait for, so everything except [load Linv_K, panel product, update] is off the critical path.
// Synchronisation between workgroups (other CUs, other XCDs): producer stores, workgroup barrier, thread 0: agent-scope
// release fence + flag store; consumer thread 0: agent-scope spin on the flag, acquire fence, workgroup barrier, plain loads
// (MI355X_MICROARCH.md, correctness boundaries).  Flags carry the EPOCH of the trial (no reset between trials).  A workgroup
// only waits for workgroups of smaller linear index (column-major tile order), so the grid cannot deadlock as long as every XCD
// starts its workgroups in index order; the launch sites keep the grid within what is resident at once anyway.  Every spin is
// bounded and also watches the failure flag (a pivot block that is not positive definite ends the factorisation for everybody).
constexpr int kFlowFlags = kFusedMaxBlocks + kFusedMaxBlocks * kFusedMaxBlocks;
__device__ __forceinline__ bool flow_wait(const unsigned* flag, unsigned epoch, double* scal)
{
    __shared__ int s_ok;
    if (threadIdx.x == 0) {
        int ok = 0;
        for (int spin = 0; spin < (1 << 21); spin++) {
            if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch) { ok = 1; break; }
            if (__longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)(scal + 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0.0) break;
            __builtin_amdgcn_s_sleep(2);
        }
        if (!ok && __longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)(scal + 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0.0)
            __hip_atomic_store((unsigned long long*)(scal + 5), (unsigned long long)__double_as_longlong(2.0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // timed out
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        s_ok = ok;
    }
    __syncthreads();
    const bool r = s_ok != 0;
    __syncthreads();
    return r;
}
__device__ __forceinline__ void flow_publish(unsigned* flag, unsigned epoch)
{
    __syncthreads();                // every thread's stores of the tile / the inverted block are issued and counted
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
__device__ __forceinline__ void chol_flow_body(double* __restrict__ S, double* __restrict__ Lp, int n, int nblk, double* __restrict__ Linv,
                                               double* __restrict__ scal, unsigned* __restrict__ flow, unsigned epoch, const int bx, double* __restrict__ sm_step)
{
    constexpr int P = NB + 1;
    double* sI = sm_step;
    double* sXi = sI + NB * P;
    double* sXj = sXi + 64 * P;
    CholVec4& sv = *(CholVec4*)(sXj + 64 * P);
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    // column-major tile order: (0,0) (1,0) .. (nblk-1,0) (1,1) (2,1) ..
    int c = 0, t = bx;
    while (t >= nblk - c) { t -= nblk - c; c++; }
    const int r = c + t;
    unsigned* fac = flow;
    unsigned* done = flow + kFusedMaxBlocks;
    const bool diag_tile = r == c;
    const int r0 = r * NB, nri = min(NB, n - r0) + (r == nblk - 1 ? 1 : 0);         // + the right-hand-side row
    const int c0 = c * NB, ncj = min(NB, n - c0);
    if (!diag_tile && c == 0) return;        // the tiles of block column 0 are final as they are: nothing to do, nothing to publish
    // the tile, in registers for the workgroup's whole life
    double Lr[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int rr = ty + 16 * a, cc = tx + 16 * b;
            Lr[a][b] = (rr < nri && cc < ncj) ? S[(size_t)(r0 + rr) * n + c0 + cc] : 0.0;
        }
    for (int K = 0; K < c; K++) {
        const int k0 = K * NB;
        // the panel inputs A_rK, A_cK: final once the workgroups (r, K), (c, K) are done (block column 0: from the start)
        if (K > 0) {
            if (!flow_wait(done + r * kFusedMaxBlocks + K, epoch, scal)) return;
            if (!diag_tile && !flow_wait(done + c * kFusedMaxBlocks + K, epoch, scal)) return;
        }
        {
            constexpr int H = NB / 2, kIt = (64 * H + 255) / 256;
            double2 vA[kIt], vB[kIt];
#pragma unroll
            for (int it = 0; it < kIt; it++) {
                const int i = tid + 256 * it, rr = i / H, q2 = i - rr * H;
                vA[it] = make_double2(0.0, 0.0); vB[it] = vA[it];
                if (rr < nri) vA[it] = *(const double2*)(S + (size_t)(r0 + rr) * n + k0 + 2 * q2);
                if (!diag_tile && rr < ncj) vB[it] = *(const double2*)(S + (size_t)(c0 + rr) * n + k0 + 2 * q2);
            }
#pragma unroll
            for (int it = 0; it < kIt; it++) {
                const int i = tid + 256 * it, rr = i / H, q2 = i - rr * H;
                if (rr < 64) {
                    sXi[rr * P + 2 * q2] = vA[it].x; sXi[rr * P + 2 * q2 + 1] = vA[it].y;
                    sXj[rr * P + 2 * q2] = vB[it].x; sXj[rr * P + 2 * q2 + 1] = vB[it].y;
                }
            }
        }
        // the inverted pivot block of column K: the critical wait
        if (!flow_wait(fac + K, epoch, scal)) return;
        {
            constexpr int H = NB / 2, kIt = (NB * H + 255) / 256;
            const double* Lk = Linv + (size_t)K * NB * NB;
            double2 vI[kIt];
#pragma unroll
            for (int it = 0; it < kIt; it++) {
                const int i = tid + 256 * it, rr = i / H, q2 = i - rr * H;
                vI[it] = make_double2(0.0, 0.0);
                if (rr < NB) vI[it] = *(const double2*)(Lk + rr * NB + 2 * q2);
            }
#pragma unroll
            for (int it = 0; it < kIt; it++) {
                const int i = tid + 256 * it, rr = i / H, q2 = i - rr * H;
                if (rr < NB) { sI[rr * P + 2 * q2] = vI[it].x; sI[rr * P + 2 * q2 + 1] = vI[it].y; }
            }
        }
        __syncthreads();
        // X = A Linv^T on the f64 matrix pipe, in place (as k_chol_step)
        {
            const int wv = tid >> 6, ln = tid & 63, lr = ln & 15, lk = ln >> 4;
            mfma_d4 xa[4], xb[4];
#pragma unroll
            for (int C = 0; C < 4; C++) { xa[C] = mfma_d4{0.0, 0.0, 0.0, 0.0}; xb[C] = xa[C]; }
            const double* pa = sXi + (16 * wv + lr) * P + lk;
            const double* pb = sXj + (16 * wv + lr) * P + lk;
#pragma unroll
            for (int ks = 0; ks < NB / 4; ks++) {
                const double av = pa[4 * ks];
                const double bv = diag_tile ? 0.0 : pb[4 * ks];
#pragma unroll
                for (int C = 0; C < 4; C++) {
                    if (ks >= 4 * C + 4) continue;
                    const int cc = 16 * C + lr;
                    const double lv = (cc < NB) ? sI[cc * P + 4 * ks + lk] : 0.0;
                    xa[C] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, lv, xa[C], 0, 0, 0);
                    if (!diag_tile) xb[C] = __builtin_amdgcn_mfma_f64_16x16x4f64(bv, lv, xb[C], 0, 0, 0);
                }
            }
#pragma unroll
            for (int C = 0; C < 4; C++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int cc = 16 * C + lr;
                    if (cc < NB) {
                        sXi[(16 * wv + lk + 4 * i) * P + cc] = xa[C][i];
                        if (!diag_tile) sXj[(16 * wv + lk + 4 * i) * P + cc] = xb[C][i];
                    }
                }
        }
        __syncthreads();
        if (c == K + 1) {       // this tile's X_r is L_rK: the substitution kernel reads it from Lp
            for (int i = tid; i < nri * NB; i += 256) { const int rr = i / NB, q = i - rr * NB; Lp[(size_t)(r0 + rr) * n + k0 + q] = sXi[rr * P + q]; }
        }
        const double* sB = diag_tile ? sXi : sXj;
        {
            const int wv = tid >> 6, ln = tid & 63, lr = ln & 15, lk = ln >> 4;
            const double* pa = sXi + (4 * wv + (lr & 3) + 16 * (lr >> 2)) * P + lk;
            const double* pb = sB + lr * P + lk;
            mfma_d4 acc[4];
#pragma unroll
            for (int C = 0; C < 4; C++) acc[C] = mfma_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ks = 0; ks < NB / 4; ks++) {
                const double av = pa[4 * ks];
#pragma unroll
                for (int C = 0; C < 4; C++) acc[C] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, pb[16 * C * P + 4 * ks], acc[C], 0, 0, 0);
            }
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) Lr[a][b] -= acc[b][a];
        }
        __syncthreads();                // sXi / sXj are free for the next block column
    }
    if (!diag_tile) {
        // final A_rc (the panel input of block column c for the tiles to its right)
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int rr = ty + 16 * a, cc = tx + 16 * b;
                if (rr < nri && cc < ncj) S[(size_t)(r0 + rr) * n + c0 + cc] = Lr[a][b];
            }
        flow_publish(done + r * kFusedMaxBlocks + c, epoch);
        return;
    }
    // diagonal tile: a right-hand-side row riding along goes back to S (the substitution reads it there), then factor + invert
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int rr = ty + 16 * a, cc = tx + 16 * b;
            if (rr < nri && cc < ncj && rr >= ncj) S[(size_t)(r0 + rr) * n + c0 + cc] = Lr[a][b];
            if (rr >= ncj || cc >= ncj) Lr[a][b] = (rr == cc) ? 1.0 : 0.0;
        }
    if (!chol_tile_mfma(Lr, ncj, Linv + (size_t)c * NB * NB, sv)) {
        if (tid == 0) __hip_atomic_store((unsigned long long*)(scal + 5), (unsigned long long)__double_as_longlong(1.0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;                         // (the waiters watch the failure flag)
    }
    flow_publish(fac + c, epoch);
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_chol_flow(double* __restrict__ S, double* __restrict__ Lp, int n, int nblk,
                                                   double* __restrict__ Linv, double* __restrict__ scal, unsigned* __restrict__ flow, unsigned epoch)
{
    extern __shared__ __align__(16) double sm_step[];
    chol_flow_body(S, Lp, n, nblk, Linv, scal, flow, epoch, (int)blockIdx.x, sm_step);
}

constexpr int kPanelRows = 64;
// nr = n + 1: the right-hand side b_schur is stored right behind S in the reduce buffer, i.e. it IS row n of an
// (n+1) x n row-major matrix; carrying it through panel/update as an extra row performs the forward substitution
// y = L^-1 b for free.
__global__ __launch_bounds__(1024) void k_chol_panel(double* __restrict__ S, int n, int nr, int k0, int nb, const double* __restrict__ Linv,
                                                     const double* __restrict__ scal)
{
    constexpr int P = NB + 1;
    __shared__ double sI[NB * P];
    __shared__ double sA[kPanelRows * P];
    if (scal[5] != 0.0) return;         // diagonal block was not positive definite
    const int tid = threadIdx.x;
    const int row0 = k0 + nb + blockIdx.x * kPanelRows;
    const int nrows = min(kPanelRows, nr - row0);
    const double* Li = Linv + (size_t)(k0 / NB) * NB * NB;
    for (int i = tid; i < NB * NB; i += 1024) { const int r = i / NB, c = i - r * NB; sI[r * P + c] = (r < nb && c < nb) ? Li[r * NB + c] : 0.0; }
    for (int i = tid; i < nrows * nb; i += 1024) { const int r = i / nb, c = i - r * nb; sA[r * P + c] = S[(size_t)(row0 + r) * n + k0 + c]; }
    __syncthreads();
    // X = A * Linv^T :  X[r][c] = sum_{q <= c} A[r][q] * Linv[c][q]   (Linv is stored with explicit zeros above the diagonal)
    // thread = (row, group of 4 adjacent columns): 4 independent accumulators share every a[q] load
    const int r = tid >> 4, cg = tid & 15;
    if (r < nrows && cg < NB / 4) {
        const double* a = sA + r * P;
        const double* l0 = sI + (4 * cg) * P;
        double acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
        const int qmax = min(nb, 4 * cg + 4);
#pragma unroll 4
        for (int q = 0; q < qmax; q++) {
            const double aq = a[q];
            acc0 += aq * l0[q]; acc1 += aq * l0[P + q]; acc2 += aq * l0[2 * P + q]; acc3 += aq * l0[3 * P + q];
        }
        double* out = S + (size_t)(row0 + r) * n + k0 + 4 * cg;
        if (4 * cg < nb) out[0] = acc0;
        if (4 * cg + 1 < nb) out[1] = acc1;
        if (4 * cg + 2 < nb) out[2] = acc2;
        if (4 * cg + 3 < nb) out[3] = acc3;
    }
}

// trailing update S22 -= L21 L21^T (lower triangle), 32x32 tiles, panel rows staged in LDS
__global__ __launch_bounds__(256) void k_chol_update(double* __restrict__ S, int n, int nr, int k0, int nb, const double* __restrict__ scal)
{
    __shared__ double sA[32 * (NB + 1)], sB[32 * (NB + 1)];
    const int base = k0 + nb;
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj > ti || scal[5] != 0.0) return;
    const int r0 = base + ti * 32, c0 = base + tj * 32;
    const int tid = threadIdx.x, P = NB + 1;
    for (int i = tid; i < 32 * nb; i += 256) {
        const int r = i / nb, q = i % nb;
        sA[r * P + q] = (r0 + r < nr) ? S[(size_t)(r0 + r) * n + k0 + q] : 0.0;
        sB[r * P + q] = (c0 + r < n) ? S[(size_t)(c0 + r) * n + k0 + q] : 0.0;
    }
    __syncthreads();
    const int tr = tid / 32, tc = tid % 32;
    for (int rr = tr; rr < 32; rr += 8) {
        const int r = r0 + rr, c = c0 + tc;
        if (r < nr && c < n && c <= r) {
            double sv = 0;
#pragma unroll 4
            for (int q = 0; q < nb; q++) sv += sA[rr * P + q] * sB[tc * P + q];
            S[(size_t)r * n + c] -= sv;
        }
    }
}

// x = L^-T y by block back-substitution with the inverted diagonal blocks (y = L^-1 b was produced by the factorisation
// itself, see k_chol_panel); one 1024-thread workgroup, 16 row groups x 64 columns, coalesced along the columns.
// (NOT a duplicate of liba::row16_allsum: that one sums with DPP row rotations, this one with a __shfl_xor butterfly.  The two
// add in different orders and differ in the last bits, and every solver's results are pinned to its own: keep both.)
__device__ __forceinline__ double row16_sum(double v)          // sum over the 16 lanes of a DPP row (every lane gets it)
{
    v += __shfl_xor(v, 1, 16); v += __shfl_xor(v, 2, 16); v += __shfl_xor(v, 4, 16); v += __shfl_xor(v, 8, 16);
    return v;
}
// PRE (the fused path, n <= 480): the L_JK rows of block K-1 are fetched into registers while block K is being processed, so the
// serial sweep never waits for global memory.
constexpr int kSolvePre = 28;       // rows below the first block of a 480-unknown system / 16 row groups, rounded up
template <bool PRE>
__device__ __forceinline__ void chol_solve_body(const double* __restrict__ S, int n, const double* __restrict__ Linv,
                                                     const double* __restrict__ yin, const double* __restrict__ yin_last,
                                                     double* __restrict__ x, const double* __restrict__ scal, int last_forward, const int bx, double* __restrict__ sm)
{
    constexpr int P = NB + 1;
    double* y = sm;
    double* t = sm + n;
    double* part = t + 64;
    double* sL = part + 16 * 64;
    const int tid = threadIdx.x;
    if (scal[5] != 0.0) { for (int i = tid; i < n; i += 1024) x[i] = 0.0; return; }
    const int nblk = (n + NB - 1) / NB;
    // fused factorisation: S = the L panels, yin = their right-hand-side row, yin_last = the updated b of the last block
    for (int i = tid; i < n; i += 1024) y[i] = (last_forward && i >= (nblk - 1) * NB) ? yin_last[i] : yin[i];
    const int g64 = tid >> 6, r64 = tid & 63;       // 16 groups x 64 rows
    // backward sweep: x_K = Linv_KK^T (y_K - sum_{J>K} L_JK^T x_J); the inverted diagonal block is staged in LDS (its loads
    // are in flight together with those of the L_JK rows)
    double pre[PRE ? kSolvePre : 1];
    double li[4];                       // the inverted diagonal block on its way to LDS (PRE: fetched one block ahead)
    for (int K = nblk - 1; K >= 0; K--) {
        const int k0 = K * NB, nb = min(NB, n - k0);
        {
            if (K == nblk - 1 || !PRE) {
                const double* Li = Linv + (size_t)K * NB * NB;
#pragma unroll
                for (int it = 0; it < 4; it++) { const int i = tid + 1024 * it; li[it] = (i < NB * NB) ? Li[i] : 0.0; }
            }
            __syncthreads();            // y complete (first round) / previous block done with sL, t, part
#pragma unroll
            for (int it = 0; it < 4; it++) { const int i = tid + 1024 * it; if (i < NB * NB) { const int r = i / NB; sL[r * P + i - r * NB] = li[it]; } }
        }
        const int col = tid >> 4, sub = tid & 15;       // 16 lanes per column for the small matrix-vector products (row-wide reductions)
        if (K == nblk - 1 && last_forward) {    // the fused factorisation stops at the last diagonal block: y = L^-1 b for that block
            __syncthreads();
            double sv = 0;
            if (col < nb)
                for (int q = sub; q <= col; q += 16) sv += y[k0 + q] * sL[col * P + q];
            sv = row16_sum(sv);
            __syncthreads();
            if (col < nb && sub == 0) y[k0 + col] = sv;
            __syncthreads();
        }
        {
            double sv = 0;
            if (PRE) {
#pragma unroll
                for (int j = 0; j < kSolvePre; j++) { const int q = k0 + nb + g64 + 16 * j; if (q < n) sv += pre[j] * y[q]; }
            } else if (r64 < nb) {
#pragma unroll 8
                for (int q = k0 + nb + g64; q < n; q += 16) sv += S[(size_t)q * n + k0 + r64] * y[q];
            }
            part[g64 * 64 + r64] = sv;
            if (PRE && K > 0) {         // rows k0 + g64 + 16 j of block column K-1 (a full block): in flight during the rest of this block
                const double* Li = Linv + (size_t)(K - 1) * NB * NB;
#pragma unroll
                for (int it = 0; it < 4; it++) { const int i = tid + 1024 * it; li[it] = (i < NB * NB) ? Li[i] : 0.0; }
#pragma unroll
                for (int j = 0; j < kSolvePre; j++) {
                    const int q = k0 + g64 + 16 * j;
                    pre[j] = 0.0;
                    if (q < n && r64 < NB) pre[j] = S[(size_t)q * n + (k0 - NB) + r64];
                }
            }
        }
        __syncthreads();
        {
            const double tot = row16_sum(part[sub * 64 + col]);
            if (sub == 0 && col < nb) t[col] = y[k0 + col] - tot;
        }
        __syncthreads();
        {
            double sv = 0;
            if (col < nb)
                for (int q = col + sub; q < nb; q += 16) sv += sL[q * P + col] * t[q];
            sv = row16_sum(sv);
            if (sub == 0 && col < nb) y[k0 + col] = sv;
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += 1024) x[i] = y[i];
}
// The dynamic LDS of a kernel built on chol_solve_body: y[n], t[64], part[16][64], Linv block [NB][NB + 1].  Declared ONCE, here:
// an `extern __shared__` array declared inside a kernel belongs to the kernel's namespace, so the kernels of two namespaces would
// get two variables, and which kernels share one changes the code the compiler's LDS lowering makes for them
// (tools/kernel_asm_diff.py: k_chol_solve<false> and k_chol_solve_update<false> came out different with an array each).  The
// LocalBA kernels that wrap chol_solve_body name this one.
extern __shared__ double sm_solve[];
template <bool PRE>
__global__ __launch_bounds__(1024) void k_chol_solve(const double* __restrict__ S, int n, const double* __restrict__ Linv,
                                                     const double* __restrict__ yin, const double* __restrict__ yin_last,
                                                     double* __restrict__ x, const double* __restrict__ scal, int last_forward)
{
    chol_solve_body<PRE>(S, n, Linv, yin, yin_last, x, scal, last_forward, (int)blockIdx.x, sm_solve);
}

// ---- host side: LDS sizes and the launch sequences ----
constexpr int kSolveFixed = 64 + 16 * 64 + NB * (NB + 1);        // doubles of sm_solve besides y[n]
constexpr size_t solve_lds_bytes(int n) { return ((size_t)n + kSolveFixed) * sizeof(double); }
constexpr int kMaxUnknowns = 160 * 1024 / (int)sizeof(double) - kSolveFixed;        // what the 160 KiB of LDS of a CU take
static_assert(solve_lds_bytes(kMaxUnknowns) <= 160 * 1024 && solve_lds_bytes(kMaxUnknowns + 1) > 160 * 1024, "kMaxUnknowns is the LDS limit");
// what the inertial launches ask for whatever their windows' sizes (<= kFusedMaxBlocks * NB unknowns need 41 KB) and the batched
// LocalBA ones are allowed: 64 KiB, the default limit of a kernel
constexpr size_t kFusedSolveLds = 65536;
static_assert(solve_lds_bytes(kFusedMaxBlocks * NB) <= kFusedSolveLds, "a fused-path substitution fits kFusedSolveLds");

// a kernel that asks for more than 64 KiB of dynamic LDS must be allowed to (a limit, not an allocation; per device)
template <class Kernel>
int allow_lds(Kernel* kernel, size_t bytes)
{
    ORBX_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return ORBX_OK;
}
// this header's own kernels, for systems of up to n unknowns; their owners allow the kernels that wrap the bodies.  Every caller
// passes kMaxUnknowns, so that the limit of a kernel does not depend on which solver was created last.
inline int raise_lds_limits(int n)
{
    const size_t solve = std::max(solve_lds_bytes(n), kFusedSolveLds);
    int r = allow_lds(k_chol_flow, kStepLds);
    if (!r) r = allow_lds(k_chol_solve<true>, solve);
    if (!r) r = allow_lds(k_chol_solve<false>, solve);
    return r;
}

// The factorisation of S ((n + 1) x n, nblk block columns) on `stream`: up to kFusedMaxBlocks block columns ONE launch, a
// workgroup per lower-triangle tile with flags between them (flow: kFlowFlags words, zero before the first use; the epoch
// counts the launches) that leaves the L panels in Lp; larger systems a diag / panel / update launch per block column, in place.
inline void enqueue_factor(hipStream_t stream, double* S, double* Lp, int n, int nblk, double* Linv, double* scal, unsigned* flow, unsigned* flow_epoch)
{
    if (nblk <= kFusedMaxBlocks) {
        hipLaunchKernelGGL(k_chol_flow, dim3(nblk * (nblk + 1) / 2), dim3(256), kStepLds, stream, S, Lp, n, nblk, Linv, scal, flow, ++*flow_epoch);
        return;
    }
    for (int K = 0; K < nblk; K++) {
        const int k0 = K * NB, nb = std::min(NB, n - k0);
        const int rows_below = (n + 1) - k0 - nb;       // includes the right-hand-side row n (always >= 1)
        hipLaunchKernelGGL(k_chol_diag, dim3(1), dim3(256), 0, stream, (const double*)S, n, k0, nb, Linv, scal);
        hipLaunchKernelGGL(k_chol_panel, dim3((rows_below + kPanelRows - 1) / kPanelRows), dim3(1024), 0, stream, S, n, n + 1, k0, nb,
                           (const double*)Linv, (const double*)scal);
        if (k0 + nb < n) {
            const int t = (rows_below + 31) / 32;
            hipLaunchKernelGGL(k_chol_update, dim3(t, t), dim3(256), 0, stream, S, n, n + 1, k0, nb, (const double*)scal);
        }
    }
}

// x = the solution of the system enqueue_factor has just factored (the same S, Lp, n, nblk, Linv, scal)
inline void enqueue_solve(hipStream_t stream, const double* S, const double* Lp, int n, int nblk, const double* Linv, double* x, const double* scal)
{
    const double* b = S + (size_t)n * n;
    if (nblk <= kFusedMaxBlocks)        // the L panels and y = L^-1 b of all but the last block are in Lp, the updated b of the last block in S
        hipLaunchKernelGGL(k_chol_solve<true>, dim3(1), dim3(1024), solve_lds_bytes(n), stream, Lp, n, Linv, Lp + (size_t)n * n, b, x, scal, 1);
    else
        hipLaunchKernelGGL(k_chol_solve<false>, dim3(1), dim3(1024), solve_lds_bytes(n), stream, S, n, Linv, b, b, x, scal, 0);
}

}  // namespace chol
