// The per-match geometry of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:561-695), restated for one
// (key frame 1 feature, neighbour feature) pair.  Plain C++ without device builtins, so that the same text is the body of
// k_new_map_points and of the host check tests/newpoints_geometry_check.cpp.  Float expressions follow the reference
// (the library is built with -ffp-contract=off); only the null vector of Triangulate's 4x4 matrix is computed in double.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define NMP_HD __host__ __device__ __forceinline__
#else
#define NMP_HD inline
#endif

namespace nmp {

struct Camera {                 // one key frame: GetPose(), GetCameraCenter(), the pinhole intrinsics and the stereo rig
    float Rcw[9], tcw[3], Ow[3];
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
};

struct Obs {                    // one key point of it
    float x, y;                 // mvKeysUn[i].pt
    float ur, depth;            // mvuRight[i], mvDepth[i]
    float kx, ky;               // mvKeys[i].pt (KeyFrame::UnprojectStereo reads the distorted key point)
    float sigma2, scale;        // mvLevelSigma2[octave], mvScaleFactors[octave]
};

struct Rule {
    int inertial, far_points;
    float th_far, ratio_factor; // mThFarPoints, 1.5f * mfScaleFactor
};

NMP_HD float dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return a0 * b0 + (a1 * b1 + a2 * b2); }   // Eigen's fixed-size redux
NMP_HD float norm3(float a0, float a1, float a2) { return sqrtf(a0 * a0 + (a1 * a1 + a2 * a2)); }

// one Jacobi rotation of the symmetric 4x4 M in the (P, Q) plane, accumulated into V (columns = eigenvectors)
template <int P, int Q>
NMP_HD void jacobi_rotate(double (&M)[4][4], double (&V)[4][4])
{
    const double apq = M[P][Q];
    if (apq == 0.0) return;
    const double theta = (M[Q][Q] - M[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));     // the smaller root: |angle| <= pi/4
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    for (int k = 0; k < 4; k++) {                       // M <- M J
        const double mkp = M[k][P], mkq = M[k][Q];
        M[k][P] = c * mkp - s * mkq;
        M[k][Q] = s * mkp + c * mkq;
    }
    for (int k = 0; k < 4; k++) {                       // M <- J^T M
        const double mpk = M[P][k], mqk = M[Q][k];
        M[P][k] = c * mpk - s * mqk;
        M[Q][k] = s * mpk + c * mqk;
    }
    M[P][Q] = 0.0; M[Q][P] = 0.0;
    for (int k = 0; k < 4; k++) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

constexpr int kJacobiSweeps = 6;        // cyclic Jacobi converges quadratically: a 4x4 is at double rounding after 4-5 sweeps

// right singular vector of the smallest singular value of the row-major float 4x4 A = eigenvector of the smallest eigenvalue
// of A^T A.  A of float inputs has a condition number far below 1e8, so its square is safe in double.
NMP_HD void null_vector(const float* A, double* v)
{
    double M[4][4], V[4][4];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double s = 0.0;
            for (int k = 0; k < 4; k++) s += (double)A[4 * k + i] * (double)A[4 * k + j];
            M[i][j] = s;
            V[i][j] = i == j ? 1.0 : 0.0;
        }
#pragma unroll
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
        jacobi_rotate<0, 1>(M, V); jacobi_rotate<0, 2>(M, V); jacobi_rotate<0, 3>(M, V);
        jacobi_rotate<1, 2>(M, V); jacobi_rotate<1, 3>(M, V); jacobi_rotate<2, 3>(M, V);
    }
    double best = M[0][0];
    v[0] = V[0][0]; v[1] = V[1][0]; v[2] = V[2][0]; v[3] = V[3][0];
    if (M[1][1] < best) { best = M[1][1]; v[0] = V[0][1]; v[1] = V[1][1]; v[2] = V[2][1]; v[3] = V[3][1]; }
    if (M[2][2] < best) { best = M[2][2]; v[0] = V[0][2]; v[1] = V[1][2]; v[2] = V[2][2]; v[3] = V[3][2]; }
    if (M[3][3] < best) { best = M[3][3]; v[0] = V[0][3]; v[1] = V[1][3]; v[2] = V[2][3]; v[3] = V[3][3]; }
}

// GeometricTools::Triangulate (src/GeometricTools.cc:47-66)
NMP_HD bool triangulate(float xn1x, float xn1y, float xn2x, float xn2y, const Camera& C1, const Camera& C2, float* x3D)
{
    float A[16];
    for (int c = 0; c < 4; c++) {
        const float t10 = c < 3 ? C1.Rcw[c] : C1.tcw[0], t11 = c < 3 ? C1.Rcw[3 + c] : C1.tcw[1], t12 = c < 3 ? C1.Rcw[6 + c] : C1.tcw[2];
        const float t20 = c < 3 ? C2.Rcw[c] : C2.tcw[0], t21 = c < 3 ? C2.Rcw[3 + c] : C2.tcw[1], t22 = c < 3 ? C2.Rcw[6 + c] : C2.tcw[2];
        A[c] = xn1x * t12 - t10;
        A[4 + c] = xn1y * t12 - t11;
        A[8 + c] = xn2x * t22 - t20;
        A[12 + c] = xn2y * t22 - t21;
    }
    double v[4];
    null_vector(A, v);
    if ((float)v[3] == 0.f) return false;               // x3Dh(3) == 0 (:59)
    x3D[0] = (float)(v[0] / v[3]); x3D[1] = (float)(v[1] / v[3]); x3D[2] = (float)(v[2] / v[3]);
    return true;
}

// KeyFrame::UnprojectStereo (src/KeyFrame.cc:755-772): mRwc = Rcw^T, mTwc.translation() = the camera centre
NMP_HD bool unproject_stereo(const Camera& C, const Obs& o, float* x3D)
{
    const float z = o.depth;
    if (!(z > 0)) return false;
    const float x = (o.kx - C.cx) * z * C.invfx;
    const float y = (o.ky - C.cy) * z * C.invfy;
    for (int r = 0; r < 3; r++) x3D[r] = (C.Rcw[r] * x + C.Rcw[3 + r] * y + C.Rcw[6 + r] * z) + C.Ow[r];
    return true;
}

// reprojection gate of one side (:625-676); mbf1 = key frame 1's mbf on BOTH sides (the reference's :669)
NMP_HD bool reprojection_ok(const Camera& C, const Obs& o, bool stereo, float mbf1, const float* x3D, float z)
{
    const float x = dot3(C.Rcw[0], C.Rcw[1], C.Rcw[2], x3D[0], x3D[1], x3D[2]) + C.tcw[0];
    const float y = dot3(C.Rcw[3], C.Rcw[4], C.Rcw[5], x3D[0], x3D[1], x3D[2]) + C.tcw[1];
    if (!stereo) {
        const float u = C.fx * x / z + C.cx, v = C.fy * y / z + C.cy;          // Pinhole::project
        const float ex = u - o.x, ey = v - o.y;
        return !((double)(ex * ex + ey * ey) > 5.991 * (double)o.sigma2);
    }
    const float invz = (float)(1.0 / (double)z);
    const float u = C.fx * x * invz + C.cx;
    const float u_r = u - mbf1 * invz;
    const float v = C.fy * y * invz + C.cy;
    const float ex = u - o.x, ey = v - o.y, er = u_r - o.ur;
    return !((double)(ex * ex + ey * ey + er * er) > 7.8 * (double)o.sigma2);
}

// :561-695 for one match.  Returns true when the reference would create the map point.
NMP_HD bool new_point(const Camera& C1, const Obs& o1, const Camera& C2, const Obs& o2, const Rule& R, float* x3D, int* point_stereo)
{
    const bool bStereo1 = o1.ur >= 0, bStereo2 = o2.ur >= 0;
    const float xn1x = (o1.x - C1.cx) / C1.fx, xn1y = (o1.y - C1.cy) / C1.fy;        // Pinhole::unprojectEig: a division
    const float xn2x = (o2.x - C2.cx) / C2.fx, xn2y = (o2.y - C2.cy) / C2.fy;
    float ray1[3], ray2[3];
    for (int r = 0; r < 3; r++) {                                                    // Rwc * xn, xn = (x, y, 1)
        ray1[r] = C1.Rcw[r] * xn1x + C1.Rcw[3 + r] * xn1y + C1.Rcw[6 + r] * 1.f;
        ray2[r] = C2.Rcw[r] * xn2x + C2.Rcw[3 + r] * xn2y + C2.Rcw[6 + r] * 1.f;
    }
    const float cosRays = dot3(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]) /
                          (norm3(ray1[0], ray1[1], ray1[2]) * norm3(ray2[0], ray2[1], ray2[2]));
    float cosStereo1 = cosRays + 1, cosStereo2 = cosRays + 1;
    if (bStereo1) cosStereo1 = cosf(2 * atan2f(C1.mb / 2, o1.depth));
    else if (bStereo2) cosStereo2 = cosf(2 * atan2f(C2.mb / 2, o2.depth));           // not computed when key point 1 is stereo (:575)
    const float cosStereo = fminf(cosStereo1, cosStereo2);

    *point_stereo = 0;
    if (cosRays < cosStereo && cosRays > 0 &&
        (bStereo1 || bStereo2 || ((double)cosRays < 0.9996 && R.inertial) || ((double)cosRays < 0.9998 && !R.inertial))) {
        if (!triangulate(xn1x, xn1y, xn2x, xn2y, C1, C2, x3D)) return false;
    } else if (bStereo1 && cosStereo1 < cosStereo2) {
        *point_stereo = 1;
        if (!unproject_stereo(C1, o1, x3D)) return false;
    } else if (bStereo2 && cosStereo2 < cosStereo1) {
        *point_stereo = 1;
        if (!unproject_stereo(C2, o2, x3D)) return false;
    } else {
        return false;                                                                // no stereo and very low parallax
    }

    const float z1 = dot3(C1.Rcw[6], C1.Rcw[7], C1.Rcw[8], x3D[0], x3D[1], x3D[2]) + C1.tcw[2];
    if (!(z1 > 0)) return false;
    const float z2 = dot3(C2.Rcw[6], C2.Rcw[7], C2.Rcw[8], x3D[0], x3D[1], x3D[2]) + C2.tcw[2];
    if (!(z2 > 0)) return false;
    if (!reprojection_ok(C1, o1, bStereo1, C1.mbf, x3D, z1)) return false;
    if (!reprojection_ok(C2, o2, bStereo2, C1.mbf, x3D, z2)) return false;

    const float dist1 = norm3(x3D[0] - C1.Ow[0], x3D[1] - C1.Ow[1], x3D[2] - C1.Ow[2]);
    const float dist2 = norm3(x3D[0] - C2.Ow[0], x3D[1] - C2.Ow[1], x3D[2] - C2.Ow[2]);
    if (dist1 == 0 || dist2 == 0) return false;
    if (R.far_points && (dist1 >= R.th_far || dist2 >= R.th_far)) return false;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = o1.scale / o2.scale;
    if (ratioDist * R.ratio_factor < ratioOctave || ratioDist > ratioOctave * R.ratio_factor) return false;
    return true;
}

// MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:433-493) of the new point: observations (kf1, neighbour) in that order,
// pRefKF = kf1.  The float expressions are those of k_normal_depth (orbm_matcher.hip), which the results equal bit for bit.
NMP_HD void normal_and_depth(const float* x3D, const float* Ow1, const float* Ow2, float level_scale, float last_scale,
                             float* normal, float* max_dist, float* min_dist)
{
    const float px = x3D[0], py = x3D[1], pz = x3D[2];
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int o = 0; o < 2; o++) {
        const float* c = o ? Ow2 : Ow1;
        const float dx = px - c[0], dy = py - c[1], dz = pz - c[2];
        const float nrm = sqrtf(dx * dx + (dy * dy + dz * dz));
        nx = nx + dx / nrm; ny = ny + dy / nrm; nz = nz + dz / nrm;
    }
    const float cx = px - Ow1[0], cy = py - Ow1[1], cz = pz - Ow1[2];
    const float dist = sqrtf(cx * cx + (cy * cy + cz * cz));
    const float mx = dist * level_scale;
    *max_dist = mx;
    *min_dist = mx / last_scale;
    const float cnt = (float)2;
    normal[0] = nx / cnt; normal[1] = ny / cnt; normal[2] = nz / cnt;
}

}  // namespace nmp
