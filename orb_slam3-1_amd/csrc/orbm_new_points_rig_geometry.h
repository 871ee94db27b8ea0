// The per-match geometry of LocalMapping::CreateNewMapPoints for two two-camera KannalaBrandt8 rigs (reference
// src/LocalMapping.cc:509-695 with mpCamera2 set on both key frames) and MapPoint::UpdateNormalAndDepth of the new point
// (src/MapPoint.cc:426-494), restated for one (key frame 1 feature, neighbour feature) pair.  Plain C++ without device builtins:
// the same text is the body of k_new_map_points_rig, of the host check tests/rig_newpoints_geometry_check.cpp and of the one-core
// baseline tools/rig_newpoints_cpu.cpp.  Built on kb8s::unproject / kb8s::project and nmp::triangulate / dot3 / norm3; float
// expressions follow the reference's operation order (the library is built with -ffp-contract=off), only the null vector of
// Triangulate's 4x4 matrix is computed in double.
//
// What the rig branches change against orbm_new_points_geometry.h:
//  - (bRight1, bRight2) select the pose, centre and camera of each side (:509-559); all four branches reset everything.
//  - bStereo1 = bStereo2 = false (`!mpCamera2 && ...`, :496 / :505): cosParallaxStereo stays cosParallaxRays + 1, so the first
//    comparison of :586 is cosRays < cosRays + 1, the UnprojectStereo branches and the 7.8 gates never run, bPointStereo is false.
//  - xn = KannalaBrandt8::unprojectEig(kp.pt) of the raw key point, the reprojection goes through KannalaBrandt8::project.
//  - mvuRight[idx] is read (:495 / :504) and never used; it is not read here.
#pragma once
#include "kb8_stereo_geometry.h"

namespace nmp_rig {

struct Side {                   // one camera of a rig key frame: GetPose() / GetRightPose(), the matching centre and camera
    nmp::Camera pose;           // Rcw, tcw, Ow; the pinhole fields are not read
    kb8s::Cam cam;
};

struct Obs {                    // one key point of it
    float x, y;                 // mvKeys[i].pt or mvKeysRight[i - NLeft].pt
    float sigma2, scale;        // mvLevelSigma2[octave], mvScaleFactors[octave]
};

// the baseline test of :447-455 for a stereo sensor: `baseline < pKF2->mb` with baseline = (Ow2 - Ow1).norm()
NMP_HD bool baseline_too_short(const float* Ow1, const float* Ow2, float mb2)
{
    return nmp::norm3(Ow2[0] - Ow1[0], Ow2[1] - Ow1[1], Ow2[2] - Ow1[2]) < mb2;
}

// the monocular reprojection gate of one side (:625-640 / :653-665)
NMP_HD bool reprojection_ok(const Side& S, const Obs& o, const float* x3D, float z)
{
    float X[3], uv[2];
    X[0] = nmp::dot3(S.pose.Rcw[0], S.pose.Rcw[1], S.pose.Rcw[2], x3D[0], x3D[1], x3D[2]) + S.pose.tcw[0];
    X[1] = nmp::dot3(S.pose.Rcw[3], S.pose.Rcw[4], S.pose.Rcw[5], x3D[0], x3D[1], x3D[2]) + S.pose.tcw[1];
    X[2] = z;
    kb8s::project(S.cam, X, uv);
    const float ex = uv[0] - o.x, ey = uv[1] - o.y;
    return !((double)(ex * ex + ey * ey) > 5.991 * (double)o.sigma2);
}

// :561-695 for one match.  Returns true when the reference would create the map point.
NMP_HD bool new_point(const Side& S1, const Obs& o1, const Side& S2, const Obs& o2, const nmp::Rule& R, float* x3D)
{
    float xn1[3], xn2[3], ray1[3], ray2[3];
    kb8s::unproject(S1.cam, o1.x, o1.y, xn1);
    kb8s::unproject(S2.cam, o2.x, o2.y, xn2);
    for (int r = 0; r < 3; r++) {                                                    // Rwc * xn, xn = (x, y, 1)
        ray1[r] = S1.pose.Rcw[r] * xn1[0] + S1.pose.Rcw[3 + r] * xn1[1] + S1.pose.Rcw[6 + r] * 1.f;
        ray2[r] = S2.pose.Rcw[r] * xn2[0] + S2.pose.Rcw[3 + r] * xn2[1] + S2.pose.Rcw[6 + r] * 1.f;
    }
    const float cosRays = nmp::dot3(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]) /
                          (nmp::norm3(ray1[0], ray1[1], ray1[2]) * nmp::norm3(ray2[0], ray2[1], ray2[2]));
    const float cosStereo = cosRays + 1;
    if (!(cosRays < cosStereo && cosRays > 0 && (((double)cosRays < 0.9996 && R.inertial) || ((double)cosRays < 0.9998 && !R.inertial))))
        return false;                                                                // no stereo and very low parallax (:607)
    if (!nmp::triangulate(xn1[0], xn1[1], xn2[0], xn2[1], S1.pose, S2.pose, x3D)) return false;

    const float z1 = nmp::dot3(S1.pose.Rcw[6], S1.pose.Rcw[7], S1.pose.Rcw[8], x3D[0], x3D[1], x3D[2]) + S1.pose.tcw[2];
    if (!(z1 > 0)) return false;
    const float z2 = nmp::dot3(S2.pose.Rcw[6], S2.pose.Rcw[7], S2.pose.Rcw[8], x3D[0], x3D[1], x3D[2]) + S2.pose.tcw[2];
    if (!(z2 > 0)) return false;
    if (!reprojection_ok(S1, o1, x3D, z1)) return false;
    if (!reprojection_ok(S2, o2, x3D, z2)) return false;

    const float dist1 = nmp::norm3(x3D[0] - S1.pose.Ow[0], x3D[1] - S1.pose.Ow[1], x3D[2] - S1.pose.Ow[2]);    // the SIDES' centres
    const float dist2 = nmp::norm3(x3D[0] - S2.pose.Ow[0], x3D[1] - S2.pose.Ow[1], x3D[2] - S2.pose.Ow[2]);
    if (dist1 == 0 || dist2 == 0) return false;
    if (R.far_points && (dist1 >= R.th_far || dist2 >= R.th_far)) return false;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = o1.scale / o2.scale;
    if (ratioDist * R.ratio_factor < ratioOctave || ratioDist > ratioOctave * R.ratio_factor) return false;
    return true;
}

// MapPoint::UpdateNormalAndDepth of the new point.  The normal is the mean of the unit vectors from the centres of the two
// observing SIDES (AddObservation files an index >= NLeft as a right observation; a sum of two floats does not depend on the
// order of the map).  The distance is taken from pRefKF->GetCameraCenter() -- key frame 1's LEFT centre, also for a right
// observation (:468).  level_scale = kf1's mvScaleFactors[octave of idx1 in the concatenated arrays].
NMP_HD void normal_and_depth(const float* x3D, const float* Ow_side1, const float* Ow_side2, const float* Ow_left1, float level_scale,
                             float last_scale, float* normal, float* max_dist, float* min_dist)
{
    const float px = x3D[0], py = x3D[1], pz = x3D[2];
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int o = 0; o < 2; o++) {
        const float* c = o ? Ow_side2 : Ow_side1;
        const float dx = px - c[0], dy = py - c[1], dz = pz - c[2];
        const float nrm = nmp::norm3(dx, dy, dz);
        nx = nx + dx / nrm; ny = ny + dy / nrm; nz = nz + dz / nrm;
    }
    const float dist = nmp::norm3(px - Ow_left1[0], py - Ow_left1[1], pz - Ow_left1[2]);
    const float mx = dist * level_scale;
    *max_dist = mx;
    *min_dist = mx / last_scale;
    const float cnt = (float)2;
    normal[0] = nx / cnt; normal[1] = ny / cnt; normal[2] = nz / cnt;
}

}  // namespace nmp_rig
