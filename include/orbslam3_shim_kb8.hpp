// orbslam3_shim_kb8.hpp -- drop-in adapters that add the monocular KannalaBrandt8 (fisheye) camera to the two visual optimisers:
//
//   int  PoseOptimizationAnyCamHIP(Frame*)                                              Optimizer::PoseOptimization, src/Optimizer.cc:814-1115
//   void LocalBundleAdjustmentAnyCamHIP(KeyFrame*, bool*, Map*, int&, int&, int&, int&) Optimizer::LocalBundleAdjustment, :1116-1498
//
// Device KB8 path: the frame -- or every key frame of the window, fixed cameras included -- has no mpCamera2 and one CAM_FISHEYE
// camera, with identical eight parameters across the window, and no observation with mvuRight >= 0 (the device's KB8 edges are
// monocular).  That camera is then set on the solver handle around the solve (pose_set_camera_kb8 / lba_set_camera_kb8 of
// orbslam3_hip_kb8.h) and reset after it.  Anything else goes to PoseOptimizationHIP / LocalBundleAdjustmentHIP of orbslam3_shim.hpp, which keep
// their own fallback to the reference (stereo-fisheye rigs with mpCamera2 end there).
// Nothing is marshalled here: the flattening of a frame's edges, the walk of the window, the problems, the solves and the write-backs
// are the pinhole adapters' own steps in orbslam3_shim.hpp (PoseOptimizationWithCamera, LocalBundleAdjustmentGraph /
// LocalBundleAdjustmentFinish), which take the camera as an optional argument and set it around the solve with CameraScope of
// orbslam3_shim_marshal.hpp; this header only decides which camera applies.  The handles are therefore the pinhole
// adapters' (one pose_solver and one lba_solver per thread): lba_set_camera_kb8(NULL) returns a handle to the bits of a fresh one.
#pragma once

#include "orbslam3_shim.hpp"

#ifdef ORBSLAM3_HIP_WITH_REFERENCE

#include "CameraModels/KannalaBrandt8.h"

namespace ORB_SLAM3 {

namespace kb8_detail {

// the eight parameters of a CAM_FISHEYE camera (mvParameters: fx fy cx cy k0 k1 k2 k3, floats) promoted to double; false for
// any other camera.  (getParameter is GeometricCamera's in the reference; the call goes through the derived class because the
// stand-in base class that the typed tests compile against does not have it, and a CAM_FISHEYE camera is a KannalaBrandt8.)
inline bool camera_of(GeometricCamera* pCamera, OrbxKB8& out)
{
    if (!pCamera || pCamera->GetType() != GeometricCamera::CAM_FISHEYE) return false;
    orbslam3_hip::kb8_in(static_cast<KannalaBrandt8*>(pCamera), out);
    return true;
}

inline bool same(const OrbxKB8& a, const OrbxKB8& b)
{
    return a.fx == b.fx && a.fy == b.fy && a.cx == b.cx && a.cy == b.cy && a.k[0] == b.k[0] && a.k[1] == b.k[1] && a.k[2] == b.k[2] && a.k[3] == b.k[3];
}

template <class KF>
inline bool is_mono_kb8(KF* p, const OrbxKB8* like, OrbxKB8& out)
{
    return !p->mpCamera2 && camera_of(p->mpCamera, out) && (!like || same(*like, out));
}

using orbslam3_hip::CameraScope;   // sets the camera on a handle for the lifetime of the object, and resets it on every way out

}  // namespace kb8_detail

inline int PoseOptimizationAnyCamHIP(Frame* pFrame)
{
    OrbxKB8 cam;
    bool kb8 = kb8_detail::is_mono_kb8(pFrame, nullptr, cam);
    for (int i = 0; kb8 && i < pFrame->N; i++)
        if (pFrame->mvpMapPoints[i] && pFrame->mvuRight[i] >= 0) kb8 = false;      // a stereo observation: not a monocular frame
    if (!kb8) return PoseOptimizationHIP(pFrame);
    return PoseOptimizationWithCamera(pFrame, &cam);                                // a monocular frame: every mvuRight of an edge is < 0
}

inline void LocalBundleAdjustmentAnyCamHIP(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs, int& num_edges)
{
    OrbxKB8 cam, other;
    bool kb8 = kb8_detail::is_mono_kb8(pKF, nullptr, cam);
    if (kb8)
        for (KeyFrame* pKFi : pKF->GetVectorCovisibleKeyFrames())
            if (!kb8_detail::is_mono_kb8(pKFi, &cam, other)) { kb8 = false; break; }
    if (!kb8) { LocalBundleAdjustmentHIP(pKF, pbStopFlag, pMap, num_fixedKF, num_OptKF, num_MPs, num_edges); return; }
    LbaGraph g;
    const bool ok = LocalBundleAdjustmentGraph(pKF, pMap, g);
    // the fixed cameras only turn up in the walk (LocalBundleAdjustmentHIP says what the walk has touched by then, and why that is harmless)
    // and so do the observations: one with mvuRight >= 0 would be a stereo edge, which the device refuses for a KB8 camera
    for (KeyFrame* pKFi : g.kfs) kb8 = kb8 && kb8_detail::is_mono_kb8(pKFi, &cam, other);
    for (uint8_t st : g.eStereo) kb8 = kb8 && !st;
    if (!kb8) { LocalBundleAdjustmentHIP(pKF, pbStopFlag, pMap, num_fixedKF, num_OptKF, num_MPs, num_edges); return; }
    LocalBundleAdjustmentFinish(g, ok, pbStopFlag, pMap, &cam, num_fixedKF, num_OptKF, num_edges);
}

}  // namespace ORB_SLAM3

#endif  // ORBSLAM3_HIP_WITH_REFERENCE
