// orbslam3_shim_fisheye.hpp -- drop-in adapter for the stereo step of a two-camera fisheye rig:
//
//   void ComputeStereoFishEyeMatchesHIP(Frame& F, orbm_matcher* m = nullptr)       Frame::ComputeStereoFishEyeMatches, src/Frame.cc:1246-1286
//
// Call it where the reference's Frame constructor calls ComputeStereoFishEyeMatches() (src/Frame.cc:1225): mvKeys / mDescriptors
// and mvKeysRight / mDescriptorsRight hold the two sides, still separate (the constructor concatenates them afterwards), Nleft,
// Nright, monoLeft and monoRight are set.  It writes what the reference writes -- mvLeftToRightMatch, mvRightToLeftMatch, mvDepth,
// mvuRight (all -1: the reference never fills it here), mvStereo3Dpoints, mnCloseMPs = 0 -- from one orbm_stereo_fisheye call
// (orbslam3_hip_fisheye.h).  m == nullptr uses the calling thread's matcher handle; a handle serves one call at a time.
// It falls back to the reference's own function when either camera is missing or not CAM_FISHEYE.
// The frame type is a template parameter (Frame in the reference tree; the adapter is a friend-free reader: it reaches the rig
// through GetRelativePoseTlr()), and so is the camera class (KannalaBrandt8: getParameter, GetPrecision), so that the header
// compiles against stand-in types.  The marshalling is orbslam3_shim_marshal.hpp's: keypoints_in, descriptors_in, fisheye_rig_in.
#pragma once

#include "orbslam3_shim.hpp"

#ifdef ORBSLAM3_HIP_WITH_REFERENCE

#include "CameraModels/KannalaBrandt8.h"

namespace ORB_SLAM3 {

template <class Fisheye = KannalaBrandt8, class FrameT>
inline void ComputeStereoFishEyeMatchesHIP(FrameT& F, orbm_matcher* m = nullptr)
{
    const bool rig = F.mpCamera && F.mpCamera2 && F.mpCamera->GetType() == GeometricCamera::CAM_FISHEYE &&
                     F.mpCamera2->GetType() == GeometricCamera::CAM_FISHEYE;
    if (!rig) { F.ComputeStereoFishEyeMatches(); return; }
    if (!m) m = orbslam3_hip::thread_handle<orbm_matcher, orbm_create>();
    const OrbxFisheyeRig g = orbslam3_hip::fisheye_rig_in(static_cast<Fisheye*>(F.mpCamera), static_cast<Fisheye*>(F.mpCamera2), F.GetRelativePoseTlr());
    const int nl = F.Nleft, nr = F.Nright;
    std::vector<uint8_t> copy_l, copy_r;
    std::vector<int32_t> ltr((size_t)std::max(nl, 0)), rtl((size_t)std::max(nr, 0));
    std::vector<float> depth((size_t)std::max(nl, 0)), p3d(3 * (size_t)std::max(nl, 0));
    orbslam3_hip::check(orbm_stereo_fisheye(m, orbslam3_hip::keypoints_in(F.mvKeys), orbslam3_hip::descriptors_in(F.mDescriptors, nl, copy_l), nl, F.monoLeft,
                                            orbslam3_hip::keypoints_in(F.mvKeysRight), orbslam3_hip::descriptors_in(F.mDescriptorsRight, nr, copy_r), nr, F.monoRight,
                                            F.mvLevelSigma2.data(), (int)F.mvLevelSigma2.size(), &g, ltr.data(), rtl.data(), depth.data(), p3d.data(),
                                            nullptr, nullptr, nullptr));
    F.mvLeftToRightMatch.assign(ltr.begin(), ltr.end());
    F.mvRightToLeftMatch.assign(rtl.begin(), rtl.end());
    F.mvDepth.assign(depth.begin(), depth.end());
    F.mvuRight.assign((size_t)std::max(nl, 0), -1.f);
    F.mvStereo3Dpoints.assign((size_t)std::max(nl, 0), Eigen::Vector3f());
    for (int i = 0; i < nl; i++) F.mvStereo3Dpoints[i] = Eigen::Vector3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
    F.mnCloseMPs = 0;
}

}  // namespace ORB_SLAM3

#endif  // ORBSLAM3_HIP_WITH_REFERENCE
