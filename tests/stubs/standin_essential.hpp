// TEST INFRASTRUCTURE -- the members of the reference's KeyFrame, MapPoint and Map that the pose-graph adapters of
// include/orbslam3_shim_loop.hpp (OptimizeEssentialGraphHIP) touch and the stand-ins of standin_orbslam3.hpp lack
// (include/KeyFrame.h: GetParent, hasChild, GetLoopEdges, GetCovisiblesByWeight, GetWeight, mTcwBefMerge, mTwcBefMerge;
// include/MapPoint.h: mnCorrectedByKF, mnCorrectedReference, GetReferenceKeyFrame; include/Map.h: GetMaxKFid), added by derivation so
// that the existing stand-ins stay as they are.  The adapters take the types as template parameters.
#pragma once
#include <algorithm>
#include <map>
#include <set>

#include "standin_orbslam3.hpp"

namespace ORB_SLAM3 {

class EssKeyFrame : public KeyFrame {
public:
    EssKeyFrame* GetParent() { return mpParent; }
    bool hasChild(EssKeyFrame* p) { return mspChildrens.count(p) != 0; }
    std::set<EssKeyFrame*> GetLoopEdges() { return mspLoopEdges; }
    int GetWeight(EssKeyFrame* p) { return mConnectedKeyFrameWeights.count(p) ? mConnectedKeyFrameWeights[p] : 0; }
    std::vector<EssKeyFrame*> GetCovisiblesByWeight(const int& w)      // KeyFrame.cc:288-312: by descending weight, those >= w
    {
        std::vector<std::pair<int, EssKeyFrame*> > v;
        for (auto& kv : mConnectedKeyFrameWeights) if (kv.second >= w) v.push_back(std::make_pair(kv.second, kv.first));
        std::stable_sort(v.begin(), v.end(), [](const std::pair<int, EssKeyFrame*>& a, const std::pair<int, EssKeyFrame*>& b) { return a.first > b.first || (a.first == b.first && a.second->mnId < b.second->mnId); });
        std::vector<EssKeyFrame*> out;
        for (auto& p : v) out.push_back(p.second);
        return out;
    }
    Sophus::SE3f mTcwBefMerge, mTwcBefMerge;

    EssKeyFrame* mpParent = nullptr;
    std::set<EssKeyFrame*> mspChildrens, mspLoopEdges;
    std::map<EssKeyFrame*, int> mConnectedKeyFrameWeights;
};

class EssMapPoint : public MapPoint {
public:
    EssKeyFrame* GetReferenceKeyFrame() { return mpRefKF; }
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;
    EssKeyFrame* mpRefKF = nullptr;
};

class EssMap : public Map {
public:
    std::vector<EssKeyFrame*> GetAllKeyFrames() { return kfs; }
    std::vector<EssMapPoint*> GetAllMapPoints() { return mps; }
    long unsigned int GetMaxKFid() { long unsigned int m = 0; for (auto* k : kfs) m = std::max(m, k->mnId); return m; }
    std::vector<EssKeyFrame*> kfs;
    std::vector<EssMapPoint*> mps;
};

}  // namespace ORB_SLAM3
