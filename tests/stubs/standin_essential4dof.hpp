// TEST INFRASTRUCTURE -- the members of the reference's KeyFrame, MapPoint and Map that the 4-DoF pose-graph adapter of
// include/orbslam3_shim_loop.hpp (OptimizeEssentialGraph4DoFHIP) touches and the stand-ins of standin_orbslam3.hpp lack
// (include/KeyFrame.h: hasChild, GetLoopEdges, GetCovisiblesByWeight, GetWeight, mNextKF; include/MapPoint.h: GetReferenceKeyFrame),
// added by derivation so that the existing stand-ins stay as they are.  mPrevKF, mImuCalib, GetImuRotation and GetImuPosition are
// the base stand-in's.  The adapter takes the types as template parameters.
#pragma once
#include <algorithm>
#include <map>
#include <set>

#include "standin_orbslam3.hpp"

namespace ORB_SLAM3 {

class Ess4KeyFrame : public KeyFrame {
public:
    bool hasChild(Ess4KeyFrame* p) { return mspChildrens.count(p) != 0; }
    std::set<Ess4KeyFrame*> GetLoopEdges() { return mspLoopEdges; }
    int GetWeight(Ess4KeyFrame* p) { return mConnectedKeyFrameWeights.count(p) ? mConnectedKeyFrameWeights[p] : 0; }
    std::vector<Ess4KeyFrame*> GetCovisiblesByWeight(const int& w)     // KeyFrame.cc:288-312: by descending weight, those >= w
    {
        std::vector<std::pair<int, Ess4KeyFrame*> > v;
        for (auto& kv : mConnectedKeyFrameWeights) if (kv.second >= w) v.push_back(std::make_pair(kv.second, kv.first));
        std::stable_sort(v.begin(), v.end(), [](const std::pair<int, Ess4KeyFrame*>& a, const std::pair<int, Ess4KeyFrame*>& b) { return a.first > b.first || (a.first == b.first && a.second->mnId < b.second->mnId); });
        std::vector<Ess4KeyFrame*> out;
        for (auto& p : v) out.push_back(p.second);
        return out;
    }
    KeyFrame* mNextKF = nullptr;

    std::set<Ess4KeyFrame*> mspChildrens, mspLoopEdges;
    std::map<Ess4KeyFrame*, int> mConnectedKeyFrameWeights;
};

class Ess4MapPoint : public MapPoint {
public:
    Ess4KeyFrame* GetReferenceKeyFrame() { return mpRefKF; }
    Ess4KeyFrame* mpRefKF = nullptr;
};

class Ess4Map : public Map {
public:
    std::vector<Ess4KeyFrame*> GetAllKeyFrames() { return kfs; }
    std::vector<Ess4MapPoint*> GetAllMapPoints() { return mps; }
    std::vector<Ess4KeyFrame*> kfs;
    std::vector<Ess4MapPoint*> mps;
};

}  // namespace ORB_SLAM3
