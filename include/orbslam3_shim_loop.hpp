// orbslam3_shim_loop.hpp -- drop-in adapters for the loop-closing geometry (LoopClosing::DetectCommonRegionsFromBoW,
// reference src/LoopClosing.cc:640-830), on top of sim3_ransac_batch / sim3_optimize_batch of orbslam3_hip.h:
//
//   class Sim3SolverHIP      the interface of class Sim3Solver                               include/Sim3Solver.h:33-50
//   int  OptimizeSim3HIP(KeyFrame*, KeyFrame*, std::vector<MapPoint*>&, g2o::Sim3&, const float, const bool,
//                        Eigen::Matrix<double,7,7>&, const bool)   = Optimizer::OptimizeSim3  include/Optimizer.h, src/Optimizer.cc:2115
//
// Like orbslam3_shim.hpp (which it includes) it is written against the reference's own types and compiles inside an ORB-SLAM3
// tree with ORBSLAM3_HIP_WITH_REFERENCE defined.  Cameras other than one pinhole per key frame fall back to the reference's
// own Sim3Solver / Optimizer::OptimizeSim3; those calls sit in template-dependent contexts (the defaulted parameters Ref / Opt),
// so that a tree without these classes still compiles the header as long as the fallback is never instantiated.
#pragma once

#include "orbslam3_shim.hpp"

#ifdef ORBSLAM3_HIP_WITH_REFERENCE

#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <type_traits>

namespace ORB_SLAM3 {

class Sim3Solver;       // include/Sim3Solver.h: only named here, used through the template parameter Ref

namespace loop_detail {

inline bool single_pinhole(KeyFrame* pKF) { return !pKF->mpCamera2 && pKF->mpCamera && pKF->mpCamera->GetType() == GeometricCamera::CAM_PINHOLE; }

inline sim3_solver* solver() { return orbslam3_hip::thread_handle<sim3_solver, sim3_create>(); }

inline void intrinsics(KeyFrame* pKF, float* K)      // fx fy cx cy as the camera model holds them (Pinhole::toK_)
{
    const Eigen::Matrix3f Km = pKF->mpCamera->toK_();
    K[0] = Km(0, 0); K[1] = Km(1, 1); K[2] = Km(0, 2); K[3] = Km(1, 2);
}

}  // namespace loop_detail

// Sim3Solver (src/Sim3Solver.cc).  The first iterate() evaluates all mRansacMaxIts hypotheses in one launch; every
// iterate(n, ...) then walks the downloaded counts in order with the reference's bookkeeping (mnIterations, mnBestInliers,
// bNoMore, bConverge), so that  while(!bConverge && !bNoMore) solver.iterate(20, ...)  (src/LoopClosing.cc:710-714) costs one launch.
// The index triples come from sim3_draw_triples (the reference draws them with libc rand): SetSeed() selects the stream and
// restarts the walk; the default depends on the two key-frame ids only, so a run is reproducible.  More than
// SIM3_MAX_HYPOTHESES (1024) iterations after SetRansacParameters (the reference's default is 300) are refused with
// orbslam3_hip::Error(ORBX_ERR_CAPACITY) at the first iterate.
template <class Ref = Sim3Solver>
class Sim3SolverHIPT {
public:
    typedef Eigen::Matrix<float, 4, 4> Matrix4;

    Sim3SolverHIPT(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale = true,
                   std::vector<KeyFrame*> vpKeyFrameMatchedMP = std::vector<KeyFrame*>())
        : mnIterations(0), mnBestInliers(0), mbFixScale(bFixScale)
    {
        reset_best();                                   // every coefficient written: Eigen does not zero a default-constructed matrix
        bool pinhole = loop_detail::single_pinhole(pKF1) && loop_detail::single_pinhole(pKF2);
        for (KeyFrame* k : vpKeyFrameMatchedMP) pinhole = pinhole && k && loop_detail::single_pinhole(k);
        if (!pinhole) { ref_.reset(new Ref(pKF1, pKF2, vpMatched12, bFixScale, vpKeyFrameMatchedMP)); return; }
        bool bDifferentKFs = false;                                                     // :40-45
        if (vpKeyFrameMatchedMP.empty()) { bDifferentKFs = true; vpKeyFrameMatchedMP = std::vector<KeyFrame*>(vpMatched12.size(), pKF2); }
        const std::vector<MapPoint*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        mN1 = (int)vpMatched12.size();
        const Sophus::SE3f T1 = pKF1->GetPose(), T2 = pKF2->GetPose();                  // GetRotation() / GetTranslation() (:61-64)
        const Eigen::Matrix3f Rcw1 = T1.rotationMatrix(), Rcw2 = T2.rotationMatrix();
        const Eigen::Vector3f tcw1 = T1.translation(), tcw2 = T2.translation();
        KeyFrame* pKFm = pKF2;
        for (int i1 = 0; i1 < mN1; i1++) {
            if (!vpMatched12[i1]) continue;
            MapPoint* pMP1 = vpKeyFrameMP1[i1];
            MapPoint* pMP2 = vpMatched12[i1];
            if (!pMP1) continue;                                                        // :78-79
            if (pMP1->isBad() || pMP2->isBad()) continue;                               // :81-82
            if (bDifferentKFs) pKFm = vpKeyFrameMatchedMP[i1];                          // :84-85
            const int indexKF1 = std::get<0>(pMP1->GetIndexInKeyFrame(pKF1));
            const int indexKF2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKFm));
            if (indexKF1 < 0 || indexKF2 < 0) continue;                                 // :90-91
            const cv::KeyPoint& kp1 = pKF1->mvKeysUn[indexKF1];
            const cv::KeyPoint& kp2 = pKFm->mvKeysUn[indexKF2];
            const float sigmaSquare1 = pKF1->mvLevelSigma2[kp1.octave];
            const float sigmaSquare2 = pKFm->mvLevelSigma2[kp2.octave];
            max_err1_.push_back((float)(size_t)(9.210 * sigmaSquare1));                 // mvnMaxError1 is a vector<size_t> (:99, Sim3Solver.h:78)
            max_err2_.push_back((float)(size_t)(9.210 * sigmaSquare2));
            mvnIndices1.push_back((size_t)i1);
            const Eigen::Vector3f X1 = Rcw1 * pMP1->GetWorldPos() + tcw1;               // :106-110
            const Eigen::Vector3f X2 = Rcw2 * pMP2->GetWorldPos() + tcw2;
            for (int k = 0; k < 3; k++) { X1c_.push_back(X1[k]); X2c_.push_back(X2[k]); }
        }
        loop_detail::intrinsics(pKF1, K1_);                                             // pCamera1 / pCamera2 (:38)
        loop_detail::intrinsics(pKF2, K2_);
        seed_ = 0x5EEDull ^ ((uint64_t)pKF1->mnId * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)pKF2->mnId << 32);
        SetRansacParameters();                                                          // :120
    }

    // another triple stream: the hypotheses are evaluated again and the walk starts over (mnIterations, mnBestInliers and the best
    // estimate are reset), whenever it is called
    void SetSeed(uint64_t seed) { seed_ = seed; launched_ = false; mnIterations = 0; mnBestInliers = 0; reset_best(); }

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)    // :123-147
    {
        if (ref_) { ref_->SetRansacParameters(probability, minInliers, maxIterations); return; }
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        mRansacMaxIts = maxIterations;
        N = (int)mvnIndices1.size();
        int nIterations = 1;
        if (N > 0 && mRansacMinInliers != N) {
            const float epsilon = (float)mRansacMinInliers / N;
            const double it = std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow(epsilon, 3)));
            nIterations = (it == it && it < 2147483647.0 && it > -2147483648.0) ? (int)it : mRansacMaxIts;   // epsilon >= 1: log of <= 0
        }
        mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
        mnIterations = 0;
        launched_ = false;
    }

    Matrix4 find(std::vector<bool>& vbInliers12, int& nInliers)                         // :296-300
    {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
    }

    Matrix4 iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)        // :149-216
    {
        if (ref_) return ref_->iterate(nIterations, bNoMore, vbInliers, nInliers);
        bool bConverge;
        const Matrix4 T = walk(nIterations, bNoMore, vbInliers, nInliers, bConverge);
        return bConverge ? T : identity();
    }

    // without convergence the reference returns bestSim3, which it only sets when a hypothesis of THIS call reached the
    // best count (:283-286) and leaves uninitialised otherwise; here that case returns the best transformation so far
    Matrix4 iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge)  // :218-294
    {
        if (ref_) return ref_->iterate(nIterations, bNoMore, vbInliers, nInliers, bConverge);
        return walk(nIterations, bNoMore, vbInliers, nInliers, bConverge);
    }

    Matrix4 GetEstimatedTransformation() { return ref_ ? ref_->GetEstimatedTransformation() : mBestT12; }
    Eigen::Matrix3f GetEstimatedRotation() { return ref_ ? ref_->GetEstimatedRotation() : mBestRotation; }
    Eigen::Vector3f GetEstimatedTranslation() { return ref_ ? ref_->GetEstimatedTranslation() : mBestTranslation; }
    float GetEstimatedScale() { return ref_ ? ref_->GetEstimatedScale() : mBestScale; }

    // TEST HOOKS, not part of the reference's interface: the flattened problem as handed to sim3_ransac_batch (the triples are
    // sim3_draw_triples(Seed(), Correspondences(), Hypotheses())), read by tests/stubs/shim_loop_toy.cpp
    int Correspondences() const { return N; }
    int Hypotheses() const { return mRansacMaxIts; }
    uint64_t Seed() const { return seed_; }
    const std::vector<size_t>& Indices1() const { return mvnIndices1; }
    const std::vector<float>& X3Dc1() const { return X1c_; }
    const std::vector<float>& X3Dc2() const { return X2c_; }
    const std::vector<float>& MaxError1() const { return max_err1_; }
    const std::vector<float>& MaxError2() const { return max_err2_; }
    bool UsesReference() const { return (bool)ref_; }

private:
    static Matrix4 identity()                           // Eigen::Matrix4f::Identity() (:158, :215), all sixteen coefficients written
    {
        Matrix4 I;
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) I(r, c) = r == c ? 1.f : 0.f;
        return I;
    }

    void reset_best()
    {
        mBestT12 = identity();
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) mBestRotation(r, c) = r == c ? 1.f : 0.f;
            mBestTranslation[r] = 0.f;
        }
        mBestScale = 1.f;
    }

    bool launch()
    {
        const int H = mRansacMaxIts;
        triples_.assign((size_t)3 * H, 0);
        count_.assign(H, 0); T12_.assign((size_t)13 * H, 0.f);
        words_ = (N + 63) / 64;
        mask_.assign((size_t)H * words_, 0);
        orbslam3_hip::check(sim3_draw_triples(seed_, N, H, triples_.data()));
        Sim3RansacProblem p;
        p.n = N; p.X1c = X1c_.data(); p.X2c = X2c_.data(); p.max_err1 = max_err1_.data(); p.max_err2 = max_err2_.data();
        p.fx1 = K1_[0]; p.fy1 = K1_[1]; p.cx1 = K1_[2]; p.cy1 = K1_[3];
        p.fx2 = K2_[0]; p.fy2 = K2_[1]; p.cx2 = K2_[2]; p.cy2 = K2_[3];
        p.fix_scale = mbFixScale ? 1 : 0; p.min_inliers = mRansacMinInliers; p.n_hyp = H; p.triples = triples_.data();
        Sim3RansacResult r;
        r.converged = 0; r.index = -1; r.scored = 0;
        r.count = count_.data(); r.T12 = T12_.data(); r.mask = mask_.data();
        orbslam3_hip::check(sim3_ransac_batch(loop_detail::solver(), &p, 1, &r));
        launched_ = true;
        return r.scored != 0;
    }

    void set_best(int h)                                                                // :194-199 / :267-272
    {
        const float* o = T12_.data() + (size_t)13 * h;
        mBestScale = o[12];
        mBestT12 = identity();
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) { mBestRotation(r, c) = o[3 * r + c]; mBestT12(r, c) = o[12] * o[3 * r + c]; }      // sR (:398-399)
            mBestTranslation[r] = o[9 + r];
            mBestT12(r, 3) = o[9 + r];
        }
    }

    Matrix4 walk(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, bool& bConverge)
    {
        bNoMore = false;
        bConverge = false;
        vbInliers = std::vector<bool>(mN1, false);
        nInliers = 0;
        if (N < mRansacMinInliers || N < 3) { bNoMore = true; return identity(); }      // :155-159 (three points are needed to draw)
        if (mRansacMaxIts > SIM3_MAX_HYPOTHESES) throw orbslam3_hip::Error(ORBX_ERR_CAPACITY);
        if (!launched_ && !launch()) { bNoMore = true; return identity(); }
        int nCurrentIterations = 0;
        while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
            const int h = mnIterations;
            nCurrentIterations++;
            mnIterations++;
            const int mnInliersi = count_[h];
            if (mnInliersi >= mnBestInliers) {
                mnBestInliers = mnInliersi;
                set_best(h);
                if (mnInliersi > mRansacMinInliers) {
                    nInliers = mnInliersi;
                    const uint64_t* m = mask_.data() + (size_t)h * words_;
                    for (int i = 0; i < N; i++)
                        if ((m[i >> 6] >> (i & 63)) & 1) vbInliers[mvnIndices1[i]] = true;
                    bConverge = true;
                    return mBestT12;
                }
            }
        }
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return mBestT12;
    }

    std::unique_ptr<Ref> ref_;          // the reference solver, for camera models outside the accelerated path
    std::vector<size_t> mvnIndices1;
    std::vector<float> X1c_, X2c_, max_err1_, max_err2_;
    float K1_[4] = {0, 0, 0, 0}, K2_[4] = {0, 0, 0, 0};
    int N = 0, mN1 = 0;
    int mnIterations, mnBestInliers;
    bool mbFixScale;
    Matrix4 mBestT12;
    Eigen::Matrix3f mBestRotation;
    Eigen::Vector3f mBestTranslation;
    float mBestScale = 1.f;
    double mRansacProb = 0.99;
    int mRansacMinInliers = 6, mRansacMaxIts = 300;
    uint64_t seed_ = 0;
    bool launched_ = false;
    int words_ = 0;
    std::vector<int32_t> triples_, count_;
    std::vector<float> T12_;
    std::vector<uint64_t> mask_;
};
typedef Sim3SolverHIPT<> Sim3SolverHIP;

// int Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, mAcumHessian, bAllPoints) (src/Optimizer.cc:2115-2381).
// Sim3T = g2o::Sim3 (rotation(), translation(), scale(), Sim3(Quaterniond, Vector3d, double)), Hessian = Eigen::Matrix<double,7,7>;
// Opt = the class whose OptimizeSim3 serves camera models outside the accelerated path.
template <class Opt = Optimizer, class Sim3T, class Hessian>
int OptimizeSim3HIP(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, Sim3T& g2oS12, const float th2, const bool bFixScale,
                    Hessian& mAcumHessian, const bool bAllPoints = false)
{
    if (!loop_detail::single_pinhole(pKF1) || !loop_detail::single_pinhole(pKF2))
        return Opt::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale, mAcumHessian, bAllPoints);
    const Sophus::SE3f T1 = pKF1->GetPose(), T2 = pKF2->GetPose();                      // :2129-2132
    const Eigen::Matrix3f R1w = T1.rotationMatrix(), R2w = T2.rotationMatrix();
    const Eigen::Vector3f t1w = T1.translation(), t2w = T2.translation();
    const int N = (int)vpMatches1.size();
    const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
    std::vector<double> X1, X2, o1, o2, w1, w2;
    std::vector<size_t> vnIndexEdge;
    for (int i = 0; i < N; i++) {
        if (!vpMatches1[i]) continue;
        MapPoint* pMP1 = vpMapPoints1[i];
        MapPoint* pMP2 = vpMatches1[i];
        const int i2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKF2));                     // :2178
        if (!pMP1) continue;                                                            // :2209-2227: a vertex without an edge
        if (pMP1->isBad() || pMP2->isBad()) continue;                                   // :2203-2207
        const Eigen::Vector3f P3D1c = R1w * pMP1->GetWorldPos() + t1w;                  // :2188-2198
        const Eigen::Vector3f P3D2c = R2w * pMP2->GetWorldPos() + t2w;
        if (i2 < 0 && !bAllPoints) continue;                                            // :2229-2233
        if (P3D2c(2) < 0) continue;                                                     // :2235-2239
        const cv::KeyPoint& kpUn1 = pKF1->mvKeysUn[i];                                  // :2244-2254
        o1.push_back(kpUn1.pt.x); o1.push_back(kpUn1.pt.y);
        w1.push_back((double)pKF1->mvInvLevelSigma2[kpUn1.octave]);
        int octave2;
        if (i2 >= 0) {                                                                  // :2265-2272
            const cv::KeyPoint& kpUn2 = pKF2->mvKeysUn[i2];
            o2.push_back(kpUn2.pt.x); o2.push_back(kpUn2.pt.y);
            octave2 = kpUn2.octave;
        } else {                                                                        // :2273-2284: normalised coordinates, in float
            const float invz = 1 / P3D2c(2);
            const float x = P3D2c(0) * invz;
            const float y = P3D2c(1) * invz;
            o2.push_back(x); o2.push_back(y);
            octave2 = pMP2->mnTrackScaleLevel;
        }
        w2.push_back((double)pKF2->mvInvLevelSigma2[octave2]);                          // :2291-2292
        for (int k = 0; k < 3; k++) { X1.push_back((double)P3D1c(k)); X2.push_back((double)P3D2c(k)); }
        vnIndexEdge.push_back((size_t)i);
    }
    Sim3OptProblem p;
    const Eigen::Quaterniond q = g2oS12.rotation();
    const Eigen::Vector3d t = g2oS12.translation();
    p.q[0] = q.x(); p.q[1] = q.y(); p.q[2] = q.z(); p.q[3] = q.w();
    p.t[0] = t[0]; p.t[1] = t[1]; p.t[2] = t[2];
    p.s = g2oS12.scale();
    p.n = (int)vnIndexEdge.size();
    p.X1c = X1.data(); p.X2c = X2.data(); p.obs1 = o1.data(); p.obs2 = o2.data(); p.inv_sigma2_1 = w1.data(); p.inv_sigma2_2 = w2.data();
    float K1[4], K2[4];
    loop_detail::intrinsics(pKF1, K1);                                                  // vSim3->pCamera1 / pCamera2 (:2140-2141)
    loop_detail::intrinsics(pKF2, K2);
    p.fx1 = K1[0]; p.fy1 = K1[1]; p.cx1 = K1[2]; p.cy1 = K1[3];
    p.fx2 = K2[0]; p.fy2 = K2[1]; p.cx2 = K2[2]; p.cy2 = K2[3];
    const float deltaHuber = std::sqrt(th2);                                            // :2157
    p.th2 = (double)th2; p.huber_delta = (double)deltaHuber; p.fix_scale = bFixScale ? 1 : 0;
    Sim3OptResult res;
    std::vector<uint8_t> keep(vnIndexEdge.size() + 1, 1);
    uint8_t* keep_ptr[1] = {keep.data()};
    orbslam3_hip::check(sim3_optimize_batch(loop_detail::solver(), &p, 1, &res, keep_ptr));
    for (size_t k = 0; k < vnIndexEdge.size(); k++)
        if (!keep[k]) vpMatches1[vnIndexEdge[k]] = static_cast<MapPoint*>(NULL);        // :2323, :2369
    if (p.n - res.n_bad < 10) return 0;                                                 // :2348-2349: g2oS12 and mAcumHessian untouched
    for (int r = 0; r < 7; r++)
        for (int c = 0; c < 7; c++) mAcumHessian(r, c) = 0.0;                           // :2356 (the reference only zeroes it)
    g2oS12 = Sim3T(Eigen::Quaterniond(res.q[3], res.q[0], res.q[1], res.q[2]), Eigen::Vector3d(res.t[0], res.t[1], res.t[2]), res.s);   // :2377-2378
    return res.n_in;
}


// ---- Optimizer::OptimizeEssentialGraph, both overloads (src/Optimizer.cc:1501-1783, :1785-2113), on essg_optimize ----
// The adapters walk the graph as the reference does and hand it over as arrays (EssentialGraphFlat); the walk is separate from
// the call so that it can be checked without a device (tests/stubs/shim_essential_toy.cpp).  KF / MP / MapT are the reference's
// KeyFrame / MapPoint / Map (template parameters, so that the stand-ins of the tests can add the members they lack by
// derivation); Sim3T = g2o::Sim3; PoseMap = LoopClosing::KeyFrameAndPose; Opt = the class whose OptimizeEssentialGraph serves what
// the device does not: invalid input (ORBX_ERR_ARG), more than ESSG_MAX_FREE_VERTICES free key frames (ORBX_ERR_CAPACITY).
// OptimizeEssentialGraph4DoF, which LoopClosing::CorrectLoop calls instead once the map's IMU is initialised (src/LoopClosing.cc:1182),
// is a different graph (yaw + translation vertices, Edge4DoF): OptimizeEssentialGraph4DoFHIP at the end of this file, on essg_optimize_4dof.
struct EssentialGraphFlat {
    std::vector<long unsigned int> id;      // mnId per vertex, in the order the reference adds them
    std::vector<double> sim3;               // [8] per vertex: q x y z w, t, s
    std::vector<uint8_t> fixed;
    std::vector<int32_t> edges;             // [2] per edge: vertex 0 (nIDi), vertex 1 (nIDj), as indices into id
    std::vector<double> meas;               // [8] per edge: Sji
    std::vector<float> points;              // loop overload: GetWorldPos() of every map point that is not bad
    std::vector<int32_t> point_ref;
    std::vector<size_t> point_index;        // its index in GetAllMapPoints()
    int dropped_edges = 0;                  // edges g2o's addEdge refuses because a vertex is missing (a bad key frame)
    int fix_scale = 0;
};

namespace essential_detail {

struct S8 { double v[8]; };     // q x y z w, t, s

inline S8 identity() { S8 a; for (int i = 0; i < 8; i++) a.v[i] = (i == 3 || i == 7) ? 1.0 : 0.0; return a; }
inline void rotate(const double* q, const double* p, double* o)         // Eigen's quaternion * vector
{
    const double ux = 2 * (q[1] * p[2] - q[2] * p[1]), uy = 2 * (q[2] * p[0] - q[0] * p[2]), uz = 2 * (q[0] * p[1] - q[1] * p[0]);
    o[0] = p[0] + q[3] * ux + (q[1] * uz - q[2] * uy);
    o[1] = p[1] + q[3] * uy + (q[2] * ux - q[0] * uz);
    o[2] = p[2] + q[3] * uz + (q[0] * uy - q[1] * ux);
}
inline S8 mul(const S8& a, const S8& b)                                  // g2o::Sim3::operator* (sim3.h:266-272)
{
    S8 o;
    double rt[3];
    rotate(a.v, b.v + 4, rt);
    o.v[3] = a.v[3] * b.v[3] - a.v[0] * b.v[0] - a.v[1] * b.v[1] - a.v[2] * b.v[2];
    o.v[0] = a.v[3] * b.v[0] + a.v[0] * b.v[3] + a.v[1] * b.v[2] - a.v[2] * b.v[1];
    o.v[1] = a.v[3] * b.v[1] + a.v[1] * b.v[3] + a.v[2] * b.v[0] - a.v[0] * b.v[2];
    o.v[2] = a.v[3] * b.v[2] + a.v[2] * b.v[3] + a.v[0] * b.v[1] - a.v[1] * b.v[0];
    for (int i = 0; i < 3; i++) o.v[4 + i] = a.v[7] * rt[i] + a.v[4 + i];
    o.v[7] = a.v[7] * b.v[7];
    return o;
}
inline S8 inverse(const S8& a)                                           // g2o::Sim3::inverse (sim3.h:233-236)
{
    S8 o;
    const double m = -1. / a.v[7];
    const double t[3] = {m * a.v[4], m * a.v[5], m * a.v[6]};
    o.v[0] = -a.v[0]; o.v[1] = -a.v[1]; o.v[2] = -a.v[2]; o.v[3] = a.v[3];
    rotate(o.v, t, o.v + 4);
    o.v[7] = 1. / a.v[7];
    return o;
}
template <class Sim3T>
inline S8 from_sim3(const Sim3T& g)
{
    S8 a;
    const Eigen::Quaterniond q = g.rotation();
    const Eigen::Vector3d t = g.translation();
    a.v[0] = q.x(); a.v[1] = q.y(); a.v[2] = q.z(); a.v[3] = q.w();
    a.v[4] = t[0]; a.v[5] = t[1]; a.v[6] = t[2]; a.v[7] = g.scale();
    return a;
}
template <class KF>
inline S8 from_pose(KF* pKF)      // g2o::Sim3(Tcw.unit_quaternion(), Tcw.translation(), 1.0) of GetPose().cast<double>() (:1551-1552)
{
    const Sophus::SE3d Tcw = pKF->GetPose().template cast<double>();
    S8 a;
    const Eigen::Quaterniond q = Tcw.unit_quaternion();
    const Eigen::Vector3d t = Tcw.translation();
    a.v[0] = q.x(); a.v[1] = q.y(); a.v[2] = q.z(); a.v[3] = q.w();
    a.v[4] = t[0]; a.v[5] = t[1]; a.v[6] = t[2]; a.v[7] = 1.0;
    return a;
}

struct Builder {
    EssentialGraphFlat& g;
    std::map<long unsigned int, int> index;
    void vertex(long unsigned int id, const S8& s, bool fixed)
    {
        index[id] = (int)g.id.size();
        g.id.push_back(id);
        g.sim3.insert(g.sim3.end(), s.v, s.v + 8);
        g.fixed.push_back(fixed ? 1 : 0);
    }
    // optimizer.addEdge refuses an edge with a vertex the optimizer does not hold (hyper_graph.cpp: a NULL vertex)
    void edge(long unsigned int idi, long unsigned int idj, const S8& Sji)
    {
        const auto a = index.find(idi), b = index.find(idj);
        if (a == index.end() || b == index.end()) { g.dropped_edges++; return; }
        g.edges.push_back(a->second); g.edges.push_back(b->second);
        g.meas.insert(g.meas.end(), Sji.v, Sji.v + 8);
    }
};

inline essg_solver* solver() { return orbslam3_hip::thread_handle<essg_solver, essg_create>(); }

}  // namespace essential_detail

// the graph of the loop overload (:1517-1726).  Vertices: the key frames of the map that are not bad.  Edges: loop connections
// first, then per key frame the spanning-tree edge, its loop edges, its covisibility edges, the inertial edge.
template <class KF, class MP, class MapT, class PoseMap, class ConnMap>
void FlattenEssentialGraph(MapT* pMap, KF* pLoopKF, KF* pCurKF, const PoseMap& NonCorrectedSim3, const PoseMap& CorrectedSim3,
                           const ConnMap& LoopConnections, const bool bFixScale, EssentialGraphFlat& g)
{
    namespace ed = essential_detail;
    ed::Builder b{g, {}};
    g.fix_scale = bFixScale ? 1 : 0;
    const std::vector<KF*> vpKFs = pMap->GetAllKeyFrames();
    const std::vector<MP*> vpMPs = pMap->GetAllMapPoints();
    std::map<long unsigned int, ed::S8> vScw;
    const int minFeat = 100;
    for (KF* pKF : vpKFs) {                                                                 // :1533-1568
        if (pKF->isBad()) continue;
        const auto it = CorrectedSim3.find(pKF);
        const ed::S8 Siw = it != CorrectedSim3.end() ? ed::from_sim3(it->second) : ed::from_pose(pKF);
        vScw[pKF->mnId] = Siw;
        b.vertex(pKF->mnId, Siw, pKF->mnId == pMap->GetInitKFid());
    }
    auto scw = [&](long unsigned int id) { const auto it = vScw.find(id); return it != vScw.end() ? it->second : ed::identity(); };   // vScw is value-initialised (:1522)
    auto non_corrected = [&](KF* pKF) { const auto it = NonCorrectedSim3.find(pKF); return it != NonCorrectedSim3.end() ? ed::from_sim3(it->second) : scw(pKF->mnId); };
    std::set<std::pair<long unsigned int, long unsigned int> > sInsertedEdges;
    for (auto mit = LoopConnections.begin(); mit != LoopConnections.end(); ++mit) {         // :1577-1605
        KF* pKF = mit->first;
        const long unsigned int nIDi = pKF->mnId;
        const ed::S8 Swi = ed::inverse(scw(nIDi));
        for (KF* pKFj : mit->second) {
            const long unsigned int nIDj = pKFj->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(pKFj) < minFeat) continue;
            b.edge(nIDi, nIDj, ed::mul(scw(nIDj), Swi));
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }
    for (KF* pKF : vpKFs) {                                                                 // :1608-1726
        const long unsigned int nIDi = pKF->mnId;
        const ed::S8 Swi = ed::inverse(non_corrected(pKF));
        KF* pParentKF = pKF->GetParent();
        if (pParentKF) b.edge(nIDi, pParentKF->mnId, ed::mul(non_corrected(pParentKF), Swi));
        const std::set<KF*> sLoopEdges = pKF->GetLoopEdges();
        for (KF* pLKF : sLoopEdges)
            if (pLKF->mnId < pKF->mnId) b.edge(nIDi, pLKF->mnId, ed::mul(non_corrected(pLKF), Swi));
        const std::vector<KF*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
        for (KF* pKFn : vpConnectedKFs) {
            if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    b.edge(nIDi, pKFn->mnId, ed::mul(non_corrected(pKFn), Swi));
                }
            }
        }
        if (pKF->bImu && pKF->mPrevKF) b.edge(nIDi, pKF->mPrevKF->mnId, ed::mul(non_corrected(static_cast<KF*>(pKF->mPrevKF)), Swi));
    }
    for (size_t i = 0; i < vpMPs.size(); i++) {                                             // :1752-1769
        MP* pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        const long unsigned int nIDr = pMP->mnCorrectedByKF == pCurKF->mnId ? pMP->mnCorrectedReference : pMP->GetReferenceKeyFrame()->mnId;
        const auto it = b.index.find(nIDr);
        g.point_ref.push_back(it != b.index.end() ? it->second : -1);                       // -1: refused by essg_optimize, the reference decides
        const Eigen::Vector3f P = pMP->GetWorldPos();
        for (int k = 0; k < 3; k++) g.points.push_back(P[k]);
        g.point_index.push_back(i);
    }
}

// the graph of the merge overload (:1806-2051): three groups of vertices, _fix_scale on the first group only in the reference
// (the members of the other two are left at the constructor's value, false: types_seven_dof_expmap.cpp), relations between two
// "good" (corrected) or two "bad" (not yet corrected) poses only.
template <class KF>
void FlattenEssentialGraphMerge(KF* /*pCurKF*/, const std::vector<KF*>& vpFixedKFs, const std::vector<KF*>& vpFixedCorrectedKFs,
                                const std::vector<KF*>& vpNonFixedKFs, EssentialGraphFlat& g)
{
    namespace ed = essential_detail;
    ed::Builder b{g, {}};
    g.fix_scale = 0;
    std::map<long unsigned int, ed::S8> vScw, vCorrectedSwc;
    std::map<long unsigned int, bool> good, bad;
    const int minFeat = 100;
    for (KF* pKFi : vpFixedKFs) {                                                           // :1815-1842
        if (pKFi->isBad()) continue;
        const ed::S8 Siw = ed::from_pose(pKFi);
        vCorrectedSwc[pKFi->mnId] = ed::inverse(Siw);
        b.vertex(pKFi->mnId, Siw, true);
        good[pKFi->mnId] = true; bad[pKFi->mnId] = false;
    }
    std::set<unsigned long> sIdKF;
    for (KF* pKFi : vpFixedCorrectedKFs) {                                                  // :1846-1877
        if (pKFi->isBad()) continue;
        const ed::S8 Siw = ed::from_pose(pKFi);
        vCorrectedSwc[pKFi->mnId] = ed::inverse(Siw);
        const Sophus::SE3d Tb = pKFi->mTcwBefMerge.template cast<double>();
        ed::S8 Sb;
        const Eigen::Quaterniond q = Tb.unit_quaternion();
        const Eigen::Vector3d t = Tb.translation();
        Sb.v[0] = q.x(); Sb.v[1] = q.y(); Sb.v[2] = q.z(); Sb.v[3] = q.w(); Sb.v[4] = t[0]; Sb.v[5] = t[1]; Sb.v[6] = t[2]; Sb.v[7] = 1.0;
        vScw[pKFi->mnId] = Sb;
        b.vertex(pKFi->mnId, Siw, true);
        sIdKF.insert(pKFi->mnId);
        good[pKFi->mnId] = true; bad[pKFi->mnId] = true;
    }
    for (KF* pKFi : vpNonFixedKFs) {                                                        // :1879-1910
        if (pKFi->isBad()) continue;
        if (sIdKF.count(pKFi->mnId)) continue;
        const ed::S8 Siw = ed::from_pose(pKFi);
        vScw[pKFi->mnId] = Siw;
        b.vertex(pKFi->mnId, Siw, false);
        sIdKF.insert(pKFi->mnId);
        good[pKFi->mnId] = false; bad[pKFi->mnId] = true;
    }
    std::vector<KF*> vpKFs;
    vpKFs.insert(vpKFs.end(), vpFixedKFs.begin(), vpFixedKFs.end());
    vpKFs.insert(vpKFs.end(), vpFixedCorrectedKFs.begin(), vpFixedCorrectedKFs.end());
    vpKFs.insert(vpKFs.end(), vpNonFixedKFs.begin(), vpNonFixedKFs.end());
    const std::set<KF*> spKFs(vpKFs.begin(), vpKFs.end());
    auto get = [](const std::map<long unsigned int, ed::S8>& m, long unsigned int id) { const auto it = m.find(id); return it != m.end() ? it->second : ed::identity(); };
    auto flag = [](const std::map<long unsigned int, bool>& m, long unsigned int id) { const auto it = m.find(id); return it != m.end() && it->second; };
    // Sjw of a relation between i and j, or false (:1944-1953 and its two repetitions)
    auto relation = [&](long unsigned int i, long unsigned int j, ed::S8& Sjw) {
        if (flag(good, i) && flag(good, j)) { Sjw = ed::inverse(get(vCorrectedSwc, j)); return true; }
        if (flag(bad, i) && flag(bad, j)) { Sjw = get(vScw, j); return true; }
        return false;
    };
    for (KF* pKFi : vpKFs) {                                                                // :1921-2051
        const long unsigned int nIDi = pKFi->mnId;
        const ed::S8 Swi = flag(bad, nIDi) ? ed::inverse(get(vScw, nIDi)) : ed::identity();     // Swi stays default-constructed for a pose that is only "good" (:1927-1932)
        ed::S8 Sjw;
        KF* pParentKFi = pKFi->GetParent();
        if (pParentKFi && spKFs.count(pParentKFi) && relation(nIDi, pParentKFi->mnId, Sjw)) b.edge(nIDi, pParentKFi->mnId, ed::mul(Sjw, Swi));
        const std::set<KF*> sLoopEdges = pKFi->GetLoopEdges();
        for (KF* pLKF : sLoopEdges)
            if (spKFs.count(pLKF) && pLKF->mnId < pKFi->mnId && relation(nIDi, pLKF->mnId, Sjw)) b.edge(nIDi, pLKF->mnId, ed::mul(Sjw, Swi));
        const std::vector<KF*> vpConnectedKFs = pKFi->GetCovisiblesByWeight(minFeat);
        for (KF* pKFn : vpConnectedKFs) {
            if (pKFn && pKFn != pParentKFi && !pKFi->hasChild(pKFn) && !sLoopEdges.count(pKFn) && spKFs.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKFi->mnId && relation(nIDi, pKFn->mnId, Sjw)) b.edge(nIDi, pKFn->mnId, ed::mul(Sjw, Swi));
            }
        }
    }
}

namespace essential_detail {
// essg_optimize on a flattened graph; false when the device refuses it (invalid input, over capacity): the caller falls back
inline bool run(const EssentialGraphFlat& g, std::vector<double>& sim3_out, std::vector<float>& q, std::vector<float>& t, std::vector<float>& pts)
{
    EssgProblem p;
    p.n_vertices = (int32_t)g.id.size(); p.sim3 = g.sim3.data(); p.fixed = g.fixed.data();
    p.n_edges = (int32_t)(g.edges.size() / 2); p.edge_vertices = g.edges.data(); p.edge_measurement = g.meas.data();
    p.fix_scale = g.fix_scale; p.max_iters = 20; p.lambda_init = 1e-16;
    p.n_points = (int32_t)g.point_ref.size(); p.points = g.points.data(); p.point_ref = g.point_ref.data();
    sim3_out.assign(g.sim3.size(), 0.0); q.assign(4 * g.id.size(), 0.f); t.assign(3 * g.id.size(), 0.f); pts.assign(g.points.size() + 3, 0.f);
    EssgResult r;
    r.sim3_out = sim3_out.data(); r.pose_q = q.data(); r.pose_t = t.data(); r.points_out = pts.data();
    const int ok = essg_check(&p, &r);                  // before a handle (and with it a device) is asked for
    if (ok == ORBX_ERR_ARG || ok == ORBX_ERR_CAPACITY) return false;
    orbslam3_hip::check(essg_optimize(solver(), &p, &r, nullptr));
    return true;
}
}  // namespace essential_detail

// void Optimizer::OptimizeEssentialGraph(Map*, KeyFrame* pLoopKF, KeyFrame* pCurKF, const KeyFrameAndPose& NonCorrectedSim3,
//                                        const KeyFrameAndPose& CorrectedSim3, const map<KeyFrame*, set<KeyFrame*>>&, const bool&)
template <class Opt = Optimizer, class KF, class MapT, class PoseMap, class ConnMap>
void OptimizeEssentialGraphHIP(MapT* pMap, KF* pLoopKF, KF* pCurKF, const PoseMap& NonCorrectedSim3, const PoseMap& CorrectedSim3,
                               const ConnMap& LoopConnections, const bool& bFixScale)
{
    typedef typename std::remove_pointer<typename decltype(pMap->GetAllMapPoints())::value_type>::type MP;
    EssentialGraphFlat g;
    FlattenEssentialGraph<KF, MP>(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale, g);
    std::vector<double> sim3_out;
    std::vector<float> q, t, pts;
    if (g.dropped_edges > 0 || !essential_detail::run(g, sim3_out, q, t, pts)) {
        Opt::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale);
        return;
    }
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                               // :1733
    const std::vector<KF*> vpKFs = pMap->GetAllKeyFrames();
    std::map<long unsigned int, int> index;
    for (size_t k = 0; k < g.id.size(); k++) index[g.id[k]] = (int)k;
    for (KF* pKFi : vpKFs) {                                                                // :1736-1749
        const auto it = index.find(pKFi->mnId);
        if (it == index.end()) continue;
        const int k = it->second;
        pKFi->SetPose(Sophus::SE3f(Eigen::Quaternionf(q[4 * k + 3], q[4 * k], q[4 * k + 1], q[4 * k + 2]), Eigen::Vector3f(t[3 * k], t[3 * k + 1], t[3 * k + 2])));
    }
    const std::vector<MP*> vpMPs = pMap->GetAllMapPoints();
    for (size_t k = 0; k < g.point_index.size(); k++) {                                     // :1752-1779
        MP* pMP = vpMPs[g.point_index[k]];
        pMP->SetWorldPos(Eigen::Vector3f(pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]));
        pMP->UpdateNormalAndDepth();
    }
    pMap->IncreaseChangeIndex();                                                            // :1782
}

// void Optimizer::OptimizeEssentialGraph(KeyFrame* pCurKF, vector<KeyFrame*>& vpFixedKFs, vector<KeyFrame*>& vpFixedCorrectedKFs,
//                                        vector<KeyFrame*>& vpNonFixedKFs, vector<MapPoint*>& vpNonCorrectedMPs)
template <class Opt = Optimizer, class KF, class MP>
void OptimizeEssentialGraphHIP(KF* pCurKF, std::vector<KF*>& vpFixedKFs, std::vector<KF*>& vpFixedCorrectedKFs, std::vector<KF*>& vpNonFixedKFs,
                               std::vector<MP*>& vpNonCorrectedMPs)
{
    EssentialGraphFlat g;
    FlattenEssentialGraphMerge(pCurKF, vpFixedKFs, vpFixedCorrectedKFs, vpNonFixedKFs, g);
    std::vector<double> s;
    std::vector<float> q, t, pts;
    if (g.dropped_edges > 0 || !essential_detail::run(g, s, q, t, pts)) {
        Opt::OptimizeEssentialGraph(pCurKF, vpFixedKFs, vpFixedCorrectedKFs, vpNonFixedKFs, vpNonCorrectedMPs);
        return;
    }
    std::unique_lock<std::mutex> lock(pCurKF->GetMap()->mMutexMapUpdate);                   // :2057
    std::map<long unsigned int, int> index;
    std::map<long unsigned int, bool> bad;
    for (size_t k = 0; k < g.id.size(); k++) index[g.id[k]] = (int)k;
    for (KF* pKFi : vpFixedCorrectedKFs) if (!pKFi->isBad()) bad[pKFi->mnId] = true;
    for (KF* pKFi : vpNonFixedKFs) {                                                        // :2060-2076: [R | t / s] in double, then to float
        if (pKFi->isBad()) continue;
        bad[pKFi->mnId] = true;
        const double* e = s.data() + 8 * (size_t)index[pKFi->mnId];
        const Sophus::SE3d Tiw(Eigen::Quaterniond(e[3], e[0], e[1], e[2]), Eigen::Vector3d(e[4], e[5], e[6]) / e[7]);
        pKFi->mTcwBefMerge = pKFi->GetPose();
        pKFi->mTwcBefMerge = pKFi->GetPoseInverse();
        pKFi->SetPose(Tiw.template cast<float>());
    }
    for (MP* pMPi : vpNonCorrectedMPs) {                                                    // :2079-2112, in float on the host as there
        if (pMPi->isBad()) continue;
        KF* pRefKF = static_cast<KF*>(pMPi->GetReferenceKeyFrame());
        while (pRefKF && pRefKF->isBad()) { pMPi->EraseObservation(pRefKF); pRefKF = static_cast<KF*>(pMPi->GetReferenceKeyFrame()); }
        if (!pRefKF || !bad.count(pRefKF->mnId)) continue;
        const Sophus::SE3f TNonCorrectedwr = pRefKF->mTwcBefMerge, Twr = pRefKF->GetPoseInverse();
        pMPi->SetWorldPos(Twr * (TNonCorrectedwr.inverse() * pMPi->GetWorldPos()));
        pMPi->UpdateNormalAndDepth();
    }
}

// ---- Optimizer::OptimizeEssentialGraph4DoF (src/Optimizer.cc:5292-5588), the pose graph of an inertial map, on essg_optimize_4dof ----
// Same split as above: FlattenEssentialGraph4DoF walks the graph as the reference does (host only, checked without a device by
// tests/stubs/shim_essential4dof_toy.cpp), OptimizeEssentialGraph4DoFHIP calls the device and writes the map back.  KF needs, besides
// what the Sim3 walk uses, mPrevKF, mNextKF, mImuCalib, GetImuRotation and GetImuPosition.  Opt = the class whose
// OptimizeEssentialGraph4DoF serves what the device does not: an edge g2o would have refused (a bad key frame has no vertex), input
// essg_check_4dof refuses (ORBX_ERR_ARG), more than ESSG_MAX_FREE_VERTICES free key frames (ORBX_ERR_CAPACITY).
struct EssentialGraph4DoFFlat {
    std::vector<long unsigned int> id;      // mnId per vertex, in the order the reference adds them
    std::vector<double> rcw, tcw, rwb, twb, rcb, tcb;   // [9] row-major / [3] per vertex: the ImuCamPose as its constructor leaves it
    std::vector<double> scw;                // [8] per vertex: vScw as q x y z w, t, s (a CorrectedSim3 entry keeps its scale here)
    std::vector<uint8_t> fixed;
    std::vector<int32_t> edges;             // [2] per edge: vertex 0 (nIDi), vertex 1 (nIDj), as indices into id
    std::vector<double> edge_rot, edge_trans;   // [9], [3] per edge: rotation and translation of Sij = Siw * Sjw^-1
    std::vector<float> points;              // GetWorldPos() of every map point that is not bad
    std::vector<int32_t> point_ref;
    std::vector<size_t> point_index;        // its index in GetAllMapPoints()
    int dropped_edges = 0;                  // edges g2o's addEdge refuses because a vertex is missing (a bad key frame)
};

namespace essential_detail {

inline void to_matrix(const double* q, double* R)                       // Eigen's QuaternionBase::toRotationMatrix, row-major
{
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}
template <class M> inline void put9(const M& m, std::vector<double>& out) { for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) out.push_back((double)m(r, c)); }
template <class V> inline void put3(const V& v, std::vector<double>& out) { for (int k = 0; k < 3; k++) out.push_back((double)v[k]); }

struct Builder4DoF {
    EssentialGraph4DoFFlat& g;
    std::map<long unsigned int, int> index;
    // VertexPose4DoF(pKF): ImuCamPose(KeyFrame*) (src/G2oTypes.cc:25-71), every member read from the key frame's float members
    // (GetRotation / GetTranslation return the rotation and translation of the pose GetPose returns)
    template <class KF>
    void vertex_from_key_frame(KF* pKF, bool fixed)
    {
        const Sophus::SE3f Tcw = pKF->GetPose();
        put9(Tcw.rotationMatrix(), g.rcw); put3(Tcw.translation(), g.tcw);
        put9(pKF->GetImuRotation(), g.rwb); put3(pKF->GetImuPosition(), g.twb);
        finish(pKF, fixed, from_pose(pKF));
    }
    // VertexPose4DoF(Rwc, twc, pKF) with Rwc, twc of Scw.inverse(), the scale dropped: ImuCamPose(Rwc, twc, pKF) (:121-146) in double
    template <class KF>
    void vertex_from_sim3(KF* pKF, bool fixed, const S8& Scw)
    {
        const S8 Swc = inverse(Scw);
        double Rwc[9], Rcb[9], tcb[3];
        to_matrix(Swc.v, Rwc);
        const double* twc = Swc.v + 4;
        const Eigen::Matrix3f Rcbf = pKF->mImuCalib.mTcb.rotationMatrix();
        const Eigen::Vector3f tcbf = pKF->mImuCalib.mTcb.translation();
        for (int r = 0; r < 3; r++) { tcb[r] = (double)tcbf[r]; for (int c = 0; c < 3; c++) Rcb[3 * r + c] = (double)Rcbf(r, c); }
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) {
                g.rcw.push_back(Rwc[3 * c + r]);                                                                            // Rcw = Rwc^T
                g.rwb.push_back(Rwc[3 * r] * Rcb[c] + Rwc[3 * r + 1] * Rcb[3 + c] + Rwc[3 * r + 2] * Rcb[6 + c]);           // Rwb = Rwc Rcb
            }
        for (int r = 0; r < 3; r++) {
            g.tcw.push_back(-(Rwc[r] * twc[0] + Rwc[3 + r] * twc[1] + Rwc[6 + r] * twc[2]));                                // tcw = -Rcw twc
            g.twb.push_back((Rwc[3 * r] * tcb[0] + Rwc[3 * r + 1] * tcb[1] + Rwc[3 * r + 2] * tcb[2]) + twc[r]);            // twb = Rwc tcb + twc
        }
        finish(pKF, fixed, Scw);
    }
    template <class KF>
    void finish(KF* pKF, bool fixed, const S8& Scw)
    {
        put9(pKF->mImuCalib.mTcb.rotationMatrix(), g.rcb); put3(pKF->mImuCalib.mTcb.translation(), g.tcb);
        index[pKF->mnId] = (int)g.id.size();
        g.id.push_back(pKF->mnId);
        g.scw.insert(g.scw.end(), Scw.v, Scw.v + 8);
        g.fixed.push_back(fixed ? 1 : 0);
    }
    // Edge4DoF(Tij) with Tij the rotation and the translation of Sij (the scale of the product stays inside its translation, as
    // g2o::Sim3::operator* leaves it); optimizer.addEdge refuses an edge with a vertex the optimizer does not hold
    void edge(long unsigned int idi, long unsigned int idj, const S8& Sij)
    {
        const auto a = index.find(idi), b = index.find(idj);
        if (a == index.end() || b == index.end()) { g.dropped_edges++; return; }
        g.edges.push_back(a->second); g.edges.push_back(b->second);
        double R[9];
        to_matrix(Sij.v, R);
        g.edge_rot.insert(g.edge_rot.end(), R, R + 9);
        g.edge_trans.insert(g.edge_trans.end(), Sij.v + 4, Sij.v + 7);
    }
};

}  // namespace essential_detail

// the graph (:5322-5539).  Vertices: the key frames of the map that are not bad, pLoopKF alone fixed.  Edges: loop connections
// first, then per key frame the inertial edge to mPrevKF, its loop edges, its covisibility edges.  pParentKF is NULL in the
// reference (:5420): there is no spanning-tree edge, and no covisible key frame is excluded for being the parent.
template <class KF, class MP, class MapT, class PoseMap, class ConnMap>
void FlattenEssentialGraph4DoF(MapT* pMap, KF* pLoopKF, KF* pCurKF, const PoseMap& NonCorrectedSim3, const PoseMap& CorrectedSim3,
                               const ConnMap& LoopConnections, EssentialGraph4DoFFlat& g)
{
    namespace ed = essential_detail;
    ed::Builder4DoF b{g, {}};
    const std::vector<KF*> vpKFs = pMap->GetAllKeyFrames();
    const std::vector<MP*> vpMPs = pMap->GetAllMapPoints();
    std::map<long unsigned int, ed::S8> vScw;
    const int minFeat = 100;
    for (KF* pKF : vpKFs) {                                                                 // :5322-5359
        if (pKF->isBad()) continue;
        const auto it = CorrectedSim3.find(pKF);
        if (it != CorrectedSim3.end()) {
            vScw[pKF->mnId] = ed::from_sim3(it->second);
            b.vertex_from_sim3(pKF, pKF == pLoopKF, vScw[pKF->mnId]);
        } else {
            vScw[pKF->mnId] = ed::from_pose(pKF);
            b.vertex_from_key_frame(pKF, pKF == pLoopKF);
        }
    }
    auto scw = [&](long unsigned int id) { const auto it = vScw.find(id); return it != vScw.end() ? it->second : ed::identity(); };   // vScw is value-initialised (:5315)
    auto non_corrected = [&](KF* pKF) { const auto it = NonCorrectedSim3.find(pKF); return it != NonCorrectedSim3.end() ? ed::from_sim3(it->second) : scw(pKF->mnId); };
    std::set<std::pair<long unsigned int, long unsigned int> > sInsertedEdges;
    for (auto mit = LoopConnections.begin(); mit != LoopConnections.end(); ++mit) {         // :5370-5400
        KF* pKF = mit->first;
        const long unsigned int nIDi = pKF->mnId;
        const ed::S8 Siw = scw(nIDi);
        for (KF* pKFj : mit->second) {
            const long unsigned int nIDj = pKFj->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(pKFj) < minFeat) continue;
            b.edge(nIDi, nIDj, ed::mul(Siw, ed::inverse(scw(nIDj))));
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }
    for (KF* pKF : vpKFs) {                                                                 // :5403-5539
        const long unsigned int nIDi = pKF->mnId;
        const ed::S8 Siw = non_corrected(pKF);
        KF* prevKF = static_cast<KF*>(pKF->mPrevKF);
        if (prevKF) b.edge(nIDi, prevKF->mnId, ed::mul(Siw, ed::inverse(non_corrected(prevKF))));
        const std::set<KF*> sLoopEdges = pKF->GetLoopEdges();
        for (KF* pLKF : sLoopEdges)
            if (pLKF->mnId < pKF->mnId) b.edge(nIDi, pLKF->mnId, ed::mul(Siw, ed::inverse(non_corrected(pLKF))));
        const std::vector<KF*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);
        for (KF* pKFn : vpConnectedKFs) {
            if (pKFn && pKFn != prevKF && pKFn != static_cast<KF*>(pKF->mNextKF) && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    b.edge(nIDi, pKFn->mnId, ed::mul(Siw, ed::inverse(non_corrected(pKFn))));
                }
            }
        }
    }
    for (size_t i = 0; i < vpMPs.size(); i++) {                                             // :5566-5583: GetReferenceKeyFrame() alone, no mnCorrectedByKF
        MP* pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        const auto it = b.index.find(pMP->GetReferenceKeyFrame()->mnId);
        g.point_ref.push_back(it != b.index.end() ? it->second : -1);                       // -1: refused by essg_check_4dof, the reference decides
        const Eigen::Vector3f P = pMP->GetWorldPos();
        for (int k = 0; k < 3; k++) g.points.push_back(P[k]);
        g.point_index.push_back(i);
    }
}

namespace essential_detail {
// essg_optimize_4dof on a flattened graph; false when the device refuses it (invalid input, over capacity): the caller falls back
inline bool run(const EssentialGraph4DoFFlat& g, std::vector<float>& q, std::vector<float>& t, std::vector<float>& pts)
{
    Essg4DofProblem p;
    p.n_vertices = (int32_t)g.id.size();
    p.rcw = g.rcw.data(); p.tcw = g.tcw.data(); p.rwb = g.rwb.data(); p.twb = g.twb.data(); p.rcb = g.rcb.data(); p.tcb = g.tcb.data();
    p.fixed = g.fixed.data();
    p.n_edges = (int32_t)(g.edges.size() / 2); p.edge_vertices = g.edges.data(); p.edge_rot = g.edge_rot.data(); p.edge_trans = g.edge_trans.data();
    for (int k = 0; k < 36; k++) p.information[k] = 0.0;
    for (int k = 0; k < 6; k++) p.information[7 * k] = k < 2 ? 1e3 : 1.0;                  // matLambda (:5363-5366): entry (2, 2) stays 1
    p.max_iters = 20; p.lambda_init = 0.0;                                                  // no setUserLambdaInit: computeLambdaInit
    p.n_points = (int32_t)g.point_ref.size(); p.points = g.points.data(); p.point_ref = g.point_ref.data();
    p.scw = p.n_points > 0 ? g.scw.data() : nullptr;
    std::vector<double> rcw_out(g.rcw.size()), tcw_out(g.tcw.size());
    q.assign(4 * g.id.size(), 0.f); t.assign(3 * g.id.size(), 0.f); pts.assign(g.points.size() + 3, 0.f);
    Essg4DofResult r;
    r.rcw_out = rcw_out.data(); r.tcw_out = tcw_out.data(); r.pose_q = q.data(); r.pose_t = t.data(); r.points_out = pts.data();
    const int ok = essg_check_4dof(&p, &r);             // before a handle (and with it a device) is asked for
    if (ok == ORBX_ERR_ARG || ok == ORBX_ERR_CAPACITY) return false;
    orbslam3_hip::check(essg_optimize_4dof(solver(), &p, &r, nullptr));
    return true;
}
}  // namespace essential_detail

// void Optimizer::OptimizeEssentialGraph4DoF(Map*, KeyFrame* pLoopKF, KeyFrame* pCurKF, const KeyFrameAndPose& NonCorrectedSim3,
//                                            const KeyFrameAndPose& CorrectedSim3, const map<KeyFrame*, set<KeyFrame*>>&)
template <class Opt = Optimizer, class KF, class MapT, class PoseMap, class ConnMap>
void OptimizeEssentialGraph4DoFHIP(MapT* pMap, KF* pLoopKF, KF* pCurKF, const PoseMap& NonCorrectedSim3, const PoseMap& CorrectedSim3,
                                   const ConnMap& LoopConnections)
{
    typedef typename std::remove_pointer<typename decltype(pMap->GetAllMapPoints())::value_type>::type MP;
    EssentialGraph4DoFFlat g;
    FlattenEssentialGraph4DoF<KF, MP>(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, g);
    std::vector<float> q, t, pts;
    if (g.dropped_edges > 0 || !essential_detail::run(g, q, t, pts)) {
        Opt::OptimizeEssentialGraph4DoF(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections);
        return;
    }
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                               // :5545
    const std::vector<KF*> vpKFs = pMap->GetAllKeyFrames();
    std::map<long unsigned int, int> index;
    for (size_t k = 0; k < g.id.size(); k++) index[g.id[k]] = (int)k;
    for (KF* pKFi : vpKFs) {                                                                // :5548-5563
        const auto it = index.find(pKFi->mnId);
        if (it == index.end()) continue;
        const int k = it->second;
        pKFi->SetPose(Sophus::SE3f(Eigen::Quaternionf(q[4 * k + 3], q[4 * k], q[4 * k + 1], q[4 * k + 2]), Eigen::Vector3f(t[3 * k], t[3 * k + 1], t[3 * k + 2])));
    }
    const std::vector<MP*> vpMPs = pMap->GetAllMapPoints();
    for (size_t k = 0; k < g.point_index.size(); k++) {                                     // :5566-5586
        MP* pMP = vpMPs[g.point_index[k]];
        pMP->SetWorldPos(Eigen::Vector3f(pts[3 * k], pts[3 * k + 1], pts[3 * k + 2]));
        pMP->UpdateNormalAndDepth();
    }
    pMap->IncreaseChangeIndex();                                                            // :5587
}

}  // namespace ORB_SLAM3

#endif  // ORBSLAM3_HIP_WITH_REFERENCE
