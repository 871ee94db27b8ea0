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

#include <memory>

namespace ORB_SLAM3 {

class Sim3Solver;       // include/Sim3Solver.h: only named here, used through the template parameter Ref

namespace loop_detail {

inline bool single_pinhole(KeyFrame* pKF) { return !pKF->mpCamera2 && pKF->mpCamera && pKF->mpCamera->GetType() == GeometricCamera::CAM_PINHOLE; }

// one handle per calling thread: a handle owns one stream and must not be shared between threads (orbslam3_hip.h)
inline sim3_solver* solver()
{
    static thread_local sim3_solver* s = nullptr;
    if (!s) orbslam3_hip::check(sim3_create(0, &s));
    return s;
}

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

}  // namespace ORB_SLAM3

#endif  // ORBSLAM3_HIP_WITH_REFERENCE
