// orbslam3_shim_preint.hpp -- drop-in adapters for IMU pre-integration on top of imu_preintegrate_batch of
// orbslam3_hip_imu_preint.h (reference include/ImuTypes.h:143-251, src/ImuTypes.cc:147-261):
//
//   bool PreintegrateIMUHIP(const std::vector<Point>& vImuFromLastFrame, double tPrev, double tCur, Pre* pFromLastKF, Pre* pFromLastFrame)
//        the loop of Tracking::PreintegrateIMU, src/Tracking.cc:1808-1851: tPrev = mCurrentFrame.mpPrevFrame->mTimeStamp, tCur =
//        mCurrentFrame.mTimeStamp, pFromLastKF = mpImuPreintegratedFromLastKF, pFromLastFrame = the accumulator the caller has just
//        made with new IMU::Preintegrated(mLastFrame.mImuBias, mCurrentFrame.mImuCalib).  ONE call integrates both.
//   bool ReintegrateHIP(const std::vector<Pre*>& v)
//        Preintegrated::Reintegrate() for every key frame of a map in ONE call: the loops of src/Optimizer.cc:3204-3220, :3370-3385.
//
// Both return false, with nothing written, when the library refuses the input (imu_preint_check: a measurement that is not finite
// or has dt <= 0): the caller then runs the reference's own loop, which is what INTEGRATION.md 4k shows.
// Like orbslam3_shim_imu_init.hpp it is written against the reference's own types and compiles inside an ORB-SLAM3 tree with
// ORBSLAM3_HIP_WITH_REFERENCE defined; Pre (IMU::Preintegrated) and Point (IMU::Point) are template parameters, so that
// tests/test_shim_preint.py runs it on the stand-in of tests/stubs/standin_imu_preint.hpp.  bu, db, mvMeasurements and mMutex are
// private in the reference (include/ImuTypes.h:224-250): every access to them is in IMU::PreintAccess, which the reference's class
// has to befriend with one line.
// Times are doubles in seconds here (IMU::Point::t, Frame::mTimeStamp), so the interpolation is done on the host in this file;
// imu_frame_measurements_batch_device is its device form for the server, where times are the int64 nanoseconds of the packets.
#pragma once

#include "orbslam3_shim.hpp"

#ifdef ORBSLAM3_HIP_WITH_REFERENCE

#include <memory>
#include <mutex>

namespace ORB_SLAM3 {

namespace IMU {
// the private members of IMU::Preintegrated, for the marshalling below only
struct PreintAccess {
    template <class Pre> static auto& bu(Pre& p) { return p.bu; }
    template <class Pre> static auto& db(Pre& p) { return p.db; }
    template <class Pre> static auto& measurements(Pre& p) { return p.mvMeasurements; }
    template <class Pre> static std::mutex& mutex(Pre& p) { return p.mMutex; }
    template <class Pre> static void push(Pre& p, const ImuMeasurement& m)
    {
        typedef typename std::remove_reference<decltype(p.mvMeasurements)>::type::value_type Integrable;
        p.mvMeasurements.push_back(Integrable(Eigen::Vector3f(m.a[0], m.a[1], m.a[2]), Eigen::Vector3f(m.w[0], m.w[1], m.w[2]), m.dt));
    }
};
}  // namespace IMU

namespace preint_detail {

inline void bias_in(const IMU::Bias& b, float* dst) { dst[0] = b.bax; dst[1] = b.bay; dst[2] = b.baz; dst[3] = b.bwx; dst[4] = b.bwy; dst[5] = b.bwz; }
inline IMU::Bias bias_out(const float* b) { return IMU::Bias(b[0], b[1], b[2], b[3], b[4], b[5]); }

// every numeric member of a pre-integration that the device reads or writes; n_meas = the length of mvMeasurements
template <class Pre>
inline void to_state(Pre& p, ImuPreintState& s)
{
    std::memset(&s, 0, sizeof(s));
    s.dT = p.dT;
    bias_in(p.b, s.b); bias_in(IMU::PreintAccess::bu(p), s.bu);
    for (int k = 0; k < 6; k++) { s.nga[k] = p.Nga.diagonal()(k); s.nga_walk[k] = p.NgaWalk.diagonal()(k); }
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) {
            s.dR[3 * r + c] = p.dR(r, c); s.JRg[3 * r + c] = p.JRg(r, c); s.JVg[3 * r + c] = p.JVg(r, c); s.JVa[3 * r + c] = p.JVa(r, c);
            s.JPg[3 * r + c] = p.JPg(r, c); s.JPa[3 * r + c] = p.JPa(r, c);
        }
        s.dV[r] = p.dV(r); s.dP[r] = p.dP(r); s.avgA[r] = p.avgA(r); s.avgW[r] = p.avgW(r);
    }
    for (int r = 0; r < 15; r++) for (int c = 0; c < 15; c++) s.C[15 * r + c] = p.C(r, c);
    s.n_meas = (int32_t)IMU::PreintAccess::measurements(p).size();
}

// the way back.  Nga / NgaWalk are written too (the device never changes them); Info, db and mvMeasurements are not part of a state
template <class Pre>
inline void from_state(const ImuPreintState& s, Pre& p)
{
    p.dT = s.dT;
    p.b = bias_out(s.b); IMU::PreintAccess::bu(p) = bias_out(s.bu);
    for (int k = 0; k < 6; k++) { p.Nga.diagonal()(k) = s.nga[k]; p.NgaWalk.diagonal()(k) = s.nga_walk[k]; }
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) {
            p.dR(r, c) = s.dR[3 * r + c]; p.JRg(r, c) = s.JRg[3 * r + c]; p.JVg(r, c) = s.JVg[3 * r + c]; p.JVa(r, c) = s.JVa[3 * r + c];
            p.JPg(r, c) = s.JPg[3 * r + c]; p.JPa(r, c) = s.JPa[3 * r + c];
        }
        p.dV(r) = s.dV[r]; p.dP(r) = s.dP[r]; p.avgA(r) = s.avgA[r]; p.avgW(r) = s.avgW[r];
    }
    for (int r = 0; r < 15; r++) for (int c = 0; c < 15; c++) p.C(r, c) = s.C[15 * r + c];
}

// what Initialize() resets beside the members of a state (src/ImuTypes.cc:158-159)
template <class Pre>
inline void clear_info_and_db(Pre& p)
{
    for (int r = 0; r < 15; r++) for (int c = 0; c < 15; c++) p.Info(r, c) = 0.f;
    for (int k = 0; k < 6; k++) IMU::PreintAccess::db(p)(k) = 0.f;
}

// the interpolation of src/Tracking.cc:1810-1845 on IMU::Point (times are doubles, their differences are rounded to float)
template <class Point>
inline std::vector<ImuMeasurement> frame_measurements(const std::vector<Point>& v, double tPrev, double tCur)
{
    const int n = (int)v.size() - 1;
    std::vector<ImuMeasurement> out;
    for (int i = 0; i < n; i++) {
        const Point &p0 = v[i], &p1 = v[i + 1];
        Eigen::Vector3f acc, angVel;
        float tstep;
        if (i == 0 && i < n - 1) {
            const float tab = p1.t - p0.t, tini = p0.t - tPrev;
            acc = (p0.a + p1.a - (p1.a - p0.a) * (tini / tab)) * 0.5f;
            angVel = (p0.w + p1.w - (p1.w - p0.w) * (tini / tab)) * 0.5f;
            tstep = p1.t - tPrev;
        } else if (i < n - 1) {
            acc = (p0.a + p1.a) * 0.5f;
            angVel = (p0.w + p1.w) * 0.5f;
            tstep = p1.t - p0.t;
        } else if (i > 0) {
            const float tab = p1.t - p0.t, tend = p1.t - tCur;
            acc = (p0.a + p1.a - (p1.a - p0.a) * (tend / tab)) * 0.5f;
            angVel = (p0.w + p1.w - (p1.w - p0.w) * (tend / tab)) * 0.5f;
            tstep = tCur - p0.t;
        } else {
            acc = p0.a; angVel = p0.w;
            tstep = tCur - tPrev;
        }
        ImuMeasurement m;
        for (int k = 0; k < 3; k++) { m.a[k] = acc(k); m.w[k] = angVel(k); }
        m.dt = tstep;
        out.push_back(m);
    }
    return out;
}

// imu_preintegrate_batch on marshalled states; false when imu_preint_check refuses the call
inline bool run(std::vector<ImuPreintState>& states, const std::vector<ImuPreintJob>& jobs, const std::vector<ImuMeasurement>& meas)
{
    if (imu_preint_check(states.data(), (int)states.size(), jobs.data(), (int)jobs.size(), meas.data(), (int)meas.size()) == ORBX_ERR_ARG) return false;
    std::vector<int32_t> status(jobs.size(), 0);
    orbslam3_hip::check(imu_preintegrate_batch(orbslam3_hip::thread_handle<imu_preint, imu_preint_create>(), states.data(), (int)states.size(), jobs.data(),
                                               (int)jobs.size(), meas.data(), (int)meas.size(), status.data()));
    return true;
}

}  // namespace preint_detail

// the loop of Tracking::PreintegrateIMU (:1808-1851) for both accumulators in one call
template <class Pre, class Point>
bool PreintegrateIMUHIP(const std::vector<Point>& vImuFromLastFrame, double tPrev, double tCur, Pre* pFromLastKF, Pre* pFromLastFrame)
{
    const std::vector<ImuMeasurement> meas = preint_detail::frame_measurements(vImuFromLastFrame, tPrev, tCur);
    if (meas.empty()) return true;
    std::unique_lock<std::mutex> lock1(IMU::PreintAccess::mutex(*pFromLastKF)), lock2(IMU::PreintAccess::mutex(*pFromLastFrame));
    std::vector<ImuPreintState> states(2);
    preint_detail::to_state(*pFromLastKF, states[0]);
    preint_detail::to_state(*pFromLastFrame, states[1]);
    std::vector<ImuPreintJob> jobs(2);
    std::memset(jobs.data(), 0, sizeof(ImuPreintJob) * 2);
    jobs[0].state = 0; jobs[0].count = (int32_t)meas.size();                                  // continuing since the last key frame
    jobs[1].state = 1; jobs[1].count = (int32_t)meas.size(); jobs[1].reset = 1;               // the accumulator of this frame starts here
    preint_detail::bias_in(pFromLastFrame->b, jobs[1].bias);
    if (!preint_detail::run(states, jobs, meas)) return false;
    preint_detail::from_state(states[0], *pFromLastKF);
    preint_detail::from_state(states[1], *pFromLastFrame);
    preint_detail::clear_info_and_db(*pFromLastFrame);
    IMU::PreintAccess::measurements(*pFromLastFrame).clear();
    for (const ImuMeasurement& m : meas) { IMU::PreintAccess::push(*pFromLastKF, m); IMU::PreintAccess::push(*pFromLastFrame, m); }
    return true;
}

// Preintegrated::Reintegrate() (:168-175) for all of v in one call; null entries are skipped
template <class Pre>
bool ReintegrateHIP(const std::vector<Pre*>& v)
{
    std::vector<Pre*> live;
    for (Pre* p : v) if (p) live.push_back(p);
    if (live.empty()) return true;
    std::vector<std::unique_ptr<std::unique_lock<std::mutex> > > locks;
    std::vector<ImuPreintState> states(live.size());
    std::vector<ImuPreintJob> jobs(live.size());
    std::vector<ImuMeasurement> meas;
    std::memset(jobs.data(), 0, sizeof(ImuPreintJob) * jobs.size());
    for (size_t i = 0; i < live.size(); i++) {
        Pre& p = *live[i];
        locks.emplace_back(new std::unique_lock<std::mutex>(IMU::PreintAccess::mutex(p)));
        preint_detail::to_state(p, states[i]);
        jobs[i].state = (int32_t)i; jobs[i].first = (int32_t)meas.size(); jobs[i].reset = 1;
        preint_detail::bias_in(IMU::PreintAccess::bu(p), jobs[i].bias);                        // Initialize(bu)
        for (const auto& m : IMU::PreintAccess::measurements(p)) {
            ImuMeasurement q;
            for (int k = 0; k < 3; k++) { q.a[k] = m.a(k); q.w[k] = m.w(k); }
            q.dt = m.t;
            meas.push_back(q);
        }
        jobs[i].count = (int32_t)meas.size() - jobs[i].first;
    }
    if (!preint_detail::run(states, jobs, meas)) return false;
    for (size_t i = 0; i < live.size(); i++) {
        preint_detail::from_state(states[i], *live[i]);
        preint_detail::clear_info_and_db(*live[i]);
    }
    return true;
}

}  // namespace ORB_SLAM3

#endif  // ORBSLAM3_HIP_WITH_REFERENCE
