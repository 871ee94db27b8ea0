// TEST INFRASTRUCTURE -- what a recording fake of a C entry point writes about the problem struct it is handed: one line per field
// on STDERR (stdout stays what the typed tests index by position).  A scalar is written as %a; an array as its length, the 64-bit
// FNV-1a hash of its bytes and its first and last element; a LibaLink field by field, because the struct has padding.
// tests/test_shim_abi_golden.py compares these lines with tests/golden/shim_abi/, byte for byte.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "orbslam3_hip.h"

namespace record_abi {

inline uint64_t fnv1a(const void* p, size_t bytes)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < bytes; i++) { h ^= static_cast<const uint8_t*>(p)[i]; h *= 0x100000001b3ull; }
    return h;
}

inline void scalar(const char* name, double v) { std::fprintf(stderr, "  %s %a\n", name, v); }

template <class T>
inline void array(const char* name, const T* p, size_t n)
{
    if (!p) { std::fprintf(stderr, "  %s NULL\n", name); return; }
    std::fprintf(stderr, "  %s len %zu fnv %016llx first %a last %a\n", name, n, (unsigned long long)fnv1a(p, n * sizeof(T)), n ? (double)p[0] : 0.0,
                 n ? (double)p[n - 1] : 0.0);
}

#define RA_S(f) scalar(#f, (double)p.f)
#define RA_A(f, n) array(#f, p.f, (size_t)(n))

inline void dump(const char* what, const LibaLink& p)
{
    std::fprintf(stderr, " %s\n", what);
    RA_S(kf1); RA_S(kf2);
    RA_A(dR, 9); RA_A(dV, 3); RA_A(dP, 3); RA_A(JRg, 9); RA_A(JVg, 9); RA_A(JVa, 9); RA_A(JPg, 9); RA_A(JPa, 9);
    RA_S(dT);
    RA_A(bias0, 6); RA_A(info9, 81); RA_A(info_gyro, 9); RA_A(info_acc, 9);
    RA_S(robust);
}

inline void dump_links(const LibaLink* links, int n)
{
    char what[32];
    for (int l = 0; l < n; l++) { std::snprintf(what, sizeof(what), "link %d", l); dump(what, links[l]); }
}

inline void dump(const OrbxKB8* c)
{
    if (!c) { std::fprintf(stderr, "OrbxKB8 NULL\n"); return; }
    const OrbxKB8& p = *c;
    std::fprintf(stderr, "OrbxKB8\n");
    RA_S(fx); RA_S(fy); RA_S(cx); RA_S(cy); RA_A(k, 4);
}

inline void dump(const PoseProblem& p)
{
    std::fprintf(stderr, "PoseProblem\n");
    RA_A(q, 4); RA_A(t, 3);
    RA_S(n);
    RA_A(Xw, 3 * p.n); RA_A(obs, 3 * p.n); RA_A(inv_sigma2, p.n); RA_A(stereo, p.n);
    RA_S(fx); RA_S(fy); RA_S(cx); RA_S(cy); RA_S(bf); RA_S(huber_mono); RA_S(huber_stereo);
}

inline void dump(const LbaProblem& p)
{
    std::fprintf(stderr, "LbaProblem\n");
    RA_S(n_poses);
    RA_A(pose_q, 4 * p.n_poses); RA_A(pose_t, 3 * p.n_poses); RA_A(pose_fixed, p.n_poses);
    RA_S(n_points);
    RA_A(points, 3 * p.n_points);
    RA_S(n_edges);
    RA_A(edge_point, p.n_edges); RA_A(edge_pose, p.n_edges); RA_A(edge_obs, 3 * p.n_edges); RA_A(edge_inv_sigma2, p.n_edges); RA_A(edge_stereo, p.n_edges);
    RA_S(fx); RA_S(fy); RA_S(cx); RA_S(cy); RA_S(bf); RA_S(huber_mono); RA_S(huber_stereo);
}

// LibaProblem and FibaProblem begin alike
template <class P>
inline void dump_inertial_window(const P& p)
{
    RA_S(n_kf);
    RA_A(Rwb, 9 * p.n_kf); RA_A(twb, 3 * p.n_kf); RA_A(vel, 3 * p.n_kf); RA_A(bg, 3 * p.n_kf); RA_A(ba, 3 * p.n_kf);
    RA_A(pose_fixed, p.n_kf); RA_A(has_imu, p.n_kf); RA_A(imu_fixed, p.n_kf);
    RA_A(Rcb, 9); RA_A(tcb, 3); RA_A(tbc, 3);
    RA_S(fx); RA_S(fy); RA_S(cx); RA_S(cy); RA_S(bf);
    RA_S(n_points);
    RA_A(points, 3 * p.n_points);
    RA_S(n_edges);
    RA_A(edge_kf, p.n_edges); RA_A(edge_point, p.n_edges); RA_A(edge_obs, 3 * p.n_edges); RA_A(edge_inv_sigma2, p.n_edges); RA_A(edge_stereo, p.n_edges);
    RA_S(n_links);
    dump_links(p.links, p.n_links);
    RA_S(huber_mono); RA_S(huber_stereo); RA_S(huber_inertial); RA_S(lambda_init); RA_S(max_iters);
}

inline void dump(const LibaProblem& p)
{
    std::fprintf(stderr, "LibaProblem\n");
    dump_inertial_window(p);
}

inline void dump(const FibaProblem& p)
{
    std::fprintf(stderr, "FibaProblem\n");
    dump_inertial_window(p);
    RA_S(shared_bias);
    RA_A(shared_bg, 3); RA_A(shared_ba, 3);
    RA_S(prior_g); RA_S(prior_a);
    scalar("stop_flag", p.stop_flag ? (double)*p.stop_flag : -1.0);
}

inline void dump(const LibaPoseProblem& p)
{
    std::fprintf(stderr, "LibaPoseProblem\n");
    RA_A(Rwb, 18); RA_A(twb, 6); RA_A(vel, 6); RA_A(bg, 6); RA_A(ba, 6);
    RA_A(Rcb, 9); RA_A(tcb, 3); RA_A(tbc, 3);
    RA_S(fx); RA_S(fy); RA_S(cx); RA_S(cy); RA_S(bf);
    RA_S(n);
    RA_A(Xw, 3 * p.n); RA_A(obs, 3 * p.n); RA_A(inv_sigma2, p.n); RA_A(stereo, p.n); RA_A(close_point, p.n);
    dump("link", p.link);
    RA_S(huber_mono); RA_S(huber_stereo); RA_S(rec_init); RA_S(last_frame);
    RA_A(prior_Rwb, 9); RA_A(prior_twb, 3); RA_A(prior_vel, 3); RA_A(prior_bg, 3); RA_A(prior_ba, 3); RA_A(prior_H, 225);
}

inline void dump(const ImuInitProblem& p)
{
    std::fprintf(stderr, "ImuInitProblem\n");
    RA_S(n_kf);
    RA_A(Rwb, 9 * p.n_kf); RA_A(twb, 3 * p.n_kf); RA_A(vel, 3 * p.n_kf);
    RA_A(bg, 3); RA_A(ba, 3); RA_A(Rwg, 9);
    RA_S(scale); RA_S(n_links);
    dump_links(p.links, p.n_links);
    RA_S(free_vel); RA_S(free_bias); RA_S(free_gdir); RA_S(free_scale); RA_S(prior_g); RA_S(prior_a); RA_S(huber_delta); RA_S(gauss_newton);
    RA_S(lambda_init); RA_S(max_iters);
}

#undef RA_S
#undef RA_A

}  // namespace record_abi
