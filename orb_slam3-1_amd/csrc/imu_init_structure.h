// The order of the unknowns of an IMU initialisation (imu_init_solver.hip).  Host only, standard library only
// (tests/imu_init_structure_dump.cpp compiles it with g++).
//
// The links kf1 -> kf2 of a map are disjoint paths (kf2's mPrevKF is kf1).  With the key frames numbered along their paths the
// normal equations over the velocities are block tridiagonal, and the kernel eliminates them in that order, so THE ORDER IS PART
// OF THE RESULT:
//   * a path starts at its head, the key frame that is kf1 of a link and kf2 of none; the paths follow each other in ascending
//     order of their heads' key-frame indices;
//   * order[p] is the key frame at chain position p, link_in[p] the link that ends there (its kf1 is order[p - 1]) or -1 when p
//     starts a path;
//   * a key frame that appears in no link has no position.
#pragma once
#include <cstddef>
#include <vector>

namespace imuinit {

enum StructureError { kOk = 0, kIndexRange, kSelfLink, kTwiceKf1, kTwiceKf2, kCycle };

inline const char* structure_error_text(int e)
{
    switch (e) {
        case kOk: return "ok";
        case kIndexRange: return "key-frame index out of range";
        case kSelfLink: return "kf1 == kf2";
        case kTwiceKf1: return "key frame is kf1 of more than one link";
        case kTwiceKf2: return "key frame is kf2 of more than one link";
        default: return "the links form a cycle";
    }
}

struct Structure {
    std::vector<int> order;         // [n_chain] key frame at chain position p
    std::vector<int> link_in;       // [n_chain] link into position p, -1: p starts a path
    int error = kOk;
    int bad_link = -1;              // the link at which the error was found (-1 for a cycle)
};

// kf1[l], kf2[l]: the two key frames of link l
inline Structure build_structure(int n_kf, int n_links, const int* kf1, const int* kf2)
{
    Structure s;
    std::vector<int> next((size_t)(n_kf > 0 ? n_kf : 0), -1), prev(next);
    for (int l = 0; l < n_links; l++) {
        const int a = kf1[l], b = kf2[l];
        s.bad_link = l;
        if (a < 0 || a >= n_kf || b < 0 || b >= n_kf) { s.error = kIndexRange; return s; }
        if (a == b) { s.error = kSelfLink; return s; }
        if (next[a] >= 0) { s.error = kTwiceKf1; return s; }
        if (prev[b] >= 0) { s.error = kTwiceKf2; return s; }
        next[a] = l; prev[b] = l;
    }
    s.bad_link = -1;
    s.order.reserve((size_t)n_links + 1);
    int walked = 0;
    for (int h = 0; h < n_kf; h++) {
        if (next[h] < 0 || prev[h] >= 0) continue;      // not a head
        s.order.push_back(h); s.link_in.push_back(-1);
        for (int l = next[h]; l >= 0; l = next[kf2[l]]) { s.order.push_back(kf2[l]); s.link_in.push_back(l); walked++; }
    }
    if (walked != n_links) { s.order.clear(); s.link_in.clear(); s.error = kCycle; }
    return s;
}

}  // namespace imuinit
