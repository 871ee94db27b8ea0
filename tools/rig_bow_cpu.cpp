// One-core baseline of SearchForTriangulation between two rig key frames for tools/rig_bow_timing.py: the reference's loops
// (src/ORBmatcher.cc:963-1112: bestDist starts at TH_LOW, a candidate at dist <= bestDist that passes the gate becomes the holder) with
// 64-bit popcounts and csrc/kb8_stereo_geometry.h -- the very function k_tri_rig runs -- as the gate, pair after pair.  Stand-alone:
// g++ -O3 -mpopcnt -ffp-contract=off.
//   rig_bow_cpu <in> <out>
// in:  int32 n_pairs, coarse, n_levels; per pair: 4 x 30 floats (the records ll, lr, rl, rr: camera 1 fx fy cx cy k0..k3 precision,
//      the same of camera 2, R12 row major, t12), n_levels floats sigma2 of key frame 1, the same of key frame 2, then per key frame:
//      int32 n, n_left, n_nodes, n_entries; desc [n][32]; has_mp [n] bytes; x, y [n] floats; octave [n] int32; node ids [n_nodes]
//      uint32; offsets [n_nodes + 1] int32; features [n_entries] uint32
// out: match12 [n1] int32 per pair
// stdout: one JSON line with the best of three passes after a warm-up, in milliseconds, and the number of matches and gate calls
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../orb_slam3-1_amd/csrc/kb8_stereo_geometry.h"

struct Side {
    int32_t n, n_left, n_nodes, n_entries;
    std::vector<uint8_t> desc, has_mp;
    std::vector<float> x, y;
    std::vector<int32_t> octave, off;
    std::vector<uint32_t> node, feat;
};
struct Pair { kb8s::Rig rigs[4]; std::vector<float> s1, s2; Side k[2]; std::vector<int32_t> match; };

template <class T>
static void get(FILE* f, T* dst, size_t n) { if (n && std::fread(dst, sizeof(T), n, f) != n) { std::fprintf(stderr, "short input\n"); std::exit(4); } }

static inline int hamming(const uint8_t* a, const uint8_t* b)
{
    uint64_t x[4], y[4];
    std::memcpy(x, a, 32); std::memcpy(y, b, 32);
    return __builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) + __builtin_popcountll(x[2] ^ y[2]) + __builtin_popcountll(x[3] ^ y[3]);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    int32_t head[3];
    get(f, head, 3);
    const int n_pairs = head[0], coarse = head[1], n_levels = head[2];
    std::vector<Pair> P(n_pairs);
    for (Pair& p : P) {
        float r[4][30];
        get(f, &r[0][0], 120);
        for (int c = 0; c < 4; c++) p.rigs[c] = kb8s::rig_from_floats(r[c]);
        p.s1.resize(n_levels); p.s2.resize(n_levels);
        get(f, p.s1.data(), n_levels); get(f, p.s2.data(), n_levels);
        for (Side& s : p.k) {
            get(f, &s.n, 4);
            s.desc.resize((size_t)s.n * 32); s.has_mp.resize(s.n); s.x.resize(s.n); s.y.resize(s.n); s.octave.resize(s.n);
            s.node.resize(s.n_nodes); s.off.resize(s.n_nodes + 1); s.feat.resize(s.n_entries);
            get(f, s.desc.data(), s.desc.size()); get(f, s.has_mp.data(), s.n); get(f, s.x.data(), s.n); get(f, s.y.data(), s.n); get(f, s.octave.data(), s.n);
            get(f, s.node.data(), s.n_nodes); get(f, s.off.data(), s.n_nodes + 1); get(f, s.feat.data(), s.n_entries);
        }
        p.match.assign(p.k[0].n, -1);
    }
    std::fclose(f);

    long matches = 0, gates = 0;
    double best = 1e30;
    for (int pass = 0; pass < 4; pass++) {                      // the first pass warms up
        const auto t0 = std::chrono::steady_clock::now();
        matches = gates = 0;
        for (Pair& p : P) {
            const Side& A = p.k[0]; const Side& B = p.k[1];
            std::fill(p.match.begin(), p.match.end(), -1);
            int a = 0, b = 0;
            while (a < A.n_nodes && b < B.n_nodes) {
                if (A.node[a] < B.node[b]) { a++; continue; }
                if (A.node[a] > B.node[b]) { b++; continue; }
                for (int e1 = A.off[a]; e1 < A.off[a + 1]; e1++) {
                    const int idx1 = (int)A.feat[e1];
                    if (A.has_mp[idx1]) continue;
                    int bestDist = 50, bestIdx2 = -1;
                    for (int e2 = B.off[b]; e2 < B.off[b + 1]; e2++) {
                        const int idx2 = (int)B.feat[e2];
                        if (B.has_mp[idx2]) continue;
                        const int dist = hamming(&A.desc[(size_t)idx1 * 32], &B.desc[(size_t)idx2 * 32]);
                        if (dist > 50 || dist > bestDist) continue;
                        if (!coarse) {
                            float q[3];
                            gates++;
                            const kb8s::Rig& g = p.rigs[2 * (idx1 >= A.n_left) + (idx2 >= B.n_left)];
                            if (!(kb8s::triangulate_matches(g, A.x[idx1], A.y[idx1], B.x[idx2], B.y[idx2], p.s1[A.octave[idx1]], p.s2[B.octave[idx2]], q) > 0.0001f)) continue;
                        }
                        bestIdx2 = idx2; bestDist = dist;
                    }
                    if (bestIdx2 >= 0) { p.match[idx1] = bestIdx2; matches++; }
                }
                a++; b++;
            }
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (pass > 0 && ms < best) best = ms;
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 5;
    for (const Pair& p : P) std::fwrite(p.match.data(), 4, p.match.size(), f);
    std::fclose(f);
    std::printf("{\"cpu_ms\": %.4f, \"matches\": %ld, \"gate_calls\": %ld}\n", best, matches, gates);
    return 0;
}
