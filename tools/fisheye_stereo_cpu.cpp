// One-core baseline of Frame::ComputeStereoFishEyeMatches for tools/fisheye_stereo_timing.py: the brute-force 2-nearest-neighbour
// Hamming search as a plain loop (64-bit popcounts) and csrc/kb8_stereo_geometry.h -- the very functions the kernels run -- for the
// survivors, frame after frame.  Stand-alone: g++ -O3 -mpopcnt -ffp-contract=off.
//   fisheye_stereo_cpu <in> <out>
// in:  int32 batch, cap, n_levels; 30 floats of the rig (left fx fy cx cy k0..k3 precision, the same of the right, Rlr row major,
//      tlr); n_levels floats; then per side (left, right): key points [batch][cap] (28 bytes), descriptors [batch][cap][32],
//      int32 n[batch], int32 mono[batch]
// out: left_to_right [batch][cap] int32, right_to_left [batch][cap] int32, depth [batch][cap] float, p3d [batch][cap][3] float
// stdout: one JSON line with the best of three passes after a warm-up, in milliseconds, and the number of matches
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../orb_slam3-1_amd/csrc/kb8_stereo_geometry.h"

struct KeyPoint { float x, y, size, angle, response; int32_t octave, class_id; };
static_assert(sizeof(KeyPoint) == 28, "cv::KeyPoint layout");

struct Side { std::vector<KeyPoint> kps; std::vector<uint8_t> desc; std::vector<int32_t> n, mono; };

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
    float r[30];
    get(f, head, 3); get(f, r, 30);
    const int batch = head[0], cap = head[1], n_levels = head[2];
    std::vector<float> sigma2(n_levels);
    get(f, sigma2.data(), n_levels);
    Side S[2];
    for (Side& s : S) {
        s.kps.resize((size_t)batch * cap); s.desc.resize((size_t)batch * cap * 32); s.n.resize(batch); s.mono.resize(batch);
        get(f, s.kps.data(), s.kps.size()); get(f, s.desc.data(), s.desc.size()); get(f, s.n.data(), batch); get(f, s.mono.data(), batch);
    }
    std::fclose(f);
    const kb8s::Rig g = kb8s::rig_from_floats(r);

    const size_t N = (size_t)batch * cap;
    std::vector<int32_t> ltr(N), rtl(N);
    std::vector<float> depth(N), p3d(3 * N);
    long matches = 0;
    double best = 1e30;
    for (int pass = 0; pass < 4; pass++) {                      // the first pass warms up
        const auto t0 = std::chrono::steady_clock::now();
        matches = 0;
        for (int b = 0; b < batch; b++) {
            const size_t row = (size_t)b * cap;
            const int n_l = S[0].n[b], mono_l = S[0].mono[b], n_r = S[1].n[b], mono_r = S[1].mono[b];
            for (int i = 0; i < n_l; i++) { ltr[row + i] = -1; depth[row + i] = -1.f; p3d[3 * (row + i)] = p3d[3 * (row + i) + 1] = p3d[3 * (row + i) + 2] = 0.f; }
            for (int j = 0; j < n_r; j++) rtl[row + j] = -1;
            for (int i = mono_l; i < n_l; i++) {
                int d0 = 0x7fffffff, d1 = 0x7fffffff, idx = -1;
                const uint8_t* a = &S[0].desc[(row + i) * 32];
                for (int j = mono_r; j < n_r; j++) {
                    const int d = hamming(a, &S[1].desc[(row + j) * 32]);
                    if (d < d0) { d1 = d0; d0 = d; idx = j; } else if (d < d1) d1 = d;
                }
                if (n_r - mono_r < 2 || !kb8s::ratio_ok(d0, d1)) continue;
                const KeyPoint& k1 = S[0].kps[row + i];
                const KeyPoint& k2 = S[1].kps[row + idx];
                float p[3];
                const float z = kb8s::triangulate_matches(g, k1.x, k1.y, k2.x, k2.y, sigma2[k1.octave], sigma2[k2.octave], p);
                if (z > 0.0001f) {
                    ltr[row + i] = idx; rtl[row + idx] = i; depth[row + i] = z;
                    for (int c = 0; c < 3; c++) p3d[3 * (row + i) + c] = p[c];
                    matches++;
                }
            }
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (pass > 0 && ms < best) best = ms;
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 5;
    std::fwrite(ltr.data(), 4, N, f); std::fwrite(rtl.data(), 4, N, f); std::fwrite(depth.data(), 4, N, f); std::fwrite(p3d.data(), 4, 3 * N, f);
    std::fclose(f);
    std::printf("{\"cpu_ms\": %.4f, \"matches\": %ld}\n", best, matches);
    return 0;
}
