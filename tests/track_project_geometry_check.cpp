// Host build of csrc/track_project_geometry.h, the text the kernels of orbm_track_project.hip compile: reads one case written by
// tests/track_project_cases.py pack(), runs the loops of the kernels row by row, writes what unpack() reads.
//   g++ -O2 -ffp-contract=off -std=c++17 -I include -o check tests/track_project_geometry_check.cpp;  check in.bin out.bin
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../orb_slam3-1_amd/csrc/track_project_geometry.h"

template <class T> static bool get(FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <class T> static void put(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[5];
    float fl[11];
    if (fread(head, 4, 5, f) != 5 || fread(fl, 4, 11, f) != 11) return 3;
    const int mode = head[0], B = head[1], rows = head[2], normalise = head[3];
    if (B < 0 || rows < 0) return 3;
    OrbmTrackCamera cam{fl[0], fl[1], fl[2], fl[3], fl[4], fl[5], fl[6], fl[7], fl[8], fl[9], head[4]};
    const float cos_limit = fl[10];
    const size_t N = (size_t)B * rows;
    std::vector<double> pose7;
    std::vector<int32_t> n;
    std::vector<float> xyz, normal, mind, maxd;
    std::vector<uint8_t> skip, bad, has_point;
    bool ok = get(f, pose7, (size_t)B * 7) && get(f, n, B) && get(f, xyz, N * 3);
    if (mode == 0) ok = ok && get(f, normal, N * 3) && get(f, mind, N) && get(f, maxd, N) && get(f, skip, N) && get(f, bad, N);
    else ok = ok && get(f, has_point, N);
    fclose(f);
    if (!ok) return 3;

    std::vector<OrbmFramePose> F(B);
    for (int b = 0; b < B; b++) tpj::frame_pose(&pose7[(size_t)b * 7], normalise, &F[b]);
    std::vector<int32_t> valid(N), level(N), n_to_match(B, 0);
    std::vector<float> u(N), v(N), vcos(N), depth(N), ur(N);
    for (int b = 0; b < B; b++)
        for (int p = 0; p < rows; p++) {
            const size_t row = (size_t)b * rows + p;
            tpj::Row r = tpj::row_none();
            if (mode == 0) {
                if (p < n[b] && !skip[row] && !bad[row])
                    r = tpj::frustum_row(cam, F[b], &xyz[row * 3], &normal[row * 3], mind[row], maxd[row], cos_limit);
            } else if (p < n[b] && has_point[row]) {
                r = tpj::project_last_row(cam, F[b], &xyz[row * 3]);
            }
            valid[row] = r.valid; level[row] = r.level; u[row] = r.u; v[row] = r.v; vcos[row] = r.view_cos; depth[row] = r.depth; ur[row] = r.ur;
            n_to_match[b] += r.valid;
        }

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    static_assert(sizeof(OrbmFramePose) == 19 * sizeof(float), "the record is 19 floats");
    put(o, F);
    put(o, valid); put(o, u); put(o, v);
    if (mode == 0) { put(o, level); put(o, vcos); put(o, depth); }
    put(o, ur);
    if (mode == 0) put(o, n_to_match);
    return fclose(o) == 0 ? 0 : 4;
}
