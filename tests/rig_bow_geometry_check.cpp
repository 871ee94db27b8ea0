// TEST INFRASTRUCTURE -- the host side of the geometry path of k_tri_rig (orb_slam3-1_amd/csrc/orbm_rig_bow.inc): one of four kb8s::Rig
// records picked by (bRight1, bRight2), kb8s::triangulate_matches of orb_slam3-1_amd/csrc/kb8_stereo_geometry.h under it, and the
// gate `> 0.0001f`.  tests/test_rig_bow_reference.py builds and runs it and compares with tests/rig_bow_reference.py.
//   rig_bow_geometry_check <in> <out>
// in:  4 x 30 floats (the records ll, lr, rl, rr: camera 1 fx fy cx cy k0..k3 precision, the same of camera 2, R12 row major, t12),
//      int32 n, n x (int32 record, 6 floats u1 v1 u2 v2 sigma1 sigma2)
// out: n floats (code or depth), n bytes (the gate)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kb8_stereo_geometry.h"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    float r[4][30];
    int32_t n = 0;
    if (std::fread(r, 4, 120, f) != 120 || std::fread(&n, 4, 1, f) != 1 || n < 0) return 4;
    std::vector<uint8_t> in(28 * (size_t)n), pass(n);
    std::vector<float> code(n);
    if (std::fread(in.data(), 1, in.size(), f) != in.size()) return 4;
    std::fclose(f);
    kb8s::Rig g[4];
    for (int c = 0; c < 4; c++) g[c] = kb8s::rig_from_floats(r[c]);
    for (int i = 0; i < n; i++) {
        int32_t sel;
        float q[6], p[3] = {0.f, 0.f, 0.f};
        std::memcpy(&sel, &in[28 * (size_t)i], 4);
        std::memcpy(q, &in[28 * (size_t)i + 4], 24);
        if (sel < 0 || sel > 3) return 6;
        code[i] = kb8s::triangulate_matches(g[sel], q[0], q[1], q[2], q[3], q[4], q[5], p);
        pass[i] = code[i] > 0.0001f;
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 5;
    std::fwrite(code.data(), 4, code.size(), f);
    std::fwrite(pass.data(), 1, pass.size(), f);
    std::fclose(f);
    return 0;
}
