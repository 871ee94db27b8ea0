// Host build of the per-match geometry the kernel k_new_map_points runs (orb_slam3-1_amd/csrc/orbm_new_points_geometry.h),
// so that its decisions and points can be checked against tests/newpoints_reference.py without a GPU.
//   newpoints_geometry_check IN OUT
// IN: float32 records of 67 values per pair: camera 1 (Rcw[9] tcw[3] Ow[3] fx fy cx cy invfx invfy mb mbf), camera 2, observation 1
// (x y ur depth kx ky sigma2 scale), observation 2, rule (inertial far_points th_far ratio_factor), mvScaleFactors[nLevels-1] of key frame 1.
// OUT: float32 records of 10 values: accept point_stereo x3d[3] normal[3] max_dist min_dist.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../orb_slam3-1_amd/csrc/orbm_new_points_geometry.h"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<float> in;
    float buf[67];
    while (fread(buf, sizeof(float), 67, f) == 67) in.insert(in.end(), buf, buf + 67);
    fclose(f);
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 2;
    for (size_t p = 0; p + 67 <= in.size(); p += 67) {
        const float* r = in.data() + p;
        nmp::Camera C[2];
        nmp::Obs o[2];
        for (int q = 0; q < 2; q++) {
            const float* c = r + 23 * q;
            std::memcpy(C[q].Rcw, c, 9 * sizeof(float)); std::memcpy(C[q].tcw, c + 9, 3 * sizeof(float)); std::memcpy(C[q].Ow, c + 12, 3 * sizeof(float));
            C[q].fx = c[15]; C[q].fy = c[16]; C[q].cx = c[17]; C[q].cy = c[18]; C[q].invfx = c[19]; C[q].invfy = c[20]; C[q].mb = c[21]; C[q].mbf = c[22];
            const float* b = r + 46 + 8 * q;
            o[q].x = b[0]; o[q].y = b[1]; o[q].ur = b[2]; o[q].depth = b[3]; o[q].kx = b[4]; o[q].ky = b[5]; o[q].sigma2 = b[6]; o[q].scale = b[7];
        }
        nmp::Rule R;
        R.inertial = r[62] != 0; R.far_points = r[63] != 0; R.th_far = r[64]; R.ratio_factor = r[65];
        const float last_scale = r[66];
        float out[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        int ps = 0;
        const bool ok = nmp::new_point(C[0], o[0], C[1], o[1], R, out + 2, &ps);
        out[0] = ok ? 1.f : 0.f; out[1] = (float)ps;
        if (ok) nmp::normal_and_depth(out + 2, C[0].Ow, C[1].Ow, o[0].scale, last_scale, out + 5, out + 8, out + 9);
        fwrite(out, sizeof(float), 10, g);
    }
    fclose(g);
    return 0;
}
