// The host half of tools/track_project_timing.py: the loops orbm_frustum_batch_device and orbm_project_last_batch_device replace, run
// on one host core through the same header the kernels compile (csrc/track_project_geometry.h).  Built by the tool with
//   g++ -O3 -ffp-contract=off -std=c++17 -shared -fPIC -I include
#include <cstddef>
#include <cstdint>

#include "../orb_slam3-1_amd/csrc/track_project_geometry.h"

extern "C" {

void tpc_frustum(const OrbmTrackCamera* cam, const OrbmFramePose* poses, const OrbmLocalPoints* pts, float cos_limit, const OrbmFrustumOut* out, int batch)
{
    for (int b = 0; b < batch; b++) {
        int n_to_match = 0;
        for (int p = 0; p < pts->pcap; p++) {
            const size_t row = (size_t)b * pts->pcap + p;
            tpj::Row r = tpj::row_none();
            if (p < pts->n[b] && !pts->skip[row] && !pts->bad[row])
                r = tpj::frustum_row(*cam, poses[b], pts->xyz + row * 3, pts->normal + row * 3, pts->min_distance[row], pts->max_distance[row], cos_limit);
            out->valid[row] = (uint8_t)r.valid; out->u[row] = r.u; out->v[row] = r.v; out->octave[row] = r.level;
            out->view_cos[row] = r.view_cos; out->track_depth[row] = r.depth; out->proj_ur[row] = r.ur;
            n_to_match += r.valid;
        }
        out->n_to_match[b] = n_to_match;
    }
}

void tpc_project_last(const OrbmTrackCamera* cam, const OrbmFramePose* poses, const float* xyz, const uint8_t* has_point, const int32_t* n, int cap,
                      const OrbmLastProjOut* out, int batch)
{
    for (int b = 0; b < batch; b++)
        for (int i = 0; i < cap; i++) {
            const size_t row = (size_t)b * cap + i;
            tpj::Row r = tpj::row_none();
            if (i < n[b] && has_point[row]) r = tpj::project_last_row(*cam, poses[b], xyz + row * 3);
            out->valid[row] = (uint8_t)r.valid; out->u[row] = r.u; out->v[row] = r.v; out->proj_ur[row] = r.ur;
        }
}

}  // extern "C"
