// The host half of tools/track_project_rig_timing.py: the loops orbm_frustum_rig_batch_device and orbm_project_last_rig_batch_device
// replace, run on one host core through the same header the kernels compile (csrc/track_project_rig_geometry.h).  Built by the tool with
//   g++ -O3 -ffp-contract=off -std=c++17 -shared -fPIC -I include
#include <cstddef>
#include <cstdint>

#include "../orb_slam3-1_amd/csrc/track_project_rig_geometry.h"

extern "C" {

void tprc_frustum(const OrbmTrackRigCamera* cam, const OrbmRigFramePose* poses, const OrbmLocalPoints* pts, float cos_limit, const OrbmRigFrustumOut* out, int batch)
{
    for (int b = 0; b < batch; b++) {
        int n_to_match = 0;
        for (int p = 0; p < pts->pcap; p++) {
            const size_t row = (size_t)b * pts->pcap + p;
            if (!(p < pts->n[b] && !pts->skip[row] && !pts->bad[row])) {
                out->in_view[row] = 0; out->in_view_r[row] = 0;
                continue;
            }
            const float* P = pts->xyz + row * 3;
            const float* Pn = pts->normal + row * 3;
            const tpr::Side l = tpr::frustum_left(*cam, poses[b], P, Pn, pts->min_distance[row], pts->max_distance[row], cos_limit);
            out->in_view[row] = (uint8_t)l.valid; out->pred_level[row] = l.level;
            if (l.valid) { out->proj_u[row] = l.u; out->proj_v[row] = l.v; out->view_cos[row] = l.view_cos; out->track_depth[row] = l.depth; }
            const tpr::Side r = tpr::frustum_right(*cam, poses[b], P, Pn, pts->min_distance[row], pts->max_distance[row], cos_limit);
            out->in_view_r[row] = (uint8_t)r.valid; out->pred_level_r[row] = r.level;
            if (r.valid) { out->proj_u_r[row] = r.u; out->proj_v_r[row] = r.v; out->view_cos_r[row] = r.view_cos; out->track_depth_r[row] = r.depth; }
            n_to_match += (l.valid || r.valid) ? 1 : 0;
        }
        out->n_to_match[b] = n_to_match;
    }
}

void tprc_project_last(const OrbmTrackRigCamera* cam, const OrbmRigFramePose* poses, const float* xyz, const uint8_t* has_point, const int32_t* n, int cap,
                       const OrbmRigLastProjOut* out, int batch)
{
    for (int b = 0; b < batch; b++)
        for (int i = 0; i < cap; i++) {
            const size_t row = (size_t)b * cap + i;
            tpr::LastRow r{0, -1.f, -1.f, -1.f, -1.f};
            if (i < n[b] && has_point[row]) r = tpr::project_last_rig_row(*cam, poses[b], xyz + row * 3);
            out->valid[row] = (uint8_t)r.valid; out->proj_u[row] = r.u; out->proj_v[row] = r.v; out->proj_u_r[row] = r.ur; out->proj_v_r[row] = r.vr;
        }
}

}  // extern "C"
