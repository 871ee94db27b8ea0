// Prints the block structure pgraph::build_structure (orb_slam3-1_amd/csrc/pose_graph_structure.h) gives a graph;
// tests/test_pose_graph_structure.py compares it with a restatement of the ordering rules.  No device.
//
// stdin, any number of graphs:  <n_vertices> <n_edges>, then n_vertices fixed flags, then n_edges vertex pairs.
// stdout per graph: "n_free <k>" and one line each for col, blk_i, blk_j, blk_off and blk_ent (the name, then the entries).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pose_graph_structure.h"

static void print(const char* name, const std::vector<int>& v)
{
    std::printf("%s", name);
    for (int x : v) std::printf(" %d", x);
    std::printf("\n");
}

int main()
{
    int nv, ne;
    while (std::scanf("%d %d", &nv, &ne) == 2) {
        if (nv < 0 || ne < 0) return 2;
        std::vector<uint8_t> fixed((size_t)nv);
        std::vector<int> ev(2 * (size_t)ne);
        for (auto& f : fixed) { int x; if (std::scanf("%d", &x) != 1) return 2; f = (uint8_t)x; }
        for (auto& x : ev) if (std::scanf("%d", &x) != 1 || x < 0 || x >= nv) return 2;
        const pgraph::Structure g = pgraph::build_structure(nv, fixed.data(), ne, ev.data());
        std::printf("n_free %d\n", g.n_free);
        print("col", g.col); print("blk_i", g.blk_i); print("blk_j", g.blk_j); print("blk_off", g.blk_off); print("blk_ent", g.blk_ent);
    }
    return 0;
}
