// Prints imuinit::build_structure (orb_slam3-1_amd/csrc/imu_init_structure.h) of the link sets on standard input, for
// tests/test_imuinit_structure.py.  Host only: g++, no device.
// Input, per set: "n_kf n_links", then n_links pairs "kf1 kf2".  Output, per set, four lines: error, bad_link, order, link_in.
#include <cstdio>
#include <vector>

#include "imu_init_structure.h"

static void line(const char* name, const std::vector<int>& v)
{
    std::printf("%s", name);
    for (int x : v) std::printf(" %d", x);
    std::printf("\n");
}

int main()
{
    int n_kf, n_links;
    while (std::scanf("%d %d", &n_kf, &n_links) == 2) {
        std::vector<int> kf1((size_t)n_links), kf2((size_t)n_links);
        for (int l = 0; l < n_links; l++)
            if (std::scanf("%d %d", &kf1[l], &kf2[l]) != 2) return 1;
        const imuinit::Structure s = imuinit::build_structure(n_kf, n_links, kf1.data(), kf2.data());
        line("error", {s.error});
        line("bad_link", {s.bad_link});
        line("order", s.order);
        line("link_in", s.link_in);
    }
    return 0;
}
