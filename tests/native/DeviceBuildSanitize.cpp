// DeviceBuildSanitize.cpp -- a stand-alone program around build_host_bvh2 (DeviceBuildHost.hip: the routines of csrc/bvh2_build.h walked on the host) for a run under
// AddressSanitizer / UndefinedBehaviorSanitizer on the CPU: `make -C bifrost3d_amd sanitize-device-build` builds and runs it. Sizes either side of every cut (leaf,
// short range, block, block of blocks), a cluster of identical triangles, and a depth budget that makes the larger sets decline with the level's remaining passes still run.
#include "../../include/hiprenderer_c.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
extern "C" int build_host_bvh2(const HiprTriangle*, uint32_t, uint32_t, HiprBvhNode*, uint32_t, uint32_t*, uint32_t*, uint32_t*, uint32_t*);
int main() {
    for (uint32_t n : {1u, 3u, 4u, 5u, 64u, 65u, 257u, 4097u, 70000u}) {
        for (uint32_t depth : {62u, 8u}) {
            std::vector<HiprTriangle> t(n);
            srand(n);
            for (auto& x : t) { float c[3]; for (float& v : c) v = rand() / float(RAND_MAX); std::memset(&x, 0, sizeof x);
                for (int k = 0; k < 3; ++k) { x.v0[k] = c[k] + 0.01f * (rand() / float(RAND_MAX)); x.v1[k] = c[k] - 0.01f * (rand() / float(RAND_MAX)); x.v2[k] = c[k]; } }
            if (n == 257) for (uint32_t i = 100; i < 110; ++i) t[i] = t[100];
            std::vector<HiprBvhNode> nodes(n > 1 ? n - 1 : 1); std::vector<uint32_t> order(n); uint32_t count = 0, deepest = 0, decline[2] = {0, 0};
            const int s = build_host_bvh2(t.data(), n, depth, nodes.data(), uint32_t(nodes.size()), &count, order.data(), &deepest, decline);
            printf("n %u depth %u: status %d nodes %u deepest %u\n", n, depth, s, count, deepest);
            if (s < 0) return 1;
        }
    }
}
