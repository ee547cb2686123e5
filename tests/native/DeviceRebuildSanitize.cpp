// DeviceRebuildSanitize.cpp -- a stand-alone program around rebuild_host_trees (DeviceRebuildHost.hip: the routines of csrc/scene_rebuild.h walked on the host, chained
// with the walks of the BVH2 build and the 8-wide collapse) for a run under AddressSanitizer / UndefinedBehaviorSanitizer on the CPU:
// `make -C bifrost3d_amd sanitize-device-rebuild` builds and runs it; it links no product library. Sets: a 16 x 16 quad mesh as one instance, the same mesh dealt to
// three instances, and 4097 random triangles of five instances; each stored in a shuffled order (the old tree's), which the flatten scatter must undo. Then the first
// set with one flatten position claimed twice, which must be refused with nothing written.
#include "../../include/hiprenderer_c.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
extern "C" int rebuild_host_trees(HiprTriangle*, uint8_t*, uint32_t, uint32_t, uint32_t, HiprBvhNode*, uint32_t*, HiprSlot8*, uint32_t*);
static HiprTriangle triangle(const float* a, const float* b, const float* c) {
    HiprTriangle t;
    std::memset(&t, 0, sizeof t);
    for (int k = 0; k < 3; ++k) { t.v0[k] = a[k]; t.v1[k] = b[k]; t.v2[k] = c[k]; }
    t.flags = HIPR_TRIANGLE_OPAQUE;
    return t;
}
static std::vector<HiprTriangle> grid(int cells) {
    std::vector<float> v(size_t(cells + 1) * (cells + 1) * 3);
    srand(16);
    for (int i = 0; i <= cells; ++i) for (int j = 0; j <= cells; ++j) { float* p = &v[(size_t(i) * (cells + 1) + j) * 3]; p[0] = float(i) / cells; p[1] = float(j) / cells; p[2] = 0.05f * (rand() / float(RAND_MAX)); }
    std::vector<HiprTriangle> t;
    auto at = [&](int i, int j) { return &v[(size_t(i) * (cells + 1) + j) * 3]; };
    for (int i = 0; i < cells; ++i) for (int j = 0; j < cells; ++j) {
        t.push_back(triangle(at(i, j), at(i + 1, j), at(i + 1, j + 1)));
        t.push_back(triangle(at(i, j), at(i + 1, j + 1), at(i, j + 1)));
    }
    return t;
}
static std::vector<HiprTriangle> random_set(uint32_t n) {
    std::vector<HiprTriangle> t(n);
    srand(n);
    for (uint32_t i = 0; i < n; ++i) {
        float c[3], corner[3][3];
        for (float& x : c) x = rand() / float(RAND_MAX);
        for (auto& p : corner) for (int k = 0; k < 3; ++k) p[k] = c[k] + 0.02f * (rand() / float(RAND_MAX) - 0.5f);
        t[i] = triangle(corner[0], corner[1], corner[2]);
    }
    return t;
}
// The flat triangles dealt to `instances` instances in runs, numbered, then stored in a shuffled order with a class byte that names the flatten position.
static void deal_and_shuffle(std::vector<HiprTriangle>& t, uint32_t instances, std::vector<uint8_t>& classes) {
    const uint32_t n = uint32_t(t.size()), run = (n + instances - 1) / instances;
    for (uint32_t i = 0; i < n; ++i) { t[i].instance_index = i / run; t[i].primitive_index = i % run; }
    classes.resize(n);
    std::vector<uint32_t> at(n);
    for (uint32_t i = 0; i < n; ++i) at[i] = i;
    srand(n + instances);
    for (uint32_t i = n; i-- > 1;) std::swap(at[i], at[uint32_t(rand()) % (i + 1)]);
    std::vector<HiprTriangle> shuffled(n);
    for (uint32_t i = 0; i < n; ++i) { shuffled[i] = t[at[i]]; classes[i] = uint8_t(at[i] & 1u); }
    t.swap(shuffled);
}
int main() {
    const char* names[3] = {"grid16 x 1", "grid16 x 3", "n4097 x 5"};
    std::vector<HiprTriangle> sets[3] = {grid(16), grid(16), random_set(4097)};
    const uint32_t instances[3] = {1, 3, 5};
    int walked = 0;
    for (int s = 0; s < 3; ++s) {
        std::vector<HiprTriangle> t = sets[s];
        std::vector<uint8_t> classes;
        deal_and_shuffle(t, instances[s], classes);
        const uint32_t n = uint32_t(t.size());
        std::vector<HiprBvhNode> nodes(n > 1 ? n - 1 : 1); std::vector<uint32_t> order(n); std::vector<HiprSlot8> slots(2 * size_t(n)); uint32_t out[13] = {};
        const int status = rebuild_host_trees(t.data(), classes.data(), n, instances[s], 62, nodes.data(), order.data(), slots.data(), out);
        printf("%s: %u triangles: status %d, %u BVH2 nodes, deepest %u, %u slots, height %u\n", names[s], n, status, out[0], out[1], out[2], out[3]);
        if (status != 0) return 1;
        std::vector<bool> seen(n, false);
        const uint32_t run = (n + instances[s] - 1) / instances[s];
        for (uint32_t k = 0; k < n; ++k) {      // `order` is a permutation, and the triangle at place k is the one of flatten position order[k], with its class byte
            if (order[k] >= n || seen[order[k]] || t[k].instance_index * run + t[k].primitive_index != order[k] || classes[k] != uint8_t(order[k] & 1u)) { printf("%s: place %u is wrong\n", names[s], k); return 1; }
            seen[order[k]] = true;
        }
        ++walked;
    }
    {   // a duplicate position: refused, nothing written
        std::vector<HiprTriangle> t = sets[0];
        std::vector<uint8_t> classes;
        deal_and_shuffle(t, 1, classes);
        t[7].primitive_index = t[8].primitive_index;
        const std::vector<HiprTriangle> before = t;
        const uint32_t n = uint32_t(t.size());
        std::vector<HiprBvhNode> nodes(n - 1); std::vector<uint32_t> order(n, 0xA5A5A5A5u); std::vector<HiprSlot8> slots(2 * size_t(n)); uint32_t out[13] = {};
        const int status = rebuild_host_trees(t.data(), classes.data(), n, 1, 62, nodes.data(), order.data(), slots.data(), out);
        printf("a position claimed twice: status %d\n", status);
        if (status != 1 || std::memcmp(t.data(), before.data(), n * sizeof(HiprTriangle)) || out[0] || order[0] != 0xA5A5A5A5u) return 1;
    }
    printf("%d sets walked\n", walked);
    return walked == 3 ? 0 : 1;
}
