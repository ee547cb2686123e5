// DeviceCollapseSanitize.cpp -- a stand-alone program around collapse_host_wide8 (DeviceCollapseHost.hip: the routines of csrc/wide8_build.h walked on the host) for a run
// under AddressSanitizer / UndefinedBehaviorSanitizer on the CPU: `make -C bifrost3d_amd sanitize-device-collapse` builds and runs it. The BVH2 it collapses comes from
// build_host_bvh2 (DeviceBuildHost.hip), so that the program links no product library. Sets: a 16 x 16 quad mesh (most records paired), a fan of 12 triangles around one
// corner, and 4097 random triangles (one past a block of blocks); each also with a slot capacity one short of the need, which must be refused.
#include "../../include/hiprenderer_c.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
extern "C" int build_host_bvh2(const HiprTriangle*, uint32_t, uint32_t, HiprBvhNode*, uint32_t, uint32_t*, uint32_t*, uint32_t*, uint32_t*);
extern "C" int collapse_host_wide8(const HiprBvhNode*, uint32_t, const HiprTriangle*, const uint32_t*, uint32_t, HiprSlot8*, uint32_t, HiprWide8BuildResult*, char*, uint32_t);
static HiprTriangle triangle(const float* a, const float* b, const float* c, uint32_t index) {
    HiprTriangle t;
    std::memset(&t, 0, sizeof t);
    for (int k = 0; k < 3; ++k) { t.v0[k] = a[k]; t.v1[k] = b[k]; t.v2[k] = c[k]; }
    t.primitive_index = index; t.flags = HIPR_TRIANGLE_OPAQUE;
    return t;
}
static std::vector<HiprTriangle> grid(int cells) {
    std::vector<float> v(size_t(cells + 1) * (cells + 1) * 3);
    srand(16);
    for (int i = 0; i <= cells; ++i) for (int j = 0; j <= cells; ++j) { float* p = &v[(size_t(i) * (cells + 1) + j) * 3]; p[0] = float(i) / cells; p[1] = float(j) / cells; p[2] = 0.05f * (rand() / float(RAND_MAX)); }
    std::vector<HiprTriangle> t;
    auto at = [&](int i, int j) { return &v[(size_t(i) * (cells + 1) + j) * 3]; };
    for (int i = 0; i < cells; ++i) for (int j = 0; j < cells; ++j) {
        t.push_back(triangle(at(i, j), at(i + 1, j), at(i + 1, j + 1), uint32_t(t.size())));
        t.push_back(triangle(at(i, j), at(i + 1, j + 1), at(i, j + 1), uint32_t(t.size())));
    }
    return t;
}
static std::vector<HiprTriangle> fan(int n) {
    std::vector<HiprTriangle> t;
    const float centre[3] = {0, 0, 0};
    std::vector<float> rim(size_t(n) * 3);
    for (int k = 0; k < n; ++k) { const float a = 6.2831853f * k / n; rim[3 * k] = std::cos(a); rim[3 * k + 1] = std::sin(a); rim[3 * k + 2] = 0.1f * std::cos(3 * a); }
    for (int k = 0; k < n; ++k) t.push_back(triangle(centre, &rim[3 * k], &rim[3 * ((k + 1) % n)], uint32_t(k)));
    return t;
}
static std::vector<HiprTriangle> random_set(uint32_t n) {
    std::vector<HiprTriangle> t(n);
    srand(n);
    for (uint32_t i = 0; i < n; ++i) {
        float c[3], corner[3][3];
        for (float& x : c) x = rand() / float(RAND_MAX);
        for (auto& p : corner) for (int k = 0; k < 3; ++k) p[k] = c[k] + 0.02f * (rand() / float(RAND_MAX) - 0.5f);
        t[i] = triangle(corner[0], corner[1], corner[2], i);
    }
    return t;
}
int main() {
    const char* names[3] = {"grid16", "fan", "n4097"};
    const std::vector<HiprTriangle> sets[3] = {grid(16), fan(12), random_set(4097)};
    int walked = 0;
    for (int s = 0; s < 3; ++s) {
        const std::vector<HiprTriangle>& t = sets[s];
        const uint32_t n = uint32_t(t.size());
        std::vector<HiprBvhNode> nodes(n > 1 ? n - 1 : 1); std::vector<uint32_t> order(n); uint32_t count = 0, deepest = 0, decline[2] = {0, 0};
        if (build_host_bvh2(t.data(), n, 62, nodes.data(), uint32_t(nodes.size()), &count, order.data(), &deepest, decline) != 0) { printf("%s: no BVH2\n", names[s]); return 1; }
        std::vector<HiprSlot8> slots(2 * size_t(n));
        HiprWide8BuildResult r = {};
        char message[256] = "";
        const int status = collapse_host_wide8(nodes.data(), count, t.data(), order.data(), n, slots.data(), uint32_t(slots.size()), &r, message, sizeof message);
        printf("%s: %u triangles, %u BVH2 nodes: status %d, %u slots, height %u, %u nodes, %u records of which %u paired\n", names[s], n, count, status, r.slot_count, r.height, r.node_count, r.leaf_count, r.paired_leaves);
        if (status != 0 || r.slot_count != r.node_count + r.leaf_count) return 1;
        std::vector<HiprSlot8> exact(r.slot_count - 1);      // one short: refused, and nothing may be written past the room
        HiprWide8BuildResult r2 = {};
        if (collapse_host_wide8(nodes.data(), count, t.data(), order.data(), n, exact.data(), uint32_t(exact.size()), &r2, message, sizeof message) != 1 || r2.slot_count != 0) return 1;
        ++walked;
    }
    printf("%d sets walked\n", walked);
    return walked == 3 ? 0 : 1;
}
