// Wide4CollapseSanitize.cpp -- a stand-alone program around collapse_host_wide4 (Wide4CollapseHost.hip: the routines of csrc/wide4_build.h walked on the host) and the
// Wide4Source wiring of build_bvh (host/BvhBuilder.cpp, compiled into the program so that the sanitizers see it too) for a run under AddressSanitizer /
// UndefinedBehaviorSanitizer on the CPU: `make -C bifrost3d_amd sanitize-wide4-collapse` builds and runs it. No GPU is touched and no product library is linked.
// Sets: one triangle (the root references its leaf twice), a fan of 12, 4097 random triangles and 140 000; each walked and held to the
// host's nodes, and with a capacity one short of the need, which must be refused with nothing written. Then build_bvh with the walk as its Wide4Source, with a source
// that declines, and with none: the same result three times.
#include "../../bifrost3d_amd/host/BvhBuilder.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace HIPRenderer;
extern "C" int collapse_host_wide4(const HiprBvhNode*, uint32_t, uint32_t, HiprWideNode*, uint32_t, HiprWide4BuildResult*, uint32_t*, char*, uint32_t);
static HiprTriangle triangle(const float* a, const float* b, const float* c, uint32_t index) {
    HiprTriangle t;
    std::memset(&t, 0, sizeof t);
    for (int k = 0; k < 3; ++k) { t.v0[k] = a[k]; t.v1[k] = b[k]; t.v2[k] = c[k]; }
    t.primitive_index = index; t.flags = HIPR_TRIANGLE_OPAQUE;
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
static int walk_as_source(void* calls, const HiprBvhNode* nodes, uint32_t node_count, uint32_t triangle_count, HiprWideNode* out_nodes, uint32_t node_capacity, HiprWide4BuildResult* out) {
    ++*static_cast<int*>(calls);
    return collapse_host_wide4(nodes, node_count, triangle_count, out_nodes, node_capacity, out, nullptr, nullptr, 0) == 0 ? HIPR_OK : HIPR_ERROR_INVALID_ARGUMENT;
}
static int declining_source(void* calls, const HiprBvhNode*, uint32_t, uint32_t, HiprWideNode*, uint32_t, HiprWide4BuildResult*) { ++*static_cast<int*>(calls); return HIPR_ERROR_UNSUPPORTED; }
static bool same(const BvhBuildResult& a, const BvhBuildResult& b) {
    return a.wide_nodes.size() == b.wide_nodes.size() && std::memcmp(a.wide_nodes.data(), b.wide_nodes.data(), a.wide_nodes.size() * sizeof(HiprWideNode)) == 0 &&
           a.wide_stack_entries == b.wide_stack_entries && a.nodes.size() == b.nodes.size() && a.order == b.order && a.max_depth == b.max_depth && a.wide8.slots.size() == b.wide8.slots.size();
}
int main() {
    const char* names[4] = {"n1", "fan", "n4097", "n140000"};
    const std::vector<HiprTriangle> sets[4] = {random_set(1), fan(12), random_set(4097), random_set(140000)};
    int walked = 0, wired = 0;
    for (int s = 0; s < 4; ++s) {
        const std::vector<HiprTriangle>& t = sets[s];
        const uint32_t n = uint32_t(t.size());
        const BvhBuildResult host = build_bvh(t);
        std::vector<HiprWideNode> wide(host.nodes.size());
        HiprWide4BuildResult r = {};
        uint32_t counters[4] = {};
        char message[256] = "";
        const int status = collapse_host_wide4(host.nodes.data(), uint32_t(host.nodes.size()), n, wide.data(), uint32_t(wide.size()), &r, counters, message, sizeof message);
        printf("%s: %u triangles, %zu BVH2 nodes: status %d, %u wide nodes on %u levels, %u stack entries, budget %u\n", names[s], n, host.nodes.size(), status, r.node_count, counters[2], r.stack_entries, counters[1]);
        if (status != 0 || r.node_count != host.wide_nodes.size() || r.stack_entries != host.wide_stack_entries || std::memcmp(wide.data(), host.wide_nodes.data(), size_t(r.node_count) * sizeof(HiprWideNode)) != 0) {
            printf("%s: the walk and the host differ\n", names[s]);
            return 1;
        }
        if (r.node_count > 1) {
            std::vector<HiprWideNode> exact(r.node_count - 1);      // one short: refused, and nothing may be written past the room
            HiprWide4BuildResult r2 = {};
            if (collapse_host_wide4(host.nodes.data(), uint32_t(host.nodes.size()), n, exact.data(), uint32_t(exact.size()), &r2, nullptr, message, sizeof message) != 1 || r2.node_count != 0) return 1;
        }
        ++walked;
        if (s == 0) continue;
        int asked = 0, declined = 0;
        Wide4SourceReport used_report, declined_report;
        const BvhBuildResult from_walk = build_bvh(t, 62, Bvh2Source(), nullptr, Wide8Source(), nullptr, Wide4Source{walk_as_source, &asked}, &used_report);
        const BvhBuildResult after_decline = build_bvh(t, 62, Bvh2Source(), nullptr, Wide8Source(), nullptr, Wide4Source{declining_source, &declined}, &declined_report);
        if (asked != 1 || declined != 1 || !used_report.asked || !used_report.used || used_report.status != 0 || !declined_report.asked || declined_report.used || declined_report.status != HIPR_ERROR_UNSUPPORTED) return 1;
        if (!same(host, from_walk) || !same(host, after_decline)) { printf("%s: the builds differ\n", names[s]); return 1; }
        ++wired;
    }
    printf("%d sets walked, %d builds wired\n", walked, wired);
    return walked == 4 && wired == 3 ? 0 : 1;
}
