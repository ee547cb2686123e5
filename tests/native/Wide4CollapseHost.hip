// Wide4CollapseHost.hip -- the routines of the device's 4-wide collapse (csrc/wide4_build.h), compiled for the HOST by hipcc's host pass
// (tests/native/libwide4_collapse_host.so).
//
// Test infrastructure (tests/test_wide4_collapse_on_host_cpu.py); nothing here is linked into or loaded by the product, which has no CPU path.
//
// wide4_build.h's routines are __host__ __device__ functions of ordinary IEEE arithmetic in a fixed order; `hipcc --cuda-host-only -ffp-contract=off` yields an x86
// build of exactly the statements the kernels run. collapse_host_wide4 walks them the way hipr_build_wide4 launches them -- the same input check and level lists, the
// BVH2 levels deepest first, the wide levels top down with their frontier lists, sizes bottom-up, positions top-down -- with the threads of every launch taken
// BACKWARDS, so that a result that depended on the order within a launch (the order of a level's frontier) would show. The CPU suite holds the result to the host's
// WideCollapse (hiprh_bvh_wide_nodes, hiprh_wide4_collapse) byte for byte without a GPU.
#define HIPR_BUILD_HOST_ONLY 1      // none of the kernels: this build holds host code only
#define HIPR_REFIT_HOST_ONLY 1
#define HIPR_COLLAPSE_HOST_ONLY 1
#include "../../bifrost3d_amd/csrc/wide4_build.h"

#include <cstring>
#include <vector>

using namespace hipr;

extern "C" {

// 0: collapsed. 1: refused as malformed (HIPR_ERROR_INVALID_ARGUMENT on the device); the outputs are untouched. -1: a collapse off its bounds. `message` (may be
// null) receives the reason of a refusal. `counters` (may be null) receives what the walk met: [0] frontier entries that left the adoption loop because one more
// child did not fit the budget, [1] the root's budget, [2] the wide levels, [3] binary_need of the root.
int collapse_host_wide4(const HiprBvhNode* nodes, uint32_t node_count, uint32_t triangle_count, HiprWideNode* out_nodes, uint32_t node_capacity, HiprWide4BuildResult* out, uint32_t* counters,
                        char* message, uint32_t message_size) {
    char local[256] = "";
    if (!message || !message_size) { message = local; message_size = sizeof(local); }
    if (!nodes || !node_count || !out_nodes || !out) { snprintf(message, message_size, "null argument or no nodes"); return 1; }
    if (node_count > BUILD_MAX_TRIANGLES) { snprintf(message, message_size, "%u nodes", node_count); return 1; }
    W8Input input;
    if (w8_check_input(nodes, node_count, nullptr, triangle_count, input, message, message_size) == W8_INPUT_INVALID) return 1;
    const uint32_t reachable = uint32_t(input.level_nodes.size()), bvh_levels = uint32_t(input.level_first.size()) - 1u;
    std::vector<uint32_t> need(node_count, 0u), status(W4_STATUS_WORDS, 0u);
    W4State S = {};
    S.nodes = nodes; S.node_count = node_count; S.level_nodes = input.level_nodes.data(); S.need = need.data(); S.status = status.data();
    // 2
    for (uint32_t l = bvh_levels; l-- > 0;)
        for (uint32_t k = input.level_first[l + 1]; k-- > input.level_first[l];) w4_need(S, input.level_nodes[k]);
    if (status[W4_STATUS_NOT_FINITE]) { snprintf(message, message_size, "a child box is not finite"); return 1; }
    const uint32_t budget = need[0] <= W4_SMALL_BUDGET ? W4_SMALL_BUDGET : W4_LARGE_BUDGET;
    // 3
    const size_t capacity = reachable;
    std::vector<uint32_t> wide_root(capacity), wide_budget(capacity), wide_size(capacity), wide_stack(capacity), wide_at(capacity);
    std::vector<HiprWideNode> made(capacity);
    S.wide_capacity = uint32_t(capacity); S.wide_root = wide_root.data(); S.wide_budget = wide_budget.data(); S.made = made.data();
    S.wide_size = wide_size.data(); S.wide_stack = wide_stack.data(); S.wide_at = wide_at.data();
    wide_root[0] = 0u; wide_budget[0] = budget;
    std::vector<uint32_t> wide_first, wide_count;
    uint32_t did_not_fit = 0;
    for (uint32_t level = 0, first = 0, count = 1; count; ++level) {
        if (level >= W4_MAX_WIDE_LEVELS || size_t(first) + count > capacity) return -1;
        for (uint32_t k = count; k-- > 0;) did_not_fit += w4_collapse(S, first + k, level, first + count) ? 1u : 0u;
        if (status[W4_STATUS_OVERFLOW]) return -1;
        wide_first.push_back(first); wide_count.push_back(count);
        first += count;
        count = status[W4_STATUS_LEVELS + level + 1];
    }
    const uint32_t wide_total = wide_first.back() + wide_count.back(), wide_levels = uint32_t(wide_first.size());
    if (wide_total > node_capacity) { snprintf(message, message_size, "the tree needs %u nodes, room for %u", wide_total, node_capacity); return 1; }
    // 4
    for (uint32_t l = wide_levels; l-- > 0;)
        for (uint32_t k = wide_count[l]; k-- > 0;) w4_size(S, wide_first[l] + k);
    if (wide_size[0] != wide_total) return -1;
    // 5
    std::vector<HiprWideNode> placed(wide_total);
    std::memset(placed.data(), 0xA5, size_t(wide_total) * sizeof(HiprWideNode));      // a position the walk left out would show
    S.out = placed.data();
    wide_at[0] = 0u;
    for (uint32_t l = 0; l < wide_levels; ++l)
        for (uint32_t k = wide_count[l]; k-- > 0;) w4_place_emit(S, wide_first[l] + k);
    std::memcpy(out_nodes, placed.data(), size_t(wide_total) * sizeof(HiprWideNode));
    out->node_count = wide_total; out->stack_entries = wide_stack[0];
    if (counters) { counters[0] = did_not_fit; counters[1] = budget; counters[2] = wide_levels; counters[3] = need[0]; }
    return 0;
}

// w4_quantise over `groups` child-box groups: boxes = 4 x (lo xyz, hi xyz) floats per group, counts = children per group (1 .. 4).
void collapse_host_wide4_quantise(const float* boxes, const uint32_t* counts, uint32_t groups, HiprWideNode* out) {
    for (uint32_t g = 0; g < groups; ++g) {
        RefitBox b[4];
        for (uint32_t k = 0; k < counts[g]; ++k)
            for (int a = 0; a < 3; ++a) { b[k].lo[a] = boxes[24 * size_t(g) + 6 * k + a]; b[k].hi[a] = boxes[24 * size_t(g) + 6 * k + 3 + a]; }
        HiprWideNode w;
        std::memset(&w, 0, sizeof(w));
        w4_quantise(b, counts[g], w);
        out[g] = w;
    }
}

}
