// DeviceCollapseHost.hip -- the routines of the device's 8-wide collapse (csrc/wide8_build.h), compiled for the HOST by hipcc's host pass
// (tests/native/libdevice_collapse_host.so).
//
// Test infrastructure (tests/test_device_collapse_on_host_cpu.py); nothing here is linked into or loaded by the product, which has no CPU path.
//
// wide8_build.h's routines are __host__ __device__ functions of ordinary IEEE arithmetic in a fixed order; `hipcc --cuda-host-only -ffp-contract=off` yields an x86
// build of exactly the statements the kernels run. collapse_host_wide8 walks them the way hipr_build_wide8 launches them -- the same input check and level lists, the
// bounds reduced block by block with the earliest-wins rule, the counts scanned block by block with scanned block sums, the BVH2 levels deepest first, the wide levels
// top down, sizes bottom-up, places top-down -- with the threads of every launch taken BACKWARDS, so that a result that depended on the order within a launch would
// show. The CPU suite holds the result to build_wide8 (hiprh_bvh_wide8_*) byte for byte without a GPU.
#define HIPR_BUILD_HOST_ONLY 1      // none of the kernels: this build holds host code only
#define HIPR_REFIT_HOST_ONLY 1
#define HIPR_COLLAPSE_HOST_ONLY 1
#include "../../bifrost3d_amd/csrc/wide8_build.h"

#include <cstring>
#include <vector>

using namespace hipr;

extern "C" {

unsigned collapse_host_max_levels() { return W8_MAX_LEVELS; }

// 0: collapsed. 1: refused as malformed (HIPR_ERROR_INVALID_ARGUMENT on the device), 2: declined (HIPR_ERROR_UNSUPPORTED); the outputs are untouched. -1: a collapse
// off its bounds. `message` (may be null) receives the reason of a refusal.
int collapse_host_wide8(const HiprBvhNode* nodes, uint32_t node_count, const HiprTriangle* triangles, const uint32_t* order, uint32_t triangle_count, HiprSlot8* out_slots, uint32_t slot_capacity,
                        HiprWide8BuildResult* out, char* message, uint32_t message_size) {
    char local[256] = "";
    if (!message || !message_size) { message = local; message_size = sizeof(local); }
    if (!nodes || !node_count || !triangles || !triangle_count || !out_slots || !out) { snprintf(message, message_size, "null argument, no nodes or no triangles"); return 1; }
    if (triangle_count > BUILD_MAX_TRIANGLES || node_count > BUILD_MAX_TRIANGLES) return 2;
    W8Input input;
    if (const int refused = w8_check_input(nodes, node_count, order, triangle_count, input, message, message_size)) return refused;
    const uint32_t reachable = uint32_t(input.level_nodes.size()), bvh_levels = uint32_t(input.level_first.size()) - 1u;
    constexpr uint32_t BLOCK = 256;
    const size_t T = triangle_count, N = node_count, scan_blocks = (T + BLOCK - 1) / BLOCK;
    std::vector<uint32_t> counts(T, 0u), block_sums(scan_blocks + 1, 0u), status(W8_STATUS_WORDS, 0u);
    W8State S = {};
    S.nodes = nodes; S.node_count = node_count; S.triangles = triangles; S.order = order; S.triangle_count = triangle_count;
    S.level_nodes = input.level_nodes.data(); S.reachable = reachable; S.single_leaf = input.single_leaf ? 1u : 0u;
    S.counts = counts.data(); S.block_sums = block_sums.data(); S.status = status.data();
    // 1: the bounds, per block then over the blocks, both backwards: the earliest of equal bounds wins whatever the order
    HiprWide8BuildResult result = {};
    {
        std::vector<RefitBound> partial(6 * scan_blocks);
        for (size_t b = scan_blocks; b-- > 0;) {
            RefitBound bound[6];
            for (int k = 0; k < 6; ++k) bound[k] = {k < 3 ? FLT_MAX : -FLT_MAX, 0xFFFFFFFFu};
            for (uint32_t t = uint32_t(std::min(T, (b + 1) * BLOCK)); t-- > b * BLOCK;) {
                if (!w8_triangle_finite(triangles[t])) status[W8_STATUS_NOT_FINITE] = 1u;
                const float* corners[3] = {triangles[t].v0, triangles[t].v1, triangles[t].v2};
                for (int k = 0; k < 3; ++k)
                    for (int a = 0; a < 3; ++a) {
                        const RefitBound p = {corners[k][a], 3u * t + uint32_t(k)};
                        bound[a] = refit_lower(bound[a], p);
                        bound[3 + a] = refit_upper(bound[3 + a], p);
                    }
            }
            for (int k = 0; k < 6; ++k) partial[6 * b + k] = bound[k];
        }
        RefitBound bound[6];
        for (int k = 0; k < 6; ++k) bound[k] = {k < 3 ? FLT_MAX : -FLT_MAX, 0xFFFFFFFFu};
        for (size_t b = scan_blocks; b-- > 0;)
            for (int k = 0; k < 6; ++k) bound[k] = k < 3 ? refit_lower(bound[k], partial[6 * b + k]) : refit_upper(bound[k], partial[6 * b + k]);
        const float lo[3] = {bound[0].v, bound[1].v, bound[2].v}, hi[3] = {bound[3].v, bound[4].v, bound[5].v};
        refit_grid(lo, hi, result.grid_min, result.grid_cell);
        for (int a = 0; a < 3; ++a) { S.grid_min[a] = result.grid_min[a]; S.grid_cell[a] = result.grid_cell[a]; }
    }
    // 2: the counts and their scan (k_w8_scan_local per block, k_build_scan_sums over the block sums and one word more for the total)
    for (uint32_t t = 2u * reachable; t-- > 0;) w8_count_leaf(S, t);
    for (size_t b = 0; b < scan_blocks; ++b) {
        uint32_t running = 0;
        for (size_t i = b * BLOCK; i < std::min(T, (b + 1) * BLOCK); ++i) { const uint32_t v = counts[i]; counts[i] = running; running += v; }
        block_sums[b] = running;
    }
    {
        uint32_t running = 0;
        for (size_t b = 0; b <= scan_blocks; ++b) { const uint32_t v = block_sums[b]; block_sums[b] = running; running += v; }
    }
    const uint32_t record_total = block_sums[scan_blocks];
    if (status[W8_STATUS_NOT_FINITE]) { snprintf(message, message_size, "a triangle corner or a child box is not finite"); return 1; }
    if (record_total == 0 || record_total > triangle_count) return -1;
    // 3, 4
    const size_t R = record_total, inner = N + R, wide_capacity = R;
    std::vector<RefitBox> box(inner + R), wide_all(wide_capacity);
    std::vector<int32_t> left(inner, -1), right(inner, -1), wide_child(8 * wide_capacity);
    std::vector<float> cost(7 * inner);
    std::vector<uint8_t> split(7 * inner), roots_used(7 * inner);
    std::vector<HiprLeaf8> records(R);
    std::vector<uint32_t> record_slot(R), wide_tree(wide_capacity), wide_size(wide_capacity), wide_base(wide_capacity), wide_slot(wide_capacity);
    S.record_total = record_total; S.leaf_base = uint32_t(inner); S.wide_capacity = uint32_t(wide_capacity);
    S.box = box.data(); S.left = left.data(); S.right = right.data(); S.cost = cost.data(); S.split = split.data(); S.roots_used = roots_used.data();
    S.records = records.data(); S.record_slot = record_slot.data();
    S.wide_tree = wide_tree.data(); S.wide_child = wide_child.data(); S.wide_all = wide_all.data(); S.wide_size = wide_size.data(); S.wide_base = wide_base.data(); S.wide_slot = wide_slot.data();
    for (uint32_t t = 2u * reachable; t-- > 0;) status[W8_STATUS_PAIRED] += w8_build_leaf(S, t, BLOCK);
    if (!input.single_leaf)
        for (uint32_t l = bvh_levels; l-- > 0;)
            for (uint32_t k = input.level_first[l + 1]; k-- > input.level_first[l];) w8_optimise(S, int32_t(input.level_nodes[k]));
    // 5
    std::vector<uint32_t> wide_first, wide_count;
    for (uint32_t level = 0, first = 0, count = 1; count; ++level) {
        if (level >= W8_MAX_WIDE_LEVELS || size_t(first) + count > wide_capacity) return -1;
        for (uint32_t k = count; k-- > 0;) w8_prepare(S, first + k, level, first + count);
        if (status[W8_STATUS_OVERFLOW]) return -1;
        wide_first.push_back(first); wide_count.push_back(count);
        first += count;
        count = status[W8_STATUS_LEVELS + level + 1];
    }
    const uint32_t wide_total = wide_first.back() + wide_count.back(), wide_levels = uint32_t(wide_first.size());
    // 6
    for (uint32_t l = wide_levels; l-- > 0;)
        for (uint32_t k = wide_count[l]; k-- > 0;) w8_size(S, wide_first[l] + k);
    const uint64_t slot_count = 1ull + wide_size[0];
    if (slot_count != uint64_t(wide_total) + record_total) return -1;
    if (slot_count > W8_MAX_SLOTS) { snprintf(message, message_size, "the tree needs %llu slots", (unsigned long long)slot_count); return 2; }
    if (slot_count > slot_capacity) { snprintf(message, message_size, "the tree needs %llu slots, room for %u", (unsigned long long)slot_count, slot_capacity); return 1; }
    // 7, 8
    std::vector<HiprSlot8> slots(slot_count);
    S.slots = slots.data();
    wide_slot[0] = 0u; wide_base[0] = 1u;
    for (uint32_t l = 0; l < wide_levels; ++l)
        for (uint32_t k = wide_count[l]; k-- > 0;) w8_place(S, wide_first[l] + k);
    for (uint32_t k = wide_total; k-- > 0;) w8_emit_node(S, k);
    for (uint32_t k = record_total; k-- > 0;) w8_emit_leaf(S, k);
    std::memcpy(out_slots, slots.data(), size_t(slot_count) * sizeof(HiprSlot8));
    result.slot_count = uint32_t(slot_count);
    result.height = wide_levels;
    result.node_count = wide_total; result.leaf_count = record_total; result.paired_leaves = status[W8_STATUS_PAIRED];
    *out = result;
    return 0;
}

}
