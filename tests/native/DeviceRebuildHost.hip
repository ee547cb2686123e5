// DeviceRebuildHost.hip -- the routines of the device rebuild of the resident scene's trees (csrc/scene_rebuild.h), compiled for the HOST by hipcc's host pass
// (tests/native/libdevice_rebuild_host.so), chained with the host walks of the BVH2 build (csrc/bvh2_build.h) and the 8-wide collapse (csrc/wide8_build.h).
//
// Test infrastructure (tests/test_device_rebuild_on_host_cpu.py); nothing here is linked into or loaded by the product, which has no CPU path.
//
// rebuild_host_trees walks what hipr_rebuild_scene_trees launches, in its order and with the threads of every launch taken BACKWARDS: the count per instance, the
// host's prefix sums, the scatter to flatten order with its claim words, the BVH2 build over the flat array as DeviceBuildHost.hip walks it, the hand-over -- the
// collapse's level lists are place[] in creation order and the build's level sizes, NOT w8_check_input's walk -- the collapse as DeviceCollapseHost.hip walks it,
// and the gather of the new resident triangles and class bytes. The CPU suite holds the result to SceneBuilder::rebuild() byte for byte without a GPU.
#define HIPR_BUILD_HOST_ONLY 1      // none of the kernels: this build holds host code only
#define HIPR_REFIT_HOST_ONLY 1
#define HIPR_COLLAPSE_HOST_ONLY 1
#define HIPR_REBUILD_HOST_ONLY 1
#include "../../bifrost3d_amd/csrc/scene_rebuild.h"
#include "../../bifrost3d_amd/csrc/wide8_build.h"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace hipr;

namespace {

// DeviceBuildHost.hip's walk, leaving the placed nodes, the order, place[] and the level sizes. 0: built; 1: declined; -1: off its bounds.
int walk_bvh2(const HiprTriangle* triangles, uint32_t count, uint32_t depth_limit, std::vector<HiprBvhNode>& placed, std::vector<uint32_t>& order, std::vector<uint32_t>& place,
              std::vector<uint32_t>& level_nodes, uint32_t& node_count, uint32_t& deepest) {
    const size_t n = count, max_open = n / 4 + 2, max_long = n / BUILD_SHORT_RANGE + 2;
    const uint32_t max_levels = std::min(depth_limit, count) + 2u;
    std::vector<BuildBox> boxes(n);
    std::vector<float> centroids(3 * n);
    std::vector<uint32_t> seg(n), order_tmp(n), seg_tmp(n), acc(max_long * ACC_WORDS), scan_local(n), sizes(n), status(STATUS_LEVELS + 2 * size_t(max_levels + 2), 0u);
    std::vector<BuildRange> ranges[2] = {std::vector<BuildRange>(max_open), std::vector<BuildRange>(max_open)};
    std::vector<BuildSetup> setup(max_long);
    std::vector<BuildSplit> split(max_long);
    std::vector<HiprBvhNode> nodes(n);
    std::memset(nodes.data(), 0, n * sizeof(HiprBvhNode));
    placed.assign(n, HiprBvhNode{}); order.assign(n, 0u); place.assign(n, 0u); level_nodes.clear();
    BuildState S = {};
    S.triangles = triangles; S.count = count; S.depth_limit = depth_limit;
    S.boxes = boxes.data(); S.centroids = centroids.data(); S.order = order.data(); S.seg = seg.data(); S.order_tmp = order_tmp.data(); S.seg_tmp = seg_tmp.data();
    S.acc = acc.data(); S.setup = setup.data(); S.split = split.data(); S.scan_local = scan_local.data(); S.block_sums = nullptr;
    S.nodes = nodes.data(); S.sizes = sizes.data(); S.place = place.data(); S.out_nodes = placed.data(); S.status = status.data();
    status[STATUS_DECLINE] = status[STATUS_DECLINE + 1] = 0xFFFFFFFFu;
    status[STATUS_LEVELS] = 1u;
    status[STATUS_LEVELS + 1] = count > BUILD_SHORT_RANGE ? 1u : 0u;
    for (uint32_t i = count; i-- > 0;) build_prepare(S, i);
    node_count = 1;
    if (count <= BUILD_LEAF_MAX) build_single_leaf(S);
    else {
        ranges[0][0] = {0u, count, 1u, BUILD_NONE, count > BUILD_SHORT_RANGE ? 0u : BUILD_NONE, 0u};
        uint32_t open = 1, long_ranges = count > BUILD_SHORT_RANGE ? 1u : 0u, node_base = 0;
        for (uint32_t level = 0; open; ++level) {
            if (level >= max_levels || node_base + open > count - 1u || open > max_open - 2 || long_ranges > max_long - 2) return -1;
            const BuildLevel L = {ranges[level & 1u].data(), ranges[(level + 1u) & 1u].data(), open, node_base, level};
            if (long_ranges) {
                for (size_t w = size_t(long_ranges) * ACC_WORDS; w-- > 0;) build_acc_init(S.acc, w);
                for (uint32_t i = count; i-- > 0;) build_bounds_element(S, L, i);
                for (uint32_t k = open; k-- > 0;) build_range_setup(S, L, k);
                for (uint32_t i = count; i-- > 0;) build_bins_element(S, L, i);
                for (uint32_t k = open; k-- > 0;) build_split_range(S, L, k, true);
                std::vector<uint32_t> prefix(n);
                uint32_t running = 0;
                for (uint32_t i = 0; i < count; ++i) { const uint32_t flag = build_left_flag(S, L, i); scan_local[i] = flag; prefix[i] = running; running += flag; }
                for (uint32_t i = count; i-- > 0;) {
                    const BuildRange* r = build_long_range(S, L, i);
                    if (r) build_scatter(S, L, i, scan_local[i], prefix[i] - prefix[r->begin]);
                }
                for (uint32_t i = count; i-- > 0;) build_copy_back(S, L, i);
                for (uint32_t k = open; k-- > 0;) build_leaves_range(S, L, k);
            }
            for (uint32_t k = open; k-- > 0;) build_split_range(S, L, k, false);
            if (status[STATUS_DECLINE] != 0xFFFFFFFFu) return 1;
            level_nodes.push_back(open);
            node_base += open;
            open = status[STATUS_LEVELS + 2 * (level + 1)];
            long_ranges = status[STATUS_LEVELS + 2 * (level + 1) + 1];
        }
        node_count = node_base;
        std::vector<uint32_t> first(level_nodes.size());
        for (size_t l = 0, at = 0; l < level_nodes.size(); at += level_nodes[l++]) first[l] = uint32_t(at);
        for (size_t l = level_nodes.size(); l-- > 0;)
            for (uint32_t k = level_nodes[l]; k-- > 0;) build_count_node(S, first[l] + k);
        for (size_t l = 0; l < level_nodes.size(); ++l)
            for (uint32_t k = level_nodes[l]; k-- > 0;) build_place_node(S, first[l] + k);
    }
    deepest = status[STATUS_DEEPEST];
    return 0;
}

// DeviceCollapseHost.hip's walk from the bounds on, over level lists that are GIVEN. 0: collapsed; 2: more slots than a node addresses; -1: off its bounds.
int walk_wide8(W8State& S, const std::vector<uint32_t>& level_first, std::vector<HiprSlot8>& slots, HiprWide8BuildResult& result) {
    constexpr uint32_t BLOCK = 256;
    const uint32_t triangle_count = S.triangle_count, reachable = S.reachable, bvh_levels = uint32_t(level_first.size()) - 1u;
    const size_t T = triangle_count, N = S.node_count, scan_blocks = (T + BLOCK - 1) / BLOCK;
    std::vector<uint32_t> counts(T, 0u), block_sums(scan_blocks + 1, 0u), status(W8_STATUS_WORDS, 0u);
    S.counts = counts.data(); S.block_sums = block_sums.data(); S.status = status.data();
    result = {};
    {
        std::vector<RefitBound> partial(6 * scan_blocks);
        for (size_t b = scan_blocks; b-- > 0;) {
            RefitBound bound[6];
            for (int k = 0; k < 6; ++k) bound[k] = {k < 3 ? FLT_MAX : -FLT_MAX, 0xFFFFFFFFu};
            for (uint32_t t = uint32_t(std::min(T, (b + 1) * BLOCK)); t-- > b * BLOCK;) {
                if (!w8_triangle_finite(S.triangles[t])) status[W8_STATUS_NOT_FINITE] = 1u;
                const float* corners[3] = {S.triangles[t].v0, S.triangles[t].v1, S.triangles[t].v2};
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
    if (status[W8_STATUS_NOT_FINITE] || record_total == 0 || record_total > triangle_count) return -1;
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
    if (!S.single_leaf)
        for (uint32_t l = bvh_levels; l-- > 0;)
            for (uint32_t k = level_first[l + 1]; k-- > level_first[l];) w8_optimise(S, int32_t(S.level_nodes[k]));
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
    for (uint32_t l = wide_levels; l-- > 0;)
        for (uint32_t k = wide_count[l]; k-- > 0;) w8_size(S, wide_first[l] + k);
    const uint64_t slot_count = 1ull + wide_size[0];
    if (slot_count != uint64_t(wide_total) + record_total) return -1;
    if (slot_count > W8_MAX_SLOTS) return 2;
    slots.assign(slot_count, HiprSlot8{});
    S.slots = slots.data();
    wide_slot[0] = 0u; wide_base[0] = 1u;
    for (uint32_t l = 0; l < wide_levels; ++l)
        for (uint32_t k = wide_count[l]; k-- > 0;) w8_place(S, wide_first[l] + k);
    for (uint32_t k = wide_total; k-- > 0;) w8_emit_node(S, k);
    for (uint32_t k = record_total; k-- > 0;) w8_emit_leaf(S, k);
    result.slot_count = uint32_t(slot_count);
    result.height = wide_levels;
    result.node_count = wide_total; result.leaf_count = record_total; result.paired_leaves = status[W8_STATUS_PAIRED];
    return 0;
}

}

extern "C" {

// The resident triangles (`triangles`, in the old tree's order) and class bytes rebuilt IN PLACE; out_nodes (room for max(count, 1) - 1, at least 1), out_order (count words),
// out_slots (room for 2 x count) and out[0..13) = {node_count, deepest, the eleven words of HiprWide8BuildResult} receive the trees. 0: rebuilt. 1: two triangles claim one
// flatten position, or one lies outside its instance's range; 2: the BVH2 build declined; 3: the trees are higher than the kernels walk, or need more slots than a
// node addresses. Every refusal leaves all arrays untouched. -1: a bad argument or a walk off its bounds.
int rebuild_host_trees(HiprTriangle* triangles, uint8_t* classes, uint32_t count, uint32_t instance_count, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t* out_order, HiprSlot8* out_slots,
                       uint32_t* out) {
    if (!triangles || !classes || !count || !out_nodes || !out_order || !out_slots || !out || count > BUILD_MAX_TRIANGLES) return -1;
    // the flatten order
    std::vector<uint32_t> instance_counts(instance_count, 0u), first(size_t(instance_count) + 1, 0u), claim(count, 0u), status(REBUILD_STATUS_WORDS, 0u);
    std::vector<HiprTriangle> flat(count);
    std::vector<uint8_t> flat_class(count, 0);
    const RebuildArrays a = {triangles, classes, count, instance_count, instance_counts.data(), first.data(), flat.data(), flat_class.data(), claim.data(), status.data()};
    for (uint32_t t = count; t-- > 0;) rebuild_count(a, t);
    uint64_t total = 0;
    for (uint32_t i = 0; i < instance_count; ++i) { total += instance_counts[i]; first[i + 1] = uint32_t(total); }
    if (total != count) return 1;
    for (uint32_t t = count; t-- > 0;) rebuild_scatter(a, t);
    if (status[REBUILD_STATUS_CLAIM]) return 1;
    // the BVH2 over the flat array
    std::vector<HiprBvhNode> placed;
    std::vector<uint32_t> order, place, level_sizes;
    uint32_t node_count = 0, deepest = 0;
    const int built = walk_bvh2(flat.data(), count, std::max(max_depth, 8u), placed, order, place, level_sizes, node_count, deepest);
    if (built) return built == 1 ? 2 : -1;
    const uint32_t bvh_levels = std::max<uint32_t>(uint32_t(level_sizes.size()), 1u);
    if (bvh_levels > W8_MAX_LEVELS || deepest + 1u > 64u) return 3;
    // the hand-over, and the collapse
    std::vector<uint32_t> level_nodes(node_count), level_first(size_t(bvh_levels) + 1, 0u);
    for (uint32_t k = node_count; k-- > 0;) rebuild_level_node(place.data(), level_nodes.data(), k);
    if (level_sizes.empty()) level_first[1] = 1u;
    else for (uint32_t l = 0; l < bvh_levels; ++l) level_first[l + 1] = level_first[l] + level_sizes[l];
    W8State S = {};
    S.nodes = placed.data(); S.node_count = node_count; S.triangles = flat.data(); S.order = order.data(); S.triangle_count = count;
    S.level_nodes = level_nodes.data(); S.reachable = node_count; S.single_leaf = level_sizes.empty() ? 1u : 0u;
    std::vector<HiprSlot8> slots;
    HiprWide8BuildResult wide8 = {};
    const int collapsed = walk_wide8(S, level_first, slots, wide8);
    if (collapsed) return collapsed == 2 ? 3 : -1;
    if (wide8.height > 33u) return 3;
    // the new resident arrays
    for (uint32_t k = count; k-- > 0;) rebuild_gather(flat.data(), flat_class.data(), order.data(), triangles, classes, k);
    std::memcpy(out_nodes, placed.data(), size_t(node_count) * sizeof(HiprBvhNode));
    std::memcpy(out_order, order.data(), size_t(count) * 4);
    std::memcpy(out_slots, slots.data(), slots.size() * sizeof(HiprSlot8));
    out[0] = node_count; out[1] = deepest;
    static_assert(sizeof(HiprWide8BuildResult) == 11 * 4, "eleven words");
    std::memcpy(out + 2, &wide8, sizeof(wide8));
    return 0;
}

}
