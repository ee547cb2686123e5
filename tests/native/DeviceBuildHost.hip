// DeviceBuildHost.hip -- the routines of the device BVH2 build (csrc/bvh2_build.h), compiled for the HOST by hipcc's host pass (tests/native/libdevice_build_host.so).
//
// Test infrastructure (tests/test_device_build_on_host_cpu.py); nothing here is linked into or loaded by the product, which has no CPU path.
//
// bvh2_build.h's routines are __host__ __device__ functions of ordinary IEEE arithmetic in a fixed order, with integer reductions that are atomics on the device and
// plain statements here; `hipcc --cuda-host-only -ffp-contract=off` yields an x86 build of exactly the statements the kernels run. build_host_bvh2 walks them the way
// hipr_build_bvh2 launches them -- level by level over the open ranges: bounds, setup, bins, split, the scan of the left flags, scatter, copy back, leaves, then the
// short ranges; then sizes bottom-up and places top-down -- with the threads of every launch taken BACKWARDS, so that a result that depended on the order of a
// reduction would show. The CPU suite holds the result to hiprh_bvh_build byte for byte without a GPU.
#define HIPR_BUILD_HOST_ONLY 1      // none of the kernels: this build holds host code only
#include "../../bifrost3d_amd/csrc/bvh2_build.h"

#include <cstring>
#include <vector>

using namespace hipr;

extern "C" {

unsigned build_host_short_range() { return BUILD_SHORT_RANGE; }
unsigned build_host_median_lane_limit() { return BUILD_MEDIAN_LANE_LIMIT; }

// 0: built. 1: declined, decline_range[0..2) = [begin, end) of the median range no lane sorts; the outputs are untouched. -1: a bad argument or a build off its bounds.
int build_host_bvh2(const HiprTriangle* triangles, uint32_t count, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t node_capacity, uint32_t* out_node_count, uint32_t* out_order,
                    uint32_t* out_deepest, uint32_t* decline_range) {
    if (!triangles || !count || !out_nodes || !out_node_count || !out_order || !out_deepest || count > BUILD_MAX_TRIANGLES) return -1;
    const uint32_t depth_limit = max_depth > 8u ? max_depth : 8u;
    const size_t n = count, max_open = n / 4 + 2, max_long = n / BUILD_SHORT_RANGE + 2;
    const uint32_t max_levels = (depth_limit < count ? depth_limit : count) + 2u;
    std::vector<BuildBox> boxes(n);
    std::vector<float> centroids(3 * n);
    std::vector<uint32_t> order(n), seg(n), order_tmp(n), seg_tmp(n), acc(max_long * ACC_WORDS), scan_local(n), sizes(n), place(n, 0u), status(STATUS_LEVELS + 2 * size_t(max_levels + 2), 0u);
    std::vector<BuildRange> ranges[2] = {std::vector<BuildRange>(max_open), std::vector<BuildRange>(max_open)};
    std::vector<BuildSetup> setup(max_long);
    std::vector<BuildSplit> split(max_long);
    std::vector<HiprBvhNode> nodes(n), placed(n);
    std::memset(nodes.data(), 0, n * sizeof(HiprBvhNode));
    BuildState S = {};
    S.triangles = triangles; S.count = count; S.depth_limit = depth_limit;
    S.boxes = boxes.data(); S.centroids = centroids.data(); S.order = order.data(); S.seg = seg.data(); S.order_tmp = order_tmp.data(); S.seg_tmp = seg_tmp.data();
    S.acc = acc.data(); S.setup = setup.data(); S.split = split.data(); S.scan_local = scan_local.data(); S.block_sums = nullptr;
    S.nodes = nodes.data(); S.sizes = sizes.data(); S.place = place.data(); S.out_nodes = placed.data(); S.status = status.data();
    status[STATUS_DECLINE] = status[STATUS_DECLINE + 1] = 0xFFFFFFFFu;
    status[STATUS_LEVELS] = 1u;
    status[STATUS_LEVELS + 1] = count > BUILD_SHORT_RANGE ? 1u : 0u;
    for (uint32_t i = count; i-- > 0;) build_prepare(S, i);
    std::vector<uint32_t> level_nodes;
    uint32_t node_count = 1;
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
                // the scan: an exclusive prefix of the left flags over all positions (k_build_scan_local, k_build_scan_sums); a range's own prefix is a difference
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
            if (status[STATUS_DECLINE] != 0xFFFFFFFFu) {
                if (decline_range) { decline_range[0] = status[STATUS_DECLINE + 1]; decline_range[1] = status[STATUS_DECLINE]; }
                return 1;
            }
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
    if (node_count > node_capacity) return -1;
    std::memcpy(out_nodes, placed.data(), size_t(node_count) * sizeof(HiprBvhNode));
    std::memcpy(out_order, order.data(), n * 4);
    *out_node_count = node_count;
    *out_deepest = status[STATUS_DEEPEST];
    return 0;
}

}
