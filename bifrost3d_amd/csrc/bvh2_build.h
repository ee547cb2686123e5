// bvh2_build.h -- the binned-SAH BVH2 of host/BvhBuilder.cpp built on the device (hipr_build_bvh2; the reference asks OptiX for a "Trbvh" build, which runs
// on the GPU, OR/Renderer.cpp:161-182,471-476).
//
// The yardstick is BYTE EQUALITY with the host builder (Builder::split / build of host/BvhBuilder.cpp): the same nodes in the same depth-first places, the same
// triangle order, the same deepest leaf. The host builder's result depends only on input order and values, so a level-synchronous build can restate it: the
// routines below restate its arithmetic and decisions operation for operation -- the two libraries do not link each other -- as __host__ __device__ functions,
// so that tests/native/DeviceBuildHost.hip can compile them for the host and the CPU suite can hold them to hiprh_bvh_build without a GPU. Everything is IEEE f32
// in a fixed order (the unit is built with -ffp-contract=off and IEEE division; this header must never reach the fast-math shade unit).
//
// Shape. The open ranges of one tree level are split by one set of launches on the context's stream; no block waits on another, nothing spins, and the host
// reads a few words per level (the ranges still open, the long ones among them, a decline) to know when to stop. Two regimes, cut at BUILD_SHORT_RANGE:
//   long ranges   one thread per triangle position: bounds and bins are integer atomics into the range's accumulator (k_build_bounds reduces a wave that lies
//                 in one range by shuffles first, k_build_bins a block that lies in one range in LDS first), one lane sweeps the bins (k_build_split), and the
//                 stable partition is a scan of the left flags -- a block scan (k_build_scan_local), a scan of the block sums (k_build_scan_sums) and the
//                 scatter (k_build_scatter) in separate launches; the difference of two prefixes of the one scan over all positions is the segmented scan;
//   short ranges  one lane per range does what the host does, serially and in place: bounds, bins, sweep, stable partition or sort.
// After the last level: subtree sizes bottom-up (k_build_count, one launch per level), then depth-first indices top-down and the nodes written to their final
// places (k_build_place): the left child is parent + 1, the right child parent + 1 + nodes(left subtree), which is the order the host's recursion appends in.
//
// What decides byte equality:
//   * Signed zeros. The host's sweeps replace a bound only by a strictly smaller / larger value, so among value-equal candidates the earliest in range order
//     wins and a bound of -0.0f or +0.0f is whichever came first. CHILD BOXES are stored in the nodes, so there the sign is visible: a long range reduces a
//     64-bit key of (ordered canonical value, position in the range) under integer atomicMin / atomicMax -- for the maximum the position is complemented, so the
//     earliest wins there too -- and the bound's bits are then fetched from that element (build_range_setup). A short range or a leaf is swept in range order
//     with the host's comparison (build_min / build_max). CENTROID BOUNDS and BIN BOXES are never stored: they feed bin_of, the extents and half areas, where
//     the sign of a zero cannot change a value that is compared (x - (+0) and x - (-0) differ only for x = 0, by the sign of a zero; a half area or a cost of
//     -0 compares like +0), so they are plain ordered-integer keys with -0 folded onto +0 -- the rule is not paid for twice.
//   * No float atomic adds anywhere: counts are integers, bounds are integer min / max.
//   * The SAH partition cannot fail: the bin of an element is one expression (build_bin_of with scale = 16 / extent by one IEEE division) in the bins and in the
//     partition, so the left side holds exactly the n_left > 0 elements the sweep counted, and the host's fall-through from a partition with an empty side to
//     the median is unreachable. The split position is therefore known from the sweep, before the partition runs.
//   * The median path (the depth budget, or coincident centroids) is a std::stable_sort by one centroid axis, whose result is fully determined: a range of at
//     most BUILD_MEDIAN_LANE_LIMIT elements is insertion-sorted by its lane. A build that meets a longer median range DECLINES (BuildStatus::decline names the
//     range): hipr_build_bvh2 returns HIPR_ERROR_UNSUPPORTED and writes nothing. A segmented device sort is a later change.
//   * Leaf size 3 and 16 bins are compiled in; a host configured otherwise (HIPR_BVH_LEAF_SIZE, HIPR_BVH_BINS, HIPR_BVH_REINSERTION) does not ask the device.
//   * Non-finite corners are refused before the device is touched: the host's int() of a NaN is undefined, so there is nothing to equal.
// The order in which ranges and nodes get their slots within a level is an integer atomic counter's, so it may differ run to run; nothing of it reaches the
// output, whose places come from the tree's shape alone.
#pragma once

#include "../../include/hiprenderer_c.h"

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#define BHD __host__ __device__ inline

namespace hipr {

constexpr int BUILD_BINS = 16;                         // BvhBuilder.cpp BIN_COUNT
constexpr uint32_t BUILD_LEAF_MAX = 3;                 // BvhBuilder.cpp leaf_max()
// Tuning value: ranges of at most this many triangles are split by one lane each, longer ones cooperatively. It bounds the accumulators (count / 64 long ranges
// at 1 416 B each, 22 B per triangle) and the private arrays of a lane. -DHIPR_BUILD_SHORT_RANGE=n builds another cut for an A/B measurement. Measured on the MI355X (profiles/device_build_vs_host.txt):
// 32 / 64 / 128 give 8.2 / 8.8 / 10.1 ms for the 251 k atrium and 215 / 201 / 194 ms for the 10 M atrium, the same tree each time: 32 is 6 % faster at 251 k and 7 % slower at 10 M, 128 is 15 % slower and 4 % faster; 64 loses least across both.
#ifndef HIPR_BUILD_SHORT_RANGE
#define HIPR_BUILD_SHORT_RANGE 64
#endif
constexpr uint32_t BUILD_SHORT_RANGE = HIPR_BUILD_SHORT_RANGE;
constexpr uint32_t BUILD_MEDIAN_LANE_LIMIT = BUILD_SHORT_RANGE;      // the longest range a lane sorts for the median path; longer ones decline
constexpr uint32_t BUILD_NONE = 0xFFFFFFFFu;
constexpr uint32_t BUILD_MAX_TRIANGLES = 1u << 28;     // leaf_ref keeps the first triangle in 28 bits

struct BuildBox { float lo[3], hi[3]; };
struct BuildRange { uint32_t begin, end, depth, parent_slot /* 2 * node + child, BUILD_NONE for the root */, long_index /* BUILD_NONE: a short range */, _pad; };
struct BuildSetup { float lo[3], hi[3], scale[3]; uint32_t force_median; };                      // a long range's centroid bounds and bin scales
struct BuildSplit { int32_t axis, bin; float lo, scale; uint32_t mid, child_slot[2], _pad; };   // a long range's partition
struct BuildBins { BuildBox box[3][BUILD_BINS]; uint32_t n[3][BUILD_BINS]; };

// A long range's accumulator, in words: the six child-box keys (64 bit), the six centroid bound keys, the bin counts, the bin boxes' keys.
constexpr uint32_t ACC_BOX = 0, ACC_CB = 12, ACC_N = 18, ACC_BIN_LO = 66, ACC_BIN_HI = 210, ACC_WORDS = 354;
// BuildState::status, in words: the decline key (64 bit: begin << 32 | end of the first range by position), the deepest leaf, then {open, long} ranges of every level.
constexpr uint32_t STATUS_DECLINE = 0, STATUS_DEEPEST = 2, STATUS_LEVELS = 4;

struct BuildState {
    const HiprTriangle* triangles; uint32_t count, depth_limit;
    BuildBox* boxes; float* centroids;                       // per input triangle
    uint32_t *order, *seg, *order_tmp, *seg_tmp;             // per position: the permutation, and the slot of the open range the position lies in (BUILD_NONE: closed)
    uint32_t* acc; BuildSetup* setup; BuildSplit* split;     // per long range of the level
    uint32_t *scan_local, *block_sums;                       // the partition's scan
    HiprBvhNode* nodes; uint32_t *sizes, *place;             // the nodes in creation order (a level's nodes are consecutive), their subtree sizes and final places
    HiprBvhNode* out_nodes;
    uint32_t* status;
};
struct BuildLevel { const BuildRange* ranges; BuildRange* next; uint32_t open, node_base, level; };

BHD uint32_t build_bits(float v) { union { float f; uint32_t u; } x; x.f = v; return x.u; }
BHD float build_float(uint32_t u) { union { float f; uint32_t u; } x; x.u = u; return x.f; }
// std::min(a, b) / std::max(a, b) as BvhBuilder.cpp's Box uses them: the first argument stays unless the second is strictly beyond it.
BHD float build_min(float a, float b) { return b < a ? b : a; }
BHD float build_max(float a, float b) { return a < b ? b : a; }
BHD void build_box_reset(BuildBox& b) { for (int a = 0; a < 3; ++a) { b.lo[a] = FLT_MAX; b.hi[a] = -FLT_MAX; } }
BHD void build_box_grow(BuildBox& b, const float* p) { for (int a = 0; a < 3; ++a) { b.lo[a] = build_min(b.lo[a], p[a]); b.hi[a] = build_max(b.hi[a], p[a]); } }
BHD void build_box_grow(BuildBox& b, const BuildBox& o) { for (int a = 0; a < 3; ++a) { b.lo[a] = build_min(b.lo[a], o.lo[a]); b.hi[a] = build_max(b.hi[a], o.hi[a]); } }
BHD float build_half_area(const BuildBox& b) {
    const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
    return dx * dy + dy * dz + dz * dx;
}
// build_bvh: the box of a triangle and its centroid.
BHD void build_triangle(const HiprTriangle& t, BuildBox& box, float* centroid) {
    build_box_reset(box);
    build_box_grow(box, t.v0); build_box_grow(box, t.v1); build_box_grow(box, t.v2);
    for (int a = 0; a < 3; ++a) centroid[a] = 0.5f * (box.lo[a] + box.hi[a]);
}
BHD int build_bin_of(float centroid, float lo, float scale) {
    const int b = int((centroid - lo) * scale);
    return b < 0 ? 0 : (b > BUILD_BINS - 1 ? BUILD_BINS - 1 : b);
}
BHD uint32_t build_levels_needed(uint32_t count) {
    uint32_t leaves = (count + BUILD_LEAF_MAX - 1) / BUILD_LEAF_MAX, levels = 0;
    while ((1u << levels) < leaves) ++levels;
    return levels;
}
BHD bool build_force_median(uint32_t depth, uint32_t count, uint32_t depth_limit) { return depth + build_levels_needed(count) >= depth_limit; }
BHD void build_scales(const BuildBox& cb, float* scale) {
    for (int axis = 0; axis < 3; ++axis) {
        const float extent = cb.hi[axis] - cb.lo[axis];
        scale[axis] = extent > 0.0f ? BUILD_BINS / extent : 0.0f;
    }
}
BHD int32_t build_leaf_ref(uint32_t first, uint32_t count) { return ~int32_t((first << 3) | (count - 1)); }
// store_child's box: the six floats of child c, nothing else of the node.
BHD void build_store_box(HiprBvhNode& n, int c, const BuildBox& b) {
    float* xy = c == 0 ? n.c0xy : n.c1xy;
    xy[0] = b.lo[0]; xy[1] = b.hi[0]; xy[2] = b.lo[1]; xy[3] = b.hi[1];
    n.cz[2 * c] = b.lo[2]; n.cz[2 * c + 1] = b.hi[2];
}

// The SAH sweep of Builder::split over the bins of one range: right-to-left areas and counts, then left-to-right; strict <, axis-major then bin order, so the first
// minimum wins; empty sides and axes without extent skipped. false: no split (the median path). `left_count`: the elements of bins 0 .. bin of the axis.
BHD bool build_sweep(const BuildBins& bins, const float* scale, int& best_axis, int& best_bin, uint32_t& left_count) {
    best_axis = -1; best_bin = -1; left_count = 0;
    float best_cost = FLT_MAX;
    for (int axis = 0; axis < 3; ++axis) {
        if (!(scale[axis] > 0.0f)) continue;
        const BuildBox* bin_box = bins.box[axis];
        const uint32_t* bin_n = bins.n[axis];
        float right_area[BUILD_BINS];
        uint32_t right_n[BUILD_BINS];
        BuildBox acc; build_box_reset(acc);
        uint32_t n = 0;
        for (int b = BUILD_BINS - 1; b > 0; --b) {
            if (bin_n[b]) build_box_grow(acc, bin_box[b]);
            n += bin_n[b];
            right_area[b] = n ? build_half_area(acc) : 0.0f;
            right_n[b] = n;
        }
        build_box_reset(acc);
        n = 0;
        for (int b = 0; b < BUILD_BINS - 1; ++b) {
            if (bin_n[b]) build_box_grow(acc, bin_box[b]);
            n += bin_n[b];
            if (n == 0 || right_n[b + 1] == 0) continue;
            const float cost = build_half_area(acc) * float(n) + right_area[b + 1] * float(right_n[b + 1]);
            if (cost < best_cost) { best_cost = cost; best_axis = axis; best_bin = b; left_count = n; }
        }
    }
    return best_axis >= 0;
}
// The axis of the median split: the widest centroid extent, the first among equals.
BHD int build_median_axis(const BuildBox& cb) {
    int axis = 0;
    for (int a = 1; a < 3; ++a)
        if (cb.hi[a] - cb.lo[a] > cb.hi[axis] - cb.lo[axis]) axis = a;
    return axis;
}

// ---- ordered keys and the integer reductions (atomics on the device; the host build of the routines runs them serially) ----
// Unsigned order = float order; -0 folds onto +0.
BHD uint32_t build_key(float v) { uint32_t u = build_bits(v); if (u == 0x80000000u) u = 0u; return (u >> 31) ? ~u : (u | 0x80000000u); }
BHD float build_unkey(uint32_t k) { return build_float((k >> 31) ? (k ^ 0x80000000u) : ~k); }
BHD unsigned long long build_lower_key(float v, uint32_t position) { return (unsigned long long)(build_key(v)) << 32 | position; }          // under min: the earliest of the smallest
BHD unsigned long long build_upper_key(float v, uint32_t position) { return (unsigned long long)(build_key(v)) << 32 | (~position); }       // under max: the earliest of the largest
BHD void build_atomic_min(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}
BHD void build_atomic_max(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}
BHD void build_atomic_min(unsigned long long* p, unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}
BHD void build_atomic_max(unsigned long long* p, unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}
BHD uint32_t build_atomic_add(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(p, v);
#else
    const uint32_t old = *p; *p = old + v; return old;
#endif
}

// ---- the passes, one call per thread ----
BHD void build_prepare(const BuildState& S, uint32_t i) {
    build_triangle(S.triangles[i], S.boxes[i], S.centroids + 3 * size_t(i));
    S.order[i] = i;
    S.seg[i] = 0u;      // the root range
}
// One word of the level's accumulators.
BHD void build_acc_init(uint32_t* acc, size_t word) {
    const uint32_t w = uint32_t(word % ACC_WORDS);
    const bool lower = w < 6u || (w >= ACC_CB && w < ACC_CB + 3u) || (w >= ACC_BIN_LO && w < ACC_BIN_HI);
    acc[word] = lower ? 0xFFFFFFFFu : 0u;
}
// The long range position i lies in, or null.
BHD const BuildRange* build_long_range(const BuildState& S, const BuildLevel& L, uint32_t i) {
    const uint32_t k = S.seg[i];
    if (k == BUILD_NONE) return nullptr;
    const BuildRange* r = L.ranges + k;
    return r->long_index == BUILD_NONE ? nullptr : r;
}
// (a) bounds of the long ranges, one element: its six box keys and six centroid keys.
BHD void build_bounds_keys(const BuildState& S, const BuildRange& r, uint32_t i, unsigned long long* box_key, uint32_t* cb_key) {
    const uint32_t t = S.order[i], position = i - r.begin;
    const BuildBox& box = S.boxes[t];
    const float* c = S.centroids + 3 * size_t(t);
    for (int a = 0; a < 3; ++a) {
        box_key[a] = build_lower_key(box.lo[a], position); box_key[3 + a] = build_upper_key(box.hi[a], position);
        cb_key[a] = build_key(c[a]); cb_key[3 + a] = cb_key[a];
    }
}
BHD void build_bounds_commit(const BuildState& S, const BuildRange& r, const unsigned long long* box_key, const uint32_t* cb_key) {
    uint32_t* acc = S.acc + size_t(r.long_index) * ACC_WORDS;
    unsigned long long* box = reinterpret_cast<unsigned long long*>(acc + ACC_BOX);
    for (int a = 0; a < 3; ++a) {
        build_atomic_min(box + a, box_key[a]); build_atomic_max(box + 3 + a, box_key[3 + a]);
        build_atomic_min(acc + ACC_CB + a, cb_key[a]); build_atomic_max(acc + ACC_CB + 3 + a, cb_key[3 + a]);
    }
}
BHD void build_bounds_element(const BuildState& S, const BuildLevel& L, uint32_t i) {
    const BuildRange* r = build_long_range(S, L, i);
    if (!r) return;
    unsigned long long box_key[6]; uint32_t cb_key[6];
    build_bounds_keys(S, *r, i, box_key, cb_key);
    build_bounds_commit(S, *r, box_key, cb_key);
}
// One lane per range after (a): a long range's child box fetched from the elements its keys name and stored in the parent, its centroid bounds, scales and budget.
BHD void build_range_setup(const BuildState& S, const BuildLevel& L, uint32_t k) {
    const BuildRange& r = L.ranges[k];
    if (r.long_index == BUILD_NONE) return;
    const uint32_t* acc = S.acc + size_t(r.long_index) * ACC_WORDS;
    if (r.parent_slot != BUILD_NONE) {
        const unsigned long long* keys = reinterpret_cast<const unsigned long long*>(acc + ACC_BOX);
        BuildBox box;
        for (int a = 0; a < 3; ++a) {
            box.lo[a] = S.boxes[S.order[r.begin + uint32_t(keys[a])]].lo[a];
            box.hi[a] = S.boxes[S.order[r.begin + ~uint32_t(keys[3 + a])]].hi[a];
        }
        build_store_box(S.nodes[r.parent_slot >> 1], int(r.parent_slot & 1u), box);
    }
    BuildSetup s;
    BuildBox cb;
    for (int a = 0; a < 3; ++a) { cb.lo[a] = s.lo[a] = build_unkey(acc[ACC_CB + a]); cb.hi[a] = s.hi[a] = build_unkey(acc[ACC_CB + 3 + a]); }
    build_scales(cb, s.scale);
    s.force_median = build_force_median(r.depth, r.end - r.begin, S.depth_limit) ? 1u : 0u;
    S.setup[r.long_index] = s;
}
// (b) bins of the long ranges, one element.
BHD void build_bins_element(const BuildState& S, const BuildLevel& L, uint32_t i) {
    const BuildRange* r = build_long_range(S, L, i);
    if (!r) return;
    const BuildSetup& s = S.setup[r->long_index];
    if (s.force_median) return;
    uint32_t* acc = S.acc + size_t(r->long_index) * ACC_WORDS;
    const uint32_t t = S.order[i];
    const BuildBox& box = S.boxes[t];
    for (int axis = 0; axis < 3; ++axis) {
        if (!(s.scale[axis] > 0.0f)) continue;
        const uint32_t slot = uint32_t(axis * BUILD_BINS + build_bin_of(S.centroids[3 * size_t(t) + axis], s.lo[axis], s.scale[axis]));
        build_atomic_add(acc + ACC_N + slot, 1u);
        for (int a = 0; a < 3; ++a) { build_atomic_min(acc + ACC_BIN_LO + 3 * slot + a, build_key(box.lo[a])); build_atomic_max(acc + ACC_BIN_HI + 3 * slot + a, build_key(box.hi[a])); }
    }
}
BHD void build_load_bins(const uint32_t* acc, BuildBins& bins) {
    for (int axis = 0; axis < 3; ++axis)
        for (int b = 0; b < BUILD_BINS; ++b) {
            const uint32_t slot = uint32_t(axis * BUILD_BINS + b);
            bins.n[axis][b] = acc[ACC_N + slot];
            for (int a = 0; a < 3; ++a) { bins.box[axis][b].lo[a] = build_unkey(acc[ACC_BIN_LO + 3 * slot + a]); bins.box[axis][b].hi[a] = build_unkey(acc[ACC_BIN_HI + 3 * slot + a]); }
        }
}
// bounds_of over positions [begin, end), in range order.
BHD BuildBox build_bounds_of(const BuildState& S, uint32_t begin, uint32_t end) {
    BuildBox b; build_box_reset(b);
    for (uint32_t i = begin; i < end; ++i) build_box_grow(b, S.boxes[S.order[i]]);
    return b;
}
BHD void build_decline(const BuildState& S, const BuildRange& r) {
    build_atomic_min(reinterpret_cast<unsigned long long*>(S.status + STATUS_DECLINE), (unsigned long long)(r.begin) << 32 | r.end);
}

// (c) one lane per range: the split of Builder::split and the node of Builder::build. A short range is also partitioned (or sorted) here, in place; a long range
// leaves its partition rule in BuildState::split for (d). Ranges whose regime is not `want_long` are left to the other launch.
BHD void build_split_range(const BuildState& S, const BuildLevel& L, uint32_t k, bool want_long) {
    const BuildRange r = L.ranges[k];
    const bool is_long = r.long_index != BUILD_NONE;
    if (is_long != want_long) return;
    const uint32_t begin = r.begin, end = r.end, count = end - begin, node = L.node_base + k;
    uint32_t ids[BUILD_SHORT_RANGE];
    BuildBox cb;
    bool force_median;
    float scale[3];
    BuildBins bins;
    if (is_long) {
        const BuildSetup& s = S.setup[r.long_index];
        for (int a = 0; a < 3; ++a) { cb.lo[a] = s.lo[a]; cb.hi[a] = s.hi[a]; scale[a] = s.scale[a]; }
        force_median = s.force_median != 0u;
        if (!force_median) build_load_bins(S.acc + size_t(r.long_index) * ACC_WORDS, bins);
    } else {
        build_box_reset(cb);
        for (uint32_t j = 0; j < count; ++j) { ids[j] = S.order[begin + j]; build_box_grow(cb, S.centroids + 3 * size_t(ids[j])); }
        if (r.parent_slot != BUILD_NONE) build_store_box(S.nodes[r.parent_slot >> 1], int(r.parent_slot & 1u), build_bounds_of(S, begin, end));
        force_median = build_force_median(r.depth, count, S.depth_limit);
        if (!force_median) {
            build_scales(cb, scale);
            for (int a = 0; a < 3; ++a) for (int b = 0; b < BUILD_BINS; ++b) { build_box_reset(bins.box[a][b]); bins.n[a][b] = 0u; }
            for (uint32_t j = 0; j < count; ++j)
                for (int axis = 0; axis < 3; ++axis) {
                    if (!(scale[axis] > 0.0f)) continue;
                    const int b = build_bin_of(S.centroids[3 * size_t(ids[j]) + axis], cb.lo[axis], scale[axis]);
                    build_box_grow(bins.box[axis][b], S.boxes[ids[j]]);
                    bins.n[axis][b]++;
                }
        }
    }
    int best_axis = -1, best_bin = -1;
    uint32_t left_count = 0, mid;
    if (!force_median && build_sweep(bins, scale, best_axis, best_bin, left_count)) {
        const float extent = cb.hi[best_axis] - cb.lo[best_axis];
        const float split_scale = BUILD_BINS / extent, lo = cb.lo[best_axis];
        mid = begin + left_count;
        if (is_long) {
            BuildSplit& sp = S.split[r.long_index];
            sp.axis = best_axis; sp.bin = best_bin; sp.lo = lo; sp.scale = split_scale; sp.mid = mid;
        } else {      // std::stable_partition
            uint32_t lw = begin, rw = mid;
            for (uint32_t j = 0; j < count; ++j) {
                if (build_bin_of(S.centroids[3 * size_t(ids[j]) + best_axis], lo, split_scale) <= best_bin) S.order[lw++] = ids[j]; else S.order[rw++] = ids[j];
            }
        }
    } else {
        if (count > BUILD_MEDIAN_LANE_LIMIT) {      // every long range that gets here
            build_decline(S, r);
            // The level's remaining launches still run: a rule that keeps every element of the range where it is, and closes it.
            if (is_long) { const BuildSplit stay = {0, BUILD_BINS, 0.0f, 0.0f, end, {BUILD_NONE, BUILD_NONE}, 0u}; S.split[r.long_index] = stay; }
            return;
        }
        const int axis = build_median_axis(cb);
        for (uint32_t j = 1; j < count; ++j) {      // std::stable_sort: an insertion sort is stable, and a stable sort has one result
            const uint32_t x = ids[j];
            const float cx = S.centroids[3 * size_t(x) + axis];
            uint32_t p = j;
            while (p > 0 && cx < S.centroids[3 * size_t(ids[p - 1]) + axis]) { ids[p] = ids[p - 1]; --p; }
            ids[p] = x;
        }
        for (uint32_t j = 0; j < count; ++j) S.order[begin + j] = ids[j];
        mid = begin + count / 2;
    }
    // Builder::build: the two children. An open child's box arrives with the next level; a leaf's is swept here (short) or after the partition (long, build_leaves_range).
    const uint32_t child_range[2][2] = {{begin, mid}, {mid, end}};
    for (int c = 0; c < 2; ++c) {
        const uint32_t b = child_range[c][0], e = child_range[c][1];
        uint32_t slot = BUILD_NONE;
        if (e - b <= BUILD_LEAF_MAX) {
            S.nodes[node].child[c] = build_leaf_ref(b, e - b);
            if (!is_long) build_store_box(S.nodes[node], c, build_bounds_of(S, b, e));
            build_atomic_max(S.status + STATUS_DEEPEST, r.depth + 1u);
        } else {
            slot = build_atomic_add(S.status + STATUS_LEVELS + 2u * (L.level + 1u), 1u);
            const uint32_t long_index = e - b > BUILD_SHORT_RANGE ? build_atomic_add(S.status + STATUS_LEVELS + 2u * (L.level + 1u) + 1u, 1u) : BUILD_NONE;
            const BuildRange child = {b, e, r.depth + 1u, 2u * node + uint32_t(c), long_index, 0u};
            L.next[slot] = child;
            S.nodes[node].child[c] = int32_t(L.node_base + L.open + slot);
        }
        if (is_long) S.split[r.long_index].child_slot[c] = slot;
        else for (uint32_t j = b; j < e; ++j) S.seg[j] = slot;
    }
}
// (d) the stable partition of the long ranges. The left flag of position i; the scatter given the left elements of its range before it.
BHD uint32_t build_left_flag(const BuildState& S, const BuildLevel& L, uint32_t i) {
    const BuildRange* r = build_long_range(S, L, i);
    if (!r) return 0u;
    const BuildSplit& sp = S.split[r->long_index];
    return build_bin_of(S.centroids[3 * size_t(S.order[i]) + sp.axis], sp.lo, sp.scale) <= sp.bin ? 1u : 0u;
}
BHD void build_scatter(const BuildState& S, const BuildLevel& L, uint32_t i, uint32_t left, uint32_t lefts_before) {
    const BuildRange* r = build_long_range(S, L, i);
    if (!r) return;
    const BuildSplit& sp = S.split[r->long_index];
    const uint32_t to = left ? r->begin + lefts_before : sp.mid + (i - r->begin - lefts_before);
    S.order_tmp[to] = S.order[i];
    S.seg_tmp[to] = sp.child_slot[left ? 0 : 1];
}
BHD void build_copy_back(const BuildState& S, const BuildLevel& L, uint32_t i) {
    if (!build_long_range(S, L, i)) return;
    S.order[i] = S.order_tmp[i];
    S.seg[i] = S.seg_tmp[i];
}
// One lane per long range after (d): the boxes of its leaf children, in the order the partition left.
BHD void build_leaves_range(const BuildState& S, const BuildLevel& L, uint32_t k) {
    if (L.ranges[k].long_index == BUILD_NONE) return;
    HiprBvhNode& n = S.nodes[L.node_base + k];
    for (int c = 0; c < 2; ++c) {
        if (n.child[c] >= 0) continue;
        const uint32_t code = uint32_t(~n.child[c]), first = code >> 3, leaf_count = (code & 7u) + 1u;
        build_store_box(n, c, build_bounds_of(S, first, first + leaf_count));
    }
}
// The numbering. Children are created after their parents, level by level: sizes from the last level up, places from the root down.
BHD void build_count_node(const BuildState& S, uint32_t node) {
    const HiprBvhNode& n = S.nodes[node];
    S.sizes[node] = 1u + (n.child[0] >= 0 ? S.sizes[n.child[0]] : 0u) + (n.child[1] >= 0 ? S.sizes[n.child[1]] : 0u);
}
BHD void build_place_node(const BuildState& S, uint32_t node) {
    HiprBvhNode n = S.nodes[node];
    const uint32_t at = S.place[node];      // place[0] = 0
    uint32_t next = at + 1u;
    for (int c = 0; c < 2; ++c) {
        if (n.child[c] < 0) continue;
        const uint32_t child = uint32_t(n.child[c]);
        S.place[child] = next;
        n.child[c] = int32_t(next);
        next += S.sizes[child];
    }
    S.out_nodes[at] = n;
}
// count <= 3: a single leaf, both children reference it.
BHD void build_single_leaf(const BuildState& S) {
    HiprBvhNode root = {};
    const BuildBox box = build_bounds_of(S, 0u, S.count);
    for (int c = 0; c < 2; ++c) { build_store_box(root, c, box); root.child[c] = build_leaf_ref(0u, S.count); }
    S.out_nodes[0] = root;
    S.status[STATUS_DEEPEST] = 1u;
}

#if defined(__HIPCC__) && !defined(HIPR_BUILD_HOST_ONLY)      // the kernels; a host build of the routines (tests/native/DeviceBuildHost.hip) leaves them out

constexpr int BUILD_BLOCK = 256;

__global__ __launch_bounds__(BUILD_BLOCK) void k_build_prepare(BuildState S) {
    const uint32_t i = blockIdx.x * uint32_t(BUILD_BLOCK) + threadIdx.x;
    if (i < S.count) build_prepare(S, i);
}
__global__ __launch_bounds__(BUILD_BLOCK) void k_build_single_leaf(BuildState S) {
    if (blockIdx.x == 0 && threadIdx.x == 0) build_single_leaf(S);
}
__global__ __launch_bounds__(BUILD_BLOCK) void k_build_acc_init(uint32_t* __restrict__ acc, uint64_t words) {
    const uint64_t w = blockIdx.x * uint64_t(BUILD_BLOCK) + threadIdx.x;
    if (w < words) build_acc_init(acc, size_t(w));
}
// (a). A wave whose 64 positions lie in one long range reduces its keys by shuffles and commits once; any other wave commits per lane.
__global__ __launch_bounds__(BUILD_BLOCK) void k_build_bounds(BuildState S, BuildLevel L) {
    const uint32_t i = blockIdx.x * uint32_t(BUILD_BLOCK) + threadIdx.x;
    const BuildRange* r = i < S.count ? build_long_range(S, L, i) : nullptr;
    const uint32_t mine = r ? r->long_index : BUILD_NONE;
    const uint32_t first = uint32_t(__shfl(int(mine), 0, 64));
    const bool uniform = __all(mine == first);
    if (uniform && first == BUILD_NONE) return;
    unsigned long long box_key[6]; uint32_t cb_key[6];
    if (r) build_bounds_keys(S, *r, i, box_key, cb_key);
    if (!uniform) { if (r) build_bounds_commit(S, *r, box_key, cb_key); return; }
    for (int mask = 32; mask >= 1; mask >>= 1)
        for (int a = 0; a < 3; ++a) {
            const unsigned long long lo = (unsigned long long)(__shfl_xor((long long)(box_key[a]), mask, 64)), hi = (unsigned long long)(__shfl_xor((long long)(box_key[3 + a]), mask, 64));
            box_key[a] = lo < box_key[a] ? lo : box_key[a]; box_key[3 + a] = hi > box_key[3 + a] ? hi : box_key[3 + a];
            const uint32_t clo = uint32_t(__shfl_xor(int(cb_key[a]), mask, 64)), chi = uint32_t(__shfl_xor(int(cb_key[3 + a]), mask, 64));
            cb_key[a] = clo < cb_key[a] ? clo : cb_key[a]; cb_key[3 + a] = chi > cb_key[3 + a] ? chi : cb_key[3 + a];
        }
    if ((threadIdx.x & 63u) == 0u) build_bounds_commit(S, *r, box_key, cb_key);
}
__global__ __launch_bounds__(BUILD_BLOCK) void k_build_range_setup(BuildState S, BuildLevel L) {
    const uint32_t k = blockIdx.x * uint32_t(BUILD_BLOCK) + threadIdx.x;
    if (k < L.open) build_range_setup(S, L, k);
}
// (b). A block whose 256 positions lie in one long range fills bins in LDS and adds them to the range's with one atomic per touched word; any other block
// goes to the range's bins directly.
__global__ __launch_bounds__(BUILD_BLOCK) void k_build_bins(BuildState S, BuildLevel L) {
    __shared__ uint32_t local[ACC_WORDS];
    __shared__ uint32_t block_range;
    const uint32_t i = blockIdx.x * uint32_t(BUILD_BLOCK) + threadIdx.x;
    const BuildRange* r = i < S.count ? build_long_range(S, L, i) : nullptr;
    const uint32_t mine = r ? r->long_index : BUILD_NONE;
    if (threadIdx.x == 0) block_range = mine;
    __syncthreads();
    const uint32_t first = block_range;
    const bool uniform = __syncthreads_and(mine == first) != 0;
    if (!uniform) { if (r) build_bins_element(S, L, i); return; }
    if (first == BUILD_NONE) return;
    const BuildSetup& s = S.setup[first];
    if (s.force_median) return;
    for (uint32_t w = threadIdx.x; w < ACC_WORDS; w += uint32_t(BUILD_BLOCK)) build_acc_init(local, w);
    __syncthreads();
    {
        const uint32_t t = S.order[i];
        const BuildBox& box = S.boxes[t];
        for (int axis = 0; axis < 3; ++axis) {
            if (!(s.scale[axis] > 0.0f)) continue;
            const uint32_t slot = uint32_t(axis * BUILD_BINS + build_bin_of(S.centroids[3 * size_t(t) + axis], s.lo[axis], s.scale[axis]));
            atomicAdd(local + ACC_N + slot, 1u);
            for (int a = 0; a < 3; ++a) { atomicMin(local + ACC_BIN_LO + 3 * slot + a, build_key(box.lo[a])); atomicMax(local + ACC_BIN_HI + 3 * slot + a, build_key(box.hi[a])); }
        }
    }
    __syncthreads();
    uint32_t* acc = S.acc + size_t(first) * ACC_WORDS;
    for (uint32_t w = ACC_N + threadIdx.x; w < ACC_WORDS; w += uint32_t(BUILD_BLOCK)) {
        const uint32_t v = local[w];
        if (w < ACC_BIN_LO) { if (v) atomicAdd(acc + w, v); }
        else if (w < ACC_BIN_HI) { if (v != 0xFFFFFFFFu) atomicMin(acc + w, v); }
        else if (v) atomicMax(acc + w, v);
    }
}
__global__ __launch_bounds__(BUILD_BLOCK) void k_build_split(BuildState S, BuildLevel L, int want_long) {
    const uint32_t k = blockIdx.x * uint32_t(BUILD_BLOCK) + threadIdx.x;
    if (k < L.open) build_split_range(S, L, k, want_long != 0);
}
// The exclusive scan of one value per thread over the block; `total` the block's sum.
__device__ __forceinline__ uint32_t build_block_scan(uint32_t value, uint32_t& total) {
    __shared__ uint32_t wave_sums[BUILD_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inclusive = value;
    for (int step = 1; step < 64; step <<= 1) {
        const uint32_t below = uint32_t(__shfl_up(int(inclusive), step, 64));
        if (lane >= uint32_t(step)) inclusive += below;
    }
    __syncthreads();      // an earlier scan's readers are done with wave_sums
    if (lane == 63u) wave_sums[wave] = inclusive;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
    for (uint32_t w = 0; w < uint32_t(BUILD_BLOCK / 64); ++w) { if (w < wave) before += wave_sums[w]; total += wave_sums[w]; }
    return before + inclusive - value;
}
// (d) 1: the left flags of a block's positions scanned, the block's sum kept.
__global__ __launch_bounds__(BUILD_BLOCK) void k_build_scan_local(BuildState S, BuildLevel L) {
    const uint32_t i = blockIdx.x * uint32_t(BUILD_BLOCK) + threadIdx.x;
    const uint32_t flag = i < S.count ? build_left_flag(S, L, i) : 0u;
    uint32_t total;
    const uint32_t before = build_block_scan(flag, total);
    if (i < S.count) S.scan_local[i] = before << 1 | flag;
    if (threadIdx.x == 0) S.block_sums[blockIdx.x] = total;
}
// (d) 2: one block scans the block sums in place, 256 at a time with a carry.
__global__ __launch_bounds__(BUILD_BLOCK) void k_build_scan_sums(uint32_t* __restrict__ block_sums, uint32_t blocks) {
    uint32_t carry = 0;
    for (uint32_t base = 0; base < blocks; base += uint32_t(BUILD_BLOCK)) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t value = b < blocks ? block_sums[b] : 0u;
        uint32_t total;
        const uint32_t before = build_block_scan(value, total);
        if (b < blocks) block_sums[b] = carry + before;
        carry += total;
    }
}
// (d) 3: every position of a long range goes to its place on its side.
__global__ __launch_bounds__(BUILD_BLOCK) void k_build_scatter(BuildState S, BuildLevel L) {
    const uint32_t i = blockIdx.x * uint32_t(BUILD_BLOCK) + threadIdx.x;
    if (i >= S.count) return;
    const BuildRange* r = build_long_range(S, L, i);
    if (!r) return;
    const uint32_t mine = S.scan_local[i], first = S.scan_local[r->begin];
    const uint32_t prefix = S.block_sums[i / uint32_t(BUILD_BLOCK)] + (mine >> 1), range_prefix = S.block_sums[r->begin / uint32_t(BUILD_BLOCK)] + (first >> 1);
    build_scatter(S, L, i, mine & 1u, prefix - range_prefix);
}
__global__ __launch_bounds__(BUILD_BLOCK) void k_build_copy_back(BuildState S, BuildLevel L) {
    const uint32_t i = blockIdx.x * uint32_t(BUILD_BLOCK) + threadIdx.x;
    if (i < S.count) build_copy_back(S, L, i);
}
__global__ __launch_bounds__(BUILD_BLOCK) void k_build_leaves(BuildState S, BuildLevel L) {
    const uint32_t k = blockIdx.x * uint32_t(BUILD_BLOCK) + threadIdx.x;
    if (k < L.open) build_leaves_range(S, L, k);
}
__global__ __launch_bounds__(BUILD_BLOCK) void k_build_count(BuildState S, uint32_t first_node, uint32_t node_count) {
    const uint32_t k = blockIdx.x * uint32_t(BUILD_BLOCK) + threadIdx.x;
    if (k < node_count) build_count_node(S, first_node + k);
}
__global__ __launch_bounds__(BUILD_BLOCK) void k_build_place(BuildState S, uint32_t first_node, uint32_t node_count) {
    const uint32_t k = blockIdx.x * uint32_t(BUILD_BLOCK) + threadIdx.x;
    if (k < node_count) build_place_node(S, first_node + k);
}

#endif // the kernels

} // namespace hipr
