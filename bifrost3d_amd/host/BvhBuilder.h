// host/BvhBuilder.h -- see BvhBuilder.cpp.
#pragma once

#include "../../include/hiprenderer_c.h"
#include "Wide8Builder.h"

#include <cstdint>
#include <vector>

namespace HIPRenderer {

struct BvhBuildResult {
    std::vector<HiprBvhNode> nodes;   // node 0 is the root; empty for an empty scene
    std::vector<uint32_t> order;      // order[k] = index of the input triangle stored at leaf slot k
    uint32_t max_depth = 0;           // upper bound of the traversal stack entries the tree needs
    // The same tree collapsed to compressed 4-wide nodes (HiprWideNode); empty when the scene is empty.
    std::vector<HiprWideNode> wide_nodes;
    uint32_t wide_stack_entries = 0;  // most entries a traversal of wide_nodes can have on its stack
    // The same tree collapsed to the 8-wide slots of include/hiprenderer_c.h "wide8" (Wide8Builder.cpp): what the persistent kernels walk.
    Wide8Result wide8;
    // Ranges the BVH2 stage split at the median (the depth budget, or coincident centroids) and the longest of them: what a device build (Bvh2Source) has to sort.
    // Zero when a source built the BVH2.
    uint32_t median_splits = 0, longest_median_range = 0;
};

// A BVH2 stage supplied by the caller in place of the host's binned-SAH builder: hipr_build_bvh2's signature behind a context pointer (csrc/bvh2_build.h builds
// the host builder's tree byte for byte on the device). Returns HIPR_OK, or the status of a decline or an error, with the outputs untouched.
struct Bvh2Source {
    int (*build)(void* context, const HiprTriangle* triangles, uint32_t count, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t node_capacity, uint32_t* out_node_count,
                 uint32_t* out_order, uint32_t* out_deepest) = nullptr;
    void* context = nullptr;
    explicit operator bool() const { return build != nullptr; }
};
// What became of the source in one build_bvh. `fall_back` is the consumer's decision: true, a source that declines or fails is followed by the host's BVH2 stage and the
// build carries on; false, build_bvh returns an empty result and the consumer hands `status` out.
struct Bvh2SourceReport {
    bool fall_back = true;
    bool asked = false;          // the source was called (it is not when the host builder is configured away from leaf size 3 / 16 bins / no reinsertion)
    bool used = false;           // ... and its tree is the result's
    int status = 0;              // what it returned
    double seconds = 0.0;        // ... and how long it took
};

// The 8-wide collapse supplied by the caller in place of build_wide8: hipr_build_wide8's signature behind a context pointer (csrc/wide8_build.h collapses to the host's
// tree byte for byte on the device, in the default configuration only). Returns HIPR_OK, or the status of a decline or an error, with the outputs untouched.
struct Wide8Source {
    int (*build)(void* context, const HiprBvhNode* nodes, uint32_t node_count, const HiprTriangle* triangles, const uint32_t* order, uint32_t triangle_count, HiprSlot8* out_slots,
                 uint32_t slot_capacity, HiprWide8BuildResult* out) = nullptr;
    void* context = nullptr;
    explicit operator bool() const { return build != nullptr; }
};
// What became of it in one build_bvh. A source that declines or fails is always followed by build_wide8, silently: the tree is the same either way.
struct Wide8SourceReport {
    bool asked = false;          // the source was called (it is not when HIPR_WIDE8_LEAF_COST or HIPR_WIDE8_LAYOUT configure the host's collapse away from its default)
    bool used = false;           // ... and its tree is the result's
    int status = 0;              // what it returned
    double seconds = 0.0;        // ... and how long it took
};

// The 4-wide collapse supplied by the caller in place of the host's WideCollapse: hipr_build_wide4's signature behind a context pointer (csrc/wide4_build.h collapses to
// the host's tree byte for byte on the device). Returns HIPR_OK, or the status of a refusal or an error, with the outputs untouched.
struct Wide4Source {
    int (*build)(void* context, const HiprBvhNode* nodes, uint32_t node_count, uint32_t triangle_count, HiprWideNode* out_nodes, uint32_t node_capacity, HiprWide4BuildResult* out) = nullptr;
    void* context = nullptr;
    explicit operator bool() const { return build != nullptr; }
};
// What became of it in one build_bvh. A source that declines or fails is always followed by the host's collapse, silently: the tree is the same either way.
struct Wide4SourceReport {
    bool asked = false;          // the source was called
    bool used = false;           // ... and its tree is the result's
    int status = 0;              // what it returned
    double seconds = 0.0;        // ... and how long it took
};

// Whether a consumer that installs a Bvh2Source installs the Wide8Source with it: HIPR_DEVICE_COLLAPSE (0: the host collapses), else DEVICE_COLLAPSE_DEFAULT.
bool device_collapse_wanted();

// Whether a consumer that installs a Bvh2Source installs the Wide4Source with it: HIPR_DEVICE_COLLAPSE4 (0: the host collapses, 1: the device), else DEVICE_COLLAPSE4_DEFAULT.
bool device_collapse4_wanted();

// `max_depth`: the deepest leaf the builder may produce (root = 1). 62 fits the 64 entry LDS stack.
BvhBuildResult build_bvh(const std::vector<HiprTriangle>& world_triangles, uint32_t max_depth = 62);
// The same with the BVH2 stage taken from `source` when one is installed; the 4-wide collapse, the 8-wide collapse and max_depth go on from either tree alike.
BvhBuildResult build_bvh(const std::vector<HiprTriangle>& world_triangles, uint32_t max_depth, const Bvh2Source& source, Bvh2SourceReport* report);
// ... and the 8-wide collapse from `wide8_source` when one is installed.
BvhBuildResult build_bvh(const std::vector<HiprTriangle>& world_triangles, uint32_t max_depth, const Bvh2Source& source, Bvh2SourceReport* report, const Wide8Source& wide8_source,
                         Wide8SourceReport* wide8_report);
// ... and the 4-wide collapse from `wide4_source` when one is installed.
BvhBuildResult build_bvh(const std::vector<HiprTriangle>& world_triangles, uint32_t max_depth, const Bvh2Source& source, Bvh2SourceReport* report, const Wide8Source& wide8_source,
                         Wide8SourceReport* wide8_report, const Wide4Source& wide4_source, Wide4SourceReport* wide4_report);
// The host's 4-wide collapse alone over a caller's BVH2 (node 0 the root, parents before children, as every BVH2 of this library is), on `threads` threads, with the
// root's budget chosen as build_bvh chooses it: the result does not depend on `threads`. `did_not_fit` (may be null): nodes that stopped adopting because one more child
// would not have fitted the budget; `budget` (may be null): the root's.
std::vector<HiprWideNode> collapse_wide4_on_host(const HiprBvhNode* nodes, size_t node_count, unsigned threads, uint32_t& stack_entries, uint32_t* did_not_fit, uint32_t* budget);
// The quantisation of one 4-wide node's child boxes (tests of csrc/wide4_build.h's restatement): boxes = lo xyz, hi xyz per child, count <= 4; `out` is zeroed first.
void quantise_wide4_children(const float* boxes_kx6, uint32_t count, HiprWideNode& out);

// Transform-only update: refits every box of `bvh` (BVH2 child boxes and the wide nodes' quantised child boxes) to `triangles`, which are
// the build's triangles in leaf order with new positions; topology and triangle order are kept. Returns bvh_child_area() of the result, or a negative value when
// the 8-wide tree could not be refitted (refit_wide8) and the caller has to rebuild.
double refit_bvh(BvhBuildResult& bvh, const std::vector<HiprTriangle>& triangles_in_leaf_order);
// Sum of the half-areas of all BVH2 child boxes: grows when a refit leaves the tree with overlapping, stretched boxes.
double bvh_child_area(const BvhBuildResult& bvh);

} // namespace HIPRenderer
