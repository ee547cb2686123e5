// DeviceRefitHost.hip -- the routines of the device refit (csrc/wide8_refit.h), compiled for the HOST by hipcc's host pass (tests/native/libdevice_refit_host.so).
//
// Test infrastructure (tests/test_device_refit_on_host_cpu.py); nothing here is linked into or loaded by the product, which has no CPU path.
//
// wide8_refit.h's record, box and quantisation routines are __host__ __device__ functions of ordinary IEEE arithmetic in a fixed order; `hipcc --cuda-host-only
// -ffp-contract=off` yields an x86 build of exactly the statements the kernels run. refit_host_scene walks them over a scene the way the four passes do -- triangles
// and bounds, leaf records, nodes level by level from the deepest, area -- so that the CPU suite can hold them to the host's refit_wide8 byte for byte without a GPU.
#define HIPR_REFIT_HOST_ONLY 1      // none of the kernels: this build holds host code only
#include "../../bifrost3d_amd/csrc/wide8_refit.h"

#include <vector>

using namespace hipr;

extern "C" {

// The device refit of hipr_refit_scene_transforms on host arrays, in place: `triangles` and `slots` are rewritten, `instances` already carry the new matrices,
// moved[i] != 0 marks the instances to recompute. Returns 1 when a leaf record could not be refitted (needs_rebuild), 0 otherwise, -1 on a malformed tree.
int refit_host_scene(HiprTriangle* triangles, uint32_t triangle_count, const HiprInstance* instances, const uint32_t* moved, const uint32_t* indices, const HiprVertexGeometry* geometry,
                     HiprSlot8* slots, uint32_t slot_count, float* grid_min3, float* grid_cell3, double* child_half_area) {
    if (!triangles || !instances || !moved || !indices || !geometry || !slots || !slot_count) return -1;
    // pass 1 (k_refit_triangles, k_refit_bounds_final)
    RefitBound bound[6];
    for (int k = 0; k < 6; ++k) bound[k] = {k < 3 ? FLT_MAX : -FLT_MAX, 0xFFFFFFFFu};
    for (uint32_t t = triangle_count; t-- > 0;) {      // backwards: the result must not depend on the order of the reduction
        HiprTriangle& tri = triangles[t];
        if (moved[tri.instance_index]) {
            const HiprInstance& inst = instances[tri.instance_index];
            const uint32_t* idx = indices + 3 * size_t(inst.index_offset + tri.primitive_index);
            float* corners[3] = {tri.v0, tri.v1, tri.v2};
            for (int k = 0; k < 3; ++k) refit_world_corner(inst.object_to_world, geometry[inst.vertex_offset + idx[k]].position, corners[k]);
        }
        const float* corners[3] = {tri.v0, tri.v1, tri.v2};
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) {
                const RefitBound p = {corners[k][a], 3u * t + uint32_t(k)};
                bound[a] = refit_lower(bound[a], p);
                bound[3 + a] = refit_upper(bound[3 + a], p);
            }
    }
    const float lo[3] = {bound[0].v, bound[1].v, bound[2].v}, hi[3] = {bound[3].v, bound[4].v, bound[5].v};
    refit_grid(lo, hi, grid_min3, grid_cell3);
    // the slot lists by kind and level (hiprenderer.hip prepare_refit)
    std::vector<uint32_t> nodes = {0u}, leaves, level_begin = {0u};
    for (size_t begin = 0; begin < nodes.size();) {
        const size_t end = nodes.size();
        level_begin.push_back(uint32_t(end));
        for (size_t i = begin; i < end; ++i) {
            const HiprNode8& n = slots[nodes[i]].node;
            const uint32_t base = n.base_valid & 0xFFFFFFu, valid = n.base_valid >> 24;
            uint32_t rank = 0;
            for (int p = 0; p < 8; ++p) {
                if (!(valid >> p & 1u)) continue;
                const uint32_t child = base + rank++;
                if (child >= slot_count || nodes.size() + leaves.size() > slot_count) return -1;
                if (n.inner_mask >> p & 1u) nodes.push_back(child); else leaves.push_back(child);
            }
        }
        begin = end;
    }
    std::vector<RefitBox> exact(slot_count);
    int needs_rebuild = 0;
    // pass 2 (k_refit_leaves)
    for (uint32_t slot : leaves) {
        const HiprLeaf8 stored = slots[slot].leaf;
        HiprLeaf8 rebuilt;
        if (refit_leaf(triangles, stored, rebuilt, exact[slot])) slots[slot].leaf = rebuilt;
        else needs_rebuild = 1;
    }
    // pass 3 (k_refit_nodes), deepest level first
    for (size_t level = level_begin.size() - 1; level-- > 0;)
        for (uint32_t i = level_begin[level]; i < level_begin[level + 1]; ++i) {
            HiprNode8 n = slots[nodes[i]].node;
            RefitBox all;
            refit_node(n, exact.data(), grid_min3, grid_cell3, all);
            exact[nodes[i]] = all;
            slots[nodes[i]].node = n;
        }
    // pass 4 (k_refit_area; the order of the f64 sum is the kernels' business, the terms are these)
    double area = 0.0;
    for (uint32_t i = 1; i < slot_count; ++i) area += double(refit_half_area(exact[i]));
    if (child_half_area) *child_half_area = area;
    return needs_rebuild;
}

// refit_quantise_node on one synthetic node: the child boxes of the positions in `valid` (lo xyz, hi xyz each).
void refit_host_quantise_node(const float* boxes_8x6, uint32_t valid, const float* grid_min3, const float* grid_cell3, HiprNode8* out) {
    RefitBox boxes[8], all;
    refit_box_reset(all);
    for (int s = 0; s < 8; ++s) {
        refit_box_reset(boxes[s]);
        if (!(valid >> s & 1u)) continue;
        for (int a = 0; a < 3; ++a) { boxes[s].lo[a] = boxes_8x6[6 * s + a]; boxes[s].hi[a] = boxes_8x6[6 * s + 3 + a]; }
        refit_box_grow(all, boxes[s]);
    }
    refit_quantise_node(boxes, valid, all, grid_min3, grid_cell3, *out);
}

// `count` nodes at once (the sweep of the CPU suite): boxes 48 floats, valid, grid 6 floats (min xyz, cell xyz) and a 64-byte node per node.
void refit_host_quantise_nodes(const float* boxes, const uint32_t* valid, const float* grids, HiprNode8* out, uint32_t count) {
    for (uint32_t i = 0; i < count; ++i) refit_host_quantise_node(boxes + 48 * size_t(i), valid[i], grids + 6 * size_t(i), grids + 6 * size_t(i) + 3, out + size_t(i));
}

// refit_leaf on one record. Returns 1 when the record was rebuilt into `out`, 0 when it is reported instead (`out` is left untouched).
int refit_host_leaf(const HiprTriangle* triangles, const HiprLeaf8* stored, HiprLeaf8* out, float* box6) {
    HiprLeaf8 rebuilt;
    RefitBox box;
    const bool ok = refit_leaf(triangles, *stored, rebuilt, box);
    for (int a = 0; a < 3; ++a) { box6[a] = box.lo[a]; box6[3 + a] = box.hi[a]; }
    if (ok) *out = rebuilt;
    return ok ? 1 : 0;
}

}
