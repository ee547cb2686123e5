// InstanceEditHost.hip -- the routines of hipr_edit_scene_instances (csrc/instance_edit.h), compiled for the HOST by hipcc's host pass
// (tests/native/libinstance_edit_host.so), chained with the walks of the BVH2 build and the 8-wide collapse that DeviceRebuildHost.hip holds.
//
// Test infrastructure (tests/test_instance_edit_on_host_cpu.py); nothing here is linked into or loaded by the product, which has no CPU path.
//
// edit_host_scene walks what hipr_edit_scene_instances launches, in its order and with the threads of every launch taken BACKWARDS: the count per OLD instance, the
// host's first[] of the NEW list and the old-to-new table, the scatter of the kept triangles, the new instances' triangles, the reduction with its claim check, the
// BVH2 build, the hand-over, the collapse and the gather. The CPU suite holds the result to SceneBuilder::remove_model / insert_model + rebuild() byte for byte.
#include "DeviceRebuildHost.hip"      // the HOST_ONLY switches, walk_bvh2 and walk_wide8

#include "../../bifrost3d_amd/csrc/instance_edit.h"

extern "C" {

// `resident` / `classes`: the scene's `count` triangles in the old tree's order and their class bytes; `pools`: the description the pools and the OLD instances are
// read from; `edits`: the new list. Outputs: out_triangles / out_classes (room for `capacity`), out_nodes (capacity - 1, at least 1), out_order (capacity),
// out_slots (2 x capacity), out[0..16) = {triangle count, node_count, deepest, the eleven words of HiprWide8BuildResult, all triangles opaque, any triangle coated}.
// 0: edited. 1: a flatten position claimed twice or not at all; 2: the BVH2 build declined; 3: trees higher than the kernels walk or more slots than a node addresses;
// 4: an index triple of a new instance outside the vertex pool; 5: a BVH2 of at most 64 nodes; 6: no triangle. Every refusal leaves all outputs untouched.
// -1: a bad argument (what the entry point checks on the host) or a walk off its bounds.
int edit_host_scene(const HiprTriangle* resident, const uint8_t* classes, uint32_t count, const HiprSceneDesc* pools, const HiprInstanceEdit* edits, uint32_t edit_count, uint32_t max_depth,
                    uint32_t capacity, HiprTriangle* out_triangles, uint8_t* out_classes, HiprBvhNode* out_nodes, uint32_t* out_order, HiprSlot8* out_slots, uint32_t* out) {
    if (!resident || !classes || !count || !pools || !edits || !edit_count || !out_triangles || !out_classes || !out_nodes || !out_order || !out_slots || !out) return -1;
    const uint32_t old_instances = pools->instance_count, primitive_total = pools->index_count / 3;
    // the list, as check_instance_edit takes it
    std::vector<HiprInstance> instances(edit_count);
    std::vector<uint32_t> source(edit_count, BUILD_NONE), primitive_count(edit_count, 0u), old_to_new(old_instances, BUILD_NONE);
    for (uint32_t i = 0; i < edit_count; ++i) {
        const HiprInstanceEdit& e = edits[i];
        if (e.source != HIPR_EDIT_NEW_INSTANCE) {
            if (e.source >= old_instances || old_to_new[e.source] != BUILD_NONE) return -1;
            old_to_new[e.source] = i; source[i] = e.source; instances[i] = pools->instances[e.source];
            continue;
        }
        if (e.instance.index_offset > primitive_total || e.primitive_count > primitive_total - e.instance.index_offset || e.instance.vertex_offset > pools->vertex_count ||
            e.instance.material_index < 0 || uint32_t(e.instance.material_index) >= pools->material_count)
            return -1;
        instances[i] = e.instance; primitive_count[i] = e.primitive_count;
    }
    // the count per old instance, first[] of the new list
    std::vector<uint32_t> instance_counts(old_instances, 0u), status(REBUILD_STATUS_WORDS, 0u);
    const RebuildArrays a = {resident, classes, count, old_instances, instance_counts.data(), nullptr, nullptr, nullptr, nullptr, status.data()};
    for (uint32_t t = count; t-- > 0;) rebuild_count(a, t);
    uint64_t total = 0;
    for (uint32_t i = 0; i < old_instances; ++i) total += instance_counts[i];
    if (total != count) return 1;
    std::vector<uint32_t> first(size_t(edit_count) + 1, 0u), created, created_first(1, 0u);
    total = 0;
    for (uint32_t i = 0; i < edit_count; ++i) {
        if (source[i] != BUILD_NONE) primitive_count[i] = instance_counts[source[i]];
        else { created.push_back(i); created_first.push_back(created_first.back() + primitive_count[i]); }
        total += primitive_count[i];
        if (total > BUILD_MAX_TRIANGLES) return -1;
        first[i + 1] = uint32_t(total);
    }
    const uint32_t n = uint32_t(total);
    if (n == 0) return 6;
    if (n > capacity) return -1;
    // the flat array of the new list
    std::vector<HiprTriangle> flat(n);
    std::vector<uint8_t> flat_class(n, 0);
    std::vector<uint32_t> claim(n, 0u);
    const EditArrays e = {resident, classes, count, old_instances, old_to_new.data(), first.data(), edit_count, n, created.data(), created_first.data(), uint32_t(created.size()), created_first.back(),
                          instances.data(), pools->materials, pools->indices, pools->geometry, pools->vertex_count, pools->texcoords, pools->textures, pools->texture_count, pools->texels,
                          flat.data(), flat_class.data(), claim.data(), status.data()};
    for (uint32_t t = count; t-- > 0;) edit_scatter(e, t);
    for (uint32_t q = created_first.back(); q-- > 0;) edit_new_triangle(e, q);
    bool all_opaque = true, any_coated = false;
    for (uint32_t k = n; k-- > 0;) {
        bool opaque = true, coated = false;
        edit_reduce(flat.data(), flat_class.data(), claim.data(), status.data(), k, opaque, coated);
        all_opaque = all_opaque && opaque; any_coated = any_coated || coated;
    }
    if (status[EDIT_STATUS_INDEX]) return 4;
    if (status[REBUILD_STATUS_CLAIM]) return 1;
    // the BVH2 over the flat array, the hand-over, the collapse: rebuild_host_trees' steps over the new count
    std::vector<HiprBvhNode> placed;
    std::vector<uint32_t> order, place, level_sizes;
    uint32_t node_count = 0, deepest = 0;
    const int built = walk_bvh2(flat.data(), n, std::max(max_depth, 8u), placed, order, place, level_sizes, node_count, deepest);
    if (built) return built == 1 ? 2 : -1;
    const uint32_t bvh_levels = std::max<uint32_t>(uint32_t(level_sizes.size()), 1u);
    if (bvh_levels > W8_MAX_LEVELS || deepest + 1u > 64u) return 3;
    if (node_count <= 64u) return 5;
    std::vector<uint32_t> level_nodes(node_count), level_first(size_t(bvh_levels) + 1, 0u);
    for (uint32_t k = node_count; k-- > 0;) rebuild_level_node(place.data(), level_nodes.data(), k);
    if (level_sizes.empty()) level_first[1] = 1u;
    else for (uint32_t l = 0; l < bvh_levels; ++l) level_first[l + 1] = level_first[l] + level_sizes[l];
    W8State S = {};
    S.nodes = placed.data(); S.node_count = node_count; S.triangles = flat.data(); S.order = order.data(); S.triangle_count = n;
    S.level_nodes = level_nodes.data(); S.reachable = node_count; S.single_leaf = level_sizes.empty() ? 1u : 0u;
    std::vector<HiprSlot8> slots;
    HiprWide8BuildResult wide8 = {};
    const int collapsed = walk_wide8(S, level_first, slots, wide8);
    if (collapsed) return collapsed == 2 ? 3 : -1;
    if (wide8.height > 33u) return 3;
    // the new resident arrays
    for (uint32_t k = n; k-- > 0;) rebuild_gather(flat.data(), flat_class.data(), order.data(), out_triangles, out_classes, k);
    std::memcpy(out_nodes, placed.data(), size_t(node_count) * sizeof(HiprBvhNode));
    std::memcpy(out_order, order.data(), size_t(n) * 4);
    std::memcpy(out_slots, slots.data(), slots.size() * sizeof(HiprSlot8));
    out[0] = n; out[1] = node_count; out[2] = deepest;
    std::memcpy(out + 3, &wide8, sizeof(wide8));
    out[14] = all_opaque ? 1u : 0u; out[15] = any_coated ? 1u : 0u;
    return 0;
}

}
