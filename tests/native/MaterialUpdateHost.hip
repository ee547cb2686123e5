// MaterialUpdateHost.hip -- the kernel bodies of the device's material update (csrc/material_update.h), compiled for the HOST by hipcc's host pass
// (tests/native/libmaterial_update_host.so).
//
// Test infrastructure (tests/test_material_update_cpu.py); nothing here is linked into or loaded by the product, which has no CPU path.
//
// update_triangle_material and update_leaf_flags are __host__ __device__ functions over the flag rules of csrc/material_rules.h; `hipcc --cuda-host-only
// -ffp-contract=off` yields an x86 build of exactly the statements the kernels run. material_update_host_scene walks them over a scene's arrays the way the
// two passes do, so that the CPU suite can hold them to SceneBuilder::update_materials byte for byte without a GPU.
#define HIPR_MATERIAL_UPDATE_HOST_ONLY 1      // none of the kernels: this build holds host code only
#include "../../bifrost3d_amd/csrc/material_update.h"

#include <vector>

using namespace hipr;

extern "C" {

// hipr_update_scene_materials' two passes on host arrays, in place. `instances` and `materials` already hold the edit, touched[i] != 0 marks the instances to
// recompute; `triangles`, `trace_triangles` (12 words per triangle), `shade_triangles` (32 words per triangle), `triangle_class` and `slots` are rewritten.
// reduction2[0] = every triangle is opaque, reduction2[1] = some triangle's material is coated. Returns 0, -1 on a malformed tree or a null array.
int material_update_host_scene(HiprTriangle* triangles, uint32_t triangle_count, const HiprInstance* instances, const HiprMaterial* materials, const uint32_t* indices, const float* texcoords,
                               const HiprTexture* textures, uint32_t texture_count, const uint8_t* texels, const uint32_t* touched, uint32_t* trace_triangles, uint32_t* shade_triangles,
                               uint8_t* triangle_class, HiprSlot8* slots, uint32_t slot_count, uint32_t* reduction2) {
    if (!triangles || !instances || !materials || !indices || !touched || !trace_triangles || !shade_triangles || !triangle_class || !reduction2) return -1;
    const MaterialUpdateArrays a = {triangles, triangle_count, instances, materials, indices, texcoords, textures, texture_count, texels, touched, trace_triangles, shade_triangles, triangle_class};
    // pass 1 (k_update_triangle_materials): the words preset, then AND / OR in any order -- backwards here
    reduction2[0] = 1u; reduction2[1] = 0u;
    for (uint32_t t = triangle_count; t-- > 0;) {
        bool opaque = true, coated = false;
        update_triangle_material(a, t, opaque, coated);
        if (!opaque) reduction2[0] &= 0u;
        if (coated) reduction2[1] |= 1u;
    }
    // pass 2 (k_update_leaf_flags) over the leaf slots, listed from the root as hiprenderer.hip prepare_refit lists them
    if (!slots || !slot_count) return 0;
    std::vector<uint32_t> nodes = {0u}, leaves;
    for (size_t i = 0; i < nodes.size(); ++i) {
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
    for (uint32_t slot : leaves) update_leaf_flags(slots, slot, triangles);
    return 0;
}

}
