// TexelUpdateHost.hip -- the kernel bodies of the device's texel update (csrc/texel_update.h), compiled for the HOST by hipcc's host pass
// (tests/native/libtexel_update_host.so).
//
// Test infrastructure (tests/test_texel_update_on_host_cpu.py); nothing here is linked into or loaded by the product, which has no CPU path.
//
// write_texel_chunk, reflag_triangle and update_leaf_flags are __host__ __device__ functions over the flag rules of csrc/material_rules.h; `hipcc --cuda-host-only
// -ffp-contract=off` yields an x86 build of exactly the statements the kernels run. texel_update_host_scene walks them over a scene's arrays the way the three
// passes do, so that the CPU suite can hold them to SceneBuilder::update_texels byte for byte without a GPU.
#define HIPR_MATERIAL_UPDATE_HOST_ONLY 1      // none of the kernels: this build holds host code only
#include "../../bifrost3d_amd/csrc/texel_update.h"

#include <vector>

using namespace hipr;

extern "C" {

// hipr_update_scene_texels' passes on host arrays, in place: `texels` (the pool), `triangles`, `trace_triangles` (12 words per triangle), `shade_triangles` (32 words
// per triangle), `triangle_class` and `slots` are rewritten. out3: every triangle is opaque, triangles decided again, triangles whose flags changed.
// Returns 0, -1 on a malformed tree or a null array. The edits are NOT checked: the caller passes what hipr_update_scene_texels accepts.
int texel_update_host_scene(HiprTriangle* triangles, uint32_t triangle_count, const HiprInstance* instances, uint32_t instance_count, const HiprMaterial* materials, const uint32_t* indices,
                            const float* texcoords, const HiprTexture* textures, uint32_t texture_count, uint8_t* texels, const HiprTexelEdit* edits, uint32_t edit_count, uint32_t* trace_triangles,
                            uint32_t* shade_triangles, uint8_t* triangle_class, HiprSlot8* slots, uint32_t slot_count, uint32_t* out3) {
    if (!triangles || !instances || !materials || !indices || !textures || !texels || (edit_count && !edits) || !trace_triangles || !shade_triangles || !triangle_class || !out3) return -1;
    // the plan and the staging buffer, as ResidentScene::update_texels makes them
    std::vector<TexelRectangle> rectangles(edit_count);
    std::vector<bool> edited(texture_count, false);
    uint64_t staging_bytes = 0;
    for (uint32_t k = 0; k < edit_count; ++k) {
        rectangles[k] = planned_rectangle(edits[k], textures[edits[k].texture_index], staging_bytes);
        edited[edits[k].texture_index] = true;
    }
    std::vector<uint8_t> staging(staging_bytes, uint8_t(0xEE));
    for (uint32_t k = 0; k < edit_count; ++k) pack_rectangle_rows(edits[k], rectangles[k], staging.data());
    std::vector<uint32_t> touched(instance_count ? instance_count : 1u, 0u);
    for (uint32_t i = 0; i < instance_count; ++i)
        if (const HiprTexture* deciding = deciding_coverage_texture(materials[instances[i].material_index], textures, texture_count)) touched[i] = edited[size_t(deciding - textures)] ? 1u : 0u;
    // pass 1 (k_write_texel_rectangle), rectangle after rectangle; within one the threads run in any order -- backwards here
    for (const TexelRectangle& r : rectangles)
        for (uint32_t row = r.height; row-- > 0;)
            for (uint32_t chunk = uint32_t((r.row_bytes + 3u) / 4u) + 2u; chunk-- > 0;) write_texel_chunk(r, staging.data(), texels, row, chunk);      // two threads past the row's end as well
    // pass 2 (k_reflag_touched_triangles): the word preset, then the AND and the counts in any order -- backwards here
    const MaterialUpdateArrays a = {triangles, triangle_count, instances, materials, indices, texcoords, textures, texture_count, texels, touched.data(), trace_triangles, shade_triangles, triangle_class};
    out3[TEXEL_WORD_OPAQUE] = 1u; out3[TEXEL_WORD_DECIDED] = 0u; out3[TEXEL_WORD_CHANGED] = 0u;
    for (uint32_t t = triangle_count; t-- > 0;) {
        bool opaque = true, decided = false, changed = false;
        reflag_triangle(a, t, opaque, decided, changed);
        if (!opaque) out3[TEXEL_WORD_OPAQUE] &= 0u;
        out3[TEXEL_WORD_DECIDED] += decided ? 1u : 0u;
        out3[TEXEL_WORD_CHANGED] += changed ? 1u : 0u;
    }
    // pass 3 (k_update_leaf_flags) over the leaf slots, listed from the root as prepare_refit lists them
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
