// material_update.h -- material edits applied to the resident scene on the device (hipr_update_scene_materials): a changed material slot or a model given
// another material is a copy into the material / instance pools plus two short passes over arrays that are resident anyway, instead of a new scene (the
// reference rewrites one slot of its material buffer, OR/Renderer.cpp:753-850).
//
// The yardstick is BYTE EQUALITY with a fresh upload of the edited scene. A material edit moves no corner, BvhBuilder.cpp never reads HiprTriangle::flags and
// Wide8Builder.cpp pairs triangles by instance only, so the trees, the triangle order and the record pairing of a fresh build are the resident ones; what a
// fresh upload would derive differently from the pools is rewritten here, with the flag rules of material_rules.h that the host's builder runs:
//   pass 1  k_update_triangle_materials   one thread per triangle. A triangle of a TOUCHED instance (its material index was reassigned or its material's slot
//                                         rewritten) gets its flags recomputed and written to `triangles` and to the copy in `trace_triangles`, its material
//                                         index written to its shading record and its class byte set; an untouched one writes nothing. Every triangle feeds
//                                         two reductions -- AND of "opaque", OR of "coated" -- by a wave ballot and at most one atomic per wave and word.
//   pass 2  k_update_leaf_flags           one thread per leaf record of the 8-wide tree: bits 0..3 of HiprLeaf8::flags follow the flags of its triangles.
// Both run on the context's stream, one after the other; integer reductions are order independent, nothing waits on another block.
//
// The bodies are __host__ __device__ so that tests/native/MaterialUpdateHost.hip can compile them for the host and the CPU suite can hold them to
// SceneBuilder::update_materials without a GPU.
#pragma once

#include "material_rules.h"

#include <hip/hip_runtime.h>

namespace hipr {

// The arrays of pass 1 as words. `instances` already hold the new material indices and `materials` the new slots.
struct MaterialUpdateArrays {
    HiprTriangle* triangles;
    uint32_t triangle_count;
    const HiprInstance* instances;
    const HiprMaterial* materials;
    const uint32_t* indices;
    const float* texcoords;             // may be null: no mesh has any
    const HiprTexture* textures;
    uint32_t texture_count;
    const uint8_t* texels;
    const uint32_t* touched;            // one word per instance
    uint32_t* trace_triangles;          // 12 words per triangle, word 11 = the flags
    uint32_t* shade_triangles;          // 32 words per triangle (kernels.h SHADE_TRIANGLE_QUADS = 8 quads), word 15 = quad 3's .w = the material index
    uint8_t* triangle_class;
};
constexpr uint32_t MATERIAL_TRACE_FLAG_WORD = 11, MATERIAL_TRACE_WORDS = 12, MATERIAL_SHADE_INDEX_WORD = 15, MATERIAL_SHADE_WORDS = 32;

// Pass 1 for triangle t; reports what the triangle contributes to the two reductions. `touched`: the triangle is recomputed (the material edit and the texel edit ask
// a.touched of its instance; the vertex edit decides per triangle, vertex_update.h).
MRHD void update_triangle_material(const MaterialUpdateArrays& a, uint32_t t, bool touched, bool& opaque, bool& coated) {
    HiprTriangle& tri = a.triangles[t];
    if (!touched) {
        opaque = (tri.flags & HIPR_TRIANGLE_OPAQUE) != 0;
        coated = (a.triangle_class[t] & 1u) != 0;
        return;
    }
    const HiprInstance& inst = a.instances[tri.instance_index];
    const HiprMaterial& m = a.materials[inst.material_index];
    const uint32_t flags = triangle_flags(m, inst, tri.primitive_index, a.indices, a.texcoords, a.textures, a.texture_count, a.texels);
    tri.flags = flags;
    a.trace_triangles[MATERIAL_TRACE_WORDS * size_t(t) + MATERIAL_TRACE_FLAG_WORD] = flags;
    a.shade_triangles[MATERIAL_SHADE_WORDS * size_t(t) + MATERIAL_SHADE_INDEX_WORD] = uint32_t(inst.material_index);
    const uint32_t cls = coated_class(m);
    a.triangle_class[t] = uint8_t(cls);
    opaque = (flags & HIPR_TRIANGLE_OPAQUE) != 0;
    coated = cls != 0;
}
MRHD void update_triangle_material(const MaterialUpdateArrays& a, uint32_t t, bool& opaque, bool& coated) {
    update_triangle_material(a, t, a.touched[a.triangles[t].instance_index] != 0, opaque, coated);
}

// Pass 2 for one leaf slot.
MRHD void update_leaf_flags(HiprSlot8* slots, uint32_t slot, const HiprTriangle* triangles) {
    const HiprLeaf8& leaf = slots[slot].leaf;
    const uint32_t flags = (leaf.flags & ~15u) | leaf_material_bits(triangles, leaf);
    if (flags != leaf.flags) slots[slot].leaf.flags = flags;
}

#if defined(__HIPCC__) && !defined(HIPR_MATERIAL_UPDATE_HOST_ONLY)      // the kernels; a host build of the bodies (tests/native/MaterialUpdateHost.hip) leaves them out

constexpr int MATERIAL_UPDATE_BLOCK = 256;

// reduction[0]: preset to 1, cleared when a triangle is not opaque; reduction[1]: preset to 0, set when a triangle's material is coated.
__global__ __launch_bounds__(MATERIAL_UPDATE_BLOCK) void k_update_triangle_materials(MaterialUpdateArrays a, uint32_t* __restrict__ reduction) {
    const uint32_t t = blockIdx.x * uint32_t(MATERIAL_UPDATE_BLOCK) + threadIdx.x;
    bool opaque = true, coated = false;      // neutral: the threads past the end
    if (t < a.triangle_count) update_triangle_material(a, t, opaque, coated);
    const unsigned long long not_opaque = __ballot(!opaque), any_coated = __ballot(coated);
    if ((threadIdx.x & 63u) == 0) {
        if (not_opaque) atomicAnd(&reduction[0], 0u);
        if (any_coated) atomicOr(&reduction[1], 1u);
    }
}

__global__ __launch_bounds__(MATERIAL_UPDATE_BLOCK) void k_update_leaf_flags(HiprSlot8* __restrict__ slots, const uint32_t* __restrict__ leaf_slots, uint32_t leaf_count,
                                                                            const HiprTriangle* __restrict__ triangles) {
    const uint32_t i = blockIdx.x * uint32_t(MATERIAL_UPDATE_BLOCK) + threadIdx.x;
    if (i >= leaf_count) return;
    update_leaf_flags(slots, leaf_slots[i], triangles);
}

#endif // the kernels

} // namespace hipr
