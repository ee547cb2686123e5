// instance_edit.h -- the passes of hipr_edit_scene_instances that hipr_rebuild_scene_trees does not have: models of the resident scene added and removed on the
// device (the reference leaves geometry where it lives, adds or removes a child of its root group and marks the acceleration dirty, OR/Renderer.cpp:138-182,
// :1043-1110). A model destroyed, or created over a mesh the scene already holds, changes no pool: a removed model's triangles are resident and carry their
// instance and primitive index, a created model's triangles are one matrix away from object-space vertices that are resident.
//
// The yardstick is BYTE EQUALITY with the host path: SceneBuilder::remove_model / insert_model, rebuild(), hipr_upload_scene on a fresh context. The flat array the
// two builds run over is the one SceneBuilder::finalize would make of the NEW instance list -- instances in order, primitives in order:
//   -  k_rebuild_count     (scene_rebuild.h) over the OLD instances. The host makes first[] of the NEW list from it -- a kept instance takes its counted size, a new
//                          one its primitive_count -- and the old-to-new index table, removed instances mapped to BUILD_NONE.
//   1  k_edit_scatter      every resident triangle of a KEPT instance and its class byte go to first[new index] + primitive_index, with instance_index rewritten
//                          to the new index; a removed instance's triangles write nothing. The claim word per position is scene_rebuild.h's.
//   2  k_edit_new_triangles  one thread per triangle of all NEW instances; it finds its instance by search over the new instances' prefix sums. Corners by
//                          SceneBuilder::finalize's expression (refit_world_corner), flags by hipr::triangle_flags over the resident pools (covered_everywhere over
//                          the resident texels included), the class byte by coated_class. Every index of the triple is checked against the vertex pool BEFORE the
//                          vertex is loaded: a bad index raises the flag and is never read through. The thread claims its position like the scatter.
//   3  k_edit_reduce       over the flat array: a position claimed not at all (or more than once) raises the claim flag; "some triangle is not opaque" and "some
//                          triangle is coated" of the NEW set by a wave ballot and at most one integer atomic per wave and word (k_update_triangle_materials' shape).
//   -  the BVH2 build, k_rebuild_levels, the collapse and k_rebuild_gather, unchanged, over the new count.
// All of it on the context's stream, launches in sequence: no block waits on another, nothing spins, integer atomics only.
//
// The routines are __host__ __device__ so that the CPU suite can walk them against SceneBuilder::rebuild() without a GPU (tests/native/InstanceEditHost.hip).
// This header includes material_rules.h: it belongs to the main unit (correctly rounded division, -ffp-contract=off), NEVER to the fast-math shade unit.
#pragma once

#include "material_rules.h"
#include "scene_rebuild.h"
#include "wide8_refit.h"

namespace hipr {

// The words of RebuildScratch::status an edit uses beside REBUILD_STATUS_CLAIM.
constexpr uint32_t EDIT_STATUS_INDEX = 1;           // an index triple of a new instance points outside the vertex pool
constexpr uint32_t EDIT_STATUS_NOT_OPAQUE = 2;      // some triangle of the new set lacks HIPR_TRIANGLE_OPAQUE
constexpr uint32_t EDIT_STATUS_COATED = 3;          // some triangle of the new set has a coated material
static_assert(EDIT_STATUS_COATED < REBUILD_STATUS_WORDS, "the status words of scene_rebuild.h hold an edit's");

struct EditArrays {
    const HiprTriangle* resident; const uint8_t* resident_class;      // the scene's triangles in the old tree's order, and their class bytes
    uint32_t resident_count, old_instance_count;
    const uint32_t* old_to_new;           // old_instance_count words: the new index of a kept instance, BUILD_NONE for a removed one
    const uint32_t* first;                // new_instance_count + 1 words: the flatten position of primitive 0 of every instance of the new list
    uint32_t new_instance_count, new_triangle_count;
    const uint32_t* created;              // created_count words: the new index of the j-th new instance, ascending
    const uint32_t* created_first;        // created_count + 1 words: the exclusive prefix sums of the new instances' primitive counts
    uint32_t created_count, created_triangles;
    const HiprInstance* instances;        // the NEW instance array
    const HiprMaterial* materials;        // the resident pools
    const uint32_t* indices;
    const HiprVertexGeometry* geometry;
    uint32_t vertex_count;
    const float* texcoords;               // may be null: no mesh has any
    const HiprTexture* textures;
    uint32_t texture_count;
    const uint8_t* texels;
    HiprTriangle* flat; uint8_t* flat_class; uint32_t* claim;      // per flatten position of the new list
    uint32_t* status;
};

// Pass 1, one resident triangle.
BHD void edit_scatter(const EditArrays& a, uint32_t t) {
    const HiprTriangle& triangle = a.resident[t];
    const uint32_t old_instance = triangle.instance_index, primitive = triangle.primitive_index;
    if (old_instance >= a.old_instance_count) { a.status[REBUILD_STATUS_CLAIM] = 1u; return; }
    const uint32_t instance = a.old_to_new[old_instance];
    if (instance == BUILD_NONE) return;      // removed
    if (instance >= a.new_instance_count || primitive >= a.first[instance + 1] - a.first[instance]) { a.status[REBUILD_STATUS_CLAIM] = 1u; return; }
    const uint32_t position = a.first[instance] + primitive;      // < first[instance + 1] <= new_triangle_count
    if (build_atomic_add(a.claim + position, 1u) != 0u) { a.status[REBUILD_STATUS_CLAIM] = 1u; return; }
    rebuild_copy_triangle(a.flat + position, &triangle);
    a.flat[position].instance_index = instance;
    a.flat_class[position] = a.resident_class[t];
}

// The new instance triangle q of all new instances' belongs to: the last j with created_first[j] <= q. created_first[0] = 0 and q < created_first[created_count].
BHD uint32_t edit_created_of(const EditArrays& a, uint32_t q) {
    uint32_t lo = 0, hi = a.created_count;      // the answer lies in [lo, hi)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (a.created_first[mid] <= q) lo = mid; else hi = mid;
    }
    return lo;
}

// Pass 2, triangle q of all new instances'.
BHD void edit_new_triangle(const EditArrays& a, uint32_t q) {
    const uint32_t j = edit_created_of(a, q), primitive = q - a.created_first[j], instance = a.created[j];
    const HiprInstance& inst = a.instances[instance];
    const uint32_t* idx = a.indices + 3 * size_t(inst.index_offset + primitive);      // inside the index pool: the host has checked (index_offset, primitive_count)
    const uint32_t vertices = a.vertex_count - inst.vertex_offset;                     // the host has checked vertex_offset <= vertex_count
    const uint32_t i0 = idx[0], i1 = idx[1], i2 = idx[2];
    if (i0 >= vertices || i1 >= vertices || i2 >= vertices) { a.status[EDIT_STATUS_INDEX] = 1u; return; }      // before any vertex is loaded
    HiprTriangle triangle;
    refit_world_corner(inst.object_to_world, a.geometry[inst.vertex_offset + i0].position, triangle.v0);
    refit_world_corner(inst.object_to_world, a.geometry[inst.vertex_offset + i1].position, triangle.v1);
    refit_world_corner(inst.object_to_world, a.geometry[inst.vertex_offset + i2].position, triangle.v2);
    triangle.instance_index = instance;
    triangle.primitive_index = primitive;
    const HiprMaterial& material = a.materials[inst.material_index];
    triangle.flags = triangle_flags(material, inst, primitive, a.indices, a.texcoords, a.textures, a.texture_count, a.texels);
    const uint32_t position = a.first[instance] + primitive;      // first[instance + 1] - first[instance] is the instance's primitive_count
    if (build_atomic_add(a.claim + position, 1u) != 0u) { a.status[REBUILD_STATUS_CLAIM] = 1u; return; }
    a.flat[position] = triangle;      // a local record: plain stores, nothing goes through memory first
    a.flat_class[position] = uint8_t(coated_class(material));
}

// Pass 3, one flatten position: what it contributes to the two switches; a position not claimed exactly once raises the claim flag.
BHD void edit_reduce(const HiprTriangle* flat, const uint8_t* flat_class, const uint32_t* claim, uint32_t* status, uint32_t k, bool& opaque, bool& coated) {
    if (claim[k] != 1u) { status[REBUILD_STATUS_CLAIM] = 1u; return; }      // flat[k] may be unwritten: not read
    opaque = (flat[k].flags & HIPR_TRIANGLE_OPAQUE) != 0;
    coated = (flat_class[k] & 1u) != 0;
}

#if defined(__HIPCC__) && !defined(HIPR_REBUILD_HOST_ONLY)      // the kernels; a host build of the routines (tests/native/InstanceEditHost.hip) leaves them out

__global__ __launch_bounds__(REBUILD_BLOCK) void k_edit_scatter(EditArrays a) {
    const uint32_t t = blockIdx.x * uint32_t(REBUILD_BLOCK) + threadIdx.x;
    if (t < a.resident_count) edit_scatter(a, t);
}
__global__ __launch_bounds__(REBUILD_BLOCK) void k_edit_new_triangles(EditArrays a) {
    const uint32_t q = blockIdx.x * uint32_t(REBUILD_BLOCK) + threadIdx.x;
    if (q < a.created_triangles) edit_new_triangle(a, q);
}
__global__ __launch_bounds__(REBUILD_BLOCK) void k_edit_reduce(const HiprTriangle* __restrict__ flat, const uint8_t* __restrict__ flat_class, const uint32_t* __restrict__ claim,
                                                               uint32_t* __restrict__ status, uint32_t triangle_count) {
    const uint32_t k = blockIdx.x * uint32_t(REBUILD_BLOCK) + threadIdx.x;
    bool opaque = true, coated = false;      // neutral: the threads past the end
    if (k < triangle_count) edit_reduce(flat, flat_class, claim, status, k, opaque, coated);
    const unsigned long long not_opaque = __ballot(!opaque), any_coated = __ballot(coated);
    if ((threadIdx.x & 63u) == 0) {
        if (not_opaque) atomicOr(&status[EDIT_STATUS_NOT_OPAQUE], 1u);
        if (any_coated) atomicOr(&status[EDIT_STATUS_COATED], 1u);
    }
}

#endif // the kernels

} // namespace hipr
