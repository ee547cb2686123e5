// scene.hip -- the scene service of the C-ABI declared in include/hiprenderer_c.h: everything that checks, uploads or edits the scene a context holds.
//
// In reading order: the pure host checks of a description and of an edit (no HIP call); ResidentScene (context.h), the one owner of the device's copy of the scene,
// with its writers -- upload, geometry update, refit, material edit, pool growth, the hand-over of rebuilt trees; the drivers of the device tree builds (BVH2,
// collapse to the 8-wide tree, both over the resident triangles); and the entry points over all of them. Nothing here is on the path of a render pass
// (hiprenderer.hip): the two meet in the context, and in check_context and finish_all, which every entry point that touches the device starts with.
// The kernels of the builders' headers below are compiled in this unit and in no other; of kernels.h and wide8_kernels.h it takes the types.
#define HIPR_SHADE_TU 1      // kernels.h: their one definition is hiprenderer.hip's
#include "context.h"
#include "triangle_records.h"
#include "wide8_refit.h"
#include "material_update.h"
#include "bvh2_build.h"
#include "wide8_build.h"
#include "wide4_build.h"
#include "scene_rebuild.h"
#include "instance_edit.h"
#include "pool_growth.h"
#include "environment_build.h"
#include "texel_update.h"
#include "vertex_update.h"
#include "vertex_pose.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace hipr;

// ---- the pure host checks: no HIP call ------------------------------------------------------------------------------------------------------------------
namespace {

// What makes ONE material unusable against a texture pool of `texture_count` entries: a texture ID outside it, an unknown shading model. The check of
// validate_scene for every material of a description, and of hipr_update_scene_materials for every slot it is given. Returns nullptr when sound.
const char* invalid_material(const HiprMaterial& m, uint32_t index, uint32_t texture_count, char* message, size_t message_size) {
    const int32_t ids[4] = {m.tint_roughness_texture_ID, m.roughness_texture_ID, m.metallic_texture_ID, m.coverage_texture_ID};
    for (int32_t id : ids)
        if (id < 0 || (id > 0 && uint32_t(id) >= texture_count)) { snprintf(message, message_size, "material %u references texture %d of %u", index, id, texture_count); return message; }
    if (m.shading_model > HIPR_SHADING_TRANSMISSIVE) { snprintf(message, message_size, "material %u has the unknown shading model %u", index, unsigned(m.shading_model)); return message; }
    return nullptr;
}

// What makes ONE texture unusable against a texel pool of `texel_bytes`: an unknown format, an empty extent, texels that do not lie inside the pool or start off
// their alignment. The check of validate_scene for every texture of a description, and of hipr_append_scene_pools for every texture it brings, against the grown pool.
const char* invalid_texture(const HiprTexture& t, uint32_t index, uint64_t texel_bytes, char* message, size_t message_size) {
    const uint64_t size = t.format == HIPR_TEXEL_R8 ? 1u : (t.format == HIPR_TEXEL_RGBA8 ? 4u : (t.format == HIPR_TEXEL_R32F ? 4u : (t.format == HIPR_TEXEL_RGBA32F ? 16u : 0u)));
    if (size == 0) { snprintf(message, message_size, "texture %u has the unknown texel format %u", index, unsigned(t.format)); return message; }
    if (t.width == 0 || t.height == 0) { snprintf(message, message_size, "texture %u is %u x %u", index, t.width, t.height); return message; }
    const uint64_t bytes = uint64_t(t.width) * t.height * size;
    if (t.texel_offset > texel_bytes || bytes > texel_bytes - t.texel_offset || t.texel_offset % (size == 16 ? 16 : 4) != 0) {
        snprintf(message, message_size, "texture %u (%u x %u, offset %llu) does not fit the %llu byte texel pool", index, t.width, t.height, (unsigned long long)t.texel_offset, (unsigned long long)texel_bytes);
        return message;
    }
    return nullptr;
}

// O(n) check of everything the kernels dereference through an index of the description (the header is public: a bad ID must be an
// error code, not an out-of-bounds read on the GPU). Also derives the worst-case stack need of the wide tree instead of trusting
// the caller's figure. Returns nullptr when the scene is sound, a message otherwise.
const char* validate_scene(const HiprSceneDesc* s, uint32_t& wide_stack_need, char* message, size_t message_size) {
#define INVALID(...) do { snprintf(message, message_size, __VA_ARGS__); return message; } while (0)
    wide_stack_need = 0;
    if (s->texture_count && !s->textures) INVALID("texture_count is %u but textures is null", s->texture_count);
    if (s->light_count && !s->lights) INVALID("light_count is %u but lights is null", s->light_count);
    if (s->texel_bytes && !s->texels) INVALID("texel_bytes is %llu but texels is null", (unsigned long long)s->texel_bytes);
    for (uint32_t i = 1; i < s->texture_count; ++i)   // slot 0 = none
        if (invalid_texture(s->textures[i], i, s->texel_bytes, message, message_size)) return message;
    for (uint32_t i = 0; i < s->material_count; ++i)
        if (invalid_material(s->materials[i], i, s->texture_count, message, message_size)) return message;
    const uint32_t primitive_total = s->index_count / 3;
    for (uint32_t i = 0; i < s->instance_count; ++i) {
        const HiprInstance& inst = s->instances[i];
        if (inst.material_index < 0 || uint32_t(inst.material_index) >= s->material_count) INVALID("instance %u references material %d of %u", i, inst.material_index, s->material_count);
        if (inst.index_offset > primitive_total || inst.vertex_offset > s->vertex_count) INVALID("instance %u starts outside the index / vertex pools", i);
    }
    for (uint32_t t = 0; t < s->triangle_count; ++t) {
        const HiprTriangle& tri = s->triangles[t];
        if (tri.instance_index >= s->instance_count) INVALID("triangle %u references instance %u of %u", t, tri.instance_index, s->instance_count);
        const HiprInstance& inst = s->instances[tri.instance_index];
        if (tri.primitive_index >= primitive_total - inst.index_offset) INVALID("triangle %u references primitive %u beyond the index pool", t, tri.primitive_index);
        if (tri.flags & HIPR_TRIANGLE_ONE_SIDED) {      // the traversal may step over hits on its back: only where the hit program would refuse them
            const HiprMaterial& m = s->materials[inst.material_index];
            if ((m.flags & (HIPR_MATERIAL_CUTOUT | HIPR_MATERIAL_THIN_WALLED)) || m.shading_model == HIPR_SHADING_TRANSMISSIVE)
                INVALID("triangle %u is flagged HIPR_TRIANGLE_ONE_SIDED but material %d is thin-walled, a cut-out or transmissive", t, inst.material_index);
        }
        const uint32_t* idx = s->indices + 3 * size_t(inst.index_offset + tri.primitive_index);
        for (int k = 0; k < 3; ++k)
            if (idx[k] >= s->vertex_count - inst.vertex_offset) INVALID("triangle %u: vertex index %u is beyond the vertex pool", t, idx[k]);
    }
    auto leaf_ok = [&](int32_t ref) { const uint32_t code = uint32_t(~ref); return uint64_t(code >> 3) + (code & 7u) + 1u <= s->triangle_count; };
    if (s->triangle_count && s->node_count == 0) INVALID("a scene with triangles needs a BVH");
    for (uint32_t n = 0; n < s->node_count; ++n)
        for (int k = 0; k < 2; ++k) {
            const int32_t ref = s->nodes[n].child[k];
            if (ref >= 0 ? uint32_t(ref) >= s->node_count : !leaf_ok(ref)) INVALID("BVH node %u: child %d is out of range", n, ref);
        }
    if (s->wide_nodes && s->wide_node_count) {
        // need(node) = (children - 1) + max need(child): iterative post-order; a node reached twice or a cycle is an error
        std::vector<uint32_t> need(s->wide_node_count, 0u);
        std::vector<uint8_t> state(s->wide_node_count, 0);   // 0 unseen, 1 open, 2 done
        std::vector<uint32_t> stack = {0u};
        while (!stack.empty()) {
            const uint32_t n = stack.back();
            const HiprWideNode& w = s->wide_nodes[n];
            if (state[n] == 0) {
                state[n] = 1;
                for (int k = 0; k < 4; ++k) {
                    const int32_t ref = w.child[k];
                    if (ref == HIPR_WIDE_EMPTY) continue;
                    if (ref < 0) { if (!leaf_ok(ref)) INVALID("wide BVH node %u: leaf %d is out of range", n, ref); continue; }
                    if (uint32_t(ref) >= s->wide_node_count || state[ref] != 0) INVALID("wide BVH node %u: child %d is out of range or shared", n, ref);
                    stack.push_back(uint32_t(ref));
                }
            } else {
                uint32_t children = 0, below = 0;
                for (int k = 0; k < 4; ++k) {
                    const int32_t ref = w.child[k];
                    if (ref == HIPR_WIDE_EMPTY) continue;
                    ++children;
                    if (ref >= 0) below = std::max(below, need[ref]);
                }
                need[n] = (children ? children - 1u : 0u) + below;
                state[n] = 2;
                stack.pop_back();
            }
        }
        wide_stack_need = need[0];
    }
    return nullptr;
#undef INVALID
}

// The 8-wide tree of a description: every slot reached at most once from the root, child ranges inside the array, leaf records referencing triangles
// of the description, finite grid. Derives the height (the stack need of the traversal). Returns nullptr when sound.
const char* validate_wide8(const HiprSceneDesc* s, uint32_t& height, char* message, size_t message_size) {
#define INVALID(...) do { snprintf(message, message_size, __VA_ARGS__); return message; } while (0)
    height = 0;
    if (!s->wide8_slots || s->wide8_slot_count == 0) return nullptr;
    if (s->wide8_slot_count > 0x1000000u) INVALID("the 8-wide tree has %u slots, more than 2^24", s->wide8_slot_count);
    for (int a = 0; a < 3; ++a)
        if (!(s->wide8_grid_cell[a] > 0.0f) || !std::isfinite(s->wide8_grid_cell[a]) || !std::isfinite(s->wide8_grid_min[a])) INVALID("the 8-wide tree's grid is not finite");
    std::vector<uint8_t> seen(s->wide8_slot_count, 0);
    struct Visit { uint32_t slot, depth; };
    std::vector<Visit> stack = {{0u, 1u}};
    seen[0] = 1;
    while (!stack.empty()) {
        const Visit v = stack.back();
        stack.pop_back();
        height = std::max(height, v.depth);
        const HiprNode8& n = s->wide8_slots[v.slot].node;
        const uint32_t base = n.base_valid & 0xFFFFFFu, valid = n.base_valid >> 24;
        const uint32_t children = uint32_t(__builtin_popcount(valid));
        if (children == 0 || uint64_t(base) + children > s->wide8_slot_count) INVALID("8-wide node in slot %u: children [%u, %u) outside the %u slots", v.slot, base, base + children, s->wide8_slot_count);
        if (n.inner_mask & ~valid) INVALID("8-wide node in slot %u marks an empty position as an inner node", v.slot);
        uint32_t rank = 0;
        for (uint32_t position = 0; position < 8; ++position) {
            if (!(valid >> position & 1u)) continue;
            const uint32_t child = base + rank++;
            if (seen[child]) INVALID("slot %u of the 8-wide tree is reached twice", child);
            seen[child] = 1;
            if (n.inner_mask >> position & 1u) stack.push_back({child, v.depth + 1u});
            else {
                const HiprLeaf8& leaf = s->wide8_slots[child].leaf;
                if (leaf.triangle[0] >= s->triangle_count || (leaf.triangle[1] != HIPR_LEAF8_NONE && leaf.triangle[1] >= s->triangle_count))
                    INVALID("leaf record in slot %u references triangles %u / %u of %u", child, leaf.triangle[0], leaf.triangle[1], s->triangle_count);
                for (int shift = 8; shift < 16; shift += 2)
                    if (((leaf.flags >> shift) & 3u) == 3u) INVALID("leaf record in slot %u has an invalid corner selector", child);
                for (int which = 0; which < 2; ++which) {
                    if (leaf.triangle[which] == HIPR_LEAF8_NONE) continue;
                    const bool one_sided = (s->triangles[leaf.triangle[which]].flags & HIPR_TRIANGLE_ONE_SIDED) != 0;
                    if ((leaf.flags >> (2 + which) & 1u) && !one_sided) INVALID("leaf record in slot %u marks triangle %u one-sided, the triangle is not", child, leaf.triangle[which]);
                }
                if ((leaf.flags & 12u) && !(leaf.facing_margin >= 0.0f && std::isfinite(leaf.facing_margin))) INVALID("leaf record in slot %u has no valid facing margin", child);
            }
        }
    }
    return nullptr;
#undef INVALID
}

// Bit mask of the shading models that instances reference; `materials`: the pool the DEVICE holds (a geometry update brings instances, not materials).
int shading_model_mask(const HiprInstance* instances, uint32_t count, const HiprMaterial* materials) {
    int models = 0;
    for (uint32_t i = 0; i < count; ++i) models |= 1 << std::min<int>(materials[instances[i].material_index].shading_model, 2);
    return models ? models : 7;
}
// Everything hipr_upload_scene and hipr_update_scene_geometry refuse a description for by looking at it alone, and what the checks derive on the way. Pure host
// code -- no context, no HIP call: hipr_validate_scene is exactly this, and the two uploads run it before they touch the device. `who`: the entry point, for the message.
int preflight_scene(const char* who, const HiprSceneDesc* s, Preflight& out) {
    if (!s) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null scene", who);
    if (s->triangle_count && (!s->nodes || !s->triangles || !s->instances || !s->indices || !s->geometry || !s->materials))
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: missing geometry arrays", who);
    char invalid[256];
    if (validate_scene(s, out.wide_stack_need, invalid, sizeof(invalid)) || validate_wide8(s, out.wide8_height, invalid, sizeof(invalid)))
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: %s", who, invalid);
    for (uint32_t i = 0; i < s->instance_count; ++i)
        if ((s->instances[i].mesh_flags & HIPR_MESH_TEXCOORDS && !s->texcoords) || (s->instances[i].mesh_flags & HIPR_MESH_TINTS && !s->tints) ||
            (s->instances[i].mesh_flags & HIPR_MESH_EMISSIVE && !s->emissions))
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: instance %u flags an attribute whose pool is null", who, i);
    if (const HiprEnvironment* env = s->environment)
        if (env->environment_map_ID <= 0 || uint32_t(env->environment_map_ID) >= s->texture_count || !env->per_pixel_PDF || !env->samples || env->sample_count == 0 ||
            env->pdf_width == 0 || env->pdf_height == 0)
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: incomplete environment description", who);
    return HIPR_OK;
}

// Items of the exhaustive search (kernels.h "Exhaustive-search items"): every triangle in order, except that a triangle (a, b, c)
// and a LATER one of the same instance and flags that is (a, c, d) in some rotation, with bit-identical shared corners and
// d = a + (c - b) within 1e-6 of the longest edge component, are merged into the parallelogram item (a, b - a, d - a) at the first
// one's place. Only scenes of at most SMALL_SCENE_TRIANGLES triangles -- the ones searched exhaustively by default -- are paired: above
// that an exhaustive search (HIPR_TRACE_VARIANT) stays per triangle and bit-identical to the BVH searches.
constexpr uint32_t PAIRING_LIMIT = SMALL_SCENE_TRIANGLES;
void build_trace_items(const HiprTriangle* triangles, uint32_t count, std::vector<float>& items) {
    auto corner = [&](uint32_t t, int k) -> const float* { const HiprTriangle& tri = triangles[t]; return k % 3 == 0 ? tri.v0 : (k % 3 == 1 ? tri.v1 : tri.v2); };
    auto same = [](const float* p, const float* q) { return std::memcmp(p, q, 12) == 0; };
    auto bits = [](uint32_t v) { float f; std::memcpy(&f, &v, 4); return f; };
    std::vector<bool> merged(count, false);
    items.clear();
    for (uint32_t i = 0; i < count; ++i) {
        if (merged[i]) continue;
        int ra = 0, rb = 0;
        uint32_t partner = UINT32_MAX;
        for (uint32_t j = i + 1; count <= PAIRING_LIMIT && j < count && partner == UINT32_MAX; ++j) {
            if (merged[j] || triangles[j].instance_index != triangles[i].instance_index || triangles[j].flags != triangles[i].flags) continue;
            for (int x = 0; x < 3 && partner == UINT32_MAX; ++x)
                for (int y = 0; y < 3 && partner == UINT32_MAX; ++y) {
                    const float *a = corner(i, x), *b = corner(i, x + 1), *c = corner(i, x + 2), *a2 = corner(j, y), *c2 = corner(j, y + 1), *d = corner(j, y + 2);
                    if (!same(a, a2) || !same(c, c2)) continue;
                    float longest = 0.0f, off = 0.0f;
                    for (int k = 0; k < 3; ++k) {
                        longest = std::fmax(longest, std::fmax(std::fabs(b[k] - a[k]), std::fabs(d[k] - a[k])));
                        off = std::fmax(off, std::fabs(d[k] - (a[k] + (c[k] - b[k]))));
                    }
                    if (off <= 1e-6f * longest) { partner = j; ra = x; rb = y; }
                }
        }
        const float *a = corner(i, ra), *b = corner(i, ra + 1), *d = partner == UINT32_MAX ? corner(i, ra + 2) : corner(partner, rb + 2);
        // stored vertex k of a triangle is corner (k - rotation) mod 3 of its half: u = weight of vertex 1, v = weight of vertex 2
        const uint32_t selectors = partner == UINT32_MAX ? 0u : uint32_t((4 - ra) % 3) | uint32_t((5 - ra) % 3) << 2 | uint32_t((4 - rb) % 3) << 4 | uint32_t((5 - rb) % 3) << 6;
        const float item[16] = {a[0], a[1], a[2], b[0] - a[0], b[1] - a[1], b[2] - a[2], d[0] - a[0], d[1] - a[1], d[2] - a[2],
                                bits(triangles[i].instance_index), bits(triangles[i].primitive_index), bits(triangles[i].flags | (partner == UINT32_MAX ? 0u : HIPR_ITEM_QUAD)),
                                bits(i), bits(partner == UINT32_MAX ? i : partner), bits(partner == UINT32_MAX ? triangles[i].primitive_index : triangles[partner].primitive_index),
                                bits(selectors)};
        items.insert(items.end(), item, item + 16);
        if (partner != UINT32_MAX) merged[partner] = true;
    }
}

// The new instance list of hipr_edit_scene_instances: what check_instance_edit makes of the caller's list, and what rebuild_trees_on_the_device runs over.
struct InstanceEdit {
    std::vector<HiprInstance> instances;      // the new list: kept entries as the device holds them, new ones as given
    std::vector<uint32_t> source;             // per entry of the new list: the resident instance kept, BUILD_NONE for a new one
    std::vector<uint32_t> primitive_count;    // per entry of the new list: a new instance's count (kept ones: filled from the count pass)
    std::vector<uint32_t> old_to_new;         // per resident instance: its new index, BUILD_NONE when removed
    uint32_t order_capacity = 0;
    uint32_t triangle_count = 0;              // out: of the new set
};
// Every refusal of hipr_edit_scene_instances that looks at the list and the host's books alone, and the new list with its tables on the way: no HIP call.
static int check_instance_edit(const ResidentScene& r, const HiprInstanceEdit* edits, uint32_t edit_count, InstanceEdit& plan) {
    const char* who = "hipr_edit_scene_instances";
    if (!edits) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null list", who);
    const uint32_t resident = uint32_t(r.uploaded_instances.size()), primitive_total = r.uploaded_index_count / 3;
    plan.instances.resize(edit_count);
    plan.source.assign(edit_count, BUILD_NONE);
    plan.primitive_count.assign(edit_count, 0u);
    plan.old_to_new.assign(resident, BUILD_NONE);
    for (uint32_t i = 0; i < edit_count; ++i) {
        const HiprInstanceEdit& e = edits[i];
        if (e.source != HIPR_EDIT_NEW_INSTANCE) {
            if (e.source >= resident) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: entry %u keeps instance %u of %u", who, i, e.source, resident);
            if (plan.old_to_new[e.source] != BUILD_NONE) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: entry %u names instance %u, which entry %u keeps already", who, i, e.source, plan.old_to_new[e.source]);
            plan.old_to_new[e.source] = i;
            plan.source[i] = e.source;
            plan.instances[i] = r.uploaded_instances[e.source];
            continue;
        }
        const HiprInstance& inst = e.instance;
        if (inst.index_offset > primitive_total || e.primitive_count > primitive_total - inst.index_offset || inst.vertex_offset > r.uploaded_vertex_count)
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: entry %u (index offset %u, %u primitives, vertex offset %u) lies outside the uploaded pools of %u triples and %u vertices", who, i, inst.index_offset,
                        e.primitive_count, inst.vertex_offset, primitive_total, r.uploaded_vertex_count);
        if (inst.material_index < 0 || size_t(inst.material_index) >= r.uploaded_materials.size())
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: entry %u references material %d of %zu", who, i, inst.material_index, r.uploaded_materials.size());
        char invalid[256];
        if (invalid_material(r.uploaded_materials[size_t(inst.material_index)], uint32_t(inst.material_index), uint32_t(r.uploaded_textures.size()), invalid, sizeof(invalid)))
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: entry %u: %s", who, i, invalid);
        if (inst.mesh_flags & (HIPR_MESH_TEXCOORDS | HIPR_MESH_TINTS | HIPR_MESH_EMISSIVE) & ~r.uploaded_mesh_attributes)
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: entry %u flags an attribute whose pool was not uploaded", who, i);
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(inst.object_to_world[k])) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the matrix of entry %u is not finite", who, i);
        plan.instances[i] = inst;
        plan.primitive_count[i] = e.primitive_count;
    }
    return HIPR_OK;
}

// The milliseconds between two points of the host clock: how every book of this unit (*_ms) is kept.
double ms(std::chrono::steady_clock::time_point from, std::chrono::steady_clock::time_point to) { return std::chrono::duration<double, std::milli>(to - from).count(); }

} // namespace

// ---- the resident scene ----------------------------------------------------------------------------------------------------------------------------------
namespace hipr {

// The pools of a checked description, queued on `stream`: all of them (an upload), or those a geometry update brings again.
int ResidentScene::upload_pools(const HiprSceneDesc* s, bool all_pools, hipStream_t stream) {
    int r = 0;
    r |= nodes.upload(s->nodes, size_t(s->node_count) * sizeof(HiprBvhNode), stream);
    if (s->wide_nodes && s->wide_node_count) r |= wide_nodes.upload(s->wide_nodes, size_t(s->wide_node_count) * sizeof(HiprWideNode), stream);
    r |= triangles.upload(s->triangles, size_t(s->triangle_count) * sizeof(HiprTriangle), stream);
    r |= instances.upload(s->instances, size_t(s->instance_count) * sizeof(HiprInstance), stream);
    r |= lights.upload(s->lights, size_t(s->light_count) * sizeof(HiprLight), stream);
    if (all_pools) {
        r |= indices.upload(s->indices, size_t(s->index_count) * 4, stream);
        r |= geometry.upload(s->geometry, size_t(s->vertex_count) * sizeof(HiprVertexGeometry), stream);
        if (s->texcoords) r |= texcoords.upload(s->texcoords, size_t(s->vertex_count) * 8, stream);
        if (s->tints) r |= tints.upload(s->tints, size_t(s->vertex_count) * 4, stream);
        if (s->emissions) r |= emissions.upload(s->emissions, size_t(s->vertex_count) * 12, stream);
        r |= materials.upload(s->materials, size_t(s->material_count) * sizeof(HiprMaterial), stream);
        r |= textures.upload(s->textures, size_t(s->texture_count) * sizeof(HiprTexture), stream);
        r |= texels.upload(s->texels, s->texel_bytes, stream);
        if (const HiprEnvironment* env = s->environment) {
            r |= environment_PDF.upload(env->per_pixel_PDF, size_t(env->pdf_width) * env->pdf_height * sizeof(float), stream);
            r |= environment_samples.upload(env->samples, size_t(env->sample_count) * sizeof(HiprLightSample), stream);
        }
    }
    if (r) return r < 0 ? r : HIPR_ERROR_HIP;
    HIP_TRY(hipStreamSynchronize(stream));      // the caller's arrays are read
    return HIPR_OK;
}

// Uploads (or re-uploads, after a refit) the 8-wide tree of a validated description; trees higher than the largest LDS stack are left to the 4-wide kernels.
int ResidentScene::upload_wide8(const HiprSceneDesc* s, uint32_t height, bool cull_backfaces, hipStream_t stream) {
    wide8 = {};
    wide8_height = 0;
    if (!s->wide8_slots || s->wide8_slot_count == 0 || height > 33u) return HIPR_OK;
    if (int r = wide8_slots.upload(s->wide8_slots, size_t(s->wide8_slot_count) * sizeof(HiprSlot8), stream)) return r;
    HIP_TRY(hipStreamSynchronize(stream));
    wide8.slots = wide8_slots.as<uint4>();
    wide8.slot_count = s->wide8_slot_count;
    for (int a = 0; a < 3; ++a) { wide8.grid_min[a] = s->wide8_grid_min[a]; wide8.grid_cell[a] = s->wide8_grid_cell[a]; }
    wide8.cull_backfaces = cull_backfaces ? 1u : 0u;
    wide8_height = height;
    new_wide8_tree();      // the slots may be another tree's: no hint taken from the old ones names a record of these
    return HIPR_OK;
}

// What an upload derives from the material, texture and light pools it brings: the host copies later calls are checked against, and the kernel instantiations
// the pools allow (ResidentScene: a geometry update keeps them).
void ResidentScene::derive_from_pools(const HiprSceneDesc* s) {
    uploaded_materials.assign(s->materials, s->materials + s->material_count);
    uploaded_textures.assign(s->textures, s->textures + s->texture_count);
    uploaded_environment = s->environment != nullptr;
    uploaded_light_types.resize(s->light_count);
    for (uint32_t l = 0; l < s->light_count; ++l) uploaded_light_types[l] = s->lights[l].flags & HIPR_LIGHT_TYPE_MASK;
    uploaded_texture_count = s->texture_count; uploaded_vertex_count = s->vertex_count; uploaded_index_count = s->index_count; uploaded_texel_bytes = s->texel_bytes;
    uploaded_mesh_attributes = (s->texcoords ? HIPR_MESH_TEXCOORDS : 0u) | (s->tints ? HIPR_MESH_TINTS : 0u) | (s->emissions ? HIPR_MESH_EMISSIVE : 0u);
    derive_switches_from_pools();
}

// The kernel instantiations the material, texture and light pools allow, from the host copies of what the device holds: after an upload, and after a material
// edit (update_materials) has rewritten slots of the material pool.
void ResidentScene::derive_switches_from_pools() {
    has_textures = has_environment = uploaded_environment;
    for (const HiprMaterial& material : uploaded_materials)
        has_textures = has_textures || material.tint_roughness_texture_ID || material.roughness_texture_ID || material.metallic_texture_ID || material.coverage_texture_ID;
    for (uint32_t type : uploaded_light_types) has_environment = has_environment || type == HIPR_LIGHT_PRESAMPLED_ENVIRONMENT;
    for (size_t t = 1; t < uploaded_textures.size(); ++t)       // float textures take the generic samplers: TEXTURES = 2 as well
        has_environment = has_environment || uploaded_textures[t].format == HIPR_TEXEL_R32F || uploaded_textures[t].format == HIPR_TEXEL_RGBA32F;
    has_textures = has_textures || has_environment;
    coverage_textures_r8 = true;
    for (const HiprMaterial& material : uploaded_materials)
        if (const int32_t id = material.coverage_texture_ID)
            coverage_textures_r8 = coverage_textures_r8 && uint32_t(id) < uploaded_textures.size() && uploaded_textures[id].format == HIPR_TEXEL_R8 && !uploaded_textures[id].is_sRGB;
}

// The shade and trace records of every triangle (k_build_shade_triangles: the per-hit attribute chain flattened; k_build_trace_triangles: the vertex + edges form
// the trace kernels test), from the pools and the triangles the device holds at the time.
void ResidentScene::queue_triangle_records(hipStream_t stream) const {
    hipLaunchKernelGGL(k_build_shade_triangles, dim3((args.triangle_count + 255) / 256), dim3(256), 0, stream, args, shade_triangles.as<float4>());
    hipLaunchKernelGGL(k_build_trace_triangles, dim3((args.triangle_count + 255) / 256), dim3(256), 0, stream, args.triangles, args.triangle_count, trace_triangles.as<float4>());
}

// What an upload and a geometry update derive from the triangles, instances and trees they bring -- over the material pool the device HOLDS (uploaded_materials): the
// per-triangle records, the listing pass's classes, the exhaustive search's items (build_trace_items), the 8-wide tree and the device refit's lists.
// `new_topology`: an upload; a geometry update keeps the tree the upload took (or left).
int ResidentScene::derive_from_triangles(const HiprSceneDesc* s, const Preflight& checked, bool new_topology, int requested_variant, bool cull_backfaces, hipStream_t stream) {
    shading_models = shading_model_mask(s->instances, s->instance_count, uploaded_materials.data());
    uploaded_instances.assign(s->instances, s->instances + s->instance_count);
    any_coated_triangle = false;
    all_triangles_opaque = true;
    args.trace_items = nullptr;
    args.trace_item_count = 0;
    if (s->triangle_count) {
        if (int r = shade_triangles.resize(size_t(s->triangle_count) * SHADE_TRIANGLE_QUADS * sizeof(float4))) return r;
        if (int r = trace_triangles.resize(size_t(s->triangle_count) * 3 * sizeof(float4))) return r;
        args.shade_triangles = shade_triangles.as<float4>();
        args.trace_triangles = trace_triangles.as<float4>();
        queue_triangle_records(stream);
        HIP_TRY(hipGetLastError());
        std::vector<unsigned char> classes(s->triangle_count, 0);      // k_classify_hits: bit 0 = the material of its instance carries a coat
        for (uint32_t t = 0; t < s->triangle_count; ++t) {
            all_triangles_opaque = all_triangles_opaque && (s->triangles[t].flags & HIPR_TRIANGLE_OPAQUE) != 0;
            classes[t] = uploaded_materials[s->instances[s->triangles[t].instance_index].material_index].coat != 0 ? 1 : 0;
            any_coated_triangle = any_coated_triangle || classes[t] != 0;
        }
        if (int r = triangle_class.upload(classes.data(), classes.size(), stream)) return r;
        HIP_TRY(hipStreamSynchronize(stream));      // `classes` is read
        if (s->triangle_count <= SMALL_SCENE_TRIANGLES || requested_variant == HIPR_TRACE_EXHAUSTIVE) {
            std::vector<float> items;
            build_trace_items(s->triangles, s->triangle_count, items);
            if (int r = trace_items.upload(items.data(), items.size() * sizeof(float), stream)) return r;
            HIP_TRY(hipStreamSynchronize(stream));
            args.trace_items = trace_items.as<float4>();
            args.trace_item_count = uint32_t(items.size() / 16);
        }
    }
    if (new_topology || wide8.slot_count)
        if (int r = upload_wide8(s, checked.wide8_height, cull_backfaces, stream)) return r;
    return prepare_refit(s, new_topology, stream);
}

// ---- device refit (wide8_refit.h) -------------------------------------------------------------------------------------------------------------------------
// refit_scratch: [0, 48) the six reduced bounds, [48, 52) the rebuild flag, [64, 72) the area sum.
constexpr size_t REFIT_SCRATCH_FLAG = 48, REFIT_SCRATCH_AREA = 64, REFIT_SCRATCH_BYTES = 128;

// Queues passes 2 - 4. WRITE = false: exact boxes and area only (the slots stay as uploaded).
template <bool WRITE>
void ResidentScene::queue_refit_tree(const float* grid_min, const float* grid_cell, hipStream_t st) const {
    HiprSlot8* slots = wide8_slots.as<HiprSlot8>();
    RefitBox* exact = refit_exact.as<RefitBox>();
    char* scratch = refit_scratch.as<char>();
    const uint32_t slot_count = wide8.slot_count;
    if (refit_leaf_count)
        hipLaunchKernelGGL((k_refit_leaves<WRITE>), dim3((refit_leaf_count + REFIT_BLOCK - 1) / REFIT_BLOCK), dim3(REFIT_BLOCK), 0, st, slots, refit_leaf_slots.as<uint32_t>(), refit_leaf_count,
                           triangles.as<HiprTriangle>(), exact, reinterpret_cast<uint32_t*>(scratch + REFIT_SCRATCH_FLAG));
    for (size_t level = refit_level_begin.size() - 1; level-- > 0;) {      // deepest first: a launch per level is the only ordering there is
        const uint32_t begin = refit_level_begin[level], count = refit_level_begin[level + 1] - begin;
        if (!count) continue;
        hipLaunchKernelGGL((k_refit_nodes<WRITE>), dim3((count + REFIT_BLOCK - 1) / REFIT_BLOCK), dim3(REFIT_BLOCK), 0, st, slots, refit_node_slots.as<uint32_t>() + begin, count, exact,
                           grid_min[0], grid_min[1], grid_min[2], grid_cell[0], grid_cell[1], grid_cell[2]);
    }
    const uint32_t blocks = (slot_count + REFIT_BLOCK - 1) / REFIT_BLOCK;
    hipLaunchKernelGGL(k_refit_area, dim3(blocks), dim3(REFIT_BLOCK), 0, st, exact, slot_count, refit_partial.as<double>());
    hipLaunchKernelGGL(k_refit_area_final, dim3(1), dim3(REFIT_BLOCK), 0, st, refit_partial.as<double>(), blocks, reinterpret_cast<double*>(scratch + REFIT_SCRATCH_AREA));
}

// After an upload (`new_topology`) or a geometry update of a scene with the 8-wide tree: the slot lists by kind and level and the
// half area the tree starts with, taken by the kernels that take it after a refit.
int ResidentScene::prepare_refit(const HiprSceneDesc* s, bool new_topology, hipStream_t st) {
    tree_stale = false;
    if (wide8.slot_count == 0) {
        refit_level_begin.clear();
        refit_node_list.clear();
        refit_node_words.clear();
        refit_leaf_count = 0;
        uploaded_half_area = current_half_area = 0.0;
        return HIPR_OK;
    }
    const uint32_t slot_count = wide8.slot_count;
    // A geometry update promises the uploaded topology, and hipr_update_scene_geometry has only compared counts and heights: the lists are kept when every node they
    // name carries the topology words they were made from -- from the root down that is the same tree, slot for slot -- and made again otherwise, so that the
    // leaf kernel never takes a node slot for a leaf record.
    if (!new_topology) {
        new_topology = refit_node_list.empty() || refit_node_words.size() != refit_node_list.size() * 2;
        for (size_t i = 0; i < refit_node_list.size() && !new_topology; ++i) {
            const HiprNode8& n = s->wide8_slots[refit_node_list[i]].node;
            new_topology = n.base_valid != refit_node_words[2 * i] || n.inner_mask != refit_node_words[2 * i + 1];
        }
    }
    if (new_topology) {
        std::vector<uint32_t> nodes = {0u}, leaves;
        nodes.reserve(slot_count / 4 + 1);
        leaves.reserve(slot_count);
        refit_level_begin.assign(1, 0u);
        for (size_t begin = 0; begin < nodes.size();) {      // the tree was validated: every child slot is in range and has one parent
            const size_t end = nodes.size();
            refit_level_begin.push_back(uint32_t(end));
            for (size_t i = begin; i < end; ++i) {
                const HiprNode8& n = s->wide8_slots[nodes[i]].node;
                const uint32_t base = n.base_valid & 0xFFFFFFu, valid = n.base_valid >> 24;
                uint32_t rank = 0;
                for (int p = 0; p < 8; ++p) {
                    if (!(valid >> p & 1u)) continue;
                    const uint32_t child = base + rank++;
                    if (n.inner_mask >> p & 1u) nodes.push_back(child); else leaves.push_back(child);
                }
            }
            begin = end;
        }
        refit_leaf_count = uint32_t(leaves.size());
        refit_node_list.clear();      // the host copies describe what the device holds: set together, once the uploads below are through
        refit_node_words.clear();
        const size_t triangle_blocks = (size_t(s->triangle_count) + REFIT_BLOCK - 1) / REFIT_BLOCK, slot_blocks = (size_t(slot_count) + REFIT_BLOCK - 1) / REFIT_BLOCK;
        int r = 0;
        r |= refit_node_slots.upload(nodes.data(), nodes.size() * 4, st);
        r |= refit_leaf_slots.upload(leaves.data(), leaves.size() * 4, st);
        r |= refit_exact.resize(size_t(slot_count) * sizeof(RefitBox));
        r |= refit_moved.resize(std::max<size_t>(s->instance_count, 1) * 4);
        r |= refit_partial.resize(std::max(triangle_blocks * 6 * sizeof(RefitBound), slot_blocks * sizeof(double)));
        r |= refit_scratch.resize(REFIT_SCRATCH_BYTES);
        if (r) return r < 0 ? r : HIPR_ERROR_HIP;
        HIP_TRY(hipStreamSynchronize(st));      // the upload reads the lists
        refit_node_words.resize(nodes.size() * 2);
        for (size_t i = 0; i < nodes.size(); ++i) {
            refit_node_words[2 * i] = s->wide8_slots[nodes[i]].node.base_valid;
            refit_node_words[2 * i + 1] = s->wide8_slots[nodes[i]].node.inner_mask;
        }
        refit_node_list = std::move(nodes);
    }
    queue_refit_tree<false>(wide8.grid_min, wide8.grid_cell, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&uploaded_half_area, refit_scratch.as<char>() + REFIT_SCRATCH_AREA, sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    current_half_area = uploaded_half_area;
    return HIPR_OK;
}

int ResidentScene::upload(const HiprSceneDesc* s, const Preflight& checked, int requested_variant, bool cull_backfaces, hipStream_t stream) {
    begin_write();
    wide4_awaits_geometry = false;
    rigs.clear();      // hipr_set_scene_rigs' ranges are coordinates of the pools that go now
    rig_records.release();
    rig_data.release();
    if (int r = upload_pools(s, true, stream)) return r;
    const HiprEnvironment* env = s->environment;
    args.nodes = nodes.as<float4>();
    args.node_count = s->node_count;
    args.wide_nodes = s->wide_nodes && s->wide_node_count ? wide_nodes.as<uint4>() : nullptr;
    args.wide_node_count = s->wide_nodes ? s->wide_node_count : 0u;
    args.triangles = triangles.as<float4>();
    args.triangle_count = s->triangle_count;
    args.instances = instances.as<HiprInstance>();
    args.indices = indices.as<uint32_t>();
    args.geometry = geometry.as<float4>();
    args.texcoords = texcoords.as<float2>();
    args.tints = tints.as<uint32_t>();
    args.emissions = emissions.as<float>();
    args.materials = materials.as<HiprMaterial>();
    args.lights = lights.as<HiprLight>();
    args.light_count = s->light_count;
    args.textures = textures.as<HiprTexture>();
    args.texels = texels.as<uint8_t>();
    args.env_map_ID = env ? env->environment_map_ID : 0;
    args.env_per_pixel_PDF = env ? environment_PDF.as<float>() : nullptr;
    args.env_samples = env ? environment_samples.as<float4>() : nullptr;
    args.env_pdf_width = env ? env->pdf_width : 0u; args.env_pdf_height = env ? env->pdf_height : 0u; args.env_sample_count = env ? env->sample_count : 0u;
    wide_stack_entries = checked.wide_stack_need;
    stack_size = s->bvh_max_depth <= 16 ? 16 : (s->bvh_max_depth <= 32 ? 32 : 64);
    derive_from_pools(s);
    if (int r = derive_from_triangles(s, checked, true, requested_variant, cull_backfaces, stream)) return r;
    choose_variant(requested_variant);
    ready = true;
    return HIPR_OK;
}

// The pools it brings again have the uploaded sizes (hipr_update_scene_geometry has compared them): no buffer moves, the pointers and counts in `args` stay.
int ResidentScene::update_geometry(const HiprSceneDesc* s, const Preflight& checked, int requested_variant, bool cull_backfaces, hipStream_t stream) {
    begin_write();
    if (int r = upload_pools(s, false, stream)) return r;
    if (wide4_awaits_geometry) {      // the 4-wide array of the rebuilt tree: the buffer may have moved and its size has changed
        args.wide_nodes = s->wide_nodes && s->wide_node_count ? wide_nodes.as<uint4>() : nullptr;
        args.wide_node_count = s->wide_nodes ? s->wide_node_count : 0u;
        wide_stack_entries = checked.wide_stack_need;
        wide4_awaits_geometry = false;
    }
    if (int r = derive_from_triangles(s, checked, false, requested_variant, cull_backfaces, stream)) return r;      // also ends the state a device refit left
    ready = true;
    return HIPR_OK;
}

// The lights ARE brought again by a geometry update and a device refit (they move), but the kernels were instantiated for the kinds of light the upload brought --
// environment code or not -- and the environment's own data is not part of either: a light may move, not change its type.
int ResidentScene::lights_keep_their_types(const char* who, const HiprLight* new_lights, uint32_t count) const {
    for (uint32_t l = 0; l < count; ++l)
        if ((new_lights[l].flags & HIPR_LIGHT_TYPE_MASK) != uploaded_light_types[l])
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: light %u changes its type (%u -> %u); upload the scene instead", who, l, uploaded_light_types[l], new_lights[l].flags & HIPR_LIGHT_TYPE_MASK);
    return HIPR_OK;
}

// The device work of hipr_refit_scene_transforms, which has checked the arguments against uploaded_instances and uploaded_light_types.
int ResidentScene::refit_transforms(const HiprInstanceTransform* moved, uint32_t moved_count, const HiprLight* new_lights, uint32_t light_count, hipStream_t st, HiprRefitResult* out) {
    begin_write();
    *out = {};
    if (new_lights && light_count) {
        if (int r = lights.upload(new_lights, size_t(light_count) * sizeof(HiprLight), st)) return r;
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (moved_count) {
        std::vector<uint32_t> flags(uploaded_instances.size(), 0u);
        std::vector<HiprInstance> moved_instances = uploaded_instances;      // becomes the host copy once the device holds it (after the last synchronise)
        for (uint32_t k = 0; k < moved_count; ++k) {
            std::memcpy(moved_instances[moved[k].instance_index].object_to_world, moved[k].object_to_world, sizeof(moved[k].object_to_world));
            flags[moved[k].instance_index] = 1u;
        }
        HIP_TRY(hipMemcpyAsync(instances.ptr, moved_instances.data(), moved_instances.size() * sizeof(HiprInstance), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(refit_moved.ptr, flags.data(), flags.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(refit_scratch.ptr, 0, REFIT_SCRATCH_BYTES, st));
        // pass 1: world-space triangles and the scene's bounds
        const uint32_t blocks = (args.triangle_count + REFIT_BLOCK - 1) / REFIT_BLOCK;
        hipLaunchKernelGGL(k_refit_triangles, dim3(blocks), dim3(REFIT_BLOCK), 0, st, triangles.as<HiprTriangle>(), args.triangle_count, instances.as<HiprInstance>(), refit_moved.as<uint32_t>(),
                           indices.as<uint32_t>(), geometry.as<HiprVertexGeometry>(), refit_partial.as<RefitBound>());
        hipLaunchKernelGGL(k_refit_bounds_final, dim3(1), dim3(REFIT_BLOCK), 0, st, refit_partial.as<RefitBound>(), blocks, refit_scratch.as<RefitBound>());
        HIP_TRY(hipGetLastError());
        RefitBound bounds[6];
        HIP_TRY(hipMemcpyAsync(bounds, refit_scratch.ptr, sizeof(bounds), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));      // `flags` and the instances are read by now as well
        const float lo[3] = {bounds[0].v, bounds[1].v, bounds[2].v}, hi[3] = {bounds[3].v, bounds[4].v, bounds[5].v};
        float grid_min[3], grid_cell[3];
        refit_grid(lo, hi, grid_min, grid_cell);      // the moved scene's bounds: node origins must not be clamped at the ends of a stale grid
        // passes 2 - 4, then the records derived from the triangles
        queue_refit_tree<true>(grid_min, grid_cell, st);
        queue_triangle_records(st);
        HIP_TRY(hipGetLastError());
        struct { uint32_t flag; uint32_t pad[3]; double area; } tail = {};
        static_assert(REFIT_SCRATCH_AREA - REFIT_SCRATCH_FLAG == 16, "the flag and the area are read back together");
        HIP_TRY(hipMemcpyAsync(&tail, refit_scratch.as<char>() + REFIT_SCRATCH_FLAG, sizeof(tail), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        uploaded_instances.swap(moved_instances);
        tree_stale = true;
        for (int a = 0; a < 3; ++a) { wide8.grid_min[a] = grid_min[a]; wide8.grid_cell[a] = grid_cell[a]; }
        current_half_area = tail.area;
        out->needs_rebuild = tail.flag ? 1 : 0;      // a pair parted: this tree cannot hold the scene any more
    }
    out->child_half_area = current_half_area;
    out->uploaded_half_area = uploaded_half_area;
    for (int a = 0; a < 3; ++a) { out->grid_min[a] = wide8.grid_min[a]; out->grid_cell[a] = wide8.grid_cell[a]; }
    ready = !out->needs_rebuild;
    awaits_rebuild = !ready;
    return HIPR_OK;
}

// The device work of hipr_update_scene_materials, which has checked every index against uploaded_materials, uploaded_instances and uploaded_textures.
int ResidentScene::update_materials(const HiprMaterialUpdate* changed, uint32_t changed_count, const HiprInstanceMaterial* assignments, uint32_t assignment_count, hipStream_t st) {
    begin_write();
    // the host copies as they will be once the device holds them (after the last synchronise); the copies below read from them
    std::vector<HiprMaterial> new_materials = uploaded_materials;
    std::vector<HiprInstance> new_instances = uploaded_instances;
    std::vector<bool> rewritten(new_materials.size(), false);
    std::vector<uint32_t> touched(std::max<size_t>(new_instances.size(), 1), 0u);
    for (uint32_t k = 0; k < changed_count; ++k) { new_materials[changed[k].material_index] = changed[k].material; rewritten[changed[k].material_index] = true; }
    for (uint32_t k = 0; k < assignment_count; ++k) { new_instances[assignments[k].instance_index].material_index = assignments[k].material_index; touched[assignments[k].instance_index] = 1u; }
    for (size_t i = 0; i < new_instances.size(); ++i)
        if (rewritten[size_t(new_instances[i].material_index)]) touched[i] = 1u;
    // 1. the changed slots and words
    for (uint32_t k = 0; k < changed_count; ++k) {
        const size_t at = changed[k].material_index;
        HIP_TRY(hipMemcpyAsync(materials.as<HiprMaterial>() + at, &new_materials[at], sizeof(HiprMaterial), hipMemcpyHostToDevice, st));
    }
    for (uint32_t k = 0; k < assignment_count; ++k) {
        const size_t at = assignments[k].instance_index;
        HIP_TRY(hipMemcpyAsync(&instances.as<HiprInstance>()[at].material_index, &new_instances[at].material_index, sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    uint32_t reduction[2] = {1u, 0u};      // all opaque, none coated: the result for a scene without triangles
    if (args.triangle_count) {
        // 2. the two passes
        if (int r = material_touched.upload(touched.data(), touched.size() * 4, st)) return r;
        if (int r = material_scratch.resize(64)) return r;
        uint32_t* words = material_scratch.as<uint32_t>();
        HIP_TRY(hipMemsetAsync(words, 0, 64, st));
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(words), 1, 1, st));
        const MaterialUpdateArrays a = {triangles.as<HiprTriangle>(), args.triangle_count, instances.as<HiprInstance>(), materials.as<HiprMaterial>(), indices.as<uint32_t>(),
                                        reinterpret_cast<const float*>(args.texcoords), textures.as<HiprTexture>(), uint32_t(uploaded_textures.size()), texels.as<uint8_t>(),
                                        material_touched.as<uint32_t>(), trace_triangles.as<uint32_t>(), shade_triangles.as<uint32_t>(), triangle_class.as<uint8_t>()};
        hipLaunchKernelGGL(k_update_triangle_materials, dim3((args.triangle_count + MATERIAL_UPDATE_BLOCK - 1) / MATERIAL_UPDATE_BLOCK), dim3(MATERIAL_UPDATE_BLOCK), 0, st, a, words);
        if (wide8.slot_count && refit_leaf_count)
            hipLaunchKernelGGL(k_update_leaf_flags, dim3((refit_leaf_count + MATERIAL_UPDATE_BLOCK - 1) / MATERIAL_UPDATE_BLOCK), dim3(MATERIAL_UPDATE_BLOCK), 0, st, wide8_slots.as<HiprSlot8>(),
                               refit_leaf_slots.as<uint32_t>(), refit_leaf_count, triangles.as<HiprTriangle>());
        HIP_TRY(hipGetLastError());
        // 3. the eight reduction bytes
        HIP_TRY(hipMemcpyAsync(reduction, words, sizeof(reduction), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));      // `touched`, new_materials and new_instances are read by now as well
    // 4., 5. the host copies in step, and what is derived from them
    uploaded_materials.swap(new_materials);
    uploaded_instances.swap(new_instances);
    shading_models = shading_model_mask(uploaded_instances.data(), uint32_t(uploaded_instances.size()), uploaded_materials.data());
    derive_switches_from_pools();
    all_triangles_opaque = reduction[0] != 0;
    any_coated_triangle = reduction[1] != 0;
    ready = true;
    return HIPR_OK;
}

// The device work of hipr_append_scene_pools (pool_growth.h). Every new buffer is allocated BEFORE the scene is touched: a failed allocation frees what it got and
// leaves the scene as found. A pool whose buffer has the room (a larger scene was uploaded before) takes its tail in place; the others get a buffer of exactly the
// new size -- no headroom: what it is worth has not been measured (the pools of the 10 M atrium are 152 MB and copy in 0.1 ms; a texel pool can be gigabytes). Then, as the other writers: not ready,
// the copies and the mirror kernel on the stream, the new pointers in `args`, the host copies, the switches -- and the state the call found, ready or awaiting a
// rebuild: no tree, triangle or instance references a tail, so nothing derived from them changes.
int ResidentScene::append_pools(const HiprPoolGrowth& g, hipStream_t st) {
    struct Pool { DeviceBuffer* pool; size_t keep, tail_bytes; const void* tail; DeviceBuffer fresh; };
    const size_t vertices = uploaded_vertex_count;
    // an attribute pool the device holds takes its tail; one it does not hold comes whole (or not at all)
    auto attribute = [&](DeviceBuffer* pool, uint32_t bit, const void* array, uint32_t covered, size_t stride) -> Pool {
        return {pool, uploaded_mesh_attributes & bit ? vertices * stride : 0u, size_t(covered) * stride, array, DeviceBuffer()};
    };
    size_t segment_words = 0;
    for (uint32_t k = 0; k < g.segment_count; ++k) segment_words += g.segments[k].index_count;
    Pool pools[] = {
        {&indices, size_t(uploaded_index_count) * 4, segment_words * 4, nullptr, DeviceBuffer()},      // its tail is the segments'
        {&geometry, vertices * sizeof(HiprVertexGeometry), size_t(g.vertex_count) * sizeof(HiprVertexGeometry), g.geometry, DeviceBuffer()},
        attribute(&texcoords, HIPR_MESH_TEXCOORDS, g.texcoords, g.texcoord_vertices, 8),
        attribute(&tints, HIPR_MESH_TINTS, g.tints, g.tint_vertices, 4),
        attribute(&emissions, HIPR_MESH_EMISSIVE, g.emissions, g.emission_vertices, 12),
        {&materials, uploaded_materials.size() * sizeof(HiprMaterial), size_t(g.material_count) * sizeof(HiprMaterial), g.materials, DeviceBuffer()},
        {&textures, uploaded_textures.size() * sizeof(HiprTexture), size_t(g.texture_count) * sizeof(HiprTexture), g.textures, DeviceBuffer()},
        {&texels, size_t(uploaded_texel_bytes), size_t(g.texel_bytes), g.texels, DeviceBuffer()},
    };
    const auto t0 = std::chrono::steady_clock::now();
    for (Pool& p : pools)
        if (p.tail_bytes && !(p.pool->ptr && p.pool->bytes >= p.keep + p.tail_bytes))
            if (p.fresh.resize(p.keep + p.tail_bytes)) {
                (void)hipGetLastError();      // the failed allocation's error is answered here: it must not meet the next call's check
                return HIPR_ERROR_OUT_OF_MEMORY;      // `pools` goes, and with it what the others got
            }
    const auto t1 = std::chrono::steady_clock::now();
    const bool was_ready = ready, awaited_rebuild = awaits_rebuild;
    begin_write();
    // the resident parts into the new allocations first; events around them tell their time from the tails' without a synchronise of their own
    for (Event& e : append_events)
        if (!e) e = make_event(hipEventDefault);
    const bool timed = append_events[0] && append_events[1] && append_events[2];
    if (timed) HIP_TRY(hipEventRecord(append_events[0], st));
    for (Pool& p : pools)
        if (p.tail_bytes && p.fresh.ptr) HIP_TRY(queue_pool_growth(p.fresh.ptr, p.pool->ptr, p.keep, nullptr, 0u, st));
    if (timed) HIP_TRY(hipEventRecord(append_events[1], st));
    for (Pool& p : pools) {
        if (!p.tail_bytes) continue;
        void* grown = p.fresh.ptr ? p.fresh.ptr : p.pool->ptr;
        HIP_TRY(queue_pool_growth(grown, grown, p.keep, p.tail, p.tail ? p.tail_bytes : 0u, st));
        if (p.pool != &indices) continue;
        // the segments in order: a mirror reads what the stream has put there by then, earlier segments of this call included
        uint32_t* words = static_cast<uint32_t*>(grown);
        size_t position = uploaded_index_count, taken = 0;
        for (uint32_t k = 0; k < g.segment_count; ++k) {
            const HiprIndexSegment& s = g.segments[k];
            if (s.mirrored_from == HIPR_SEGMENT_FROM_HOST) {
                if (s.index_count) HIP_TRY(hipMemcpyAsync(words + position, g.indices + taken, size_t(s.index_count) * 4, hipMemcpyHostToDevice, st));
                taken += s.index_count;
            } else queue_mirror_triples(words, s.mirrored_from, uint32_t(position / 3), s.index_count / 3, st);
            position += s.index_count;
        }
        HIP_TRY(hipGetLastError());
    }
    if (timed) HIP_TRY(hipEventRecord(append_events[2], st));
    HIP_TRY(hipStreamSynchronize(st));      // the caller's arrays are read; the old buffers are free to go
    float copies_ms = 0.0f, tails_ms = 0.0f;
    if (timed) { HIP_TRY(hipEventElapsedTime(&copies_ms, append_events[0], append_events[1])); HIP_TRY(hipEventElapsedTime(&tails_ms, append_events[1], append_events[2])); }
    append_ms[0] = ms(t0, t1); append_ms[1] = copies_ms; append_ms[2] = tails_ms;
    for (Pool& p : pools)
        if (p.fresh.ptr) std::swap(*p.pool, p.fresh);      // the old buffer goes with `pools`
    args.indices = indices.as<uint32_t>();
    args.geometry = geometry.as<float4>();
    args.texcoords = texcoords.as<float2>();
    args.tints = tints.as<uint32_t>();
    args.emissions = emissions.as<float>();
    args.materials = materials.as<HiprMaterial>();
    args.textures = textures.as<HiprTexture>();
    args.texels = texels.as<uint8_t>();
    uploaded_materials.insert(uploaded_materials.end(), g.materials, g.materials + g.material_count);
    uploaded_textures.insert(uploaded_textures.end(), g.textures, g.textures + g.texture_count);
    uploaded_texture_count = uint32_t(uploaded_textures.size());
    uploaded_vertex_count += g.vertex_count;
    uploaded_index_count += uint32_t(segment_words);
    uploaded_mesh_attributes |= (g.texcoord_vertices ? HIPR_MESH_TEXCOORDS : 0u) | (g.tint_vertices ? HIPR_MESH_TINTS : 0u) | (g.emission_vertices ? HIPR_MESH_EMISSIVE : 0u);
    uploaded_texel_bytes += g.texel_bytes;
    derive_switches_from_pools();
    ready = was_ready;
    awaits_rebuild = awaited_rebuild;
    return HIPR_OK;
}

// The device work of hipr_update_scene_lighting (environment_build.h). The scratch and every new buffer -- the lights', the environment's PDF image and samples --
// are allocated BEFORE the scene is touched: a failed allocation leaves the scene as found. The kernels write scratch and the new buffers only; the resident ones
// are exchanged for them at the end, when nothing can fail any more. Then, as the other writers: the new pointers and counts in `args`, the host copies, the
// switches -- and the state the call found, ready or awaiting a rebuild: no triangle, tree or pool has changed.
int ResidentScene::update_lighting(const HiprLight* new_lights, uint32_t light_count, int action, const HiprEnvironmentBuild* build, float* out_per_pixel_PDF, HiprLightSample* out_samples,
                                   LightingScratch& x, hipStream_t st, HiprLightingResult* out) {
    const auto t0 = std::chrono::steady_clock::now();
    const bool builds = action == HIPR_ENVIRONMENT_BUILD;
    DeviceBuffer fresh_lights, fresh_PDF, fresh_samples;
    EnvTexture texture = {};
    uint32_t width = 0, height = 0, samples = 0;
    bool blurs = false;
    int r = fresh_lights.resize((size_t(light_count) + 1) * sizeof(HiprLight));
    if (builds) {
        const HiprTexture& t = uploaded_textures[size_t(build->environment_map_ID)];
        texture = {t.width, t.height, t.format, t.wrap_u, t.wrap_v, t.filter, texels.as<uint8_t>() + t.texel_offset, nullptr};
        width = t.width; height = build->pdf_height; samples = build->sample_count;
        blurs = (t.filter & 1u) != 0 || height != t.height;      // compute_distribution's filter_pixels
        const size_t texel_count = size_t(width) * height;
        r |= fresh_PDF.resize(texel_count * sizeof(float));
        r |= fresh_samples.resize(size_t(samples) * sizeof(HiprLightSample));
        r |= x.row_sines.resize(size_t(height) * sizeof(float));
        r |= x.srgb_decode.resize(256 * sizeof(float));
        r |= x.draw_points.resize(size_t(samples) * 2 * sizeof(float));
        r |= x.importance.resize(texel_count * sizeof(float));
        if (blurs) r |= x.blurred.resize(texel_count * sizeof(float));
        r |= x.conditional.resize(size_t(width + 1) * height * sizeof(float));
        r |= x.marginal_raw.resize((size_t(height) + 1) * sizeof(float));
        r |= x.marginal.resize((size_t(height) + 1) * sizeof(float));
        r |= x.totals.resize(size_t(height) * sizeof(float));
        r |= x.integral.resize(sizeof(float));
        for (Event& e : x.events)
            if (!e) e = make_event(hipEventDefault);
    }
    if (r) {
        (void)hipGetLastError();      // the failed allocation's error is answered here: it must not meet the next call's check
        return HIPR_ERROR_OUT_OF_MEMORY;      // the new buffers go with this frame
    }
    const bool was_ready = ready, awaited_rebuild = awaits_rebuild;
    begin_write();
    const bool timed = x.events[0] && x.events[1] && x.events[2] && x.events[3];
    bool disabled = false;
    float kernel_ms[2] = {0.0f, 0.0f};
    double finish_ms = 0.0, readback_ms = 0.0;
    auto t1 = t0;
    std::vector<HiprLightSample> finished;
    if (builds) {
        HIP_TRY(hipMemcpyAsync(x.row_sines.ptr, build->row_sines, size_t(height) * sizeof(float), hipMemcpyHostToDevice, st));
        if (build->srgb_decode) { HIP_TRY(hipMemcpyAsync(x.srgb_decode.ptr, build->srgb_decode, 256 * sizeof(float), hipMemcpyHostToDevice, st)); texture.srgb_decode = x.srgb_decode.as<float>(); }
        HIP_TRY(hipMemcpyAsync(x.draw_points.ptr, build->draw_points, size_t(samples) * 2 * sizeof(float), hipMemcpyHostToDevice, st));
        t1 = std::chrono::steady_clock::now();
        const size_t texel_count = size_t(width) * height;
        const uint32_t texel_blocks = uint32_t((texel_count + ENV_BLOCK - 1) / ENV_BLOCK);
        if (timed) HIP_TRY(hipEventRecord(x.events[0], st));
        hipLaunchKernelGGL(k_env_importance, dim3(texel_blocks), dim3(ENV_BLOCK), 0, st, texture, height, x.row_sines.as<float>(), x.importance.as<float>());
        if (blurs) hipLaunchKernelGGL(k_env_blur, dim3(texel_blocks), dim3(ENV_BLOCK), 0, st, x.importance.as<float>(), width, height, x.blurred.as<float>());
        const float* function = blurs ? x.blurred.as<float>() : x.importance.as<float>();
        hipLaunchKernelGGL(k_env_row_sums, dim3((height + ENV_BAND_ROWS - 1) / ENV_BAND_ROWS), dim3(ENV_BLOCK), 0, st, function, width, height, x.conditional.as<float>());
        hipLaunchKernelGGL(k_env_marginal, dim3(1), dim3(64), 0, st, x.conditional.as<float>(), width, height, x.marginal_raw.as<float>(), x.totals.as<float>(), x.integral.as<float>());
        HIP_TRY(hipGetLastError());
        if (timed) HIP_TRY(hipEventRecord(x.events[1], st));
        float integral = 0.0f;
        HIP_TRY(hipMemcpyAsync(&integral, x.integral.ptr, sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));      // the tables are read by now as well; the branch below is presample_environment's, taken where it takes it
        if (timed) HIP_TRY(hipEventElapsedTime(&kernel_ms[0], x.events[0], x.events[1]));
        disabled = integral < 0.00001f;
        if (disabled) {
            width = height = samples = 1;
            finished.assign(1, HiprLightSample{{0, 0, 0}, 0.0f, {0, 1, 0}, 0.0f});      // LightSample::none()
            HIP_TRY(hipMemsetAsync(fresh_PDF.ptr, 0, sizeof(float), st));
        } else {
            const float PDF_scale = float(int(width) * int(height)) * (1.0f / (2.0f * 3.14159265358979323846f * 3.14159265358979323846f));
            const size_t entries = size_t(width + 1) * height;
            if (timed) HIP_TRY(hipEventRecord(x.events[2], st));
            hipLaunchKernelGGL(k_env_normalise, dim3(uint32_t((entries + ENV_BLOCK - 1) / ENV_BLOCK)), dim3(ENV_BLOCK), 0, st, x.marginal_raw.as<float>(), x.totals.as<float>(), width, height,
                               x.marginal.as<float>(), x.conditional.as<float>());
            hipLaunchKernelGGL(k_env_pdf_image, dim3(texel_blocks), dim3(ENV_BLOCK), 0, st, x.marginal.as<float>(), x.conditional.as<float>(), width, height, PDF_scale, fresh_PDF.as<float>());
            hipLaunchKernelGGL(k_env_draws, dim3((samples + ENV_BLOCK - 1) / ENV_BLOCK), dim3(ENV_BLOCK), 0, st, texture, x.marginal.as<float>(), x.conditional.as<float>(), height,
                               x.draw_points.as<float>(), samples, fresh_samples.as<HiprLightSample>());
            HIP_TRY(hipGetLastError());
            if (timed) HIP_TRY(hipEventRecord(x.events[3], st));
            finished.resize(samples);
            const auto r0 = std::chrono::steady_clock::now();
            HIP_TRY(hipMemcpyAsync(finished.data(), fresh_samples.ptr, size_t(samples) * sizeof(HiprLightSample), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (timed) HIP_TRY(hipEventElapsedTime(&kernel_ms[1], x.events[2], x.events[3]));
            const auto r1 = std::chrono::steady_clock::now();
            for (HiprLightSample& s : finished) finish_environment_sample(s);
            finish_ms = ms(r1, std::chrono::steady_clock::now());
            readback_ms = ms(r0, r1);
        }
        const auto r2 = std::chrono::steady_clock::now();
        HIP_TRY(hipMemcpyAsync(fresh_samples.ptr, finished.data(), finished.size() * sizeof(HiprLightSample), hipMemcpyHostToDevice, st));
        if (out_per_pixel_PDF) HIP_TRY(hipMemcpyAsync(out_per_pixel_PDF, fresh_PDF.ptr, size_t(width) * height * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (out_samples) std::memcpy(out_samples, finished.data(), finished.size() * sizeof(HiprLightSample));
        readback_ms += ms(r2, std::chrono::steady_clock::now());
    }
    // the new list, with the environment's light last when the environment that is resident from here on takes part in next event estimation
    const uint32_t resident_samples = builds ? samples : (action == HIPR_ENVIRONMENT_KEEP && uploaded_environment ? args.env_sample_count : 0u);
    std::vector<HiprLight> list(new_lights, new_lights + light_count);
    if (resident_samples > 1) {      // next_event_estimation_possible (SceneBuilder::set_environment)
        HiprLight light = {};
        light.flags = HIPR_LIGHT_PRESAMPLED_ENVIRONMENT;
        list.push_back(light);
    }
    const auto l0 = std::chrono::steady_clock::now();
    if (!list.empty()) HIP_TRY(hipMemcpyAsync(fresh_lights.ptr, list.data(), list.size() * sizeof(HiprLight), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));      // `list` is read; nothing is queued any more: the resident buffers change hands
    const double lights_ms = ms(l0, std::chrono::steady_clock::now());
    std::swap(lights, fresh_lights);      // the old buffers go with this frame
    args.lights = lights.as<HiprLight>();
    args.light_count = uint32_t(list.size());
    if (builds) {
        std::swap(environment_PDF, fresh_PDF);
        std::swap(environment_samples, fresh_samples);
        args.env_map_ID = build->environment_map_ID;
        args.env_per_pixel_PDF = environment_PDF.as<float>();
        args.env_samples = environment_samples.as<float4>();
        args.env_pdf_width = width; args.env_pdf_height = height; args.env_sample_count = samples;
        uploaded_environment = true;
    } else if (action == HIPR_ENVIRONMENT_REMOVE) {
        args.env_map_ID = 0;
        args.env_per_pixel_PDF = nullptr;
        args.env_samples = nullptr;
        args.env_pdf_width = args.env_pdf_height = args.env_sample_count = 0u;
        uploaded_environment = false;
    }
    uploaded_light_types.resize(list.size());
    for (size_t l = 0; l < list.size(); ++l) uploaded_light_types[l] = list[l].flags & HIPR_LIGHT_TYPE_MASK;
    derive_switches_from_pools();
    x.upload_ms = ms(t0, t1) + lights_ms; x.kernel_ms = double(kernel_ms[0]) + double(kernel_ms[1]); x.finish_ms = finish_ms; x.readback_ms = readback_ms;
    *out = {};
    out->pdf_width = args.env_pdf_width; out->pdf_height = args.env_pdf_height; out->sample_count = args.env_sample_count;
    out->importance_sampling_disabled = disabled ? 1u : 0u;
    out->light_count = args.light_count;
    out->switches = (has_textures ? HIPR_SWITCH_TEXTURES : 0u) | (has_environment ? HIPR_SWITCH_ENVIRONMENT : 0u);
    ready = was_ready;
    awaits_rebuild = awaited_rebuild;
    return HIPR_OK;
}

// The device work of hipr_update_scene_texels (texel_update.h). The scratch is allocated BEFORE the scene is touched: a failed allocation leaves the scene as found.
// Then, as the other writers: not ready, the copies and the passes on the stream, the host copies -- and the state the call found, ready or awaiting a rebuild: no
// tree, corner or pool other than the texels has changed. The flag pass is left out when no resident instance wears a material that leaves its triangles' flags to an
// edited texture (the host copies answer that): a tint texture's edit is the rectangle writes alone.
int ResidentScene::update_texels(const HiprTexelEdit* edits, uint32_t edit_count, TexelScratch& x, hipStream_t st, HiprTexelUpdateResult* out) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<TexelRectangle> rectangles(edit_count);
    std::vector<bool> edited(uploaded_textures.size(), false);
    uint64_t staging_bytes = 0;
    bool environment_stale = false;
    for (uint32_t k = 0; k < edit_count; ++k) {
        rectangles[k] = planned_rectangle(edits[k], uploaded_textures[edits[k].texture_index], staging_bytes);
        edited[edits[k].texture_index] = true;
        environment_stale = environment_stale || (uploaded_environment && args.env_map_ID == int32_t(edits[k].texture_index));
    }
    // `touched`: the instances whose material's deciding coverage texture is an edited one
    std::vector<uint32_t> touched(std::max<size_t>(uploaded_instances.size(), 1), 0u);
    bool decides_flags = false;
    for (size_t i = 0; i < uploaded_instances.size(); ++i)
        if (const HiprTexture* deciding = deciding_coverage_texture(uploaded_materials[size_t(uploaded_instances[i].material_index)], uploaded_textures.data(), uint32_t(uploaded_textures.size())))
            if (edited[size_t(deciding - uploaded_textures.data())]) { touched[i] = 1u; decides_flags = true; }
    decides_flags = decides_flags && args.triangle_count != 0;
    std::vector<uint8_t> packed(staging_bytes, uint8_t(0));
    for (uint32_t k = 0; k < edit_count; ++k) pack_rectangle_rows(edits[k], rectangles[k], packed.data());
    int r = x.staging.resize(staging_bytes);
    if (decides_flags) {
        r |= x.touched.resize(touched.size() * sizeof(uint32_t));
        r |= x.words.resize(TEXEL_SCRATCH_WORDS * sizeof(uint32_t));
    }
    if (r) {
        (void)hipGetLastError();      // the failed allocation's error is answered here: it must not meet the next call's check
        return HIPR_ERROR_OUT_OF_MEMORY;
    }
    for (Event& e : x.events)
        if (!e) e = make_event(hipEventDefault);
    const bool timed = x.events[0] && x.events[1] && x.events[2] && x.events[3];
    const bool was_ready = ready, awaited_rebuild = awaits_rebuild;
    begin_write();
    // 1. the rows, then the rectangles in list order
    HIP_TRY(hipMemcpyAsync(x.staging.ptr, packed.data(), staging_bytes, hipMemcpyHostToDevice, st));
    const auto t1 = std::chrono::steady_clock::now();
    if (timed) HIP_TRY(hipEventRecord(x.events[0], st));
    for (const TexelRectangle& rectangle : rectangles) {
        const uint64_t chunks = (rectangle.row_bytes + 3u) / 4u;
        hipLaunchKernelGGL(k_write_texel_rectangle, dim3(uint32_t((chunks + TEXEL_UPDATE_BLOCK - 1) / TEXEL_UPDATE_BLOCK), std::min(rectangle.height, 65535u)), dim3(TEXEL_UPDATE_BLOCK), 0, st, rectangle,
                           x.staging.as<uint8_t>(), texels.as<uint8_t>());
    }
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(x.events[1], st));
    uint32_t words[3] = {all_triangles_opaque ? 1u : 0u, 0u, 0u};      // what stays when no flag follows the edit
    if (decides_flags) {
        // 2. the flags of the touched instances' triangles; 3. the leaf records (queued whatever pass 2 finds: it writes only where a record's bits differ)
        HIP_TRY(hipMemcpyAsync(x.touched.ptr, touched.data(), touched.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(x.words.ptr, 0, TEXEL_SCRATCH_WORDS * sizeof(uint32_t), st));
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(x.words.ptr), 1, 1, st));
        const MaterialUpdateArrays a = {triangles.as<HiprTriangle>(), args.triangle_count, instances.as<HiprInstance>(), materials.as<HiprMaterial>(), indices.as<uint32_t>(),
                                        reinterpret_cast<const float*>(args.texcoords), textures.as<HiprTexture>(), uint32_t(uploaded_textures.size()), texels.as<uint8_t>(),
                                        x.touched.as<uint32_t>(), trace_triangles.as<uint32_t>(), shade_triangles.as<uint32_t>(), triangle_class.as<uint8_t>()};
        hipLaunchKernelGGL(k_reflag_touched_triangles, dim3((args.triangle_count + TEXEL_UPDATE_BLOCK - 1) / TEXEL_UPDATE_BLOCK), dim3(TEXEL_UPDATE_BLOCK), 0, st, a, x.words.as<uint32_t>());
        if (timed) HIP_TRY(hipEventRecord(x.events[2], st));
        if (wide8.slot_count && refit_leaf_count)
            hipLaunchKernelGGL(k_update_leaf_flags, dim3((refit_leaf_count + MATERIAL_UPDATE_BLOCK - 1) / MATERIAL_UPDATE_BLOCK), dim3(MATERIAL_UPDATE_BLOCK), 0, st, wide8_slots.as<HiprSlot8>(),
                               refit_leaf_slots.as<uint32_t>(), refit_leaf_count, triangles.as<HiprTriangle>());
        HIP_TRY(hipGetLastError());
        if (timed) HIP_TRY(hipEventRecord(x.events[3], st));
        HIP_TRY(hipMemcpyAsync(words, x.words.ptr, sizeof(words), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));      // `packed` and `touched` are read by now as well
    float write_ms = 0.0f, flag_ms = 0.0f, leaf_ms = 0.0f;
    if (timed) {
        HIP_TRY(hipEventElapsedTime(&write_ms, x.events[0], x.events[1]));
        if (decides_flags) { HIP_TRY(hipEventElapsedTime(&flag_ms, x.events[1], x.events[2])); HIP_TRY(hipEventElapsedTime(&leaf_ms, x.events[2], x.events[3])); }
    }
    x.staging_ms = ms(t0, t1); x.write_ms = write_ms; x.coverage_ms = flag_ms; x.leaf_ms = leaf_ms;
    all_triangles_opaque = words[TEXEL_WORD_OPAQUE] != 0;
    derive_switches_from_pools();
    *out = {words[TEXEL_WORD_DECIDED], words[TEXEL_WORD_CHANGED], all_triangles_opaque ? 1u : 0u, environment_stale ? 1u : 0u};
    ready = was_ready;
    awaits_rebuild = awaited_rebuild;
    return HIPR_OK;
}

// The device work of hipr_update_scene_vertices (vertex_update.h). The scratch is allocated BEFORE the scene is touched: a failed allocation leaves the scene as
// found. Then, as the other writers: not ready, ONE staging copy (the segment table, a word per instance, the rows), the passes on the stream, the host copies. What
// follows the pool writes depends on what the edits carry: geometry -- the moved triangles with the bounds, the refit of the tree and the records, and the state
// refit_transforms leaves (tree_stale; awaits_rebuild when a pair parted; the per-pixel trace hints stay, a refit keeps the kinds of the slots); texcoords or tints --
// the records; texcoords, when a resident instance's material leaves its triangles' flags to its coverage texture (the host copies answer that) -- the flag pass and
// the leaf pass. Two synchronises, the refit's: for the bounds, and at the end.
int ResidentScene::update_vertices(const HiprVertexEdit* edits, uint32_t edit_count, VertexScratch& x, hipStream_t st, HiprVertexUpdateResult* out) {
    const auto t0 = std::chrono::steady_clock::now();
    VertexPlan plan;
    plan_vertex_edits(edits, edit_count, plan);
    std::vector<uint32_t> decides(std::max<size_t>(uploaded_instances.size(), 1), 0u);
    bool decides_flags = false;
    if (plan.carries[VERTEX_POOL_TEXCOORDS])
        for (size_t i = 0; i < uploaded_instances.size(); ++i)
            if ((uploaded_instances[i].mesh_flags & HIPR_MESH_TEXCOORDS) &&
                deciding_coverage_texture(uploaded_materials[size_t(uploaded_instances[i].material_index)], uploaded_textures.data(), uint32_t(uploaded_textures.size()))) { decides[i] = 1u; decides_flags = true; }
    const bool moves = plan.carries[VERTEX_POOL_GEOMETRY];
    const bool records = moves || plan.carries[VERTEX_POOL_TEXCOORDS] || plan.carries[VERTEX_POOL_TINTS];
    // the staging buffer: the table, the instance words, the rows -- each part a multiple of 16 bytes
    const size_t table_bytes = plan.table.size() * sizeof(VertexSegment), decides_bytes = (decides.size() * sizeof(uint32_t) + 15u) & ~size_t(15);
    const size_t staging_bytes = table_bytes + decides_bytes + size_t(plan.word_count) * 4u;
    std::vector<uint8_t> packed(staging_bytes, uint8_t(0));
    std::memcpy(packed.data(), plan.table.data(), table_bytes);
    std::memcpy(packed.data() + table_bytes, decides.data(), decides.size() * sizeof(uint32_t));
    pack_vertex_rows(plan, packed.data() + table_bytes + decides_bytes);
    int r = x.staging.resize(staging_bytes);
    r |= x.words.resize(VERTEX_SCRATCH_WORDS * sizeof(uint32_t));
    if (moves) r |= x.marks_geometry.resize(std::max<size_t>(uploaded_vertex_count, 1));
    if (decides_flags) r |= x.marks_texcoords.resize(std::max<size_t>(uploaded_vertex_count, 1));
    if (r) {
        (void)hipGetLastError();      // the failed allocation's error is answered here: it must not meet the next call's check
        return HIPR_ERROR_OUT_OF_MEMORY;
    }
    for (Event& e : x.events)
        if (!e) e = make_event(hipEventDefault);
    const bool timed = x.events[0] && x.events[1] && x.events[2] && x.events[3];
    begin_write();
    // 1. the staging copy, then the words and the marks
    HIP_TRY(hipMemcpyAsync(x.staging.ptr, packed.data(), staging_bytes, hipMemcpyHostToDevice, st));
    const auto t1 = std::chrono::steady_clock::now();
    if (timed) HIP_TRY(hipEventRecord(x.events[0], st));
    if (moves) HIP_TRY(hipMemsetAsync(x.marks_geometry.ptr, 0, uploaded_vertex_count, st));
    if (decides_flags) HIP_TRY(hipMemsetAsync(x.marks_texcoords.ptr, 0, uploaded_vertex_count, st));
    HIP_TRY(hipMemsetAsync(x.words.ptr, 0, VERTEX_SCRATCH_WORDS * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(x.words.ptr), 1, 1, st));
    const VertexPools pools = {{geometry.as<uint32_t>(), texcoords.as<uint32_t>(), tints.as<uint32_t>(), emissions.as<uint32_t>()},
                               {moves ? x.marks_geometry.as<uint8_t>() : nullptr, decides_flags ? x.marks_texcoords.as<uint8_t>() : nullptr}};
    hipLaunchKernelGGL(k_write_vertex_words, dim3(uint32_t((plan.word_count + VERTEX_UPDATE_BLOCK - 1) / VERTEX_UPDATE_BLOCK)), dim3(VERTEX_UPDATE_BLOCK), 0, st,
                       reinterpret_cast<const VertexSegment*>(x.staging.as<uint8_t>()), uint32_t(plan.table.size()), reinterpret_cast<const uint32_t*>(x.staging.as<uint8_t>() + table_bytes + decides_bytes),
                       plan.word_count, pools);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(x.events[1], st));
    float grid_min[3] = {wide8.grid_min[0], wide8.grid_min[1], wide8.grid_min[2]}, grid_cell[3] = {wide8.grid_cell[0], wide8.grid_cell[1], wide8.grid_cell[2]};
    // 2. the moved triangles and the scene's bounds, then the tree (wide8_refit.h); `packed` is read once that has synchronised
    if (moves)
        if (int status = queue_refit_of_marked(x.marks_geometry.as<uint8_t>(), x.words.as<uint32_t>(), grid_min, grid_cell, st)) return status;
    if (records) queue_triangle_records(st);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(x.events[2], st));
    if (decides_flags) {
        // 3. the flags of the triangles that read a marked texture coordinate, then the leaf records (queued whatever the pass finds: it writes only where bits differ)
        const MaterialUpdateArrays a = {triangles.as<HiprTriangle>(), args.triangle_count, instances.as<HiprInstance>(), materials.as<HiprMaterial>(), indices.as<uint32_t>(),
                                        reinterpret_cast<const float*>(args.texcoords), textures.as<HiprTexture>(), uint32_t(uploaded_textures.size()), texels.as<uint8_t>(),
                                        reinterpret_cast<const uint32_t*>(x.staging.as<uint8_t>() + table_bytes), trace_triangles.as<uint32_t>(), shade_triangles.as<uint32_t>(), triangle_class.as<uint8_t>()};
        hipLaunchKernelGGL(k_reflag_marked_triangles, dim3((args.triangle_count + VERTEX_UPDATE_BLOCK - 1) / VERTEX_UPDATE_BLOCK), dim3(VERTEX_UPDATE_BLOCK), 0, st, a, x.marks_texcoords.as<uint8_t>(),
                           x.words.as<uint32_t>());
        if (wide8.slot_count && refit_leaf_count)
            hipLaunchKernelGGL(k_update_leaf_flags, dim3((refit_leaf_count + MATERIAL_UPDATE_BLOCK - 1) / MATERIAL_UPDATE_BLOCK), dim3(MATERIAL_UPDATE_BLOCK), 0, st, wide8_slots.as<HiprSlot8>(),
                               refit_leaf_slots.as<uint32_t>(), refit_leaf_count, triangles.as<HiprTriangle>());
        HIP_TRY(hipGetLastError());
    }
    if (timed) HIP_TRY(hipEventRecord(x.events[3], st));
    // 4. the read-backs, the books and the answer
    if (int status = finish_vertex_writes(moves, decides_flags, x.words.as<uint32_t>(), grid_min, grid_cell, st, out)) return status;
    float write_ms = 0.0f, refit_ms = 0.0f, flag_ms = 0.0f;
    if (timed) {
        HIP_TRY(hipEventElapsedTime(&write_ms, x.events[0], x.events[1]));
        HIP_TRY(hipEventElapsedTime(&refit_ms, x.events[1], x.events[2]));
        HIP_TRY(hipEventElapsedTime(&flag_ms, x.events[2], x.events[3]));
    }
    x.staging_ms = ms(t0, t1); x.write_ms = write_ms; x.refit_ms = refit_ms; x.flag_ms = flag_ms;
    return HIPR_OK;
}

// What update_vertices and pose_rigs share after their writes into the geometry pool (vertex_update.h pass 2, then the refit of the tree): the triangles that read a
// marked vertex get their corners again and are counted in words[VERTEX_WORD_MOVED], every triangle feeds the bounds, ONE synchronise brings the bounds to the
// host for the grid, and the tree's refit is queued.
int ResidentScene::queue_refit_of_marked(const uint8_t* marks, uint32_t* words, float* grid_min, float* grid_cell, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(refit_scratch.ptr, 0, REFIT_SCRATCH_BYTES, st));
    const uint32_t blocks = (args.triangle_count + REFIT_BLOCK - 1) / REFIT_BLOCK;
    hipLaunchKernelGGL(k_refit_marked_triangles, dim3(blocks), dim3(REFIT_BLOCK), 0, st, triangles.as<HiprTriangle>(), args.triangle_count, instances.as<HiprInstance>(), marks,
                       indices.as<uint32_t>(), geometry.as<HiprVertexGeometry>(), refit_partial.as<RefitBound>(), words);
    hipLaunchKernelGGL(k_refit_bounds_final, dim3(1), dim3(REFIT_BLOCK), 0, st, refit_partial.as<RefitBound>(), blocks, refit_scratch.as<RefitBound>());
    HIP_TRY(hipGetLastError());
    RefitBound bounds[6];
    HIP_TRY(hipMemcpyAsync(bounds, refit_scratch.ptr, sizeof(bounds), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));      // the caller's staging copy is read by now as well
    const float lo[3] = {bounds[0].v, bounds[1].v, bounds[2].v}, hi[3] = {bounds[3].v, bounds[4].v, bounds[5].v};
    refit_grid(lo, hi, grid_min, grid_cell);
    queue_refit_tree<true>(grid_min, grid_cell, st);
    return HIPR_OK;
}

// The end of both calls, everything queued: the refit's flag and area and the passes' four words read back, then the books, the state refit_transforms leaves
// (tree_stale; awaits_rebuild when a pair parted) and the answer. decides_flags: the flag pass ran, its words count.
int ResidentScene::finish_vertex_writes(bool moves, bool decides_flags, const uint32_t* device_words, const float* grid_min, const float* grid_cell, hipStream_t st, HiprVertexUpdateResult* out) {
    struct { uint32_t flag; uint32_t pad[3]; double area; } tail = {};
    uint32_t words[4] = {all_triangles_opaque ? 1u : 0u, 0u, 0u, 0u};
    if (moves) HIP_TRY(hipMemcpyAsync(&tail, refit_scratch.as<char>() + REFIT_SCRATCH_FLAG, sizeof(tail), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(words, device_words, sizeof(words), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (decides_flags) {
        all_triangles_opaque = words[VERTEX_WORD_OPAQUE] != 0;
        derive_switches_from_pools();
    }
    int needs_rebuild = 0;
    if (moves) {
        tree_stale = true;
        for (int a = 0; a < 3; ++a) { wide8.grid_min[a] = grid_min[a]; wide8.grid_cell[a] = grid_cell[a]; }
        current_half_area = tail.area;
        needs_rebuild = tail.flag ? 1 : 0;      // a pair parted: this tree cannot hold the scene any more
    }
    out->refit.needs_rebuild = needs_rebuild;
    out->refit.child_half_area = current_half_area;
    out->refit.uploaded_half_area = uploaded_half_area;
    for (int a = 0; a < 3; ++a) { out->refit.grid_min[a] = wide8.grid_min[a]; out->refit.grid_cell[a] = wide8.grid_cell[a]; }
    out->moved_triangles = words[VERTEX_WORD_MOVED];
    out->candidate_triangles = decides_flags ? words[VERTEX_WORD_DECIDED] : 0u;
    out->changed_triangles = decides_flags ? words[VERTEX_WORD_CHANGED] : 0u;
    out->all_triangles_opaque = all_triangles_opaque ? 1u : 0u;
    ready = !needs_rebuild;
    awaits_rebuild = !ready;
    return HIPR_OK;
}

static_assert(POSE_LDS_JOINTS == 32u, "ResidentScene::pose_lds_joints starts at the budget that ships (context.h)");
static_assert(sizeof(ResidentScene::Rig) == sizeof(RigBook) && offsetof(ResidentScene::Rig, first_vertex) == offsetof(RigBook, first_vertex) &&
              offsetof(ResidentScene::Rig, vertex_count) == offsetof(RigBook, vertex_count) && offsetof(ResidentScene::Rig, joint_count) == offsetof(RigBook, joint_count) &&
              offsetof(ResidentScene::Rig, target_count) == offsetof(RigBook, target_count) && offsetof(ResidentScene::Rig, flags) == offsetof(RigBook, flags),
              "ResidentScene::Rig is RigBook member for member: check_rig_poses and plan_rig_poses read either");

// The device work of hipr_set_scene_rigs (vertex_pose.h): the rigs packed in the resident layout, the new buffers allocated and filled, and only then the old
// ones let go and the book replaced -- a failed allocation leaves the old set bound. The scene's state is not touched: no pool, triangle or tree changes.
int ResidentScene::set_rigs(const HiprRigDesc* descs, uint32_t count, hipStream_t st) {
    std::vector<uint32_t> words;
    std::vector<PoseRig> records(count);
    std::vector<Rig> book(count);
    for (uint32_t k = 0; k < count; ++k) {
        RigBook b;
        pack_rig(descs[k], words, records[k], b);
        book[k] = {b.first_vertex, b.vertex_count, b.joint_count, b.target_count, b.flags};
    }
    DeviceBuffer new_records, new_data;
    if (count) {
        int r = new_records.resize(records.size() * sizeof(PoseRig));
        r |= new_data.resize(std::max<size_t>(words.size(), 4) * sizeof(uint32_t));
        if (r) {
            (void)hipGetLastError();
            return HIPR_ERROR_OUT_OF_MEMORY;
        }
        HIP_TRY(hipMemcpyAsync(new_records.ptr, records.data(), records.size() * sizeof(PoseRig), hipMemcpyHostToDevice, st));
        if (!words.empty()) HIP_TRY(hipMemcpyAsync(new_data.ptr, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));      // `records` and `words` are read
    }
    rig_records = std::move(new_records);      // the old buffers go with the temporaries
    rig_data = std::move(new_data);
    rigs = std::move(book);
    return HIPR_OK;
}

// The device work of hipr_pose_scene_rigs (vertex_pose.h). The scratch is allocated BEFORE the scene is touched. Then, as the other writers: not ready, ONE staging
// copy (the block table, the calls, all matrices and target weights), ONE launch of k_pose_vertices, and what update_vertices runs after an edit of geometry:
// queue_refit_of_marked, the records, finish_vertex_writes. A pose carries no texture coordinates: the flag and leaf passes are not queued.
int ResidentScene::pose_rigs(const HiprRigPose* poses, uint32_t pose_count, PoseScratch& x, VertexScratch& v, hipStream_t st, HiprVertexUpdateResult* out) {
    const auto t0 = std::chrono::steady_clock::now();
    PosePlan plan;
    plan_rig_poses(poses, pose_count, rigs.data(), plan);
    int r = x.staging.resize(plan.staging.size());
    r |= v.words.resize(VERTEX_SCRATCH_WORDS * sizeof(uint32_t));
    r |= v.marks_geometry.resize(std::max<size_t>(uploaded_vertex_count, 1));
    if (r) {
        (void)hipGetLastError();      // the failed allocation's error is answered here: it must not meet the next call's check
        return HIPR_ERROR_OUT_OF_MEMORY;
    }
    for (Event& e : x.events)
        if (!e) e = make_event(hipEventDefault);
    const bool timed = x.events[0] && x.events[1] && x.events[2];
    begin_write();
    HIP_TRY(hipMemcpyAsync(x.staging.ptr, plan.staging.data(), plan.staging.size(), hipMemcpyHostToDevice, st));
    const auto t1 = std::chrono::steady_clock::now();
    if (timed) HIP_TRY(hipEventRecord(x.events[0], st));
    HIP_TRY(hipMemsetAsync(v.marks_geometry.ptr, 0, uploaded_vertex_count, st));
    HIP_TRY(hipMemsetAsync(v.words.ptr, 0, VERTEX_SCRATCH_WORDS * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(v.words.ptr), 1, 1, st));
    const uint8_t* staging = x.staging.as<uint8_t>();
    hipLaunchKernelGGL(k_pose_vertices, dim3(plan.block_count), dim3(POSE_BLOCK), 0, st, reinterpret_cast<const PoseBlock*>(staging), reinterpret_cast<const PoseCall*>(staging + plan.calls_at),
                       reinterpret_cast<const float*>(staging + plan.floats_at), rig_records.as<PoseRig>(), rig_data.as<uint32_t>(), std::min(pose_lds_joints, POSE_LDS_CAPACITY),
                       geometry.as<HiprVertexGeometry>(), v.marks_geometry.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(x.events[1], st));
    float grid_min[3] = {wide8.grid_min[0], wide8.grid_min[1], wide8.grid_min[2]}, grid_cell[3] = {wide8.grid_cell[0], wide8.grid_cell[1], wide8.grid_cell[2]};
    if (int status = queue_refit_of_marked(v.marks_geometry.as<uint8_t>(), v.words.as<uint32_t>(), grid_min, grid_cell, st)) return status;      // plan.staging is read by now
    queue_triangle_records(st);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(x.events[2], st));
    if (int status = finish_vertex_writes(true, false, v.words.as<uint32_t>(), grid_min, grid_cell, st, out)) return status;
    float pose_ms = 0.0f, refit_ms = 0.0f;
    if (timed) {
        HIP_TRY(hipEventElapsedTime(&pose_ms, x.events[0], x.events[1]));
        HIP_TRY(hipEventElapsedTime(&refit_ms, x.events[1], x.events[2]));
    }
    x.staging_ms = ms(t0, t1); x.pose_ms = pose_ms; x.refit_ms = refit_ms;
    return HIPR_OK;
}

// The last step of hipr_rebuild_scene_trees, which has refused everything it refuses: the new resident arrays, and what an upload derives from them. The pools, the
// instances and the lights stay; all_triangles_opaque, any_coated_triangle and the other switches cannot change under a permutation of the triangles and stay. The
// 4-wide array is not rebuilt: tree_stale stays set until the next upload or geometry update, as after the refit.
// After hipr_edit_scene_instances (`built.new_set`) the set of triangles and the instance list are other ones: every per-triangle and per-instance array takes the new
// size, the instance array and its host copy become the new list, and the switches that follow the triangles and the instances are the ones reduced over the new set.
// The pools stay, and with them the switches derived from them.
int ResidentScene::install_rebuilt_trees(const RebuiltTrees& built, hipStream_t st) {
    begin_write();
    if (const RebuiltTrees::NewSet* set = built.new_set) {
        const size_t t = set->triangle_count, i = set->instances->size();
        int r = 0;
        r |= triangles.resize(t * sizeof(HiprTriangle));
        r |= triangle_class.resize(t);
        r |= shade_triangles.resize(t * SHADE_TRIANGLE_QUADS * sizeof(float4));
        r |= trace_triangles.resize(t * 3 * sizeof(float4));
        r |= instances.resize(i * sizeof(HiprInstance));
        if (r) return r < 0 ? r : HIPR_ERROR_HIP;
        HIP_TRY(hipMemcpyAsync(instances.ptr, set->device_instances, i * sizeof(HiprInstance), hipMemcpyDeviceToDevice, st));
        args.triangles = triangles.as<float4>();
        args.triangle_count = set->triangle_count;
        args.shade_triangles = shade_triangles.as<float4>();
        args.trace_triangles = trace_triangles.as<float4>();
        args.instances = instances.as<HiprInstance>();
        uploaded_instances = *set->instances;
        shading_models = shading_model_mask(uploaded_instances.data(), uint32_t(uploaded_instances.size()), uploaded_materials.data());
        all_triangles_opaque = set->all_triangles_opaque;
        any_coated_triangle = set->any_coated_triangle;
    }
    const uint32_t triangle_count = args.triangle_count;
    hipLaunchKernelGGL(k_rebuild_gather, dim3((triangle_count + REBUILD_BLOCK - 1) / REBUILD_BLOCK), dim3(REBUILD_BLOCK), 0, st, built.flat, built.flat_class, built.order,
                       triangles.as<HiprTriangle>(), triangle_class.as<uint8_t>(), triangle_count);
    HIP_TRY(hipGetLastError());
    if (int r = nodes.resize(size_t(built.node_count) * sizeof(HiprBvhNode))) return r;
    if (int r = wide8_slots.resize(size_t(built.wide8.slot_count) * sizeof(HiprSlot8))) return r;
    HIP_TRY(hipMemcpyAsync(nodes.ptr, built.nodes, size_t(built.node_count) * sizeof(HiprBvhNode), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(wide8_slots.ptr, built.slots, size_t(built.wide8.slot_count) * sizeof(HiprSlot8), hipMemcpyDeviceToDevice, st));
    args.nodes = nodes.as<float4>();
    args.node_count = built.node_count;
    wide8.slots = wide8_slots.as<uint4>();
    wide8.slot_count = built.wide8.slot_count;
    for (int a = 0; a < 3; ++a) { wide8.grid_min[a] = built.wide8.grid_min[a]; wide8.grid_cell[a] = built.wide8.grid_cell[a]; }
    wide8_height = built.wide8.height;
    new_wide8_tree();
    const uint32_t bvh_max_depth = built.deepest + 1u;      // BvhBuildResult::max_depth
    stack_size = bvh_max_depth <= 16 ? 16 : (bvh_max_depth <= 32 ? 32 : 64);
    queue_triangle_records(st);
    HIP_TRY(hipGetLastError());
    HiprSceneDesc lists = {};      // what prepare_refit reads of a description
    lists.wide8_slots = built.host_slots; lists.wide8_slot_count = built.wide8.slot_count;
    lists.triangle_count = triangle_count; lists.instance_count = uint32_t(uploaded_instances.size());
    if (int r = prepare_refit(&lists, true, st)) return r;      // the slot lists by kind and level with their host copies, and uploaded_half_area by the kernels that take it at upload
    tree_stale = true;
    wide4_awaits_geometry = true;
    ready = true;
    return HIPR_OK;
}

} // namespace hipr

// ---- the tree builds on the device ------------------------------------------------------------------------------------------------------------------------
namespace {

// What the device work of a BVH2 build leaves beside the context's BuildScratch (out_nodes, order, place, status): the nodes, and the nodes created per level.
struct Bvh2Built { uint32_t node_count = 1; std::vector<uint32_t> level_nodes; };
// The device-to-device core hipr_build_bvh2 and hipr_rebuild_scene_trees share: scratch, kernels and the words read per level, on the context's stream, ending
// synchronised. `host_triangles` are uploaded into the scratch first (`uploaded` is the time after that); otherwise the build runs over `device_triangles` where they
// lie. `who` names the entry point in the messages. The caller holds the ScratchGuard of the build scratch and has checked count and corners.
static int build_bvh2_on_the_device(HiprContext* c, const char* who, const HiprTriangle* host_triangles, const HiprTriangle* device_triangles, uint32_t count, uint32_t depth_limit, Bvh2Built& built,
                                    std::chrono::steady_clock::time_point& uploaded) {
    const uint32_t max_levels = std::min(depth_limit, count) + 2u;      // a range's depth grows by one per level and never passes the limit
    const size_t n = count, max_open = n / 4 + 2, max_long = n / BUILD_SHORT_RANGE + 2, blocks = (n + BUILD_BLOCK - 1) / BUILD_BLOCK;
    const size_t status_words = STATUS_LEVELS + 2 * size_t(max_levels + 2);
    BuildScratch& b = c->build;
    hipStream_t stream = c->stream;
    if (b.boxes.resize(n * sizeof(BuildBox)) | b.centroids.resize(n * 12) | b.order.resize(n * 4) | b.seg.resize(n * 4) | b.order_tmp.resize(n * 4) | b.seg_tmp.resize(n * 4) |
        b.ranges[0].resize(max_open * sizeof(BuildRange)) | b.ranges[1].resize(max_open * sizeof(BuildRange)) | b.acc.resize(max_long * ACC_WORDS * 4) | b.setup.resize(max_long * sizeof(BuildSetup)) |
        b.split.resize(max_long * sizeof(BuildSplit)) | b.scan_local.resize(n * 4) | b.block_sums.resize(blocks * 4) | b.nodes.resize(n * sizeof(HiprBvhNode)) | b.sizes.resize(n * 4) |
        b.place.resize(n * 4) | b.out_nodes.resize(n * sizeof(HiprBvhNode)) | b.status.resize(status_words * 4))
        return HIPR_ERROR_OUT_OF_MEMORY;
    if (host_triangles) {
        if (int st = b.triangles.upload(host_triangles, n * sizeof(HiprTriangle), stream)) return st;
        HIP_TRY(hipStreamSynchronize(stream));
    }
    uploaded = std::chrono::steady_clock::now();

    BuildState S = {};
    S.triangles = host_triangles ? b.triangles.as<HiprTriangle>() : device_triangles; S.count = count; S.depth_limit = depth_limit;
    S.boxes = b.boxes.as<BuildBox>(); S.centroids = b.centroids.as<float>();
    S.order = b.order.as<uint32_t>(); S.seg = b.seg.as<uint32_t>(); S.order_tmp = b.order_tmp.as<uint32_t>(); S.seg_tmp = b.seg_tmp.as<uint32_t>();
    S.acc = b.acc.as<uint32_t>(); S.setup = b.setup.as<BuildSetup>(); S.split = b.split.as<BuildSplit>();
    S.scan_local = b.scan_local.as<uint32_t>(); S.block_sums = b.block_sums.as<uint32_t>();
    S.nodes = b.nodes.as<HiprBvhNode>(); S.sizes = b.sizes.as<uint32_t>(); S.place = b.place.as<uint32_t>(); S.out_nodes = b.out_nodes.as<HiprBvhNode>();
    S.status = b.status.as<uint32_t>();

    std::vector<uint32_t> status(status_words, 0u);
    status[STATUS_DECLINE] = status[STATUS_DECLINE + 1] = 0xFFFFFFFFu;
    status[STATUS_LEVELS] = 1u;
    status[STATUS_LEVELS + 1] = count > BUILD_SHORT_RANGE ? 1u : 0u;
    HIP_TRY(hipMemcpyAsync(S.status, status.data(), status_words * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(S.nodes, 0, n * sizeof(HiprBvhNode), stream));
    HIP_TRY(hipMemsetAsync(S.place, 0, 4, stream));
    const dim3 block(BUILD_BLOCK), per_position{uint32_t(blocks)};
    hipLaunchKernelGGL(k_build_prepare, per_position, block, 0, stream, S);
    std::vector<uint32_t>& level_nodes = built.level_nodes;      // the open ranges = new nodes of every level
    level_nodes.clear();
    uint32_t node_count = 1;
    if (count <= BUILD_LEAF_MAX) hipLaunchKernelGGL(k_build_single_leaf, dim3(1), block, 0, stream, S);
    else {
        const BuildRange root = {0u, count, 1u, BUILD_NONE, count > BUILD_SHORT_RANGE ? 0u : BUILD_NONE, 0u};
        HIP_TRY(hipMemcpyAsync(b.ranges[0].ptr, &root, sizeof(root), hipMemcpyHostToDevice, stream));
        uint32_t open = 1, long_ranges = root.long_index == BUILD_NONE ? 0u : 1u, node_base = 0;
        for (uint32_t level = 0; open; ++level) {
            if (level >= max_levels || node_base + open > count - 1u || open > max_open - 2 || long_ranges > max_long - 2)
                return fail(HIPR_ERROR_HIP, "%s: the build left its bounds at level %u (%u open ranges, %u nodes)", who, level, open, node_base);
            const BuildLevel L = {b.ranges[level & 1u].as<BuildRange>(), b.ranges[(level + 1u) & 1u].as<BuildRange>(), open, node_base, level};
            const dim3 per_range((open + BUILD_BLOCK - 1) / BUILD_BLOCK);
            if (long_ranges) {
                const uint64_t words = uint64_t(long_ranges) * ACC_WORDS;
                hipLaunchKernelGGL(k_build_acc_init, dim3(uint32_t((words + BUILD_BLOCK - 1) / BUILD_BLOCK)), block, 0, stream, S.acc, words);
                hipLaunchKernelGGL(k_build_bounds, per_position, block, 0, stream, S, L);
                hipLaunchKernelGGL(k_build_range_setup, per_range, block, 0, stream, S, L);
                hipLaunchKernelGGL(k_build_bins, per_position, block, 0, stream, S, L);
                hipLaunchKernelGGL(k_build_split, per_range, block, 0, stream, S, L, 1);
                hipLaunchKernelGGL(k_build_scan_local, per_position, block, 0, stream, S, L);
                hipLaunchKernelGGL(k_build_scan_sums, dim3(1), block, 0, stream, S.block_sums, uint32_t(blocks));
                hipLaunchKernelGGL(k_build_scatter, per_position, block, 0, stream, S, L);
                hipLaunchKernelGGL(k_build_copy_back, per_position, block, 0, stream, S, L);
                hipLaunchKernelGGL(k_build_leaves, per_range, block, 0, stream, S, L);
            }
            hipLaunchKernelGGL(k_build_split, per_range, block, 0, stream, S, L, 0);
            HIP_TRY(hipMemcpyAsync(status.data(), S.status, (STATUS_LEVELS + 2 * size_t(level + 2)) * 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (status[STATUS_DECLINE] != 0xFFFFFFFFu) {
                b.levels = level + 1;
                return fail(HIPR_ERROR_UNSUPPORTED, "%s: the range [%u, %u) of %u triangles at level %u takes the median path (the depth budget, or coincident centroids) and is longer than the %u a lane sorts; build on the host",
                            who, status[STATUS_DECLINE + 1], status[STATUS_DECLINE], status[STATUS_DECLINE] - status[STATUS_DECLINE + 1], level, BUILD_MEDIAN_LANE_LIMIT);
            }
            level_nodes.push_back(open);
            node_base += open;
            open = status[STATUS_LEVELS + 2 * (level + 1)];
            long_ranges = status[STATUS_LEVELS + 2 * (level + 1) + 1];
        }
        node_count = node_base;
        std::vector<uint32_t> first(level_nodes.size());
        for (size_t l = 0, at = 0; l < level_nodes.size(); at += level_nodes[l++]) first[l] = uint32_t(at);
        for (size_t l = level_nodes.size(); l-- > 0;) hipLaunchKernelGGL(k_build_count, dim3((level_nodes[l] + BUILD_BLOCK - 1) / BUILD_BLOCK), block, 0, stream, S, first[l], level_nodes[l]);
        for (size_t l = 0; l < level_nodes.size(); ++l) hipLaunchKernelGGL(k_build_place, dim3((level_nodes[l] + BUILD_BLOCK - 1) / BUILD_BLOCK), block, 0, stream, S, first[l], level_nodes[l]);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    built.node_count = node_count;
    b.levels = uint32_t(level_nodes.size());
    return HIPR_OK;
}

// The device-to-device core hipr_build_wide8 and hipr_rebuild_scene_trees share: the passes of wide8_build.h over a BVH2, its triangles, their order and the level lists
// the device already holds (W8State's input members, the scratch of collapse_scratch_for cleared), on the context's stream, ending synchronised with the slots in
// CollapseScratch::slots. `level_first`: level l is level_nodes[level_first[l] .. level_first[l + 1]). `who` names the entry point in the messages. The caller holds
// the ScratchGuard of the collapse scratch.
static int collapse_on_the_device(HiprContext* c, const char* who, W8State& S, const std::vector<uint32_t>& level_first, uint32_t slot_capacity, HiprWide8BuildResult& result) {
    CollapseScratch& b = c->collapse;
    hipStream_t stream = c->stream;
    const uint32_t triangle_count = S.triangle_count, node_count = S.node_count, reachable = S.reachable, bvh_levels = uint32_t(level_first.size()) - 1u;
    const size_t T = triangle_count, N = node_count, scan_blocks = (T + W8_BLOCK - 1) / W8_BLOCK;
    const dim3 block(W8_BLOCK), per_triangle{uint32_t(scan_blocks)}, per_reference((2u * reachable + W8_BLOCK - 1) / W8_BLOCK);
    auto blocks_for = [](uint32_t threads) { return dim3((threads + W8_BLOCK - 1) / W8_BLOCK); };
    // 1, 2: the bounds and the record numbers; the host reads both together
    hipLaunchKernelGGL(k_w8_bounds, per_triangle, block, 0, stream, S.triangles, triangle_count, b.partial.as<RefitBound>(), S.status);
    hipLaunchKernelGGL(k_refit_bounds_final, dim3(1), block, 0, stream, b.partial.as<RefitBound>(), uint32_t(scan_blocks), b.bounds.as<RefitBound>());
    hipLaunchKernelGGL(k_w8_count_leaf, per_reference, block, 0, stream, S);
    hipLaunchKernelGGL(k_w8_scan_local, per_triangle, block, 0, stream, S);
    hipLaunchKernelGGL(k_build_scan_sums, dim3(1), block, 0, stream, S.block_sums, uint32_t(scan_blocks + 1));
    RefitBound bounds[6];
    uint32_t record_total = 0, not_finite = 0;
    HIP_TRY(hipMemcpyAsync(bounds, b.bounds.ptr, sizeof(bounds), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&record_total, S.block_sums + scan_blocks, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&not_finite, S.status + W8_STATUS_NOT_FINITE, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (not_finite) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: a triangle corner or a child box is not finite", who);
    if (record_total == 0 || record_total > triangle_count) return fail(HIPR_ERROR_HIP, "%s: %u records of %u triangles", who, record_total, triangle_count);
    result = {};
    {
        const float lo[3] = {bounds[0].v, bounds[1].v, bounds[2].v}, hi[3] = {bounds[3].v, bounds[4].v, bounds[5].v};
        refit_grid(lo, hi, result.grid_min, result.grid_cell);
        for (int a = 0; a < 3; ++a) { S.grid_min[a] = result.grid_min[a]; S.grid_cell[a] = result.grid_cell[a]; }
    }
    // 3, 4: the tree over the records and its dynamic program
    const size_t R = record_total, inner = N + R, wide_capacity = R;
    if (b.box.resize((inner + R) * sizeof(RefitBox)) | b.left.resize(inner * 4) | b.right.resize(inner * 4) | b.cost.resize(inner * 28) | b.split.resize(inner * 7) | b.roots_used.resize(inner * 7) |
        b.records.resize(R * sizeof(HiprLeaf8)) | b.record_slot.resize(R * 4) | b.wide_tree.resize(wide_capacity * 4) | b.wide_child.resize(wide_capacity * 32) | b.wide_all.resize(wide_capacity * sizeof(RefitBox)) |
        b.wide_size.resize(wide_capacity * 4) | b.wide_base.resize(wide_capacity * 4) | b.wide_slot.resize(wide_capacity * 4))
        return HIPR_ERROR_OUT_OF_MEMORY;
    S.record_total = record_total; S.leaf_base = uint32_t(inner); S.wide_capacity = uint32_t(wide_capacity);
    S.box = b.box.as<RefitBox>(); S.left = b.left.as<int32_t>(); S.right = b.right.as<int32_t>(); S.cost = b.cost.as<float>(); S.split = b.split.as<uint8_t>(); S.roots_used = b.roots_used.as<uint8_t>();
    S.records = b.records.as<HiprLeaf8>(); S.record_slot = b.record_slot.as<uint32_t>();
    S.wide_tree = b.wide_tree.as<uint32_t>(); S.wide_child = b.wide_child.as<int32_t>(); S.wide_all = b.wide_all.as<RefitBox>();
    S.wide_size = b.wide_size.as<uint32_t>(); S.wide_base = b.wide_base.as<uint32_t>(); S.wide_slot = b.wide_slot.as<uint32_t>();
    hipLaunchKernelGGL(k_w8_leaf, per_reference, block, 0, stream, S);
    if (!S.single_leaf)
        for (uint32_t l = bvh_levels; l-- > 0;) {
            const uint32_t first = level_first[l], count = level_first[l + 1] - first;
            hipLaunchKernelGGL(k_w8_optimise, blocks_for(count), block, 0, stream, S, first, count);
        }
    // 5: the wide nodes, level by level
    std::vector<uint32_t> wide_first, wide_count;
    uint32_t status[W8_STATUS_WORDS] = {};
    for (uint32_t level = 0, first = 0, count = 1; count; ++level) {
        if (level >= W8_MAX_WIDE_LEVELS || size_t(first) + count > wide_capacity) return fail(HIPR_ERROR_HIP, "%s: the collapse left its bounds at wide level %u (%u nodes from %u, room for %zu)", who, level, count, first, wide_capacity);
        hipLaunchKernelGGL(k_w8_prepare, blocks_for(count), block, 0, stream, S, first, count, level);
        HIP_TRY(hipMemcpyAsync(status, S.status, (W8_STATUS_LEVELS + level + 2) * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (status[W8_STATUS_OVERFLOW]) return fail(HIPR_ERROR_HIP, "%s: more wide nodes than a tree over %u records holds", who, record_total);
        wide_first.push_back(first); wide_count.push_back(count);
        first += count;
        count = status[W8_STATUS_LEVELS + level + 1];
    }
    const uint32_t wide_total = wide_first.back() + wide_count.back(), wide_levels = uint32_t(wide_first.size());
    // 6: the sizes; the slots needed are known before one is written
    for (uint32_t l = wide_levels; l-- > 0;) hipLaunchKernelGGL(k_w8_size, blocks_for(wide_count[l]), block, 0, stream, S, wide_first[l], wide_count[l]);
    uint32_t size_below_root = 0;
    HIP_TRY(hipMemcpyAsync(&size_below_root, S.wide_size, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint64_t slot_count = 1ull + size_below_root;
    if (slot_count != uint64_t(wide_total) + record_total) return fail(HIPR_ERROR_HIP, "%s: %llu slots below the root, %u nodes and %u records", who, (unsigned long long)slot_count, wide_total, record_total);
    if (slot_count > W8_MAX_SLOTS) return fail(HIPR_ERROR_UNSUPPORTED, "%s: the tree needs %llu slots, a node addresses %u", who, (unsigned long long)slot_count, W8_MAX_SLOTS);
    if (slot_count > slot_capacity) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the tree needs %llu slots, room for %u", who, (unsigned long long)slot_count, slot_capacity);
    if (b.slots.resize(size_t(slot_count) * sizeof(HiprSlot8))) return HIPR_ERROR_OUT_OF_MEMORY;
    S.slots = b.slots.as<HiprSlot8>();
    // 7, 8: the places, then the slots
    const uint32_t root_place[2] = {0u, 1u};
    HIP_TRY(hipMemcpyAsync(S.wide_slot, &root_place[0], 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(S.wide_base, &root_place[1], 4, hipMemcpyHostToDevice, stream));
    for (uint32_t l = 0; l < wide_levels; ++l) hipLaunchKernelGGL(k_w8_place, blocks_for(wide_count[l]), block, 0, stream, S, wide_first[l], wide_count[l]);
    hipLaunchKernelGGL(k_w8_emit_nodes, blocks_for(wide_total), block, 0, stream, S, wide_total);
    hipLaunchKernelGGL(k_w8_emit_leaves, blocks_for(record_total), block, 0, stream, S);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    result.slot_count = uint32_t(slot_count);
    result.height = wide_levels;
    result.node_count = wide_total; result.leaf_count = record_total; result.paired_leaves = status[W8_STATUS_PAIRED];
    return HIPR_OK;
}
// The scratch every collapse starts from, sized and cleared (queued on `stream`).
static int collapse_scratch_for(CollapseScratch& b, size_t T, hipStream_t stream) {
    const size_t scan_blocks = (T + W8_BLOCK - 1) / W8_BLOCK;
    if (b.counts.resize(T * 4) | b.block_sums.resize((scan_blocks + 1) * 4) | b.partial.resize(scan_blocks * 6 * sizeof(RefitBound)) | b.bounds.resize(6 * sizeof(RefitBound)) | b.status.resize(W8_STATUS_WORDS * 4))
        return HIPR_ERROR_OUT_OF_MEMORY;
    HIP_TRY(hipMemsetAsync(b.counts.ptr, 0, T * 4, stream));
    HIP_TRY(hipMemsetAsync(b.block_sums.ptr, 0, (scan_blocks + 1) * 4, stream));
    HIP_TRY(hipMemsetAsync(b.status.ptr, 0, W8_STATUS_WORDS * 4, stream));
    return HIPR_OK;
}

// The trees of the resident scene rebuilt on the device, in place, from the triangles it holds (scene_rebuild.h): flatten order, the BVH2 build, the hand-over, the
// collapse -- all in scratch, where every refusal still leaves the scene as the call found it -- and then ResidentScene::install_rebuilt_trees.
//
// hipr_edit_scene_instances is the same call with another instance list going in and another triangle count coming out: `edit`, which its entry point has checked
// (check_instance_edit), names the new list. The count per OLD instance is taken as without it; the flat array is then the NEW list's -- kept triangles through
// the old-to-new table, new ones made in place (instance_edit.h) -- and everything from the BVH2 build on runs over the new count.
static int rebuild_trees_on_the_device(HiprContext* c, const char* who, InstanceEdit* edit, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t node_capacity, uint32_t* out_order,
                                       HiprSlot8* out_slots, uint32_t slot_capacity, HiprSceneRebuildResult* out) {
    if (int st = check_context(c)) return st;
    ResidentScene& r = c->scene;
    if (!r.ready && !r.awaits_rebuild) return fail(HIPR_ERROR_NOT_READY, "%s: no scene uploaded, or one a failed call left behind", who);
    const uint32_t count = r.args.triangle_count, instance_count = uint32_t(r.uploaded_instances.size());
    // the conditions hipr_refit_scene_transforms refuses on: the arrays another search walks are the ones this call leaves stale, and the exhaustive search's items are the host's
    if (r.wide8.slot_count == 0 || !c->use_wide8() || r.args.trace_item_count != 0 || count > 0x55555555u || count == 0)
        return fail(HIPR_ERROR_UNSUPPORTED, "%s: the resident scene is not traced through the 8-wide tree; rebuild on the host and call hipr_upload_scene", who);
    if (count > BUILD_MAX_TRIANGLES) return fail(HIPR_ERROR_UNSUPPORTED, "%s: %u triangles, a leaf reference holds %u", who, count, BUILD_MAX_TRIANGLES);
    if (!out) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null result", who);
    // the room the outputs need for `triangles` triangles; an edit knows its count once the kept instances are counted, and is checked there
    auto outputs_fit = [&](uint32_t triangles) {
        const uint32_t nodes_needed = std::max(std::max(triangles, 1u) - 1u, 1u), slots_needed = uint32_t(std::min<uint64_t>(2ull * triangles, W8_MAX_SLOTS));
        if (out_nodes && node_capacity < nodes_needed) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: room for %u nodes, %u triangles can need %u", who, node_capacity, triangles, nodes_needed);
        if (out_slots && slot_capacity < slots_needed) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: room for %u slots, %u triangles can need %u", who, slot_capacity, triangles, slots_needed);
        if (edit && out_order && edit->order_capacity < triangles) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: room for %u order words, the new list has %u triangles", who, edit->order_capacity, triangles);
        return int(HIPR_OK);
    };
    if (!edit)
        if (int st = outputs_fit(count)) return st;
    if (int finish_status = finish_all(c)) return finish_status;      // no pending pass may go on over the new trees
    const uint32_t depth_limit = std::max(max_depth, 8u);
    BuildScratch& b = c->build;
    CollapseScratch& w = c->collapse;
    RebuildScratch& x = c->rebuild;
    const ScratchGuard build_guard{b};
    const ScratchGuard collapse_guard{w};
    const ScratchGuard rebuild_guard{x};
    hipStream_t stream = c->stream;
    c->break_chain(stream);
    const auto t0 = std::chrono::steady_clock::now();

    // the flatten order: the triangles per resident instance ...
    if (x.instance_counts.resize(size_t(instance_count) * 4) | x.status.resize(REBUILD_STATUS_WORDS * 4)) return HIPR_ERROR_OUT_OF_MEMORY;
    HIP_TRY(hipMemsetAsync(x.instance_counts.ptr, 0, size_t(instance_count) * 4, stream));
    HIP_TRY(hipMemsetAsync(x.status.ptr, 0, REBUILD_STATUS_WORDS * 4, stream));
    RebuildArrays a = {r.triangles.as<HiprTriangle>(), r.triangle_class.as<uint8_t>(), count, instance_count, x.instance_counts.as<uint32_t>(), nullptr, nullptr, nullptr, nullptr, x.status.as<uint32_t>()};
    const dim3 block(REBUILD_BLOCK), per_triangle((count + REBUILD_BLOCK - 1) / REBUILD_BLOCK);
    hipLaunchKernelGGL(k_rebuild_count, per_triangle, block, 0, stream, a);      // reads the resident triangles, writes the counts and the flag
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> counted(size_t(instance_count) + 1, 0u);
    HIP_TRY(hipMemcpyAsync(counted.data(), x.instance_counts.ptr, size_t(instance_count) * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    uint64_t total = 0;
    for (uint32_t i = 0; i < instance_count; ++i) total += counted[i];
    if (total != count) return fail(HIPR_ERROR_UNSUPPORTED, "%s: %llu of %u resident triangles belong to one of the %u instances", who, (unsigned long long)total, count, instance_count);
    // ... and first[] of the list the flat array is made for: the resident instances, or the edit's
    const uint32_t list_count = edit ? uint32_t(edit->instances.size()) : instance_count;
    std::vector<uint32_t> first(size_t(list_count) + 1, 0u), created, created_first(1, 0u);
    total = 0;
    for (uint32_t i = 0; i < list_count; ++i) {
        if (edit && edit->source[i] != BUILD_NONE) edit->primitive_count[i] = counted[edit->source[i]];
        if (edit && edit->source[i] == BUILD_NONE) { created.push_back(i); created_first.push_back(created_first.back() + edit->primitive_count[i]); }      // below 2^32: each count is inside the index pool, checked against the total next
        total += edit ? edit->primitive_count[i] : counted[i];
        if (total > BUILD_MAX_TRIANGLES) return fail(HIPR_ERROR_UNSUPPORTED, "%s: the new list has more than %u triangles, what a leaf reference holds", who, BUILD_MAX_TRIANGLES);
        first[i + 1] = uint32_t(total);
    }
    const size_t n = size_t(total);
    const uint32_t new_count = uint32_t(total);
    if (edit) {
        if (new_count == 0) return fail(HIPR_ERROR_UNSUPPORTED, "%s: the new list yields no triangle", who);
        if (int st = outputs_fit(new_count)) return st;
    }
    if (b.triangles.resize(n * sizeof(HiprTriangle)) | x.flat_class.resize(n) | x.claim.resize(n * 4) | x.first.resize((size_t(list_count) + 1) * 4)) return HIPR_ERROR_OUT_OF_MEMORY;
    HIP_TRY(hipMemsetAsync(x.claim.ptr, 0, n * 4, stream));
    HIP_TRY(hipMemcpyAsync(x.first.ptr, first.data(), first.size() * 4, hipMemcpyHostToDevice, stream));
    a.first = x.first.as<uint32_t>(); a.flat = b.triangles.as<HiprTriangle>(); a.flat_class = x.flat_class.as<uint8_t>(); a.claim = x.claim.as<uint32_t>();
    if (!edit) hipLaunchKernelGGL(k_rebuild_scatter, per_triangle, block, 0, stream, a);
    else {
        const uint32_t created_count = uint32_t(created.size()), created_triangles = created_first.back();
        if (x.old_to_new.upload(edit->old_to_new.data(), edit->old_to_new.size() * 4, stream) | x.created.upload(created.data(), created.size() * 4, stream) |
            x.created_first.upload(created_first.data(), created_first.size() * 4, stream) | x.instances.upload(edit->instances.data(), edit->instances.size() * sizeof(HiprInstance), stream))
            return HIPR_ERROR_OUT_OF_MEMORY;
        const EditArrays e = {a.resident, a.resident_class, count, instance_count, x.old_to_new.as<uint32_t>(), a.first, list_count, new_count, x.created.as<uint32_t>(), x.created_first.as<uint32_t>(),
                              created_count, created_triangles, x.instances.as<HiprInstance>(), r.materials.as<HiprMaterial>(), r.indices.as<uint32_t>(), r.geometry.as<HiprVertexGeometry>(),
                              r.uploaded_vertex_count, r.uploaded_mesh_attributes & HIPR_MESH_TEXCOORDS ? reinterpret_cast<const float*>(r.args.texcoords) : nullptr, r.textures.as<HiprTexture>(), uint32_t(r.uploaded_textures.size()), r.texels.as<uint8_t>(),
                              a.flat, a.flat_class, a.claim, a.status};
        hipLaunchKernelGGL(k_edit_scatter, per_triangle, block, 0, stream, e);
        if (created_triangles) hipLaunchKernelGGL(k_edit_new_triangles, dim3((created_triangles + REBUILD_BLOCK - 1) / REBUILD_BLOCK), block, 0, stream, e);
        hipLaunchKernelGGL(k_edit_reduce, dim3((new_count + REBUILD_BLOCK - 1) / REBUILD_BLOCK), block, 0, stream, e.flat, e.flat_class, e.claim, e.status, new_count);
    }
    HIP_TRY(hipGetLastError());
    uint32_t flatten_status[REBUILD_STATUS_WORDS] = {};
    HIP_TRY(hipMemcpyAsync(flatten_status, x.status.ptr, sizeof(flatten_status), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));      // the host's lists are read by now as well
    if (edit && flatten_status[EDIT_STATUS_INDEX]) return fail(HIPR_ERROR_UNSUPPORTED, "%s: an index triple of a new instance points outside the vertex pool", who);
    if (edit && flatten_status[REBUILD_STATUS_CLAIM]) return fail(HIPR_ERROR_UNSUPPORTED, "%s: a flatten position (instance, primitive) is claimed twice or not at all; rebuild on the host", who);
    if (flatten_status[REBUILD_STATUS_CLAIM]) return fail(HIPR_ERROR_UNSUPPORTED, "%s: two resident triangles claim one flatten position (instance, primitive); rebuild on the host", who);
    const auto t1 = std::chrono::steady_clock::now();

    // the BVH2 over the flat array
    Bvh2Built built;
    std::chrono::steady_clock::time_point unused;
    if (int st = build_bvh2_on_the_device(c, who, nullptr, b.triangles.as<HiprTriangle>(), new_count, depth_limit, built, unused)) return st;
    uint32_t build_status[STATUS_LEVELS] = {};
    HIP_TRY(hipMemcpyAsync(build_status, b.status.ptr, STATUS_LEVELS * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint32_t node_count = built.node_count, deepest = build_status[STATUS_DEEPEST];
    const uint32_t bvh_levels = std::max<uint32_t>(uint32_t(built.level_nodes.size()), 1u);
    if (bvh_levels > W8_MAX_LEVELS || deepest + 1u > 64u)
        return fail(HIPR_ERROR_UNSUPPORTED, "%s: the new BVH2 has %u levels of nodes and its deepest leaf at %u, the kernels walk 64", who, bvh_levels, deepest);
    // a fresh upload of so small a scene would choose another search (ResidentScene::choose_variant) and build other arrays: the host path serves it
    if (edit && node_count <= 64u) return fail(HIPR_ERROR_UNSUPPORTED, "%s: the new BVH2 has %u nodes, the 8-wide search serves more than 64; rebuild on the host and call hipr_upload_scene", who, node_count);
    const auto t2 = std::chrono::steady_clock::now();

    // the hand-over and the collapse
    if (x.level_nodes.resize(size_t(node_count) * 4)) return HIPR_ERROR_OUT_OF_MEMORY;
    if (int st = collapse_scratch_for(w, n, stream)) return st;
    hipLaunchKernelGGL(k_rebuild_levels, dim3((node_count + REBUILD_BLOCK - 1) / REBUILD_BLOCK), block, 0, stream, b.place.as<uint32_t>(), x.level_nodes.as<uint32_t>(), node_count);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> level_first(size_t(bvh_levels) + 1, 0u);
    if (built.level_nodes.empty()) level_first[1] = 1u;      // at most three triangles: the root references one leaf twice
    else for (uint32_t l = 0; l < bvh_levels; ++l) level_first[l + 1] = level_first[l] + built.level_nodes[l];
    W8State S = {};
    S.nodes = b.out_nodes.as<HiprBvhNode>(); S.node_count = node_count;
    S.triangles = b.triangles.as<HiprTriangle>(); S.order = b.order.as<uint32_t>(); S.triangle_count = new_count;
    S.level_nodes = x.level_nodes.as<uint32_t>(); S.reachable = node_count; S.single_leaf = built.level_nodes.empty() ? 1u : 0u;
    S.counts = w.counts.as<uint32_t>(); S.block_sums = w.block_sums.as<uint32_t>(); S.status = w.status.as<uint32_t>();
    HiprWide8BuildResult wide8 = {};
    if (int st = collapse_on_the_device(c, who, S, level_first, 0xFFFFFFFFu, wide8)) return st == HIPR_ERROR_INVALID_ARGUMENT ? HIPR_ERROR_UNSUPPORTED : st;
    if (wide8.height > 33u) return fail(HIPR_ERROR_UNSUPPORTED, "%s: the new 8-wide tree is %u levels high, the kernels' stacks hold 33; rebuild on the host", who, wide8.height);
    if ((out_nodes && node_count > node_capacity) || (out_slots && wide8.slot_count > slot_capacity)) return fail(HIPR_ERROR_HIP, "%s: %u nodes and %u slots built, more than the bounds checked", who, node_count, wide8.slot_count);
    std::vector<HiprSlot8> host_slots(wide8.slot_count);      // the refit's lists are made from the host's copy, as at upload
    HIP_TRY(hipMemcpyAsync(host_slots.data(), S.slots, host_slots.size() * sizeof(HiprSlot8), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const auto t3 = std::chrono::steady_clock::now();

    // nothing refuses from here on: the new resident arrays
    const ResidentScene::RebuiltTrees::NewSet new_set = {new_count, x.instances.as<HiprInstance>(), edit ? &edit->instances : nullptr, flatten_status[EDIT_STATUS_NOT_OPAQUE] == 0,
                                                         flatten_status[EDIT_STATUS_COATED] != 0};
    const ResidentScene::RebuiltTrees trees = {b.triangles.as<HiprTriangle>(), x.flat_class.as<uint8_t>(), b.order.as<uint32_t>(), b.out_nodes.as<HiprBvhNode>(), node_count, deepest,
                                               S.slots, host_slots.data(), wide8, edit ? &new_set : nullptr};
    if (int st = r.install_rebuilt_trees(trees, stream)) return st;
    if (edit) edit->triangle_count = new_count;
    const auto t4 = std::chrono::steady_clock::now();
    if (out_nodes) HIP_TRY(hipMemcpyAsync(out_nodes, b.out_nodes.ptr, size_t(node_count) * sizeof(HiprBvhNode), hipMemcpyDeviceToHost, stream));
    if (out_order) HIP_TRY(hipMemcpyAsync(out_order, b.order.ptr, n * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (out_slots) std::memcpy(out_slots, host_slots.data(), host_slots.size() * sizeof(HiprSlot8));
    out->node_count = node_count; out->deepest = deepest; out->wide8 = wide8; out->half_area = r.uploaded_half_area;
    const auto t5 = std::chrono::steady_clock::now();
    x.flatten_ms = ms(t0, t1); x.bvh2_ms = ms(t1, t2); x.collapse_ms = ms(t2, t3); x.install_ms = ms(t3, t4); x.readback_ms = ms(t4, t5);
    if (std::getenv("HIPR_BVH_TIMING"))
        fprintf(stderr, "[hipr] %s: %u triangles, %u nodes, %u slots: flatten order %.3f ms, BVH2 %.3f ms, collapse + slots to the host %.3f ms, new resident arrays %.3f ms, read-back %.3f ms\n", who, new_count, node_count,
                wide8.slot_count, x.flatten_ms, x.bvh2_ms, x.collapse_ms, x.install_ms, x.readback_ms);
    return HIPR_OK;
}

} // namespace

// ---- the entry points ---------------------------------------------------------------------------------------------------------------------------------------
extern "C" {

int hipr_validate_scene(const HiprSceneDesc* s) {
    Preflight checked;
    return preflight_scene("hipr_validate_scene", s, checked);
}

int hipr_upload_scene(HiprContext* c, const HiprSceneDesc* s) {
    if (int st = check_context(c)) return st;
    Preflight checked;
    if (int st = preflight_scene("hipr_upload_scene", s, checked)) return st;
    // what the kernels cannot serve (a description hipr_validate_scene finds sound may still meet these)
    if (s->bvh_max_depth > 64) return fail(HIPR_ERROR_UNSUPPORTED, "BVH depth %u exceeds the 64 entry LDS stack", s->bvh_max_depth);
    if (checked.wide_stack_need > 32u + uint32_t(TRACE_SPILL_ENTRIES))
        return fail(HIPR_ERROR_UNSUPPORTED, "the wide BVH needs %u stack entries, more than the %u the traversal kernels provide", checked.wide_stack_need, 32u + uint32_t(TRACE_SPILL_ENTRIES));
    if (s->environment) {
        const uint8_t format = s->textures[s->environment->environment_map_ID].format;
        if (format != HIPR_TEXEL_RGBA8 && format != HIPR_TEXEL_RGBA32F)
            return fail(HIPR_ERROR_UNSUPPORTED, "only environments with 4 channels are supported (OptiXRenderer/Renderer.cpp:1141-1158)");
    }
    if (int finish_status = finish_all(c)) return finish_status;
    return c->scene.upload(s, checked, c->knobs.trace_variant, c->knobs.cull_backfaces, c->stream);
}

int hipr_update_scene_geometry(HiprContext* c, const HiprSceneDesc* s) {
    if (int st = check_context(c)) return st;
    Preflight checked;
    if (int st = preflight_scene("hipr_update_scene_geometry", s, checked)) return st;
    const ResidentScene& r = c->scene;
    if (!r.ready) return fail(HIPR_ERROR_NOT_READY, "hipr_update_scene_geometry: no scene uploaded");
    // Meshes, materials and textures stay on the device as uploaded: the description was validated against ITS pools, so those must be the
    // uploaded ones in size -- an index that is in range for a larger pool of the description would read out of bounds on the device.
    if (s->material_count != r.uploaded_materials.size() || s->texture_count != r.uploaded_texture_count || s->vertex_count != r.uploaded_vertex_count ||
        s->index_count != r.uploaded_index_count || s->texel_bytes != r.uploaded_texel_bytes)
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_geometry: material, texture, vertex, index and texel pool sizes must equal the uploaded scene's (those pools are not re-uploaded)");
    const bool wide4_follows = r.wide4_awaits_geometry;      // after hipr_rebuild_scene_trees the 4-wide tree is a new one: it is taken, not compared
    if (s->node_count != r.args.node_count || s->triangle_count != r.args.triangle_count || (!wide4_follows && (s->wide_nodes ? s->wide_node_count : 0u) != r.args.wide_node_count) ||
        s->light_count != r.args.light_count || s->instance_count != r.uploaded_instances.size())
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_geometry: node, triangle, instance and light counts must equal the uploaded scene's (a refit keeps the topology)");
    if (!wide4_follows && checked.wide_stack_need != r.wide_stack_entries) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_geometry: the wide BVH's topology changed");
    if (wide4_follows && (checked.wide_stack_need > 32u + uint32_t(TRACE_SPILL_ENTRIES) || s->bvh_max_depth > 64))
        return fail(HIPR_ERROR_UNSUPPORTED, "hipr_update_scene_geometry: the rebuilt scene's trees need more stack than the traversal kernels provide");
    if (r.wide8.slot_count && (s->wide8_slot_count != r.wide8.slot_count || checked.wide8_height != r.wide8_height))
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_geometry: the 8-wide tree's topology changed");
    if (int st = r.lights_keep_their_types("hipr_update_scene_geometry", s->lights, s->light_count)) return st;
    if (int finish_status = finish_all(c)) return finish_status;      // pipelined passes included: no pending pass may go on over the new geometry
    return c->scene.update_geometry(s, checked, c->knobs.trace_variant, c->knobs.cull_backfaces, c->stream);
}

int hipr_refit_scene_transforms(HiprContext* c, const HiprInstanceTransform* moved, uint32_t moved_count, const HiprLight* lights, uint32_t light_count, HiprRefitResult* out) {
    if (int st = check_context(c)) return st;
    if (!out || (moved_count && !moved)) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_refit_scene_transforms: null argument");
    const ResidentScene& r = c->scene;
    if (!r.ready) return fail(HIPR_ERROR_NOT_READY, "hipr_refit_scene_transforms: no scene uploaded");
    // Scenes that are not traced through the 8-wide tree have at most 64 BVH2 nodes (or a tree too high for the kernels, or a search forced for an experiment): the
    // host path costs nothing there, and the arrays their search walks are the ones this call leaves stale. The exhaustive search's items are built on the host.
    if (r.wide8.slot_count == 0 || !c->use_wide8() || r.args.trace_item_count != 0 || r.args.triangle_count > 0x55555555u)
        return fail(HIPR_ERROR_UNSUPPORTED, "hipr_refit_scene_transforms: the uploaded scene is not traced through the 8-wide tree; refit on the host and call hipr_update_scene_geometry");
    for (uint32_t k = 0; k < moved_count; ++k) {
        if (moved[k].instance_index >= r.uploaded_instances.size())
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_refit_scene_transforms: instance %u of %zu", moved[k].instance_index, r.uploaded_instances.size());
        for (int e = 0; e < 12; ++e)
            if (!std::isfinite(moved[k].object_to_world[e])) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_refit_scene_transforms: the matrix of instance %u is not finite", moved[k].instance_index);
        // A mirrored instance is drawn from index triples of its own (two corners exchanged): that changes the triangle array, which stays the host path's business.
        if (refit_mirrors(moved[k].object_to_world) != refit_mirrors(r.uploaded_instances[moved[k].instance_index].object_to_world))
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_refit_scene_transforms: the matrix of instance %u changes its handedness; refit on the host", moved[k].instance_index);
    }
    if (lights) {
        if (light_count != r.args.light_count) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_refit_scene_transforms: %u lights given, the uploaded scene has %u", light_count, r.args.light_count);
        if (int st = r.lights_keep_their_types("hipr_refit_scene_transforms", lights, light_count)) return st;
    }
    if (int finish_status = finish_all(c)) return finish_status;      // no pending pass may go on over the new geometry
    return c->scene.refit_transforms(moved, moved_count, lights, light_count, c->stream, out);
}

// Not part of the public header: every refusal of hipr_update_scene_materials, and nothing else -- the device and the books stay as they are. The group asks
// every member before any member writes.
int hipr_internal_check_material_update(HiprContext* c, const HiprMaterialUpdate* materials, uint32_t material_count, const HiprInstanceMaterial* assignments, uint32_t assignment_count) {
    if (int st = check_context(c)) return st;
    const ResidentScene& r = c->scene;
    if (!r.ready) return fail(HIPR_ERROR_NOT_READY, "hipr_update_scene_materials: no scene uploaded");
    if ((material_count && !materials) || (assignment_count && !assignments)) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_materials: null array with a non-zero count");
    for (uint32_t k = 0; k < material_count; ++k) {
        if (materials[k].material_index >= r.uploaded_materials.size())
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_materials: material %u of %zu (the material pool does not grow; upload the scene instead)", materials[k].material_index, r.uploaded_materials.size());
        char invalid[256];
        if (invalid_material(materials[k].material, materials[k].material_index, uint32_t(r.uploaded_textures.size()), invalid, sizeof(invalid)))
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_materials: %s", invalid);
    }
    for (uint32_t k = 0; k < assignment_count; ++k) {
        if (assignments[k].instance_index >= r.uploaded_instances.size())
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_materials: instance %u of %zu", assignments[k].instance_index, r.uploaded_instances.size());
        if (assignments[k].material_index < 0 || size_t(assignments[k].material_index) >= r.uploaded_materials.size())
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_materials: instance %u is given material %d of %zu", assignments[k].instance_index, assignments[k].material_index, r.uploaded_materials.size());
    }
    // The exhaustive search's items pair triangles of equal flags (build_trace_items): there a material edit changes a topology, which only the host builds.
    if (r.args.trace_item_count != 0)
        return fail(HIPR_ERROR_UNSUPPORTED, "hipr_update_scene_materials: the uploaded scene carries the exhaustive search's items, which pair triangles by their flags; upload the scene instead");
    return HIPR_OK;
}

int hipr_update_scene_materials(HiprContext* c, const HiprMaterialUpdate* materials, uint32_t material_count, const HiprInstanceMaterial* assignments, uint32_t assignment_count) {
    if (int st = hipr_internal_check_material_update(c, materials, material_count, assignments, assignment_count)) return st;
    if (int finish_status = finish_all(c)) return finish_status;      // no pending pass may go on over the new materials
    return c->scene.update_materials(materials, material_count, assignments, assignment_count, c->stream);
}

// The BVH2 of host/BvhBuilder.cpp built by the kernels of bvh2_build.h. Nothing of the resident scene is read or written; the outputs are written only once the
// whole build has succeeded.
int hipr_build_bvh2(HiprContext* c, const HiprTriangle* triangles, uint32_t count, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t node_capacity, uint32_t* out_node_count,
                    uint32_t* out_order, uint32_t* out_deepest) {
    if (int st = check_context(c)) return st;
    const auto t_validate = std::chrono::steady_clock::now();
    if (!triangles || !count || !out_nodes || !out_node_count || !out_order || !out_deepest) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_build_bvh2: null argument or no triangles");
    if (count > BUILD_MAX_TRIANGLES) return fail(HIPR_ERROR_UNSUPPORTED, "hipr_build_bvh2: %u triangles, a leaf reference holds %u", count, BUILD_MAX_TRIANGLES);
    if (node_capacity < std::max(std::max(count, 1u) - 1u, 1u)) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_build_bvh2: room for %u nodes, %u triangles can need %u", node_capacity, count, std::max(count - 1u, 1u));
    for (uint32_t i = 0; i < count; ++i)
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(triangles[i].v0[k]) || !std::isfinite(triangles[i].v1[k]) || !std::isfinite(triangles[i].v2[k]))
                return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_build_bvh2: triangle %u has a corner that is not finite", i);
    const uint32_t depth_limit = std::max(max_depth, 8u);
    const size_t n = count;
    BuildScratch& b = c->build;
    const ScratchGuard guard{b};
    hipStream_t stream = c->stream;
    c->break_chain(stream);
    const auto t0 = std::chrono::steady_clock::now();
    Bvh2Built built;
    std::chrono::steady_clock::time_point t1;
    if (int st = build_bvh2_on_the_device(c, "hipr_build_bvh2", triangles, nullptr, count, depth_limit, built, t1)) return st;
    const uint32_t node_count = built.node_count;
    uint32_t status[STATUS_LEVELS] = {};
    const auto t2 = std::chrono::steady_clock::now();
    if (node_count > node_capacity) return fail(HIPR_ERROR_HIP, "hipr_build_bvh2: %u nodes built, room for %u", node_count, node_capacity);
    HIP_TRY(hipMemcpyAsync(status, b.status.ptr, STATUS_LEVELS * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out_nodes, b.out_nodes.ptr, size_t(node_count) * sizeof(HiprBvhNode), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out_order, b.order.ptr, n * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *out_node_count = node_count;
    *out_deepest = status[STATUS_DEEPEST];
    const auto t3 = std::chrono::steady_clock::now();
    b.validate_ms = ms(t_validate, t0); b.upload_ms = ms(t0, t1); b.kernel_ms = ms(t1, t2); b.readback_ms = ms(t2, t3);
    if (std::getenv("HIPR_BVH_TIMING"))
        fprintf(stderr, "[hipr] hipr_build_bvh2: %u triangles, %u nodes, %u levels: argument checks %.3f ms, allocation + upload %.3f ms, kernels %.3f ms, read-back %.3f ms (transfers %.0f %% of %.3f ms)\n", count, node_count, b.levels,
                b.validate_ms, b.upload_ms, b.kernel_ms, b.readback_ms, 100.0 * (b.upload_ms + b.readback_ms) / (b.validate_ms + b.upload_ms + b.kernel_ms + b.readback_ms),
                b.validate_ms + b.upload_ms + b.kernel_ms + b.readback_ms);
    return HIPR_OK;
}

int hipr_debug_build_times(HiprContext* c, double* out4_ms) {
    if (!c || !out4_ms) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_build_times: null argument");
    out4_ms[0] = c->build.validate_ms; out4_ms[1] = c->build.upload_ms; out4_ms[2] = c->build.kernel_ms; out4_ms[3] = c->build.readback_ms;
    return HIPR_OK;
}

// The 8-wide tree of host/Wide8Builder.cpp collapsed from a BVH2 by the kernels of wide8_build.h. Nothing of the resident scene is read or written; the outputs are
// written only once the whole collapse has succeeded.
int hipr_build_wide8(HiprContext* c, const HiprBvhNode* nodes, uint32_t node_count, const HiprTriangle* triangles, const uint32_t* order, uint32_t triangle_count, HiprSlot8* out_slots,
                     uint32_t slot_capacity, HiprWide8BuildResult* out) {
    if (int st = check_context(c)) return st;
    const auto t_validate = std::chrono::steady_clock::now();
    if (!nodes || !node_count || !triangles || !triangle_count || !out_slots || !out) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_build_wide8: null argument, no nodes or no triangles");
    if (triangle_count > BUILD_MAX_TRIANGLES || node_count > BUILD_MAX_TRIANGLES) return fail(HIPR_ERROR_UNSUPPORTED, "hipr_build_wide8: %u triangles and %u nodes, a leaf reference holds %u", triangle_count, node_count, BUILD_MAX_TRIANGLES);
    W8Input input;
    char reason[256] = "";
    if (const int refused = w8_check_input(nodes, node_count, order, triangle_count, input, reason, sizeof(reason)))
        return fail(refused == W8_INPUT_DECLINED ? HIPR_ERROR_UNSUPPORTED : HIPR_ERROR_INVALID_ARGUMENT, "hipr_build_wide8: %s", reason);
    const uint32_t reachable = uint32_t(input.level_nodes.size()), bvh_levels = uint32_t(input.level_first.size()) - 1u;
    CollapseScratch& b = c->collapse;
    const ScratchGuard guard{b};
    hipStream_t stream = c->stream;
    c->break_chain(stream);
    const auto t0 = std::chrono::steady_clock::now();
    const size_t T = triangle_count, N = node_count;
    if (int st = collapse_scratch_for(b, T, stream)) return st;
    if (int st = b.nodes.upload(nodes, N * sizeof(HiprBvhNode), stream)) return st;
    if (int st = b.triangles.upload(triangles, T * sizeof(HiprTriangle), stream)) return st;
    if (order) if (int st = b.order.upload(order, T * 4, stream)) return st;
    if (int st = b.level_nodes.upload(input.level_nodes.data(), size_t(reachable) * 4, stream)) return st;
    HIP_TRY(hipStreamSynchronize(stream));
    const auto t1 = std::chrono::steady_clock::now();

    W8State S = {};
    S.nodes = b.nodes.as<HiprBvhNode>(); S.node_count = node_count;
    S.triangles = b.triangles.as<HiprTriangle>(); S.order = order ? b.order.as<uint32_t>() : nullptr; S.triangle_count = triangle_count;
    S.level_nodes = b.level_nodes.as<uint32_t>(); S.reachable = reachable; S.single_leaf = input.single_leaf ? 1u : 0u;
    S.counts = b.counts.as<uint32_t>(); S.block_sums = b.block_sums.as<uint32_t>(); S.status = b.status.as<uint32_t>();
    HiprWide8BuildResult result = {};
    if (int st = collapse_on_the_device(c, "hipr_build_wide8", S, input.level_first, slot_capacity, result)) return st;
    const uint32_t record_total = result.leaf_count,wide_total = result.node_count, wide_levels = result.height;
    const uint64_t slot_count = result.slot_count;
    const auto t2 = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpyAsync(out_slots, S.slots, size_t(slot_count) * sizeof(HiprSlot8), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *out = result;
    const auto t3 = std::chrono::steady_clock::now();
    b.validate_ms = ms(t_validate, t0); b.upload_ms = ms(t0, t1); b.kernel_ms = ms(t1, t2); b.readback_ms = ms(t2, t3);
    if (std::getenv("HIPR_BVH_TIMING"))
        fprintf(stderr, "[hipr] hipr_build_wide8: %u triangles, %u BVH2 nodes on %u levels, %u records, %u wide nodes on %u levels, %u slots: index walk %.3f ms, allocation + upload %.3f ms, kernels %.3f ms, read-back %.3f ms\n",
                triangle_count, node_count, bvh_levels, record_total, wide_total, wide_levels, result.slot_count, b.validate_ms, b.upload_ms, b.kernel_ms, b.readback_ms);
    return HIPR_OK;
}

int hipr_debug_collapse_times(HiprContext* c, double* out4_ms) {
    if (!c || !out4_ms) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_collapse_times: null argument");
    out4_ms[0] = c->collapse.validate_ms; out4_ms[1] = c->collapse.upload_ms; out4_ms[2] = c->collapse.kernel_ms; out4_ms[3] = c->collapse.readback_ms;
    return HIPR_OK;
}

// The compressed 4-wide tree of host/BvhBuilder.cpp's WideCollapse collapsed from a BVH2 by the kernels of wide4_build.h. Nothing of the resident scene is read or
// written; the outputs are written only once the whole collapse has succeeded.
int hipr_build_wide4(HiprContext* c, const HiprBvhNode* nodes, uint32_t node_count, uint32_t triangle_count, HiprWideNode* out_nodes, uint32_t node_capacity, HiprWide4BuildResult* out) {
    const char* who = "hipr_build_wide4";
    if (int st = check_context(c)) return st;
    const auto t_validate = std::chrono::steady_clock::now();
    if (!nodes || !node_count || !out_nodes || !out) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null argument or no nodes", who);
    if (node_count > BUILD_MAX_TRIANGLES) return fail(HIPR_ERROR_UNSUPPORTED, "%s: %u nodes, a leaf reference holds %u", who, node_count, BUILD_MAX_TRIANGLES);
    W8Input input;
    char reason[256] = "";
    if (w8_check_input(nodes, node_count, nullptr, triangle_count, input, reason, sizeof(reason)) == W8_INPUT_INVALID) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: %s", who, reason);
    const uint32_t reachable = uint32_t(input.level_nodes.size()), bvh_levels = uint32_t(input.level_first.size()) - 1u;
    Collapse4Scratch& b = c->collapse4;
    const ScratchGuard guard{b};
    hipStream_t stream = c->stream;
    c->break_chain(stream);
    const auto t0 = std::chrono::steady_clock::now();
    const size_t N = node_count, capacity = reachable;      // every wide node is rooted at a distinct reachable BVH2 node
    if (b.need.resize(N * 4) | b.wide_root.resize(capacity * 4) | b.wide_budget.resize(capacity * 4) | b.made.resize(capacity * sizeof(HiprWideNode)) | b.wide_size.resize(capacity * 4) |
        b.wide_stack.resize(capacity * 4) | b.wide_at.resize(capacity * 4) | b.status.resize(W4_STATUS_WORDS * 4))
        return HIPR_ERROR_OUT_OF_MEMORY;
    if (int st = b.nodes.upload(nodes, N * sizeof(HiprBvhNode), stream)) return st;
    if (int st = b.level_nodes.upload(input.level_nodes.data(), size_t(reachable) * 4, stream)) return st;
    HIP_TRY(hipMemsetAsync(b.status.ptr, 0, W4_STATUS_WORDS * 4, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const auto t1 = std::chrono::steady_clock::now();

    W4State S = {};
    S.nodes = b.nodes.as<HiprBvhNode>(); S.node_count = node_count; S.level_nodes = b.level_nodes.as<uint32_t>(); S.need = b.need.as<uint32_t>();
    S.wide_capacity = uint32_t(capacity); S.wide_root = b.wide_root.as<uint32_t>(); S.wide_budget = b.wide_budget.as<uint32_t>(); S.made = b.made.as<HiprWideNode>();
    S.wide_size = b.wide_size.as<uint32_t>(); S.wide_stack = b.wide_stack.as<uint32_t>(); S.wide_at = b.wide_at.as<uint32_t>(); S.status = b.status.as<uint32_t>();
    const dim3 block(W8_BLOCK);
    auto blocks_for = [](uint32_t threads) { return dim3((threads + W8_BLOCK - 1) / W8_BLOCK); };
    // 2: binary_need, deepest level first, and the finite check; the host chooses the root's budget
    for (uint32_t l = bvh_levels; l-- > 0;) {
        const uint32_t first = input.level_first[l], count = input.level_first[l + 1] - first;
        hipLaunchKernelGGL(k_w4_need, blocks_for(count), block, 0, stream, S, first, count);
    }
    uint32_t root_need = 0, not_finite = 0;
    HIP_TRY(hipMemcpyAsync(&root_need, S.need, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&not_finite, S.status + W4_STATUS_NOT_FINITE, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (not_finite) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: a child box is not finite", who);
    if (root_need == 0 || root_need > W8_MAX_LEVELS) return fail(HIPR_ERROR_HIP, "%s: the root needs %u entries on %u levels", who, root_need, bvh_levels);
    const uint32_t root_entry[2] = {0u, root_need <= W4_SMALL_BUDGET ? W4_SMALL_BUDGET : W4_LARGE_BUDGET};
    HIP_TRY(hipMemcpyAsync(S.wide_root, &root_entry[0], 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(S.wide_budget, &root_entry[1], 4, hipMemcpyHostToDevice, stream));
    // 3: the wide nodes, level by level
    std::vector<uint32_t> wide_first, wide_count;
    uint32_t status[W4_STATUS_WORDS] = {};
    for (uint32_t level = 0, first = 0, count = 1; count; ++level) {
        if (level >= W4_MAX_WIDE_LEVELS || size_t(first) + count > capacity) return fail(HIPR_ERROR_HIP, "%s: the collapse left its bounds at wide level %u (%u nodes from %u, room for %zu)", who, level, count, first, capacity);
        hipLaunchKernelGGL(k_w4_collapse, blocks_for(count), block, 0, stream, S, first, count, level);
        HIP_TRY(hipMemcpyAsync(status, S.status, (W4_STATUS_LEVELS + level + 2) * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (status[W4_STATUS_OVERFLOW]) return fail(HIPR_ERROR_HIP, "%s: more wide nodes than the %u BVH2 nodes reached", who, reachable);
        wide_first.push_back(first); wide_count.push_back(count);
        first += count;
        count = status[W4_STATUS_LEVELS + level + 1];
    }
    const uint32_t wide_total = wide_first.back() + wide_count.back(), wide_levels = uint32_t(wide_first.size());
    if (wide_total > node_capacity) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the tree needs %u nodes, room for %u", who, wide_total, node_capacity);
    if (b.out.resize(size_t(wide_total) * sizeof(HiprWideNode))) return HIPR_ERROR_OUT_OF_MEMORY;
    S.out = b.out.as<HiprWideNode>();
    // 4: sizes and stack needs, bottom-up; 5: positions and the nodes in place, top-down
    for (uint32_t l = wide_levels; l-- > 0;) hipLaunchKernelGGL(k_w4_size, blocks_for(wide_count[l]), block, 0, stream, S, wide_first[l], wide_count[l]);
    HIP_TRY(hipMemsetAsync(S.wide_at, 0, 4, stream));
    for (uint32_t l = 0; l < wide_levels; ++l) hipLaunchKernelGGL(k_w4_place_emit, blocks_for(wide_count[l]), block, 0, stream, S, wide_first[l], wide_count[l]);
    uint32_t root_words[2] = {0u, 0u};
    HIP_TRY(hipMemcpyAsync(&root_words[0], S.wide_size, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&root_words[1], S.wide_stack, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    if (root_words[0] != wide_total) return fail(HIPR_ERROR_HIP, "%s: %u nodes below the root, %u made", who, root_words[0], wide_total);
    const auto t2 = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpyAsync(out_nodes, S.out, size_t(wide_total) * sizeof(HiprWideNode), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    out->node_count = wide_total; out->stack_entries = root_words[1];
    const auto t3 = std::chrono::steady_clock::now();
    b.validate_ms = ms(t_validate, t0); b.upload_ms = ms(t0, t1); b.kernel_ms = ms(t1, t2); b.readback_ms = ms(t2, t3);
    if (std::getenv("HIPR_BVH_TIMING"))
        fprintf(stderr, "[hipr] %s: %u BVH2 nodes on %u levels, need %u, %u wide nodes on %u levels, %u stack entries: index walk %.3f ms, allocation + upload %.3f ms, kernels %.3f ms, read-back %.3f ms\n", who,
                node_count, bvh_levels, root_need, wide_total, wide_levels, root_words[1], b.validate_ms, b.upload_ms, b.kernel_ms, b.readback_ms);
    return HIPR_OK;
}

int hipr_debug_collapse4_times(HiprContext* c, double* out4_ms) {
    if (!c || !out4_ms) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_collapse4_times: null argument");
    out4_ms[0] = c->collapse4.validate_ms; out4_ms[1] = c->collapse4.upload_ms; out4_ms[2] = c->collapse4.kernel_ms; out4_ms[3] = c->collapse4.readback_ms;
    return HIPR_OK;
}

int hipr_rebuild_scene_trees(HiprContext* c, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t node_capacity, uint32_t* out_order, HiprSlot8* out_slots, uint32_t slot_capacity,
                             HiprSceneRebuildResult* out) {
    return rebuild_trees_on_the_device(c, "hipr_rebuild_scene_trees", nullptr, max_depth, out_nodes, node_capacity, out_order, out_slots, slot_capacity, out);
}

// Models added and removed on the device (instance_edit.h): the list checked on the host, then the rebuild's core over the new list.
int hipr_edit_scene_instances(HiprContext* c, const HiprInstanceEdit* edits, uint32_t edit_count, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t node_capacity, uint32_t* out_order,
                              uint32_t order_capacity, HiprSlot8* out_slots, uint32_t slot_capacity, HiprSceneEditResult* out) {
    const char* who = "hipr_edit_scene_instances";
    if (int st = check_context(c)) return st;
    const ResidentScene& r = c->scene;
    if (!r.ready && !r.awaits_rebuild) return fail(HIPR_ERROR_NOT_READY, "%s: no scene uploaded, or one a failed call left behind", who);
    if (!out) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null result", who);
    InstanceEdit plan;
    plan.order_capacity = order_capacity;
    if (int st = check_instance_edit(r, edits, edit_count, plan)) return st;
    if (edit_count == 0) return fail(HIPR_ERROR_UNSUPPORTED, "%s: an empty list; a scene without models is the host path's", who);
    HiprSceneRebuildResult trees = {};
    if (int st = rebuild_trees_on_the_device(c, who, &plan, max_depth, out_nodes, node_capacity, out_order, out_slots, slot_capacity, &trees)) return st;
    *out = {};
    out->triangle_count = plan.triangle_count; out->instance_count = edit_count;
    out->node_count = trees.node_count; out->deepest = trees.deepest; out->wide8 = trees.wide8; out->half_area = trees.half_area;
    return HIPR_OK;
}

// Not part of the public header: every refusal of hipr_append_scene_pools that is not a failed allocation, and nothing else -- no HIP call, the device and the
// books stay as they are. The group asks every member before any member writes.
int hipr_internal_check_pool_growth(HiprContext* c, const HiprPoolGrowth* g) {
    const char* who = "hipr_append_scene_pools";
    if (int st = check_context(c)) return st;
    const ResidentScene& r = c->scene;
    if (!r.ready && !r.awaits_rebuild) return fail(HIPR_ERROR_NOT_READY, "%s: no scene uploaded, or one a failed call left behind", who);
    if (!g) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null description", who);
    if ((g->vertex_count && !g->geometry) || (g->texcoord_vertices && !g->texcoords) || (g->tint_vertices && !g->tints) || (g->emission_vertices && !g->emissions) || (g->index_count && !g->indices) ||
        (g->segment_count && !g->segments) || (g->material_count && !g->materials) || (g->texture_count && !g->textures) || (g->texel_bytes && !g->texels))
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null array with a non-zero count", who);
    const uint64_t limit = 0xFFFFFFFFull, vertices = uint64_t(r.uploaded_vertex_count) + g->vertex_count;
    if (vertices > limit) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: %u + %u vertices do not fit 32 bits", who, r.uploaded_vertex_count, g->vertex_count);
    const struct { const char* name; uint32_t bit, covered; } attributes[3] = {{"texcoords", HIPR_MESH_TEXCOORDS, g->texcoord_vertices}, {"tints", HIPR_MESH_TINTS, g->tint_vertices},
                                                                               {"emissions", HIPR_MESH_EMISSIVE, g->emission_vertices}};
    for (const auto& a : attributes) {
        if (r.uploaded_mesh_attributes & a.bit) {
            if (a.covered != g->vertex_count)
                return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the %s pool is resident and takes its tail, %u entries; %u given", who, a.name, g->vertex_count, a.covered);
        } else if (a.covered != 0 && a.covered != vertices)
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the %s pool is not resident and comes whole, %llu entries, or not at all; %u given", who, a.name, (unsigned long long)vertices, a.covered);
    }
    if (g->segment_count && r.uploaded_index_count % 3u) return fail(HIPR_ERROR_UNSUPPORTED, "%s: the uploaded index pool of %u words is not one of whole triples", who, r.uploaded_index_count);
    uint64_t position = r.uploaded_index_count, from_host = 0;
    for (uint32_t k = 0; k < g->segment_count; ++k) {
        const HiprIndexSegment& s = g->segments[k];
        if (s.index_count % 3u) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: segment %u has %u index words, not whole triples", who, k, s.index_count);
        if (s.mirrored_from == HIPR_SEGMENT_FROM_HOST) from_host += s.index_count;
        else if (3ull * s.mirrored_from + s.index_count > position)
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: segment %u mirrors %u triples from triple %u on, the pool holds %llu there", who, k, s.index_count / 3u, s.mirrored_from, (unsigned long long)(position / 3u));
        position += s.index_count;
        if (position > limit) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the grown index pool does not fit 32 bits", who);
    }
    if (from_host != g->index_count) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the host segments take %llu index words, %u given", who, (unsigned long long)from_host, g->index_count);
    const uint64_t material_total = uint64_t(r.uploaded_materials.size()) + g->material_count, texture_total = uint64_t(r.uploaded_textures.size()) + g->texture_count;
    if (material_total > limit || texture_total > limit || g->texel_bytes > ~0ull - r.uploaded_texel_bytes) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the grown material, texture or texel pool does not fit its count", who);
    char invalid[256];
    for (uint32_t k = 0; k < g->texture_count; ++k)
        if (invalid_texture(g->textures[k], uint32_t(r.uploaded_textures.size()) + k, r.uploaded_texel_bytes + g->texel_bytes, invalid, sizeof(invalid))) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: %s", who, invalid);
    for (uint32_t k = 0; k < g->material_count; ++k)
        if (invalid_material(g->materials[k], uint32_t(r.uploaded_materials.size()) + k, uint32_t(texture_total), invalid, sizeof(invalid))) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: %s", who, invalid);
    return HIPR_OK;
}

// The resident pools grown at their tails (pool_growth.h): the description checked on the host, then ResidentScene::append_pools.
int hipr_append_scene_pools(HiprContext* c, const HiprPoolGrowth* g) {
    if (int st = hipr_internal_check_pool_growth(c, g)) return st;
    if (!g->vertex_count && !g->texcoord_vertices && !g->tint_vertices && !g->emission_vertices && !g->segment_count && !g->material_count && !g->texture_count && !g->texel_bytes) return HIPR_OK;
    if (int finish_status = finish_all(c)) return finish_status;      // no pending pass may go on over buffers that are about to move
    c->break_chain(c->stream);
    return c->scene.append_pools(*g, c->stream);
}

int hipr_debug_append_times(HiprContext* c, double* out3_ms) {
    if (!c || !out3_ms) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_append_times: null argument");
    for (int k = 0; k < 3; ++k) out3_ms[k] = c->scene.append_ms[k];
    return HIPR_OK;
}

// Not part of the public header: every refusal of hipr_update_scene_lighting that is not a failed allocation, and nothing else -- no HIP call, the device and the
// books stay as they are. The group asks every member before any member writes.
int hipr_internal_check_lighting_update(HiprContext* c, const HiprLight* lights, uint32_t light_count, int action, const HiprEnvironmentBuild* b, const float* out_per_pixel_PDF, uint64_t pdf_capacity,
                                        const HiprLightSample* out_samples, uint32_t sample_capacity, const HiprLightingResult* out) {
    const char* who = "hipr_update_scene_lighting";
    if (int st = check_context(c)) return st;
    const ResidentScene& r = c->scene;
    if (!r.ready && !r.awaits_rebuild) return fail(HIPR_ERROR_NOT_READY, "%s: no scene uploaded, or one a failed call left behind", who);
    if (!out) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null result", who);
    if (light_count && !lights) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null array with a non-zero count", who);
    if (light_count == 0xFFFFFFFFu) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the list with the environment's light does not fit 32 bits", who);
    for (uint32_t l = 0; l < light_count; ++l)
        if ((lights[l].flags & HIPR_LIGHT_TYPE_MASK) == HIPR_LIGHT_PRESAMPLED_ENVIRONMENT)
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: light %u is the environment's; the call appends it by itself", who, l);
    if (action != HIPR_ENVIRONMENT_KEEP && action != HIPR_ENVIRONMENT_REMOVE && action != HIPR_ENVIRONMENT_BUILD) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: unknown environment action %d", who, action);
    if ((action == HIPR_ENVIRONMENT_BUILD) != (b != nullptr)) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: HIPR_ENVIRONMENT_BUILD comes with a description, the other actions without", who);
    if (!b) return HIPR_OK;
    if (b->environment_map_ID <= 0 || size_t(b->environment_map_ID) >= r.uploaded_textures.size())
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: environment map %d of %zu resident textures (hipr_append_scene_pools brings a new one)", who, b->environment_map_ID, r.uploaded_textures.size());
    const HiprTexture& t = r.uploaded_textures[size_t(b->environment_map_ID)];
    if (b->pdf_height != std::max(t.height, ENV_MINIMUM_PDF_HEIGHT)) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: pdf_height is %u, a texture of %u rows takes %u", who, b->pdf_height, t.height, std::max(t.height, ENV_MINIMUM_PDF_HEIGHT));
    if (!b->row_sines || !b->draw_points) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null array with a non-zero count", who);
    if (t.is_sRGB && !b->srgb_decode) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: texture %d is sRGB and needs srgb_decode", who, b->environment_map_ID);
    if (!t.is_sRGB && b->srgb_decode) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: texture %d is linear; srgb_decode must be null", who, b->environment_map_ID);
    if (b->sample_count < 2u || (b->sample_count & (b->sample_count - 1u))) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: %u samples; a power of two >= 2 is needed", who, b->sample_count);
    for (size_t k = 0; k < size_t(b->sample_count) * 2; ++k)
        if (!(b->draw_points[k] >= 0.0f && b->draw_points[k] < 1.0f)) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: draw point %zu lies outside [0, 1)", who, k / 2);
    for (uint32_t y = 0; y < b->pdf_height; ++y)
        if (!std::isfinite(b->row_sines[y])) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: row_sines[%u] is not finite", who, y);
    for (uint32_t k = 0; b->srgb_decode && k < 256u; ++k)
        if (!std::isfinite(b->srgb_decode[k])) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: srgb_decode[%u] is not finite", who, k);
    const uint64_t texel_count = uint64_t(t.width) * b->pdf_height;
    if ((out_per_pixel_PDF && pdf_capacity < texel_count) || (out_samples && sample_capacity < b->sample_count))
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the outputs need room for %llu PDF texels and %u samples", who, (unsigned long long)texel_count, b->sample_count);
    if (t.format != HIPR_TEXEL_RGBA8 && t.format != HIPR_TEXEL_RGBA32F) return fail(HIPR_ERROR_UNSUPPORTED, "%s: only environments with 4 channels are supported (OptiXRenderer/Renderer.cpp:1141-1158)", who);
    if (t.is_sRGB && t.format == HIPR_TEXEL_RGBA32F) return fail(HIPR_ERROR_UNSUPPORTED, "%s: an sRGB texture of floats is decoded by pow per texel, which a table of bytes cannot serve; upload the scene instead", who);
    if (texel_count > (1ull << 30)) return fail(HIPR_ERROR_UNSUPPORTED, "%s: a PDF image of %llu texels is more than the kernels index", who, (unsigned long long)texel_count);
    return HIPR_OK;
}

// The lights and the environment of the resident scene replaced on the device (environment_build.h): the arguments checked on the host, then ResidentScene::update_lighting.
int hipr_update_scene_lighting(HiprContext* c, const HiprLight* lights, uint32_t light_count, int action, const HiprEnvironmentBuild* b, float* out_per_pixel_PDF, uint64_t pdf_capacity,
                               HiprLightSample* out_samples, uint32_t sample_capacity, HiprLightingResult* out) {
    if (int st = hipr_internal_check_lighting_update(c, lights, light_count, action, b, out_per_pixel_PDF, pdf_capacity, out_samples, sample_capacity, out)) return st;
    if (int finish_status = finish_all(c)) return finish_status;      // no pending pass may go on over buffers that are about to change hands
    c->break_chain(c->stream);
    ScratchGuard<LightingScratch> guard(c->lighting);
    return c->scene.update_lighting(lights, light_count, action, b, out_per_pixel_PDF, out_samples, c->lighting, c->stream, out);
}

int hipr_debug_lighting_times(HiprContext* c, double* out4_ms) {
    if (!c || !out4_ms) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_lighting_times: null argument");
    const LightingScratch& x = c->lighting;
    out4_ms[0] = x.upload_ms; out4_ms[1] = x.kernel_ms; out4_ms[2] = x.finish_ms; out4_ms[3] = x.readback_ms;
    return HIPR_OK;
}

// Not part of the public header: every refusal of hipr_update_scene_texels that is not a failed allocation, and nothing else -- no HIP call, the device and the
// books stay as they are. The group asks every member before any member writes.
int hipr_internal_check_texel_update(HiprContext* c, const HiprTexelEdit* edits, uint32_t edit_count, const HiprTexelUpdateResult* out) {
    const char* who = "hipr_update_scene_texels";
    if (int st = check_context(c)) return st;
    const ResidentScene& r = c->scene;
    if (!r.ready && !r.awaits_rebuild) return fail(HIPR_ERROR_NOT_READY, "%s: no scene uploaded, or one a failed call left behind", who);
    if (!out) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null result", who);
    if (edit_count && !edits) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null array with a non-zero count", who);
    for (uint32_t k = 0; k < edit_count; ++k) {
        const HiprTexelEdit& e = edits[k];
        if (!e.texels) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: edit %u has no texels", who, k);
        if (e.texture_index == 0 || e.texture_index >= r.uploaded_textures.size())
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: edit %u names texture %u of %zu resident textures (hipr_append_scene_pools brings a new one)", who, k, e.texture_index, r.uploaded_textures.size());
        const HiprTexture& t = r.uploaded_textures[e.texture_index];
        if (e.width == 0 || e.height == 0 || e.x >= t.width || e.y >= t.height || e.width > t.width - e.x || e.height > t.height - e.y)
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: edit %u is %u x %u texels at (%u, %u) of a texture of %u x %u", who, k, e.width, e.height, e.x, e.y, t.width, t.height);
        if (e.row_pitch_bytes < uint64_t(e.width) * hipr::texel_bytes_of(t.format))
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: edit %u has a pitch of %llu bytes, a row takes %llu", who, k, (unsigned long long)e.row_pitch_bytes, (unsigned long long)(uint64_t(e.width) * hipr::texel_bytes_of(t.format)));
    }
    // The exhaustive search's items pair triangles of equal flags (build_trace_items): there a flag that follows a texel changes a topology, which only the host builds.
    if (r.args.trace_item_count != 0)
        for (uint32_t k = 0; k < edit_count; ++k)
            for (const HiprMaterial& m : r.uploaded_materials)
                if (m.coverage_texture_ID > 0 && uint32_t(m.coverage_texture_ID) == edits[k].texture_index)
                    return fail(HIPR_ERROR_UNSUPPORTED, "%s: the uploaded scene carries the exhaustive search's items, which pair triangles by their flags, and texture %u is a material's coverage texture; upload the scene instead", who, edits[k].texture_index);
    return HIPR_OK;
}

// Pixel edits of resident images (texel_update.h): the rectangles checked on the host, then ResidentScene::update_texels.
int hipr_update_scene_texels(HiprContext* c, const HiprTexelEdit* edits, uint32_t edit_count, HiprTexelUpdateResult* out) {
    if (int st = hipr_internal_check_texel_update(c, edits, edit_count, out)) return st;
    if (!edit_count) { *out = {0u, 0u, c->scene.all_triangles_opaque ? 1u : 0u, 0u}; return HIPR_OK; }
    if (int finish_status = finish_all(c)) return finish_status;      // no pending pass may go on over texels and flags that are about to change
    c->break_chain(c->stream);
    ScratchGuard<TexelScratch> guard(c->texel_update);
    return c->scene.update_texels(edits, edit_count, c->texel_update, c->stream, out);
}

int hipr_debug_texel_update_times(HiprContext* c, double* out4_ms) {
    if (!c || !out4_ms) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_texel_update_times: null argument");
    const TexelScratch& x = c->texel_update;
    out4_ms[0] = x.staging_ms; out4_ms[1] = x.write_ms; out4_ms[2] = x.coverage_ms; out4_ms[3] = x.leaf_ms;
    return HIPR_OK;
}

// Not part of the public header: every refusal of hipr_update_scene_vertices that is not a failed allocation, and nothing else -- no HIP call, the device and the
// books stay as they are. The group asks every member before any member writes.
int hipr_internal_check_vertex_update(HiprContext* c, const HiprVertexEdit* edits, uint32_t edit_count, const HiprVertexUpdateResult* out) {
    const char* who = "hipr_update_scene_vertices";
    if (int st = check_context(c)) return st;
    const ResidentScene& r = c->scene;
    if (!r.ready) return fail(HIPR_ERROR_NOT_READY, "%s: no scene uploaded, one a failed call left behind, or one that awaits hipr_rebuild_scene_trees", who);
    if (!out) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null result", who);
    if (edit_count && !edits) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null array with a non-zero count", who);
    for (uint32_t k = 0; k < edit_count; ++k) {
        const HiprVertexEdit& e = edits[k];
        if (e.vertex_count == 0) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: edit %u has no vertices", who, k);
        if (!e.geometry && !e.texcoords && !e.tints && !e.emissions) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: edit %u carries no attribute", who, k);
        if (uint64_t(e.first_vertex) + e.vertex_count > r.uploaded_vertex_count)
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: edit %u is %u vertices from %u on, the resident pools hold %u", who, k, e.vertex_count, e.first_vertex, r.uploaded_vertex_count);
        if ((e.texcoords && !(r.uploaded_mesh_attributes & HIPR_MESH_TEXCOORDS)) || (e.tints && !(r.uploaded_mesh_attributes & HIPR_MESH_TINTS)) ||
            (e.emissions && !(r.uploaded_mesh_attributes & HIPR_MESH_EMISSIVE)))
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: edit %u carries an attribute whose pool the device does not hold (hipr_append_scene_pools brings one)", who, k);
        for (uint32_t v = 0; v < e.vertex_count; ++v) {
            if (e.geometry && !(std::isfinite(e.geometry[v].position[0]) && std::isfinite(e.geometry[v].position[1]) && std::isfinite(e.geometry[v].position[2])))
                return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: edit %u: the position of vertex %u is not finite", who, k, e.first_vertex + v);
            if (e.texcoords && !(std::isfinite(e.texcoords[2 * size_t(v)]) && std::isfinite(e.texcoords[2 * size_t(v) + 1])))
                return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: edit %u: the texture coordinate of vertex %u is not finite", who, k, e.first_vertex + v);
        }
    }
    // what hipr_refit_scene_transforms refuses: the arrays another search walks are the ones this call leaves stale, and the exhaustive search's items are built on the host
    if (r.wide8.slot_count == 0 || !c->use_wide8() || r.args.trace_item_count != 0 || r.args.triangle_count > 0x55555555u)
        return fail(HIPR_ERROR_UNSUPPORTED, "%s: the uploaded scene is not traced through the 8-wide tree; edit on the host and upload the scene instead", who);
    return HIPR_OK;
}

// Vertex edits of resident meshes (vertex_update.h): the ranges checked on the host, then ResidentScene::update_vertices.
int hipr_update_scene_vertices(HiprContext* c, const HiprVertexEdit* edits, uint32_t edit_count, HiprVertexUpdateResult* out) {
    if (int st = hipr_internal_check_vertex_update(c, edits, edit_count, out)) return st;
    if (!edit_count) {
        const ResidentScene& r = c->scene;
        out->refit.needs_rebuild = 0; out->refit.child_half_area = r.current_half_area; out->refit.uploaded_half_area = r.uploaded_half_area;
        for (int a = 0; a < 3; ++a) { out->refit.grid_min[a] = r.wide8.grid_min[a]; out->refit.grid_cell[a] = r.wide8.grid_cell[a]; }
        out->moved_triangles = out->candidate_triangles = out->changed_triangles = 0u;
        out->all_triangles_opaque = r.all_triangles_opaque ? 1u : 0u;
        return HIPR_OK;
    }
    if (int finish_status = finish_all(c)) return finish_status;      // no pending pass may go on over vertices and triangles that are about to change
    c->break_chain(c->stream);
    ScratchGuard<VertexScratch> guard(c->vertex_update);
    return c->scene.update_vertices(edits, edit_count, c->vertex_update, c->stream, out);
}

int hipr_debug_vertex_update_times(HiprContext* c, double* out4_ms) {
    if (!c || !out4_ms) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_vertex_update_times: null argument");
    const VertexScratch& x = c->vertex_update;
    out4_ms[0] = x.staging_ms; out4_ms[1] = x.write_ms; out4_ms[2] = x.refit_ms; out4_ms[3] = x.flag_ms;
    return HIPR_OK;
}

// Not part of the public header: every refusal of hipr_set_scene_rigs that is not a failed allocation, and nothing else -- no HIP call. The group asks every member
// before any member writes.
int hipr_internal_check_scene_rigs(HiprContext* c, const HiprRigDesc* rigs, uint32_t count) {
    const char* who = "hipr_set_scene_rigs";
    if (int st = check_context(c)) return st;
    const ResidentScene& r = c->scene;
    if (!r.ready) return fail(HIPR_ERROR_NOT_READY, "%s: no scene uploaded, one a failed call left behind, or one that awaits hipr_rebuild_scene_trees", who);
    if (const char* why = check_rig_descs(rigs, count, r.uploaded_vertex_count)) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: %s", who, why);
    return HIPR_OK;
}

// The resident rig set replaced (vertex_pose.h): checked on the host, then ResidentScene::set_rigs.
int hipr_set_scene_rigs(HiprContext* c, const HiprRigDesc* rigs, uint32_t count) {
    if (int st = hipr_internal_check_scene_rigs(c, rigs, count)) return st;
    if (int finish_status = finish_all(c)) return finish_status;
    return c->scene.set_rigs(rigs, count, c->stream);
}

// ... and every refusal of hipr_pose_scene_rigs that is not a failed allocation.
int hipr_internal_check_rig_poses(HiprContext* c, const HiprRigPose* poses, uint32_t pose_count, const HiprVertexUpdateResult* out) {
    const char* who = "hipr_pose_scene_rigs";
    if (int st = check_context(c)) return st;
    const ResidentScene& r = c->scene;
    if (!r.ready) return fail(HIPR_ERROR_NOT_READY, "%s: no scene uploaded, one a failed call left behind, or one that awaits hipr_rebuild_scene_trees", who);
    if (!out) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null result", who);
    if (const char* why = check_rig_poses(poses, pose_count, r.rigs.data(), r.rigs.size())) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: %s", who, why);
    // what hipr_refit_scene_transforms refuses, as hipr_update_scene_vertices
    if (r.wide8.slot_count == 0 || !c->use_wide8() || r.args.trace_item_count != 0 || r.args.triangle_count > 0x55555555u)
        return fail(HIPR_ERROR_UNSUPPORTED, "%s: the uploaded scene is not traced through the 8-wide tree; pose on the host and upload the scene instead", who);
    return HIPR_OK;
}

// Bound rigs posed on the device (vertex_pose.h): the poses checked on the host, then ResidentScene::pose_rigs.
int hipr_pose_scene_rigs(HiprContext* c, const HiprRigPose* poses, uint32_t pose_count, HiprVertexUpdateResult* out) {
    if (int st = hipr_internal_check_rig_poses(c, poses, pose_count, out)) return st;
    if (!pose_count) return hipr_update_scene_vertices(c, nullptr, 0, out);      // what is resident
    if (int finish_status = finish_all(c)) return finish_status;      // no pending pass may go on over vertices and triangles that are about to change
    c->break_chain(c->stream);
    ScratchGuard<PoseScratch> guard(c->vertex_pose);
    ScratchGuard<VertexScratch> marks_guard(c->vertex_update);
    return c->scene.pose_rigs(poses, pose_count, c->vertex_pose, c->vertex_update, c->stream, out);
}

int hipr_debug_vertex_pose_times(HiprContext* c, double* out4_ms) {
    if (!c || !out4_ms) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_vertex_pose_times: null argument");
    const PoseScratch& x = c->vertex_pose;
    out4_ms[0] = x.staging_ms; out4_ms[1] = x.pose_ms; out4_ms[2] = x.refit_ms; out4_ms[3] = 0.0;
    return HIPR_OK;
}

int hipr_debug_set_pose_lds_joints(HiprContext* c, uint32_t joints) {
    if (int st = check_context(c)) return st;
    if (joints > POSE_LDS_CAPACITY) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_set_pose_lds_joints: the kernel's LDS holds %u joints", POSE_LDS_CAPACITY);
    c->scene.pose_lds_joints = joints;
    return HIPR_OK;
}

int hipr_debug_rebuild_times(HiprContext* c, double* out5_ms) {
    if (!c || !out5_ms) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_rebuild_times: null argument");
    const RebuildScratch& x = c->rebuild;
    out5_ms[0] = x.flatten_ms; out5_ms[1] = x.bvh2_ms; out5_ms[2] = x.collapse_ms; out5_ms[3] = x.install_ms; out5_ms[4] = x.readback_ms;
    return HIPR_OK;
}

// Where the device holds scene array `which`, and how many bytes of it the scene's counts make readable; false for an unknown array.
static bool scene_buffer(const ResidentScene& r, int which, const void*& from, uint64_t& bytes) {
    const uint64_t triangles = r.args.triangle_count, vertices = r.uploaded_vertex_count;
    auto attribute = [&](const DeviceBuffer& pool, uint32_t bit, uint64_t stride) { from = pool.ptr; bytes = r.uploaded_mesh_attributes & bit ? vertices * stride : 0u; };      // an absent pool: zero bytes
    if (which == HIPR_SCENE_BUFFER_TRIANGLES) { from = r.triangles.ptr; bytes = triangles * sizeof(HiprTriangle); }
    else if (which == HIPR_SCENE_BUFFER_WIDE8_SLOTS) { from = r.wide8_slots.ptr; bytes = uint64_t(r.wide8.slot_count) * sizeof(HiprSlot8); }
    else if (which == HIPR_SCENE_BUFFER_TRACE_TRIANGLES) { from = r.trace_triangles.ptr; bytes = triangles * 3 * sizeof(float4); }
    else if (which == HIPR_SCENE_BUFFER_SHADE_TRIANGLES) { from = r.shade_triangles.ptr; bytes = triangles * SHADE_TRIANGLE_QUADS * sizeof(float4); }
    else if (which == HIPR_SCENE_BUFFER_TRIANGLE_CLASS) { from = r.triangle_class.ptr; bytes = triangles; }
    else if (which == HIPR_SCENE_BUFFER_MATERIALS) { from = r.materials.ptr; bytes = uint64_t(r.uploaded_materials.size()) * sizeof(HiprMaterial); }
    else if (which == HIPR_SCENE_BUFFER_INSTANCES) { from = r.instances.ptr; bytes = uint64_t(r.uploaded_instances.size()) * sizeof(HiprInstance); }
    else if (which == HIPR_SCENE_BUFFER_NODES) { from = r.nodes.ptr; bytes = uint64_t(r.args.node_count) * sizeof(HiprBvhNode); }
    else if (which == HIPR_SCENE_BUFFER_INDICES) { from = r.indices.ptr; bytes = uint64_t(r.uploaded_index_count) * 4; }
    else if (which == HIPR_SCENE_BUFFER_GEOMETRY) { from = r.geometry.ptr; bytes = vertices * sizeof(HiprVertexGeometry); }
    else if (which == HIPR_SCENE_BUFFER_TEXCOORDS) attribute(r.texcoords, HIPR_MESH_TEXCOORDS, 8);
    else if (which == HIPR_SCENE_BUFFER_TINTS) attribute(r.tints, HIPR_MESH_TINTS, 4);
    else if (which == HIPR_SCENE_BUFFER_EMISSIONS) attribute(r.emissions, HIPR_MESH_EMISSIVE, 12);
    else if (which == HIPR_SCENE_BUFFER_TEXTURES) { from = r.textures.ptr; bytes = uint64_t(r.uploaded_textures.size()) * sizeof(HiprTexture); }
    else if (which == HIPR_SCENE_BUFFER_TEXELS) { from = r.texels.ptr; bytes = r.uploaded_texel_bytes; }
    else if (which == HIPR_SCENE_BUFFER_LIGHTS) { from = r.lights.ptr; bytes = uint64_t(r.args.light_count) * sizeof(HiprLight); }
    else if (which == HIPR_SCENE_BUFFER_ENVIRONMENT_PDF) { from = r.environment_PDF.ptr; bytes = r.uploaded_environment ? uint64_t(r.args.env_pdf_width) * r.args.env_pdf_height * sizeof(float) : 0u; }
    else if (which == HIPR_SCENE_BUFFER_ENVIRONMENT_SAMPLES) { from = r.environment_samples.ptr; bytes = r.uploaded_environment ? uint64_t(r.args.env_sample_count) * sizeof(HiprLightSample) : 0u; }
    else return false;
    return true;
}

int hipr_debug_read_scene_buffer(HiprContext* c, int which, void* out, uint64_t capacity_bytes) {
    if (int st = check_context(c)) return st;
    if (!out) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_read_scene_buffer: null output");
    if (c->scene.args.triangle_count == 0 && c->scene.wide8.slot_count == 0) return fail(HIPR_ERROR_NOT_READY, "hipr_debug_read_scene_buffer: no scene uploaded");
    const void* from = nullptr;
    uint64_t bytes = 0;
    if (!scene_buffer(c->scene, which, from, bytes)) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_read_scene_buffer: unknown buffer %d", which);
    if (capacity_bytes < bytes) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_read_scene_buffer: %llu bytes needed, %llu given", (unsigned long long)bytes, (unsigned long long)capacity_bytes);
    if (int finish_status = finish_all(c)) return finish_status;
    if (bytes) HIP_TRY(hipMemcpy(out, from, bytes, hipMemcpyDeviceToHost));
    return HIPR_OK;
}

int hipr_debug_scene_buffer_bytes(HiprContext* c, int which, uint64_t* out_bytes) {
    if (int st = check_context(c)) return st;
    if (!out_bytes) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_scene_buffer_bytes: null output");
    if (c->scene.args.triangle_count == 0 && c->scene.wide8.slot_count == 0) return fail(HIPR_ERROR_NOT_READY, "hipr_debug_scene_buffer_bytes: no scene uploaded");
    const void* from = nullptr;
    if (!scene_buffer(c->scene, which, from, *out_bytes)) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_scene_buffer_bytes: unknown buffer %d", which);
    return HIPR_OK;
}

} // extern "C"
