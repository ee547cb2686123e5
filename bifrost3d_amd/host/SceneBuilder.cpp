// host/SceneBuilder.cpp -- see SceneBuilder.h.
#include "SceneBuilder.h"

#include "../csrc/material_rules.h"      // the flag rules, shared with the kernels that apply a material edit on the device
#include "RNG.h"                         // the draw points of staged_environment_build

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cmath>
#include <cstring>

namespace HIPRenderer {

SceneBuilder::SceneBuilder() {
    // Slot 0 holds the invalid material / "no texture", as in the reference where per-ID arrays are
    // sized capacity() and index 0 is the invalid sentinel (OptiXRenderer/Renderer.cpp:821, :528-562).
    HiprMaterial invalid = {};
    m_materials.push_back(invalid);
    HiprTexture none = {};
    m_textures.push_back(none);
    m_state.next_event_sample_count = 3;   // Renderer.cpp:479
}

uint16_t SceneBuilder::unorm16(float v) {
    v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
    return (uint16_t)(v * 65535.0f + 0.5f);
}

HiprMaterial SceneBuilder::make_material(RGB tint, float roughness, float specularity, float metallic, uint16_t flags, uint16_t shading_model) {
    HiprMaterial m = {};
    m.flags = flags;
    m.shading_model = shading_model;
    m.tint[0] = tint.r; m.tint[1] = tint.g; m.tint[2] = tint.b;
    m.roughness = roughness;
    m.specularity = specularity;
    m.metallic = metallic;
    m.coverage = 1.0f;
    return m;
}

HiprLight SceneBuilder::sphere_light(Vector3f position, RGB power, float radius) {
    HiprLight l = {};
    l.flags = HIPR_LIGHT_SPHERE;
    l.data[0] = power.r; l.data[1] = power.g; l.data[2] = power.b;
    l.data[3] = position.x; l.data[4] = position.y; l.data[5] = position.z;
    l.data[6] = radius;
    return l;
}

HiprLight SceneBuilder::spot_light(Vector3f position, Vector3f direction, RGB power, float radius, float cos_angle) {
    HiprLight l = sphere_light(position, power, radius);
    l.flags = HIPR_LIGHT_SPOT;
    l.data[7] = direction.x; l.data[8] = direction.y; l.data[9] = direction.z;
    l.data[10] = cos_angle;
    return l;
}

HiprLight SceneBuilder::directional_light(Vector3f direction, RGB radiance) {
    HiprLight l = {};
    l.flags = HIPR_LIGHT_DIRECTIONAL;
    l.data[0] = radiance.r; l.data[1] = radiance.g; l.data[2] = radiance.b;
    l.data[3] = direction.x; l.data[4] = direction.y; l.data[5] = direction.z;
    return l;
}

uint32_t SceneBuilder::add_mesh(MeshData mesh) {
    // load_mesh, OptiXRenderer/Renderer.cpp:92-136
    MeshRecord r;
    r.index_offset = uint32_t(m_indices.size() / 3);
    r.vertex_offset = uint32_t(m_geometry.size());
    r.primitive_count = uint32_t(mesh.primitives.size());
    r.vertex_count = uint32_t(mesh.positions.size());
    r.flags = 0;
    if (!mesh.normals.empty()) r.flags |= HIPR_MESH_NORMALS;
    if (!mesh.texcoords.empty()) r.flags |= HIPR_MESH_TEXCOORDS;
    if (!mesh.tints.empty()) r.flags |= HIPR_MESH_TINTS;
    if (!mesh.emission.empty()) r.flags |= HIPR_MESH_EMISSIVE;

    for (const Vector3ui& p : mesh.primitives) { m_indices.push_back(p.x); m_indices.push_back(p.y); m_indices.push_back(p.z); }
    m_index_log.push_back({HIPR_SEGMENT_FROM_HOST, 3u * r.primitive_count});
    for (uint32_t i = 0; i < r.vertex_count; ++i) {
        m_geometry.push_back(vertex_geometry(mesh.positions[i], (r.flags & HIPR_MESH_NORMALS) ? &mesh.normals[i] : nullptr));
        Vector2f tc = (r.flags & HIPR_MESH_TEXCOORDS) ? mesh.texcoords[i] : Vector2f{0, 0};
        m_texcoords.push_back(tc.x); m_texcoords.push_back(tc.y);
        m_tints.push_back((r.flags & HIPR_MESH_TINTS) ? mesh.tints[i] : 0xFFFFFFFFu);
        Vector3f em = (r.flags & HIPR_MESH_EMISSIVE) ? mesh.emission[i] : Vector3f(0, 0, 0);
        m_emissions.push_back(em.x); m_emissions.push_back(em.y); m_emissions.push_back(em.z);
    }
    m_any_texcoords |= (r.flags & HIPR_MESH_TEXCOORDS) != 0;
    m_any_tints |= (r.flags & HIPR_MESH_TINTS) != 0;
    m_any_emission |= (r.flags & HIPR_MESH_EMISSIVE) != 0;
    m_meshes.push_back(r);
    m_pools_grew = true;
    return uint32_t(m_meshes.size() - 1);
}

HiprVertexGeometry SceneBuilder::vertex_geometry(Vector3f position, const Vector3f* normal) {
    HiprVertexGeometry g = {};
    g.position[0] = position.x; g.position[1] = position.y; g.position[2] = position.z;
    if (normal) {
        OctahedralNormal e = OctahedralNormal::encode_precise(*normal);
        g.oct_normal[0] = e.encoding.x; g.oct_normal[1] = e.encoding.y;
    }
    return g;
}

bool SceneBuilder::mesh_range(uint32_t mesh, uint32_t (&out)[5]) const {
    if (mesh >= m_meshes.size()) return false;
    const MeshRecord& r = m_meshes[mesh];
    out[0] = r.vertex_offset; out[1] = r.vertex_count; out[2] = r.index_offset; out[3] = r.primitive_count; out[4] = r.flags;
    return true;
}

uint32_t SceneBuilder::add_material(const HiprMaterial& material) {
    m_materials.push_back(material);
    m_pools_grew = true;
    return uint32_t(m_materials.size() - 1);
}

uint32_t SceneBuilder::add_texture(const ImageData& image, bool repeat_u, bool repeat_v, bool linear_mag, bool linear_min) {
    HiprTexture t = {};
    t.width = image.width; t.height = image.height;
    while (m_texels.size() % 16) m_texels.push_back(0);
    t.texel_offset = uint64_t(m_texels.size());
    t.format = image.format;
    t.wrap_u = repeat_u; t.wrap_v = repeat_v;
    t.filter = uint8_t((linear_mag ? 1 : 0) | (linear_min ? 2 : 0));
    t.is_sRGB = image.is_sRGB;
    m_texels.insert(m_texels.end(), image.pixels.begin(), image.pixels.end());
    m_textures.push_back(t);
    m_pools_grew = true;
    return uint32_t(m_textures.size() - 1);
}

static bool mirrors(const float* M) {
    const double det = double(M[0]) * (double(M[5]) * M[10] - double(M[6]) * M[9]) - double(M[1]) * (double(M[4]) * M[10] - double(M[6]) * M[8]) +
                       double(M[2]) * (double(M[4]) * M[9] - double(M[5]) * M[8]);
    return det < 0.0;
}

uint32_t SceneBuilder::index_offset_for(uint32_t mesh, const float* object_to_world) {
    MeshRecord& r = m_meshes[mesh];
    if (!mirrors(object_to_world)) return r.index_offset;
    if (r.mirrored_index_offset == 0xFFFFFFFFu) {
        r.mirrored_index_offset = uint32_t(m_indices.size() / 3);
        m_pools_grew = true;
        m_index_log.push_back({r.index_offset, 3u * r.primitive_count});
        for (uint32_t p = 0; p < r.primitive_count; ++p) {
            const size_t at = 3 * size_t(r.index_offset + p);
            const uint32_t a = m_indices[at], b = m_indices[at + 1], c = m_indices[at + 2];
            m_indices.push_back(a); m_indices.push_back(c); m_indices.push_back(b);
        }
    }
    return r.mirrored_index_offset;
}

uint32_t SceneBuilder::add_model(uint32_t mesh, uint32_t material, const Transform& transform, uint32_t explicit_model_index) {
    return insert_model(uint32_t(m_instances.size()), mesh, material, transform, explicit_model_index);
}

// An edit of the instance list of a built scene leaves the triangles and the trees behind, as a staged transform does.
void SceneBuilder::note_instance_edit() {
    if (!m_built) return;
    m_staged = true;
    // a move staged before the edit is marked by the old list's indices: from here on only a rebuild sorts it out, which is what m_staged_flips asks for
    m_staged_flips = m_staged_flips || std::find(m_staged_moved.begin(), m_staged_moved.end(), true) != m_staged_moved.end();
    m_staged_moved.assign(m_instances.size(), false);
}

bool SceneBuilder::has_staged_edits() const {
    if (!m_built) return false;
    if (m_built_index.size() != m_built_instance_count) return true;
    for (size_t i = 0; i < m_built_index.size(); ++i)
        if (m_built_index[i] != i) return true;
    return false;
}

bool SceneBuilder::remove_model(uint32_t model_index) {
    bool found = false;
    for (size_t i = m_instances.size(); i-- > 0;)
        if (uint32_t(m_instances[i].instance_id) == ((1u << 30) | model_index)) {
            m_instances.erase(m_instances.begin() + ptrdiff_t(i));
            m_instance_mesh.erase(m_instance_mesh.begin() + ptrdiff_t(i));
            m_built_index.erase(m_built_index.begin() + ptrdiff_t(i));
            found = true;
        }
    if (found) note_instance_edit();
    return found;
}

bool SceneBuilder::model_info(uint32_t model_index, uint32_t& mesh, uint32_t& material, uint32_t& position) const {
    for (size_t i = 0; i < m_instances.size(); ++i)
        if (uint32_t(m_instances[i].instance_id) == ((1u << 30) | model_index)) {
            mesh = m_instance_mesh[i]; material = uint32_t(m_instances[i].material_index); position = uint32_t(i);
            return true;
        }
    return false;
}

uint32_t SceneBuilder::insert_model(uint32_t position, uint32_t mesh, uint32_t material, const Transform& transform, uint32_t explicit_model_index) {
    // create_model + transformable_model, OptiXRenderer/Renderer.cpp:138-182
    const MeshRecord& r = m_meshes[mesh];
    HiprInstance inst = {};
    Matrix3x4f m = to_matrix3x4(transform);
    std::memcpy(inst.object_to_world, m.begin(), sizeof(inst.object_to_world));
    const uint32_t vertex_offset = r.vertex_offset, mesh_flags = r.flags;      // `r` may move: the mirrored copy grows m_indices only, but keep to values
    inst.index_offset = index_offset_for(mesh, inst.object_to_world);
    inst.vertex_offset = vertex_offset;
    const uint32_t model_index = explicit_model_index ? explicit_model_index : uint32_t(m_instances.size()) + 1;   // UID index, 0 is invalid
    inst.instance_id = int32_t((1u << 30) | model_index);                 // InstanceID::make(MeshModel, index)
    inst.material_index = int32_t(material);
    inst.mesh_flags = mesh_flags;
    const size_t at = std::min<size_t>(position, m_instances.size());
    m_instances.insert(m_instances.begin() + ptrdiff_t(at), inst);
    m_instance_mesh.insert(m_instance_mesh.begin() + ptrdiff_t(at), mesh);
    m_built_index.insert(m_built_index.begin() + ptrdiff_t(at), NOT_BUILT);
    note_instance_edit();
    return model_index;
}

void SceneBuilder::add_light(const HiprLight& light) { m_lights.push_back(light); }

void SceneBuilder::set_environment(uint32_t texture_index, uint32_t pdf_width, uint32_t pdf_height, std::vector<float> per_pixel_PDF, std::vector<HiprLightSample> samples) {
    m_environment_PDF = std::move(per_pixel_PDF);
    m_environment_samples = std::move(samples);
    m_environment = {int32_t(texture_index), pdf_width, pdf_height, nullptr, nullptr, uint32_t(m_environment_samples.size())};
    m_has_environment = true;
    m_environment_set_since = m_built;
    m_environment_texels_edited = false;
    if (m_environment_samples.size() > 1) {   // next_event_estimation_possible (PresampledEnvironmentMap.h:64)
        HiprLight light = {};
        light.flags = HIPR_LIGHT_PRESAMPLED_ENVIRONMENT;
        m_lights.push_back(light);
    }
}

void SceneBuilder::force_shading_model(uint16_t shading_model) {
    for (size_t i = 1; i < m_materials.size(); ++i) m_materials[i].shading_model = shading_model;
}

// The world-space triangles of one instance, primitives in order, appended to `world`; m_bounds grows with them.
void SceneBuilder::flatten_instance(uint32_t i, std::vector<HiprTriangle>& world) {
    const HiprInstance& inst = m_instances[i];
    const MeshRecord& mesh = m_meshes[m_instance_mesh[i]];
    const float* M = inst.object_to_world;
    const HiprMaterial& material = m_materials[inst.material_index];
    auto to_world = [&](uint32_t v, float* out) {
        const float* p = m_geometry[mesh.vertex_offset + v].position;
        for (int r = 0; r < 3; ++r) out[r] = M[4 * r] * p[0] + M[4 * r + 1] * p[1] + M[4 * r + 2] * p[2] + M[4 * r + 3];
        m_bounds.grow_to_contain(Vector3f(out[0], out[1], out[2]));
    };
    for (uint32_t p = 0; p < mesh.primitive_count; ++p) {
        const uint32_t* idx = &m_indices[3 * size_t(inst.index_offset + p)];      // the instance's triples: mirrored instances have their own
        HiprTriangle t = {};
        to_world(idx[0], t.v0); to_world(idx[1], t.v1); to_world(idx[2], t.v2);
        t.instance_index = i;
        t.primitive_index = p;
        // covered_everywhere: a triangle of a material that is not statically opaque may still be
        t.flags = hipr::triangle_flags(material, inst, p, m_indices.data(), m_texcoords.data(), m_textures.data(), uint32_t(m_textures.size()), m_texels.data());
        world.push_back(t);
    }
}

void SceneBuilder::finalize(uint32_t bvh_max_depth) {
    const auto t_start = std::chrono::steady_clock::now();
    std::vector<HiprTriangle> world;
    m_bounds = AABB::invalid();
    for (uint32_t i = 0; i < m_instances.size(); ++i) flatten_instance(i, world);

    m_bvh_max_depth_limit = bvh_max_depth;
    const auto t_flat = std::chrono::steady_clock::now();
    Bvh2SourceReport report;      // fall_back: a scene builder's build carries on with the host's stage
    Wide8SourceReport wide8_report;
    build_trees_over(world, m_bvh2_source, report, m_wide8_source, wide8_report);
    if (report.used) ++m_build_counts.device_builds; else if (report.asked) ++m_build_counts.declined_builds;
    if (wide8_report.used) ++m_collapse_counts.device_collapses; else if (wide8_report.asked) ++m_collapse_counts.declined_collapses;
    if (std::getenv("HIPR_BVH_TIMING"))
        fprintf(stderr, "[hipr] finalize: %zu triangles: flatten %.3f s, build_bvh %.3f s (BVH2 source: %s, %.3f s)\n", world.size(), std::chrono::duration<double>(t_flat - t_start).count(),
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t_flat).count(), report.used ? "used" : (report.asked ? "declined" : "none"), report.seconds);
}

// The trees over the triangles in flatten order, the triangles in the trees' order and the description: what finalize() does after its flatten, and what
// adopt_rebuilt_trees() does with sources that hand back the trees it was given.
void SceneBuilder::build_trees_over(const std::vector<HiprTriangle>& world, const Bvh2Source& bvh2_source, Bvh2SourceReport& report, const Wide8Source& wide8_source, Wide8SourceReport& wide8_report) {
    Wide4SourceReport wide4_report;
    m_bvh = build_bvh(world, m_bvh_max_depth_limit, bvh2_source, &report, wide8_source, &wide8_report, m_wide4_source, &wide4_report);
    if (wide4_report.used) ++m_wide4_collapse_counts.device_collapses; else if (wide4_report.asked) ++m_wide4_collapse_counts.declined_collapses;
    m_built_bvh_area = bvh_child_area(m_bvh);
    m_triangles.resize(world.size());
    for (size_t k = 0; k < world.size(); ++k) m_triangles[k] = world[m_bvh.order[k]];
    m_built = true; m_pools_grew = false;      // the triangles and the trees are those of the instance list and the pools as they stand
    m_built_instance_count = uint32_t(m_instances.size());
    m_built_pools = {m_indices.size(), m_geometry.size(), m_materials.size(), m_textures.size(), m_texels.size(), m_lights.size(), m_any_texcoords, m_any_tints, m_any_emission};
    m_index_log.clear();
    m_environment_set_since = false;
    m_built_index.resize(m_instances.size());
    for (size_t i = 0; i < m_built_index.size(); ++i) m_built_index[i] = uint32_t(i);

    HiprSceneDesc& d = m_desc;
    d = {};
    d.nodes = m_bvh.nodes.data(); d.node_count = uint32_t(m_bvh.nodes.size());
    d.triangles = m_triangles.data(); d.triangle_count = uint32_t(m_triangles.size());
    d.instances = m_instances.data(); d.instance_count = uint32_t(m_instances.size());
    d.indices = m_indices.data(); d.index_count = uint32_t(m_indices.size());
    d.geometry = m_geometry.data(); d.vertex_count = uint32_t(m_geometry.size());
    d.texcoords = m_any_texcoords ? m_texcoords.data() : nullptr;
    d.tints = m_any_tints ? m_tints.data() : nullptr;
    d.emissions = m_any_emission ? m_emissions.data() : nullptr;
    d.materials = m_materials.data(); d.material_count = uint32_t(m_materials.size());
    d.lights = m_lights.data(); d.light_count = uint32_t(m_lights.size());
    d.textures = m_textures.data(); d.texture_count = uint32_t(m_textures.size());
    d.texels = m_texels.data(); d.texel_bytes = uint64_t(m_texels.size());
    d.bvh_max_depth = m_bvh.max_depth;
    d.wide_nodes = m_bvh.wide_nodes.data(); d.wide_node_count = uint32_t(m_bvh.wide_nodes.size());
    d.wide_stack_entries = m_bvh.wide_stack_entries;
    d.wide8_slots = m_bvh.wide8.slots.data(); d.wide8_slot_count = uint32_t(m_bvh.wide8.slots.size()); d.wide8_height = m_bvh.wide8.height;
    for (int a = 0; a < 3; ++a) { d.wide8_grid_min[a] = m_bvh.wide8.grid_min[a]; d.wide8_grid_cell[a] = m_bvh.wide8.grid_cell[a]; }
    m_environment.per_pixel_PDF = m_environment_PDF.data();
    m_environment.samples = m_environment_samples.data();
    d.environment = m_has_environment ? &m_environment : nullptr;
}

bool SceneBuilder::record_model_transforms(const std::vector<std::pair<uint32_t, Transform>>& model_transforms, std::vector<HiprInstanceTransform>* moved_instances) {
    if (m_staged_moved.size() != m_instances.size()) m_staged_moved.assign(m_instances.size(), false);
    // Decided before anything is touched: does an update turn an instance inside out? Such an instance is drawn from its own index triples (two corners
    // exchanged, index_offset_for), so the triangle array is rebuilt from the instances -- with EVERY update of the batch applied first; the caller is told
    // "rebuilt" (false) and uploads a desc() that carries all the new poses.
    bool flips = false;
    for (const auto& update : model_transforms)
        for (size_t i = 0; i < m_instances.size(); ++i)
            if (uint32_t(m_instances[i].instance_id) == ((1u << 30) | update.first)) {
                Matrix3x4f m = to_matrix3x4(update.second);
                flips = flips || mirrors(m.begin()) != mirrors(m_instances[i].object_to_world);
                std::memcpy(m_instances[i].object_to_world, m.begin(), sizeof(m_instances[i].object_to_world));
                m_staged_moved[i] = true;
                if (moved_instances) {
                    HiprInstanceTransform t = {};
                    t.instance_index = uint32_t(i);
                    std::memcpy(t.object_to_world, m.begin(), sizeof(t.object_to_world));
                    moved_instances->push_back(t);
                }
            }
    m_staged_flips = m_staged_flips || flips;
    return !flips;
}

bool SceneBuilder::stage_model_transforms(const std::vector<std::pair<uint32_t, Transform>>& model_transforms, std::vector<HiprInstanceTransform>& moved_instances) {
    const size_t before = moved_instances.size();
    const bool no_flip = record_model_transforms(model_transforms, &moved_instances);
    m_staged = m_staged || moved_instances.size() != before;
    return no_flip;
}

void SceneBuilder::rebuild() {
    apply_staged_poses();
    m_staged = false; m_staged_flips = false;
    m_staged_moved.assign(m_instances.size(), false);
    for (size_t i = 0; i < m_instances.size(); ++i) m_instances[i].index_offset = index_offset_for(m_instance_mesh[i], m_instances[i].object_to_world);
    finalize(m_bvh_max_depth_limit);
}

bool SceneBuilder::update_model_transforms(const std::vector<std::pair<uint32_t, Transform>>& model_transforms, double rebuild_threshold) {
    record_model_transforms(model_transforms, nullptr);
    m_staged = true;
    return apply_staged_transforms(rebuild_threshold);
}

bool SceneBuilder::apply_staged_transforms(double rebuild_threshold) {
    if (!m_staged) return true;
    apply_staged_poses();
    if (has_staged_edits()) { rebuild(); return false; }      // another set of triangles: nothing to refit
    const std::vector<bool> moved = m_staged_moved;
    const bool flips = m_staged_flips;
    m_staged = false; m_staged_flips = false;
    m_staged_moved.assign(m_instances.size(), false);
    if (flips) {
        for (size_t i = 0; i < m_instances.size(); ++i)
            if (moved[i]) m_instances[i].index_offset = index_offset_for(m_instance_mesh[i], m_instances[i].object_to_world);
        finalize(m_bvh_max_depth_limit);
        return false;
    }
    move_triangles(moved);
    const double area = refit_bvh(m_bvh, m_triangles);
    for (int a = 0; a < 3; ++a) { m_desc.wide8_grid_min[a] = m_bvh.wide8.grid_min[a]; m_desc.wide8_grid_cell[a] = m_bvh.wide8.grid_cell[a]; }     // the refit moves the grid with the scene
    if (area < 0.0 || (m_built_bvh_area > 0.0 && area > rebuild_threshold * m_built_bvh_area)) {      // area < 0: a leaf record of the 8-wide tree could not be refitted
        finalize(m_bvh_max_depth_limit);      // the instances already carry the new transforms
        return false;
    }
    return true;
}

bool SceneBuilder::write_vertex_edits(const std::vector<VertexEdit>& edits, std::vector<HiprVertexEdit>* pool_edits) {
    if (!m_built || has_staged_edits()) return false;
    for (const VertexEdit& e : edits) {
        if (e.mesh >= m_meshes.size() || e.vertex_count == 0 || (!e.geometry && !e.texcoords && !e.tints && !e.emissions)) return false;
        const MeshRecord& r = m_meshes[e.mesh];
        if (uint64_t(e.first_vertex) + e.vertex_count > r.vertex_count || size_t(r.vertex_offset) + r.vertex_count > m_built_pools.vertices) return false;
        if ((e.texcoords && !m_built_pools.texcoords) || (e.tints && !m_built_pools.tints) || (e.emissions && !m_built_pools.emission)) return false;
        for (uint32_t v = 0; v < e.vertex_count; ++v) {
            if (e.geometry && !(std::isfinite(e.geometry[v].position[0]) && std::isfinite(e.geometry[v].position[1]) && std::isfinite(e.geometry[v].position[2]))) return false;
            if (e.texcoords && !(std::isfinite(e.texcoords[2 * size_t(v)]) && std::isfinite(e.texcoords[2 * size_t(v) + 1]))) return false;
        }
    }
    apply_staged_poses();      // a staged pose lands first, so that what is written now wins over it: the catch-up must not replay it over these rows
    std::vector<bool> moved_mesh(m_meshes.size(), false), mapped_mesh(m_meshes.size(), false);
    bool any_mapped = false;
    for (const VertexEdit& e : edits) {
        const size_t at = size_t(m_meshes[e.mesh].vertex_offset) + e.first_vertex, n = e.vertex_count;
        if (e.geometry) { std::copy(e.geometry, e.geometry + n, m_geometry.begin() + ptrdiff_t(at)); moved_mesh[e.mesh] = true; }
        if (e.texcoords) { std::copy(e.texcoords, e.texcoords + 2 * n, m_texcoords.begin() + ptrdiff_t(2 * at)); mapped_mesh[e.mesh] = true; any_mapped = true; }
        if (e.tints) std::copy(e.tints, e.tints + n, m_tints.begin() + ptrdiff_t(at));
        if (e.emissions) std::copy(e.emissions, e.emissions + 3 * n, m_emissions.begin() + ptrdiff_t(3 * at));
        if (pool_edits) pool_edits->push_back({uint32_t(at), e.vertex_count, e.geometry, e.texcoords, e.tints, e.emissions});
    }
    if (any_mapped) {      // the flags that follow texture coordinates (csrc/material_rules.h), and the leaf records' copies
        bool flags_changed = false;
        for (HiprTriangle& triangle : m_triangles) {
            if (!mapped_mesh[m_instance_mesh[triangle.instance_index]]) continue;
            const HiprInstance& inst = m_instances[triangle.instance_index];
            const uint32_t before = triangle.flags;
            triangle.flags = hipr::triangle_flags(m_materials[size_t(inst.material_index)], inst, triangle.primitive_index, m_indices.data(), m_texcoords.data(), m_textures.data(), uint32_t(m_textures.size()), m_texels.data());
            flags_changed = flags_changed || triangle.flags != before;
        }
        if (flags_changed) refresh_leaf_material_bits();
    }
    if (m_staged_moved.size() != m_instances.size()) m_staged_moved.assign(m_instances.size(), false);
    for (size_t i = 0; i < m_instances.size(); ++i)
        if (moved_mesh[m_instance_mesh[i]]) { m_staged_moved[i] = true; m_staged = true; }
    return true;
}

bool SceneBuilder::update_vertices(const std::vector<VertexEdit>& edits, double rebuild_threshold, bool* refused) {
    const bool written = write_vertex_edits(edits, nullptr);
    if (refused) *refused = !written;
    return written && apply_staged_transforms(rebuild_threshold);
}

bool SceneBuilder::stage_vertex_edits(const std::vector<VertexEdit>& edits, std::vector<HiprVertexEdit>& pool_edits) { return write_vertex_edits(edits, &pool_edits); }

bool SceneBuilder::set_rigs(const std::vector<RigDesc>& rigs) {
    if (!m_built) return false;
    std::vector<HiprRigDesc> pooled;
    std::vector<uint32_t> meshes;
    for (const RigDesc& d : rigs) {
        if (d.mesh >= m_meshes.size()) return false;
        const MeshRecord& r = m_meshes[d.mesh];
        if (uint64_t(d.rig.first_vertex) + d.rig.vertex_count > r.vertex_count || size_t(r.vertex_offset) + r.vertex_count > m_built_pools.vertices) return false;
        if ((d.rig.rest_normals != nullptr) != ((r.flags & HIPR_MESH_NORMALS) != 0)) return false;
        HiprRigDesc p = d.rig;
        p.first_vertex += r.vertex_offset;
        pooled.push_back(p);
        meshes.push_back(d.mesh);
    }
    if (hipr::check_rig_descs(pooled.data(), uint32_t(pooled.size()), m_built_pools.vertices)) return false;
    apply_staged_poses();      // poses of the rigs that go are not lost
    m_rig_words.clear();
    m_rig_records.assign(pooled.size(), hipr::PoseRig{});
    m_rig_books.assign(pooled.size(), hipr::RigBook{});
    for (size_t k = 0; k < pooled.size(); ++k) hipr::pack_rig(pooled[k], m_rig_words, m_rig_records[k], m_rig_books[k]);
    m_rig_mesh = meshes;
    m_staged_poses.assign(pooled.size(), StagedPose{});
    return true;
}

void SceneBuilder::pose_rig_rows(uint32_t rig, const float* matrices, const float* weights, HiprVertexGeometry* out) const {
    const hipr::PoseRigView view = hipr::view_of(m_rig_records[rig], m_rig_words.data());
    for (uint32_t v = 0; v < view.vertex_count; ++v) out[v] = hipr::pose_vertex(view, v, matrices, 12u, weights);
}

void SceneBuilder::apply_staged_poses() {
    for (size_t k = 0; k < m_staged_poses.size(); ++k) {
        StagedPose& p = m_staged_poses[k];
        if (!p.staged) continue;
        pose_rig_rows(uint32_t(k), p.matrices.data(), p.weights.data(), m_geometry.data() + m_rig_books[k].first_vertex);
        p = StagedPose{};
    }
}

bool SceneBuilder::pose_rigs(const std::vector<HiprRigPose>& poses, double rebuild_threshold, bool* refused) {
    if (refused) *refused = true;
    if (!m_built || has_staged_edits() || hipr::check_rig_poses(poses.data(), uint32_t(poses.size()), m_rig_books.data(), m_rig_books.size())) return false;
    std::vector<std::vector<HiprVertexGeometry>> rows(poses.size());
    std::vector<VertexEdit> edits;
    for (size_t k = 0; k < poses.size(); ++k) {
        const hipr::RigBook& b = m_rig_books[poses[k].rig];
        rows[k].resize(b.vertex_count);
        pose_rig_rows(poses[k].rig, poses[k].joint_matrices, poses[k].target_weights, rows[k].data());
        const uint32_t mesh = m_rig_mesh[poses[k].rig];
        edits.push_back({mesh, b.first_vertex - m_meshes[mesh].vertex_offset, b.vertex_count, rows[k].data(), nullptr, nullptr, nullptr});
    }
    return update_vertices(edits, rebuild_threshold, refused);
}

bool SceneBuilder::stage_rig_poses(const std::vector<HiprRigPose>& poses, std::vector<HiprRigPose>& pool_poses) {
    if (!m_built || has_staged_edits() || hipr::check_rig_poses(poses.data(), uint32_t(poses.size()), m_rig_books.data(), m_rig_books.size())) return false;
    if (m_staged_moved.size() != m_instances.size()) m_staged_moved.assign(m_instances.size(), false);
    for (const HiprRigPose& p : poses) {
        const hipr::RigBook& b = m_rig_books[p.rig];
        StagedPose& s = m_staged_poses[p.rig];
        s.staged = true;
        s.matrices.assign(p.joint_matrices, p.joint_matrices + (b.joint_count ? 12u * size_t(b.joint_count) : 0u));
        s.weights.assign(p.target_weights, p.target_weights + (b.target_count ? b.target_count : 0u));
        for (size_t i = 0; i < m_instances.size(); ++i)
            if (m_instance_mesh[i] == m_rig_mesh[p.rig]) { m_staged_moved[i] = true; m_staged = true; }
        pool_poses.push_back(p);
    }
    return true;
}

bool SceneBuilder::posed_geometry(const HiprRigDesc& rig, const HiprRigPose& pose, HiprVertexGeometry* out) {
    HiprRigDesc alone = rig;
    alone.first_vertex = 0;
    HiprRigPose p = pose;
    p.rig = 0;
    if (!out || hipr::check_rig_descs(&alone, 1, alone.vertex_count)) return false;
    std::vector<uint32_t> words;
    hipr::PoseRig record;
    hipr::RigBook book;
    hipr::pack_rig(alone, words, record, book);
    if (hipr::check_rig_poses(&p, 1, &book, 1)) return false;
    const hipr::PoseRigView view = hipr::view_of(record, words.data());
    for (uint32_t v = 0; v < view.vertex_count; ++v) out[v] = hipr::pose_vertex(view, v, pose.joint_matrices, 12u, pose.target_weights);
    return true;
}

// The world-space corners of the triangles of the instances flagged in `moved`, recomputed in place from the instances' matrices, and the scene's bounds.
void SceneBuilder::move_triangles(const std::vector<bool>& moved) {
    m_bounds = AABB::invalid();
    for (HiprTriangle& t : m_triangles) {
        if (moved[t.instance_index]) {
            const HiprInstance& inst = m_instances[t.instance_index];
            const MeshRecord& mesh = m_meshes[m_instance_mesh[t.instance_index]];
            const float* M = inst.object_to_world;
            const uint32_t* idx = &m_indices[3 * size_t(inst.index_offset + t.primitive_index)];
            float* corners[3] = {t.v0, t.v1, t.v2};
            for (int k = 0; k < 3; ++k) {
                const float* p = m_geometry[mesh.vertex_offset + idx[k]].position;
                for (int r = 0; r < 3; ++r) corners[k][r] = M[4 * r] * p[0] + M[4 * r + 1] * p[1] + M[4 * r + 2] * p[2] + M[4 * r + 3];
            }
        }
        m_bounds.grow_to_contain(Vector3f(t.v0[0], t.v0[1], t.v0[2]));
        m_bounds.grow_to_contain(Vector3f(t.v1[0], t.v1[1], t.v1[2]));
        m_bounds.grow_to_contain(Vector3f(t.v2[0], t.v2[1], t.v2[2]));
    }
}

namespace {
// Sources that hand build_bvh the trees a device rebuild made (hipr_rebuild_scene_trees), so that the 4-wide collapse, the depth and the description go on from
// them exactly as after the host's own stages.
struct AdoptedTrees { const HiprBvhNode* nodes; uint32_t node_count; const uint32_t* order; uint32_t deepest; const HiprSlot8* slots; HiprWide8BuildResult wide8; };
int adopted_bvh2(void* context, const HiprTriangle*, uint32_t count, uint32_t, HiprBvhNode* out_nodes, uint32_t node_capacity, uint32_t* out_node_count, uint32_t* out_order, uint32_t* out_deepest) {
    const AdoptedTrees& t = *static_cast<const AdoptedTrees*>(context);
    if (t.node_count > node_capacity) return HIPR_ERROR_INVALID_ARGUMENT;
    std::copy(t.nodes, t.nodes + t.node_count, out_nodes);
    std::copy(t.order, t.order + count, out_order);
    *out_node_count = t.node_count; *out_deepest = t.deepest;
    return HIPR_OK;
}
int adopted_wide8(void* context, const HiprBvhNode*, uint32_t, const HiprTriangle*, const uint32_t*, uint32_t, HiprSlot8* out_slots, uint32_t slot_capacity, HiprWide8BuildResult* out) {
    const AdoptedTrees& t = *static_cast<const AdoptedTrees*>(context);
    if (t.wide8.slot_count > slot_capacity) return HIPR_ERROR_INVALID_ARGUMENT;
    std::copy(t.slots, t.slots + t.wide8.slot_count, out_slots);
    *out = t.wide8;
    return HIPR_OK;
}
}

// What both adoptions ask of trees over `n` triangles before they touch anything: counts that fit, an `order` that is a permutation, child and leaf references in range.
bool SceneBuilder::trees_fit(uint32_t n, const HiprBvhNode* nodes, uint32_t node_count, const uint32_t* order, const HiprSlot8* slots, const HiprWide8BuildResult& wide8) const {
    auto refuse = [] { return false; };
    if (!nodes || !order || !slots || n == 0) return refuse();
    if (node_count == 0 || node_count > std::max(n, 2u) - 1u || wide8.slot_count == 0 || wide8.slot_count > std::min<uint64_t>(2ull * n, 0xFFFFFFull)) return refuse();
    std::vector<bool> seen(n, false);
    for (uint32_t k = 0; k < n; ++k) {      // a permutation
        if (order[k] >= n || seen[order[k]]) return refuse();
        seen[order[k]] = true;
    }
    for (uint32_t i = 0; i < node_count; ++i)
        for (int c = 0; c < 2; ++c) {
            const int32_t ref = nodes[i].child[c];
            if (ref >= 0 ? uint32_t(ref) >= node_count || uint32_t(ref) <= i : uint64_t(uint32_t(~ref) >> 3) + (uint32_t(~ref) & 7u) + 1u > n) return refuse();
        }
    {   // the 8-wide tree from the root: every child slot in range, every record's triangles in range
        std::vector<uint32_t> walk = {0u};
        for (size_t i = 0; i < walk.size(); ++i) {
            const HiprNode8& node = slots[walk[i]].node;
            const uint32_t base = node.base_valid & 0xFFFFFFu, valid = node.base_valid >> 24;
            uint32_t rank = 0;
            for (int p = 0; p < 8; ++p) {
                if (!(valid >> p & 1u)) continue;
                const uint32_t child = base + rank++;
                if (child >= wide8.slot_count || child <= walk[i] || walk.size() > wide8.slot_count) return refuse();
                if (node.inner_mask >> p & 1u) walk.push_back(child);
                else if (slots[child].leaf.triangle[0] >= n || (slots[child].leaf.triangle[1] != HIPR_LEAF8_NONE && slots[child].leaf.triangle[1] >= n)) return refuse();
            }
        }
    }
    return true;
}

bool SceneBuilder::adopt_rebuilt_trees(const HiprBvhNode* nodes, uint32_t node_count, const uint32_t* order, uint32_t deepest, const HiprSlot8* slots, const HiprWide8BuildResult& wide8) {
    const uint32_t n = uint32_t(m_triangles.size());
    auto refuse = [&] { ++m_rebuild_counts.refused; return false; };
    apply_staged_poses();      // the pools are the source data: staged poses reach them whatever follows
    // counts that do not fit; an instance turned inside out is drawn from other index triples, which changes the set of triangles -- and so does an edited instance list
    if (m_bvh.order.size() != n || m_staged_flips || has_staged_edits() || !trees_fit(n, nodes, node_count, order, slots, wide8)) return refuse();
    // everything staged reaches the builder's own triangles, without a refit of trees that are about to be replaced and without a flatten
    const std::vector<bool> moved = m_staged_moved.size() == m_instances.size() ? m_staged_moved : std::vector<bool>(m_instances.size(), false);
    m_staged = false;
    m_staged_moved.assign(m_instances.size(), false);
    move_triangles(moved);
    std::vector<HiprTriangle> world(n);      // the flatten order, through the old order
    for (uint32_t k = 0; k < n; ++k) world[m_bvh.order[k]] = m_triangles[k];
    m_bounds = AABB::invalid();      // grown in the order finalize() grows them in
    for (const HiprTriangle& t : world) {
        m_bounds.grow_to_contain(Vector3f(t.v0[0], t.v0[1], t.v0[2]));
        m_bounds.grow_to_contain(Vector3f(t.v1[0], t.v1[1], t.v1[2]));
        m_bounds.grow_to_contain(Vector3f(t.v2[0], t.v2[1], t.v2[2]));
    }
    AdoptedTrees adopted = {nodes, node_count, order, deepest, slots, wide8};
    Bvh2SourceReport report;
    Wide8SourceReport wide8_report;
    build_trees_over(world, Bvh2Source{adopted_bvh2, &adopted}, report, Wide8Source{adopted_wide8, &adopted}, wide8_report);      // a host configured away from the default trees builds its own, as rebuild() would
    ++m_rebuild_counts.adopted;
    return true;
}

bool SceneBuilder::staged_instance_edits(std::vector<HiprInstanceEdit>& edits) const {
    edits.clear();
    return !m_pools_grew && list_instance_edits(edits);
}

bool SceneBuilder::staged_scene_growth(StagedGrowth& out, std::vector<HiprInstanceEdit>& edits) const {
    out = {};
    edits.clear();
    const PoolSizes& b = m_built_pools;
    if (m_environment_set_since || m_lights.size() != b.lights || !list_instance_edits(edits)) { edits.clear(); return false; }
    HiprPoolGrowth& g = out.growth;
    const size_t vertices = m_geometry.size(), created = vertices - b.vertices;
    g.vertex_count = uint32_t(created);
    g.geometry = created ? m_geometry.data() + b.vertices : nullptr;
    // a pool that existed takes its tail; one that has come into being since comes whole, with whatever add_mesh put there for the meshes without the attribute
    if (b.texcoords) { g.texcoord_vertices = uint32_t(created); g.texcoords = created ? m_texcoords.data() + 2 * b.vertices : nullptr; }
    else if (m_any_texcoords) { g.texcoord_vertices = uint32_t(vertices); g.texcoords = m_texcoords.data(); }
    if (b.tints) { g.tint_vertices = uint32_t(created); g.tints = created ? m_tints.data() + b.vertices : nullptr; }
    else if (m_any_tints) { g.tint_vertices = uint32_t(vertices); g.tints = m_tints.data(); }
    if (b.emission) { g.emission_vertices = uint32_t(created); g.emissions = created ? m_emissions.data() + 3 * b.vertices : nullptr; }
    else if (m_any_emission) { g.emission_vertices = uint32_t(vertices); g.emissions = m_emissions.data(); }
    // the index tail: the log's ranges in order, neighbouring mesh ranges as one segment
    size_t words = 0, from_host = 0;
    bool mirrors_between = false;
    for (const HiprIndexSegment& range : m_index_log) {
        if (range.mirrored_from == HIPR_SEGMENT_FROM_HOST) { mirrors_between = mirrors_between || from_host != words; from_host += range.index_count; }
        if (range.mirrored_from == HIPR_SEGMENT_FROM_HOST && !out.segments.empty() && out.segments.back().mirrored_from == HIPR_SEGMENT_FROM_HOST) out.segments.back().index_count += range.index_count;
        else out.segments.push_back(range);
        words += range.index_count;
    }
    if (b.index_words + words != m_indices.size()) { out = {}; edits.clear(); return false; }      // the log does not tell the tail: the full path
    if (mirrors_between) {
        size_t at = b.index_words;
        for (const HiprIndexSegment& range : m_index_log) {
            if (range.mirrored_from == HIPR_SEGMENT_FROM_HOST) out.host_indices.insert(out.host_indices.end(), m_indices.begin() + ptrdiff_t(at), m_indices.begin() + ptrdiff_t(at + range.index_count));
            at += range.index_count;
        }
    }
    g.index_count = uint32_t(from_host);
    g.indices = !from_host ? nullptr : (mirrors_between ? out.host_indices.data() : m_indices.data() + b.index_words);
    g.segment_count = uint32_t(out.segments.size());
    g.segments = out.segments.empty() ? nullptr : out.segments.data();
    g.material_count = uint32_t(m_materials.size() - b.materials);
    g.materials = g.material_count ? m_materials.data() + b.materials : nullptr;
    g.texture_count = uint32_t(m_textures.size() - b.textures);
    g.textures = g.texture_count ? m_textures.data() + b.textures : nullptr;
    g.texel_bytes = uint64_t(m_texels.size() - b.texel_bytes);
    g.texels = g.texel_bytes ? m_texels.data() + b.texel_bytes : nullptr;
    return true;
}

bool SceneBuilder::list_instance_edits(std::vector<HiprInstanceEdit>& edits) const {
    edits.clear();
    if (!m_built || m_staged_flips || std::find(m_staged_moved.begin(), m_staged_moved.end(), true) != m_staged_moved.end()) return false;
    edits.resize(m_instances.size());
    for (size_t i = 0; i < m_instances.size(); ++i) {
        HiprInstanceEdit& e = edits[i];
        e = {};
        e.source = m_built_index[i] == NOT_BUILT ? HIPR_EDIT_NEW_INSTANCE : m_built_index[i];
        if (m_built_index[i] == NOT_BUILT) { e.instance = m_instances[i]; e.primitive_count = m_meshes[m_instance_mesh[i]].primitive_count; }
    }
    return true;
}

bool SceneBuilder::adopt_edited_trees(const HiprBvhNode* nodes, uint32_t node_count, const uint32_t* order, uint32_t order_count, uint32_t deepest, const HiprSlot8* slots, const HiprWide8BuildResult& wide8) {
    apply_staged_poses();      // the pools are the source data: staged poses reach them whatever follows
    auto refuse = [&] { ++m_rebuild_counts.refused; return false; };
    std::vector<HiprInstanceEdit> unused;
    StagedGrowth unused_growth;
    if (!staged_scene_growth(unused_growth, unused) || m_bvh.order.size() != m_triangles.size()) return refuse();      // what the device could not have been given
    // first[] of the list as it stands, and where the built list's instances went
    std::vector<uint32_t> first(m_instances.size() + 1, 0u), new_index(m_built_instance_count, NOT_BUILT);
    uint64_t total = 0;
    for (size_t i = 0; i < m_instances.size(); ++i) {
        total += m_meshes[m_instance_mesh[i]].primitive_count;
        first[i + 1] = uint32_t(total);
        if (m_built_index[i] != NOT_BUILT) new_index[m_built_index[i]] = uint32_t(i);
    }
    if (total == 0 || total > 0xFFFFFFFFull || order_count != total || !trees_fit(uint32_t(total), nodes, node_count, order, slots, wide8)) return refuse();
    const uint32_t n = uint32_t(total);
    std::vector<HiprTriangle> world(n);
    std::vector<bool> placed(n, false);
    for (const HiprTriangle& t : m_triangles) {      // kept triangles to their place in the new flatten order; removed ranges are dropped
        const uint32_t to = t.instance_index < new_index.size() ? new_index[t.instance_index] : NOT_BUILT;
        if (to == NOT_BUILT) continue;
        if (t.primitive_index >= first[to + 1] - first[to] || placed[first[to] + t.primitive_index]) return refuse();
        HiprTriangle& w = world[first[to] + t.primitive_index];
        w = t;
        w.instance_index = to;
        placed[first[to] + t.primitive_index] = true;
    }
    const AABB bounds_before = m_bounds;
    std::vector<HiprTriangle> created;
    for (size_t i = 0; i < m_instances.size(); ++i) {      // only the new instances are flattened
        if (m_built_index[i] != NOT_BUILT) continue;
        created.clear();
        flatten_instance(uint32_t(i), created);
        for (size_t p = 0; p < created.size(); ++p) { world[first[i] + p] = created[p]; placed[first[i] + p] = true; }
    }
    if (std::find(placed.begin(), placed.end(), false) != placed.end()) { m_bounds = bounds_before; return refuse(); }
    m_staged = false; m_staged_flips = false;
    m_staged_moved.assign(m_instances.size(), false);
    m_bounds = AABB::invalid();      // grown in the order finalize() grows them in
    for (const HiprTriangle& t : world) {
        m_bounds.grow_to_contain(Vector3f(t.v0[0], t.v0[1], t.v0[2]));
        m_bounds.grow_to_contain(Vector3f(t.v1[0], t.v1[1], t.v1[2]));
        m_bounds.grow_to_contain(Vector3f(t.v2[0], t.v2[1], t.v2[2]));
    }
    AdoptedTrees adopted = {nodes, node_count, order, deepest, slots, wide8};
    Bvh2SourceReport report;
    Wide8SourceReport wide8_report;
    build_trees_over(world, Bvh2Source{adopted_bvh2, &adopted}, report, Wide8Source{adopted_wide8, &adopted}, wide8_report);
    ++m_rebuild_counts.adopted;
    return true;
}

bool SceneBuilder::update_materials(const std::vector<HiprMaterialUpdate>& changed, const std::vector<HiprInstanceMaterial>& assignments) {
    for (const HiprMaterialUpdate& c : changed)
        if (c.material_index >= m_materials.size()) return false;
    for (const HiprInstanceMaterial& a : assignments)
        if (a.instance_index >= m_instances.size() || a.material_index < 0 || size_t(a.material_index) >= m_materials.size()) return false;
    // `rewritten`: slots whose new contents can give a triangle other flags -- the rules read a material's flags, shading model, coverage and coverage texture and
    // nothing else, so a roughness slider leaves every triangle and every leaf record alone
    std::vector<bool> rewritten(m_materials.size(), false), touched(m_instances.size(), false);
    for (const HiprMaterialUpdate& c : changed) {
        const HiprMaterial& was = m_materials[c.material_index];
        if (was.flags != c.material.flags || was.shading_model != c.material.shading_model || std::memcmp(&was.coverage, &c.material.coverage, sizeof(float)) != 0 ||
            was.coverage_texture_ID != c.material.coverage_texture_ID)
            rewritten[c.material_index] = true;
        m_materials[c.material_index] = c.material;
    }
    for (const HiprInstanceMaterial& a : assignments) { m_instances[a.instance_index].material_index = a.material_index; touched[a.instance_index] = true; }
    for (size_t i = 0; i < m_instances.size(); ++i) touched[i] = touched[i] || rewritten[size_t(m_instances[i].material_index)];
    if (std::find(touched.begin(), touched.end(), true) == touched.end()) return true;
    bool flags_changed = false;
    for (HiprTriangle& t : m_triangles) {
        if (!touched[t.instance_index]) continue;
        const HiprInstance& inst = m_instances[t.instance_index];
        const uint32_t before = t.flags;
        t.flags = hipr::triangle_flags(m_materials[size_t(inst.material_index)], inst, t.primitive_index, m_indices.data(), m_texcoords.data(), m_textures.data(), uint32_t(m_textures.size()), m_texels.data());
        flags_changed = flags_changed || t.flags != before;
    }
    if (!flags_changed) return true;
    refresh_leaf_material_bits();
    return true;
}

// The leaf records of the 8-wide tree repeat the flags of their triangles; the tree is walked from the root, children in consecutive slots.
void SceneBuilder::refresh_leaf_material_bits() {
    std::vector<HiprSlot8>& slots = m_bvh.wide8.slots;
    std::vector<uint32_t> nodes;
    if (!slots.empty()) nodes.push_back(0u);
    for (size_t i = 0; i < nodes.size(); ++i) {
        const HiprNode8 n = slots[nodes[i]].node;
        const uint32_t base = n.base_valid & 0xFFFFFFu, valid = n.base_valid >> 24;
        uint32_t rank = 0;
        for (int p = 0; p < 8; ++p) {
            if (!(valid >> p & 1u)) continue;
            const uint32_t child = base + rank++;
            if (n.inner_mask >> p & 1u) nodes.push_back(child);
            else slots[child].leaf.flags = (slots[child].leaf.flags & ~15u) | hipr::leaf_material_bits(m_triangles.data(), slots[child].leaf);
        }
    }
}

bool SceneBuilder::update_texels(uint32_t texture_index, uint32_t x, uint32_t y, uint32_t width, uint32_t height, const void* pixels, uint64_t row_pitch_bytes) {
    if (!m_built || !pixels || texture_index == 0 || texture_index >= m_textures.size() || texture_index >= m_built_pools.textures) return false;
    const HiprTexture& t = m_textures[texture_index];
    const uint64_t size = t.format == HIPR_TEXEL_R8 ? 1u : (t.format == HIPR_TEXEL_RGBA8 || t.format == HIPR_TEXEL_R32F ? 4u : 16u), row_bytes = uint64_t(width) * size;
    if (width == 0 || height == 0 || x >= t.width || y >= t.height || width > t.width - x || height > t.height - y || row_pitch_bytes < row_bytes) return false;
    // `affected`: the materials that leave their triangles' HIPR_TRIANGLE_OPAQUE to this texture (csrc/material_rules.h)
    std::vector<bool> affected(m_materials.size(), false);
    bool any_affected = false, names_coverage = false;
    for (size_t k = 0; k < m_materials.size(); ++k) {
        affected[k] = hipr::deciding_coverage_texture(m_materials[k], m_textures.data(), uint32_t(m_textures.size())) == &t;
        any_affected = any_affected || affected[k];
        names_coverage = names_coverage || (m_materials[k].coverage_texture_ID > 0 && uint32_t(m_materials[k].coverage_texture_ID) == texture_index);
    }
    if (names_coverage && m_triangles.size() <= 64) return false;      // the exhaustive search's items pair triangles by their flags: the device refuses, as for a material edit
    for (uint32_t row = 0; row < height; ++row)
        std::memcpy(m_texels.data() + t.texel_offset + (uint64_t(y + row) * t.width + x) * size, static_cast<const uint8_t*>(pixels) + row * row_pitch_bytes, size_t(row_bytes));
    if (m_has_environment && m_environment.environment_map_ID == int32_t(texture_index)) m_environment_texels_edited = true;
    if (!any_affected) return true;
    bool flags_changed = false;
    for (HiprTriangle& triangle : m_triangles) {
        const HiprInstance& inst = m_instances[triangle.instance_index];
        if (!affected[size_t(inst.material_index)]) continue;
        const uint32_t before = triangle.flags;
        triangle.flags = hipr::triangle_flags(m_materials[size_t(inst.material_index)], inst, triangle.primitive_index, m_indices.data(), m_texcoords.data(), m_textures.data(), uint32_t(m_textures.size()), m_texels.data());
        flags_changed = flags_changed || triangle.flags != before;
    }
    if (flags_changed) refresh_leaf_material_bits();
    return true;
}

bool SceneBuilder::replace_lights(const std::vector<HiprLight>& lights) {
    const size_t environment_lights = m_has_environment && m_environment_samples.size() > 1 ? 1 : 0;
    if (lights.size() + environment_lights != m_lights.size()) return false;
    std::copy(lights.begin(), lights.end(), m_lights.begin());      // the presampled environment light, if any, stays last
    return true;
}

bool SceneBuilder::set_lights(const std::vector<HiprLight>& lights) {
    if (!m_built) return false;
    for (const HiprLight& light : lights)
        if ((light.flags & HIPR_LIGHT_TYPE_MASK) == HIPR_LIGHT_PRESAMPLED_ENVIRONMENT) return false;
    m_lights = lights;
    if (m_has_environment && m_environment_samples.size() > 1) {      // set_environment's rule: the environment's light stays last
        HiprLight light = {};
        light.flags = HIPR_LIGHT_PRESAMPLED_ENVIRONMENT;
        m_lights.push_back(light);
    }
    m_desc.lights = m_lights.data(); m_desc.light_count = uint32_t(m_lights.size());
    m_built_pools.lights = m_lights.size();      // the device follows: a growth staged afterwards is the device's to apply again
    return true;
}

bool SceneBuilder::staged_environment_build(uint32_t texture_index, uint32_t sample_count, StagedEnvironmentBuild& staged) const {
    staged = {};
    if (texture_index == 0 || texture_index >= m_textures.size()) return false;
    const HiprTexture& t = m_textures[texture_index];
    const int height = int(std::max(t.height, 128u));      // InfiniteAreaLight::MINIMUM_PDF_HEIGHT
    staged.row_sines.resize(size_t(height));
    for (int y = 0; y < height; ++y) staged.row_sines[size_t(y)] = std::sin(PI<float>() * (y + 0.5f) / float(height));      // compute_distribution's sin_theta
    if (t.is_sRGB) {
        staged.srgb_decode.resize(256);
        const float unorm8 = 1.0f / 255.0f;
        for (int b = 0; b < 256; ++b) {      // get_pixel's sRGB_to_linear of the byte's value (Color.h:356-361)
            const float v = (unsigned char)b * unorm8;
            staged.srgb_decode[size_t(b)] = v < 0.04045f ? v * 0.0773993808f : std::pow(v * 0.9478672986f + 0.0521327014f, 2.4f);
        }
    }
    // presample_environment's points in the order it visits them
    unsigned int count = 1;
    while (count < sample_count) count *= 2;
    count = std::max(2u, count);
    if (m_draw_points.size() != size_t(count) * 2) {      // the points depend on the count alone and cost tens of milliseconds at 8192: made once per count, kept
        const int exponent = int(std::log2(float(count)));
        std::vector<Vector2f> points(count);
        RNG::fill_progressive_multijittered_bluenoise_samples(points.data(), points.data() + count);
        m_draw_points.resize(size_t(count) * 2);
        for (unsigned int i = 0; i < count; ++i) {
            const unsigned int adjusted = RNG::reverse_bits(i) >> (32 - exponent);
            m_draw_points[2 * size_t(i)] = points[adjusted].x;
            m_draw_points[2 * size_t(i) + 1] = points[adjusted].y;
        }
    }
    staged.draw_points = m_draw_points;
    staged.build.environment_map_ID = int32_t(texture_index);
    staged.build.row_sines = staged.row_sines.data();
    staged.build.pdf_height = uint32_t(height);
    staged.build.srgb_decode = t.is_sRGB ? staged.srgb_decode.data() : nullptr;
    staged.build.draw_points = staged.draw_points.data();
    staged.build.sample_count = count;
    return true;
}

bool SceneBuilder::adopt_lighting(const std::vector<HiprLight>& lights, int environment_action, uint32_t texture_index, const HiprLightingResult& result, std::vector<float> per_pixel_PDF,
                                  std::vector<HiprLightSample> samples) {
    if (!m_built) return false;
    for (const HiprLight& light : lights)
        if ((light.flags & HIPR_LIGHT_TYPE_MASK) == HIPR_LIGHT_PRESAMPLED_ENVIRONMENT) return false;
    if (environment_action == HIPR_ENVIRONMENT_BUILD) {
        if (texture_index == 0 || texture_index >= m_textures.size() || result.sample_count == 0 || samples.size() != result.sample_count ||
            per_pixel_PDF.size() != size_t(result.pdf_width) * result.pdf_height)
            return false;
        m_environment_PDF = std::move(per_pixel_PDF);
        m_environment_samples = std::move(samples);
        m_environment = {int32_t(texture_index), result.pdf_width, result.pdf_height, m_environment_PDF.data(), m_environment_samples.data(), uint32_t(m_environment_samples.size())};
        m_has_environment = true;
    } else if (environment_action == HIPR_ENVIRONMENT_REMOVE) {
        m_environment_PDF.clear();
        m_environment_samples.clear();
        m_environment = {};
        m_has_environment = false;
    } else if (environment_action != HIPR_ENVIRONMENT_KEEP) return false;
    m_environment_set_since = false;
    if (environment_action != HIPR_ENVIRONMENT_KEEP) m_environment_texels_edited = false;
    m_desc.environment = m_has_environment ? &m_environment : nullptr;
    return set_lights(lights);
}

HiprCameraState make_camera_state(const CameraDescription& camera, float aspect_ratio, uint32_t accumulations, float path_regularization_PDF_scale) {
    Matrix4x4f inverse_projection = {};
    if (camera.orthographic) {
        // compute_orthographic_projection, Bifrost/Scene/Camera.cpp:268-286
        inverse_projection[0][0] = 0.5f * camera.ortho_width;
        inverse_projection[1][1] = 0.5f * camera.ortho_height;
        inverse_projection[2][2] = 0.5f * camera.ortho_depth;
        inverse_projection[2][3] = 0.5f * camera.ortho_depth;
        inverse_projection[3][3] = 1.0f;
    } else {
        // compute_perspective_projection, Bifrost/Scene/Camera.cpp:237-266
        const float n = camera.near_plane, fa = camera.far_plane;
        const float f = 1.0f / std::tan(camera.field_of_view * 0.5f);
        const float a = (fa + n) / (n - fa);
        const float b = (2.0f * fa * n) / (n - fa);
        Matrix4x4f projection = {};
        projection[0][0] = f / aspect_ratio;
        projection[1][1] = f;
        projection[2][2] = -a;
        projection[2][3] = b;
        projection[3][2] = 1.0f;
        inverse_projection[0][0] = 1.0f / projection[0][0];
        inverse_projection[1][1] = 1.0f / projection[1][1];
        inverse_projection[2][3] = 1.0f;
        inverse_projection[3][2] = 1.0f / projection[2][3];
        inverse_projection[3][3] = -projection[2][2] / projection[2][3];
    }

    // Cameras::get_inverse_view_projection_matrix = to_matrix4x4(inverse view transform) * inverse projection (Camera.h:112-114)
    Matrix4x4f inverse_view_projection = to_matrix4x4(camera.transform) * inverse_projection;
    Matrix3x3f rotation = to_matrix3x3(camera.transform.rotation);   // Renderer.cpp:1238-1239

    HiprCameraState s = {};
    std::memcpy(s.view_to_world_rotation, rotation.begin(), sizeof(s.view_to_world_rotation));
    std::memcpy(s.inverse_projection_matrix, inverse_projection.begin(), sizeof(s.inverse_projection_matrix));
    std::memcpy(s.inverse_view_projection_matrix, inverse_view_projection.begin(), sizeof(s.inverse_view_projection_matrix));
    s.accumulations = accumulations;
    s.max_bounce_count = camera.max_bounce_count;
    s.path_regularization_PDF_scale = path_regularization_PDF_scale;
    return s;
}

} // namespace HIPRenderer
