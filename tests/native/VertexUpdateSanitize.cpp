// VertexUpdateSanitize.cpp -- a stand-alone program around the vertex update's staging plan and the host walk of its kernel bodies (vertex_update_host_scene,
// VertexUpdateHost.hip: csrc/vertex_update.h walked in the kernels' shape) and SceneBuilder::update_vertices / stage_vertex_edits for a run under AddressSanitizer /
// UndefinedBehaviorSanitizer on the CPU: `make -C bifrost3d_amd sanitize-vertex-update` builds and runs it, the scene builder and its tree builders compiled in; it
// links no product library.
// The scene: a 7 x 7 quad mesh with texture coordinates under a cut-out material, worn by a model and by a mirrored one, and a 5 x 5 mesh with tints and emissions.
// 40 rounds of random edit lists -- up to 12 edits of random ranges and attributes, overlapping, the pools' first and last vertex among them -- are walked over
// copies of the builder's arrays and applied to the builder, alternately through update_vertices and through stage_vertex_edits + apply_staged_transforms; the
// pools, the triangles and the slots must agree byte for byte after every round. A last round asks the builder for every refusal.
#include "../../bifrost3d_amd/host/SceneBuilder.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace HIPRenderer;
extern "C" int vertex_update_host_scene(HiprTriangle* triangles, uint32_t triangle_count, const HiprInstance* instances, uint32_t instance_count, const HiprMaterial* materials, const uint32_t* indices,
                                        HiprVertexGeometry* geometry, float* texcoords, uint32_t* tints, float* emissions, uint32_t vertex_count, const HiprTexture* textures, uint32_t texture_count,
                                        const uint8_t* texels, const HiprVertexEdit* edits, uint32_t edit_count, uint32_t* trace_triangles, uint32_t* shade_triangles, uint8_t* triangle_class, HiprSlot8* slots,
                                        uint32_t slot_count, float* grid_min3, float* grid_cell3, double* child_half_area, uint32_t* out4);
static float unit() { return rand() / float(RAND_MAX); }
static MeshData grid(int cells, bool mapped, bool tinted) {
    MeshData m;
    for (int i = 0; i <= cells; ++i)
        for (int j = 0; j <= cells; ++j) {
            m.positions.push_back(Vector3f(float(i) / cells, float(j) / cells, 0.05f * unit()));
            m.normals.push_back(Vector3f(0, 0, 1));
            if (mapped) m.texcoords.push_back(Vector2f{float(i) / cells, float(j) / cells});
            if (tinted) { m.tints.push_back(0xFF000000u + uint32_t(rand())); m.emission.push_back(Vector3f(unit(), unit(), unit())); }
        }
    auto at = [&](int i, int j) { return uint32_t(i * (cells + 1) + j); };
    for (int i = 0; i < cells; ++i)
        for (int j = 0; j < cells; ++j) { m.primitives.push_back(Vector3ui{at(i, j), at(i + 1, j), at(i + 1, j + 1)}); m.primitives.push_back(Vector3ui{at(i, j), at(i + 1, j + 1), at(i, j + 1)}); }
    return m;
}
static int fail(const char* what, int round) { printf("FAILED: %s (round %d)\n", what, round); return 1; }
// Copies of the builder's arrays, as the device would hold them.
struct Held {
    std::vector<HiprTriangle> triangles; std::vector<HiprSlot8> slots; std::vector<HiprVertexGeometry> geometry; std::vector<float> texcoords, emissions; std::vector<uint32_t> tints, trace, shade;
    std::vector<uint8_t> classes; float grid_min[3], grid_cell[3];
    explicit Held(const HiprSceneDesc& d)
        : triangles(d.triangles, d.triangles + d.triangle_count), slots(d.wide8_slots, d.wide8_slots + d.wide8_slot_count), geometry(d.geometry, d.geometry + d.vertex_count),
          texcoords(d.texcoords, d.texcoords + 2 * size_t(d.vertex_count)), emissions(d.emissions, d.emissions + 3 * size_t(d.vertex_count)), tints(d.tints, d.tints + d.vertex_count),
          trace(12 * size_t(d.triangle_count), 0u), shade(32 * size_t(d.triangle_count), 0u), classes(d.triangle_count, uint8_t(0)) {
        for (int a = 0; a < 3; ++a) { grid_min[a] = d.wide8_grid_min[a]; grid_cell[a] = d.wide8_grid_cell[a]; }
    }
    bool equals(const HiprSceneDesc& d) const {
        return !std::memcmp(triangles.data(), d.triangles, triangles.size() * sizeof(HiprTriangle)) && !std::memcmp(slots.data(), d.wide8_slots, slots.size() * sizeof(HiprSlot8)) &&
               !std::memcmp(geometry.data(), d.geometry, geometry.size() * sizeof(HiprVertexGeometry)) && !std::memcmp(texcoords.data(), d.texcoords, texcoords.size() * 4) &&
               !std::memcmp(tints.data(), d.tints, tints.size() * 4) && !std::memcmp(emissions.data(), d.emissions, emissions.size() * 4) && !std::memcmp(grid_min, d.wide8_grid_min, 12) &&
               !std::memcmp(grid_cell, d.wide8_grid_cell, 12);
    }
};
int main() {
    srand(11);
    SceneBuilder sb;
    ImageData image;
    image.width = image.height = 16; image.format = HIPR_TEXEL_R8;
    for (int k = 0; k < 256; ++k) image.pixels.push_back(k % 16 < 12 && k / 16 < 12 ? 255 : 0);
    const uint32_t coverage = sb.add_texture(image, true, true, false, false);
    HiprMaterial lace = SceneBuilder::make_material(RGB(0.8f), 0.7f, 0.04f, 0.0f, HIPR_MATERIAL_CUTOUT | HIPR_MATERIAL_THIN_WALLED);
    lace.coverage_texture_ID = int32_t(coverage);
    lace.coverage = 0.5f;
    const uint32_t cutout = sb.add_material(lace), matte = sb.add_material(SceneBuilder::make_material(RGB(0.5f), 0.5f, 0.04f, 0.0f));
    const uint32_t mapped = sb.add_mesh(grid(7, true, false)), tinted = sb.add_mesh(grid(5, false, true));
    sb.add_model(mapped, cutout, Transform(Vector3f(0, 0, 0)));
    sb.add_model(mapped, cutout, Transform(Vector3f(2, 0, 0), Quaternionf::identity(), -1.0f));      // mirrored: index triples of its own
    sb.add_model(tinted, matte, Transform(Vector3f(0, 2, 0)));
    sb.add_light(SceneBuilder::sphere_light(Vector3f(0, 2, 2), RGB(1.0f), 0.1f));
    sb.finalize();
    const uint32_t mesh_vertices[2] = {64, 36}, mesh_of[2] = {mapped, tinted};
    uint32_t ranges[2][5];
    for (int m = 0; m < 2; ++m) { uint32_t r[5]; if (!sb.mesh_range(mesh_of[m], r) || r[1] != mesh_vertices[m]) return fail("mesh_range", -1); std::memcpy(ranges[m], r, sizeof(r)); }
    unsigned moved_total = 0, changed_total = 0;
    for (int round = 0; round < 40; ++round) {
        const HiprSceneDesc& before = sb.desc();
        Held held(before);
        // the edits, and the arrays they point into
        const int count = 1 + rand() % 12;
        std::vector<std::vector<HiprVertexGeometry>> geometry(count);
        std::vector<std::vector<float>> texcoords(count), emissions(count);
        std::vector<std::vector<uint32_t>> tints(count);
        std::vector<SceneBuilder::VertexEdit> edits;
        std::vector<HiprVertexEdit> pool_edits;
        for (int k = 0; k < count; ++k) {
            const int m = rand() % 2;
            const uint32_t n = mesh_vertices[m];
            uint32_t first = uint32_t(rand()) % n, length = 1 + uint32_t(rand()) % (n - first);
            if (k == 0) { first = 0; length = 1 + uint32_t(rand()) % n; }                 // the pools' first vertex (mesh 0 comes first) ...
            if (k == 1) { first = n - 1 - uint32_t(rand()) % 3; length = n - first; }      // ... and a mesh's last
            const int which = 1 + rand() % 15;
            if (which & 1) for (uint32_t v = 0; v < length; ++v) {
                const HiprVertexGeometry& g = before.geometry[ranges[m][0] + first + v];
                const Vector3f normal(0.1f * unit(), 0.1f * unit(), 1.0f);
                geometry[k].push_back(SceneBuilder::vertex_geometry(Vector3f(g.position[0], g.position[1], g.position[2] + 0.02f * (unit() - 0.5f)), &normal));
            }
            if (which & 2) for (uint32_t v = 0; v < 2 * length; ++v) texcoords[k].push_back(1.5f * unit() - 0.25f);
            if (which & 4) for (uint32_t v = 0; v < length; ++v) tints[k].push_back(uint32_t(rand()));
            if (which & 8) for (uint32_t v = 0; v < 3 * length; ++v) emissions[k].push_back(unit());
            edits.push_back({mesh_of[m], first, length, geometry[k].empty() ? nullptr : geometry[k].data(), texcoords[k].empty() ? nullptr : texcoords[k].data(), tints[k].empty() ? nullptr : tints[k].data(),
                             emissions[k].empty() ? nullptr : emissions[k].data()});
            pool_edits.push_back({ranges[m][0] + first, length, edits.back().geometry, edits.back().texcoords, edits.back().tints, edits.back().emissions});
        }
        double area = 0.0;
        uint32_t out4[4];
        const int walked = vertex_update_host_scene(held.triangles.data(), before.triangle_count, before.instances, before.instance_count, before.materials, before.indices, held.geometry.data(),
                                                    held.texcoords.data(), held.tints.data(), held.emissions.data(), before.vertex_count, before.textures, before.texture_count, before.texels,
                                                    pool_edits.data(), uint32_t(pool_edits.size()), held.trace.data(), held.shade.data(), held.classes.data(), held.slots.data(),
                                                    before.wide8_slot_count, held.grid_min, held.grid_cell, &area, out4);
        if (walked != 0) return fail("the walk asked for a rebuild or refused", round);
        moved_total += out4[3]; changed_total += out4[2];
        if (round % 2 == 0) {
            bool refused = false;
            if (!sb.update_vertices(edits, 1e30, &refused) || refused) return fail("update_vertices", round);
        } else {
            std::vector<HiprVertexEdit> staged;
            if (!sb.stage_vertex_edits(edits, staged) || staged.size() != pool_edits.size()) return fail("stage_vertex_edits", round);
            for (size_t k = 0; k < staged.size(); ++k)
                if (staged[k].first_vertex != pool_edits[k].first_vertex || staged[k].vertex_count != pool_edits[k].vertex_count) return fail("the staged edits' pool coordinates", round);
            if (!sb.apply_staged_transforms(1e30)) return fail("apply_staged_transforms", round);
        }
        if (!held.equals(sb.desc())) return fail("the walk and the builder disagree", round);
    }
    if (!moved_total || !changed_total) return fail("no triangle moved or no flag changed: the rounds tested nothing", 40);
    // the refusals: nothing may be touched
    Held kept(sb.desc());
    const uint32_t word = 0;
    const float bad[2] = {0.0f, HUGE_VALF};
    bool refused = false;
    const std::vector<SceneBuilder::VertexEdit> refusals = {{99, 0, 1, nullptr, nullptr, &word, nullptr}, {mapped, 64, 1, nullptr, nullptr, &word, nullptr}, {mapped, 63, 2, nullptr, nullptr, &word, nullptr},
                                                            {mapped, 0, 0, nullptr, nullptr, &word, nullptr}, {mapped, 0, 1, nullptr, nullptr, nullptr, nullptr}, {mapped, 0, 1, nullptr, bad, nullptr, nullptr},
                                                            {mapped, 0xFFFFFFFFu, 2, nullptr, nullptr, &word, nullptr}};
    for (const SceneBuilder::VertexEdit& e : refusals) {
        std::vector<HiprVertexEdit> staged;
        if (sb.update_vertices({e}, 1.5, &refused) || !refused || sb.stage_vertex_edits({e}, staged) || sb.has_staged_transforms()) return fail("a refusal was taken", 41);
    }
    if (!kept.equals(sb.desc())) return fail("a refusal touched the scene", 41);
    printf("40 rounds of vertex edits walked and applied (%u triangles moved, %u flags changed); 7 refusals left the scene alone\n", moved_total, changed_total);
    return 0;
}
