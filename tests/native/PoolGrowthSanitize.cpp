// PoolGrowthSanitize.cpp -- a stand-alone program around SceneBuilder::staged_scene_growth and grow_host_indices (PoolGrowthHost.hip: the mirror routine of
// csrc/pool_growth.h walked on the host in the kernel's shape) for a run under AddressSanitizer / UndefinedBehaviorSanitizer on the CPU:
// `make -C bifrost3d_amd sanitize-pool-growth` builds and runs it, the scene builder and its tree builders compiled in; it links no product library.
// The scene: a 12 x 12 quad mesh drawn by three instances. Four growths, each staged, walked over a copy of the pools as they were and held to the builder's own
// pools after rebuild(): a new mesh with a model; a mirrored copy of a resident mesh (a mirror segment alone); a new mesh with a model and its mirror in one call; a
// mesh, its mirror and another mesh -- the first with texcoords -- with a texture and a material. Then a mirror range that reaches past the pool as it stands: refused.
#include "../../bifrost3d_amd/host/SceneBuilder.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace HIPRenderer;
extern "C" long long grow_host_indices(uint32_t* pool, uint32_t resident, uint64_t capacity, const HiprPoolGrowth* growth);
static MeshData grid(int cells, float lift, bool texcoords) {
    MeshData m;
    for (int i = 0; i <= cells; ++i)
        for (int j = 0; j <= cells; ++j) {
            m.positions.push_back(Vector3f(float(i) / cells, float(j) / cells, lift * (rand() / float(RAND_MAX))));
            if (texcoords) m.texcoords.push_back(Vector2f{float(i) / cells, float(j) / cells});
        }
    auto at = [&](int i, int j) { return uint32_t(i * (cells + 1) + j); };
    for (int i = 0; i < cells; ++i)
        for (int j = 0; j < cells; ++j) { m.primitives.push_back(Vector3ui{at(i, j), at(i + 1, j), at(i + 1, j + 1)}); m.primitives.push_back(Vector3ui{at(i, j), at(i + 1, j + 1), at(i, j + 1)}); }
    return m;
}
// The pools of a built scene, copied: what the device holds until the next growth.
struct Pools {
    std::vector<uint32_t> indices, tints;
    std::vector<HiprVertexGeometry> geometry;
    std::vector<float> texcoords, emissions;
    std::vector<HiprMaterial> materials;
    std::vector<HiprTexture> textures;
    std::vector<uint8_t> texels;
    explicit Pools(const HiprSceneDesc& d)
        : indices(d.indices, d.indices + d.index_count), geometry(d.geometry, d.geometry + d.vertex_count), materials(d.materials, d.materials + d.material_count),
          textures(d.textures, d.textures + d.texture_count), texels(d.texels, d.texels + d.texel_bytes) {
        if (d.texcoords) texcoords.assign(d.texcoords, d.texcoords + 2 * size_t(d.vertex_count));
        if (d.tints) tints.assign(d.tints, d.tints + d.vertex_count);
        if (d.emissions) emissions.assign(d.emissions, d.emissions + 3 * size_t(d.vertex_count));
    }
};
template <typename T> static void append(std::vector<T>& pool, const T* tail, size_t count) { if (count) pool.insert(pool.end(), tail, tail + count); }
// An attribute pool: its tail behind a resident pool, the whole pool where there was none.
template <typename T> static bool attribute(std::vector<T>& pool, const T* array, uint32_t covered, size_t stride, size_t created, size_t vertices) {
    if (!pool.empty()) { if (covered != created) return false; append(pool, array, stride * covered); return true; }
    if (covered != 0 && covered != vertices) return false;
    append(pool, array, stride * covered);
    return true;
}
template <typename T> static bool same(const std::vector<T>& pool, const T* array, size_t count) { return pool.size() == count && (count == 0 || std::memcmp(pool.data(), array, count * sizeof(T)) == 0); }
// What hipr_append_scene_pools does with the staged growth, on copies of the pools as they were; then rebuild(), whose pools must be the same bytes.
static bool staged_walked_and_rebuilt(SceneBuilder& sb, Pools pools, size_t expected_segments, size_t expected_edits) {
    SceneBuilder::StagedGrowth staged;
    std::vector<HiprInstanceEdit> edits;
    if (!sb.staged_scene_growth(staged, edits) || staged.segments.size() != expected_segments || edits.size() != expected_edits) return false;
    const HiprPoolGrowth& g = staged.growth;
    size_t words = pools.indices.size();
    for (const HiprIndexSegment& s : staged.segments) words += s.index_count;
    const uint32_t resident = uint32_t(pools.indices.size());
    pools.indices.resize(words, 0xA5A5A5A5u);
    if (grow_host_indices(pools.indices.data(), resident, pools.indices.size(), &g) != (long long)words) return false;
    const size_t vertices = pools.geometry.size() + g.vertex_count;
    append(pools.geometry, g.geometry, g.vertex_count);
    if (!attribute(pools.texcoords, g.texcoords, g.texcoord_vertices, 2, g.vertex_count, vertices) || !attribute(pools.tints, g.tints, g.tint_vertices, 1, g.vertex_count, vertices) ||
        !attribute(pools.emissions, g.emissions, g.emission_vertices, 3, g.vertex_count, vertices))
        return false;
    append(pools.materials, g.materials, g.material_count);
    append(pools.textures, g.textures, g.texture_count);
    append(pools.texels, g.texels, size_t(g.texel_bytes));
    sb.rebuild();
    const HiprSceneDesc& d = sb.desc();
    return same(pools.indices, d.indices, d.index_count) && same(pools.geometry, d.geometry, d.vertex_count) && same(pools.texcoords, d.texcoords, d.texcoords ? 2 * size_t(d.vertex_count) : 0) &&
           same(pools.tints, d.tints, d.tints ? size_t(d.vertex_count) : 0) && same(pools.emissions, d.emissions, d.emissions ? 3 * size_t(d.vertex_count) : 0) &&
           same(pools.materials, d.materials, d.material_count) && same(pools.textures, d.textures, d.texture_count) && same(pools.texels, d.texels, size_t(d.texel_bytes)) &&
           d.instance_count == expected_edits;
}
static int fail(const char* what) { printf("FAILED: %s\n", what); return 1; }
int main() {
    srand(12);
    SceneBuilder sb;
    const uint32_t matte = sb.add_material(SceneBuilder::make_material(RGB(0.8f), 0.7f, 0.04f, 0.0f));
    const uint32_t mesh = sb.add_mesh(grid(12, 0.05f, false));
    sb.add_model(mesh, matte, Transform(Vector3f(0, 0, 0)));
    sb.add_model(mesh, matte, Transform(Vector3f(1.5f, 0, 0.2f)));
    sb.add_model(mesh, matte, Transform(Vector3f(3.0f, 0.1f, 0)));
    sb.add_light(SceneBuilder::sphere_light(Vector3f(0, 2, 0), RGB(1.0f), 0.1f));
    sb.finalize();
    const Transform mirror(Vector3f(0.5f, 1.5f, 0), Quaternionf::identity(), -0.5f);
    // 1: a new mesh with a model
    {
        const Pools pools(sb.desc());
        const uint32_t small = sb.add_mesh(grid(3, 0.02f, false));
        sb.insert_model(1, small, matte, Transform(Vector3f(0.2f, 1.2f, 0)));
        if (!staged_walked_and_rebuilt(sb, pools, 1, 4)) return fail("a new mesh with a model");
    }
    // 2: a mirrored copy of a resident mesh
    {
        const Pools pools(sb.desc());
        sb.insert_model(0, mesh, matte, mirror);
        if (!staged_walked_and_rebuilt(sb, pools, 1, 5)) return fail("a mirrored copy of a resident mesh");
    }
    // 3: a new mesh with a model and its mirror in one call
    {
        const Pools pools(sb.desc());
        const uint32_t five = sb.add_mesh(grid(5, 0.03f, false));
        sb.insert_model(1000, five, matte, Transform(Vector3f(2.0f, 1.3f, 0)));
        sb.insert_model(2, five, matte, Transform(Vector3f(3.0f, 1.3f, 0), Quaternionf::identity(), -1.0f));
        if (!staged_walked_and_rebuilt(sb, pools, 2, 7)) return fail("a new mesh with a model and its mirror");
    }
    // 4: a mesh with the scene's first texcoords, its mirror, another mesh; a texture and a material
    {
        const Pools pools(sb.desc());
        ImageData image;
        image.width = 4; image.height = 4; image.format = HIPR_TEXEL_R8;
        for (int k = 0; k < 16; ++k) image.pixels.push_back(uint8_t(17 * k));
        const uint32_t texture = sb.add_texture(image, true, true, false, false);
        HiprMaterial cut = SceneBuilder::make_material(RGB(0.5f), 0.5f, 0.04f, 0.0f, HIPR_MATERIAL_CUTOUT | HIPR_MATERIAL_THIN_WALLED);
        cut.coverage = 0.5f; cut.coverage_texture_ID = int32_t(texture);
        const uint32_t cutout = sb.add_material(cut);
        const uint32_t textured = sb.add_mesh(grid(2, 0.0f, true));
        sb.insert_model(3, textured, cutout, mirror);
        const uint32_t plain = sb.add_mesh(grid(4, 0.01f, false));
        sb.insert_model(1000, plain, matte, Transform(Vector3f(4.0f, 1.0f, 0.3f)));
        if (!staged_walked_and_rebuilt(sb, pools, 3, 9)) return fail("a mesh, its mirror and another mesh with a texture and a material");
    }
    printf("4 growths staged and walked: the pools equal the rebuilt builder's\n");
    // a mirror range that reaches into the segment's own place
    {
        const HiprSceneDesc& d = sb.desc();
        std::vector<uint32_t> pool(d.indices, d.indices + d.index_count);
        const uint32_t resident = uint32_t(pool.size()), triples = resident / 3;
        pool.resize(resident + 30, 0xA5A5A5A5u);
        const HiprIndexSegment past = {triples - 9, 30};      // ten triples from nine before the end
        HiprPoolGrowth g = {};
        g.segments = &past; g.segment_count = 1;
        if (grow_host_indices(pool.data(), resident, pool.size(), &g) != -1) return fail("a mirror range past the pool was taken");
        for (size_t k = resident; k < pool.size(); ++k)
            if (pool[k] != 0xA5A5A5A5u) return fail("a refused segment wrote");
        printf("a mirror range past the pool: refused\n");
    }
    return 0;
}
