// InstanceEditSanitize.cpp -- a stand-alone program around edit_host_scene (InstanceEditHost.hip: the routines of csrc/instance_edit.h walked on the host, chained with
// the walks of the BVH2 build and the 8-wide collapse) for a run under AddressSanitizer / UndefinedBehaviorSanitizer on the CPU:
// `make -C bifrost3d_amd sanitize-instance-edit` builds and runs it; it links no product library. The scene: a 12 x 12 quad mesh drawn by three instances, stored in a
// shuffled order (the old tree's). The edits: the middle instance removed; a fourth appended; the first removed, one inserted in the middle and one appended in one
// call. Then a new instance whose index triple points past the vertex pool, and a resident position claimed twice: both refused with nothing written.
#include "../../include/hiprenderer_c.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
extern "C" int edit_host_scene(const HiprTriangle*, const uint8_t*, uint32_t, const HiprSceneDesc*, const HiprInstanceEdit*, uint32_t, uint32_t, uint32_t, HiprTriangle*, uint8_t*, HiprBvhNode*, uint32_t*,
                               HiprSlot8*, uint32_t*);
static const int CELLS = 12;
static HiprInstance instance_at(float x, float y, float z, int32_t id) {
    HiprInstance i;
    std::memset(&i, 0, sizeof i);
    i.object_to_world[0] = i.object_to_world[5] = i.object_to_world[10] = 1.0f;
    i.object_to_world[3] = x; i.object_to_world[7] = y; i.object_to_world[11] = z;
    i.instance_id = (1 << 30) | id;
    i.material_index = 1;
    return i;
}
static HiprInstanceEdit kept(uint32_t source) { HiprInstanceEdit e; std::memset(&e, 0, sizeof e); e.source = source; return e; }
static HiprInstanceEdit created(const HiprInstance& i, uint32_t primitives) { HiprInstanceEdit e; std::memset(&e, 0, sizeof e); e.source = HIPR_EDIT_NEW_INSTANCE; e.primitive_count = primitives; e.instance = i; return e; }
int main() {
    // the pools: one mesh, two materials (slot 0 the invalid one), no textures
    std::vector<HiprVertexGeometry> geometry(size_t(CELLS + 1) * (CELLS + 1));
    std::memset(geometry.data(), 0, geometry.size() * sizeof(HiprVertexGeometry));
    srand(12);
    for (int i = 0; i <= CELLS; ++i) for (int j = 0; j <= CELLS; ++j) { float* p = geometry[size_t(i) * (CELLS + 1) + j].position; p[0] = float(i) / CELLS; p[1] = float(j) / CELLS; p[2] = 0.05f * (rand() / float(RAND_MAX)); }
    std::vector<uint32_t> indices;
    auto at = [](int i, int j) { return uint32_t(i * (CELLS + 1) + j); };
    for (int i = 0; i < CELLS; ++i) for (int j = 0; j < CELLS; ++j) {
        const uint32_t quad[6] = {at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j), at(i + 1, j + 1), at(i, j + 1)};
        indices.insert(indices.end(), quad, quad + 6);
    }
    const uint32_t primitives = uint32_t(indices.size() / 3);
    std::vector<HiprMaterial> materials(2);
    std::memset(materials.data(), 0, materials.size() * sizeof(HiprMaterial));
    materials[1].coverage = 1.0f;
    HiprTexture none;
    std::memset(&none, 0, sizeof none);
    std::vector<HiprInstance> instances = {instance_at(0, 0, 0, 1), instance_at(1.5f, 0, 0.2f, 2), instance_at(3.0f, 0.1f, 0, 3)};
    // the resident triangles: flattened as the scene builder does, then shuffled with a class byte that names instance + primitive
    std::vector<HiprTriangle> flat;
    for (uint32_t i = 0; i < instances.size(); ++i)
        for (uint32_t p = 0; p < primitives; ++p) {
            HiprTriangle t;
            std::memset(&t, 0, sizeof t);
            float* corners[3] = {t.v0, t.v1, t.v2};
            for (int k = 0; k < 3; ++k) for (int r = 0; r < 3; ++r) corners[k][r] = geometry[indices[3 * p + k]].position[r] + instances[i].object_to_world[4 * r + 3];
            t.instance_index = i; t.primitive_index = p; t.flags = HIPR_TRIANGLE_OPAQUE | HIPR_TRIANGLE_ONE_SIDED;
            flat.push_back(t);
        }
    const uint32_t n = uint32_t(flat.size());
    std::vector<uint32_t> where(n);
    for (uint32_t i = 0; i < n; ++i) where[i] = i;
    for (uint32_t i = n; i-- > 1;) std::swap(where[i], where[uint32_t(rand()) % (i + 1)]);
    std::vector<HiprTriangle> resident(n);
    std::vector<uint8_t> classes(n);
    for (uint32_t i = 0; i < n; ++i) { resident[i] = flat[where[i]]; classes[i] = uint8_t((flat[where[i]].instance_index + flat[where[i]].primitive_index) & 1u); }
    HiprSceneDesc pools;
    std::memset(&pools, 0, sizeof pools);
    pools.instances = instances.data(); pools.instance_count = uint32_t(instances.size());
    pools.indices = indices.data(); pools.index_count = uint32_t(indices.size());
    pools.geometry = geometry.data(); pools.vertex_count = uint32_t(geometry.size());
    pools.materials = materials.data(); pools.material_count = uint32_t(materials.size());
    pools.textures = &none; pools.texture_count = 1;

    const HiprInstance fourth = instance_at(1.5f, 1.5f, 0, 4), fifth = instance_at(0.2f, -1.5f, 0.3f, 5);
    const std::vector<std::vector<HiprInstanceEdit>> lists = {
        {kept(0), kept(2)},
        {kept(0), kept(1), kept(2), created(fourth, primitives)},
        {kept(1), created(fifth, primitives), kept(2), created(fourth, primitives)},
    };
    const uint32_t capacity = 4 * n;
    int walked = 0;
    for (const std::vector<HiprInstanceEdit>& list : lists) {
        std::vector<HiprTriangle> triangles(capacity); std::vector<uint8_t> out_classes(capacity); std::vector<HiprBvhNode> nodes(capacity); std::vector<uint32_t> order(capacity);
        std::vector<HiprSlot8> slots(2 * size_t(capacity)); uint32_t out[16] = {};
        const int status = edit_host_scene(resident.data(), classes.data(), n, &pools, list.data(), uint32_t(list.size()), 62, capacity, triangles.data(), out_classes.data(), nodes.data(), order.data(),
                                           slots.data(), out);
        printf("a list of %zu: status %d, %u triangles, %u BVH2 nodes, deepest %u, %u slots, height %u\n", list.size(), status, out[0], out[1], out[2], out[3], out[4]);
        if (status != 0 || out[0] != primitives * list.size() || out[14] != 1u || out[15] != 1u) return 1;      // every triangle opaque; some kept class bytes are set
        std::vector<bool> seen(out[0], false);
        for (uint32_t k = 0; k < out[0]; ++k) {      // `order` is a permutation, and the triangle at place k is the one of flatten position order[k] of the NEW list
            const HiprTriangle& t = triangles[k];
            if (order[k] >= out[0] || seen[order[k]] || t.instance_index >= list.size() || t.instance_index * primitives + t.primitive_index != order[k]) { printf("place %u is wrong\n", k); return 1; }
            seen[order[k]] = true;
            const HiprInstance& inst = list[t.instance_index].source == HIPR_EDIT_NEW_INSTANCE ? list[t.instance_index].instance : instances[list[t.instance_index].source];
            if (t.v0[0] != geometry[indices[3 * t.primitive_index]].position[0] + inst.object_to_world[3]) { printf("place %u holds another corner\n", k); return 1; }
            const uint32_t source = list[t.instance_index].source;      // a kept triangle's class byte goes along, a new one's is its material's (no coat)
            if (out_classes[k] != (source == HIPR_EDIT_NEW_INSTANCE ? 0u : uint8_t((source + t.primitive_index) & 1u))) { printf("place %u holds another class byte\n", k); return 1; }
        }
        ++walked;
    }
    for (int refusal = 0; refusal < 2; ++refusal) {
        std::vector<uint32_t> bad_indices = indices;
        std::vector<HiprTriangle> bad_resident = resident;
        if (refusal == 0) bad_indices[3 * 17 + 1] = uint32_t(geometry.size());      // one past the pool
        else bad_resident[5].primitive_index = bad_resident[6].instance_index == bad_resident[5].instance_index ? bad_resident[6].primitive_index : (bad_resident[5].primitive_index + 1) % primitives;
        HiprSceneDesc p = pools;
        p.indices = bad_indices.data();
        std::vector<HiprTriangle> triangles(capacity); std::vector<uint8_t> out_classes(capacity); std::vector<HiprBvhNode> nodes(capacity); std::vector<uint32_t> order(capacity, 0xA5A5A5A5u);
        std::vector<HiprSlot8> slots(2 * size_t(capacity)); uint32_t out[16] = {};
        const int status = edit_host_scene(bad_resident.data(), classes.data(), n, &p, lists[1].data(), uint32_t(lists[1].size()), 62, capacity, triangles.data(), out_classes.data(), nodes.data(), order.data(),
                                           slots.data(), out);
        printf("%s: status %d\n", refusal == 0 ? "an index past the vertex pool" : "a position claimed twice", status);
        if (status != (refusal == 0 ? 4 : 1) || out[0] || order[0] != 0xA5A5A5A5u) return 1;
    }
    printf("%d lists walked\n", walked);
    return walked == 3 ? 0 : 1;
}
