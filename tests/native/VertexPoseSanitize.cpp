// VertexPoseSanitize.cpp -- a stand-alone program around the rig poses' host side (csrc/vertex_pose.h: the checks, the packing, the plan) with the host walk of the
// pose kernel's body (vertex_pose_host_walk, VertexPoseHost.hip) and SceneBuilder::set_rigs / pose_rigs / stage_rig_poses / posed_geometry for a run under
// AddressSanitizer / UndefinedBehaviorSanitizer on the CPU: `make -C bifrost3d_amd sanitize-vertex-pose` builds and runs it, the scene builder and its tree
// builders compiled in; it links no product library.
// The scene: a 9 x 9 grid mesh worn by a model and by a mirrored one, and a 5 x 5 mesh without normals. 30 rounds: random rigs over random ranges of both meshes
// (the pool's first and last vertex among them; 1 to 400 joints, so that both matrix paths are walked; 0 to 3 targets with and without normals), a random pose of
// each, walked over a copy of the builder's geometry pool with a random LDS budget and applied to the builder, alternately through pose_rigs and through
// stage_rig_poses twice + apply_staged_transforms; the pools must agree byte for byte after every round, and so must posed_geometry. A last round asks for refusals.
#include "../../bifrost3d_amd/host/SceneBuilder.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace HIPRenderer;
extern "C" long long vertex_pose_host_walk(const HiprRigDesc* rigs, uint32_t rig_count, const HiprRigPose* poses, uint32_t pose_count, uint32_t lds_joints, HiprVertexGeometry* geometry, uint8_t* marks,
                                           uint32_t vertex_count);
static float unit() { return rand() / float(RAND_MAX); }
static MeshData grid(int cells, bool normals) {
    MeshData m;
    for (int i = 0; i <= cells; ++i)
        for (int j = 0; j <= cells; ++j) {
            m.positions.push_back(Vector3f(float(i) / cells, float(j) / cells, 0.05f * unit()));
            if (normals) m.normals.push_back(Vector3f(0, 0, 1));
        }
    auto at = [&](int i, int j) { return uint32_t(i * (cells + 1) + j); };
    for (int i = 0; i < cells; ++i)
        for (int j = 0; j < cells; ++j) { m.primitives.push_back(Vector3ui{at(i, j), at(i + 1, j), at(i + 1, j + 1)}); m.primitives.push_back(Vector3ui{at(i, j), at(i + 1, j + 1), at(i, j + 1)}); }
    return m;
}
static int fail(const char* what, int round) { printf("FAILED: %s (round %d)\n", what, round); return 1; }
// A rig's arrays and a pose's, kept alive beside the descriptions that point into them.
struct RigData {
    std::vector<float> positions, normals, weights, target_positions, target_normals, matrices, target_weights, other_matrices, other_target_weights;
    std::vector<uint16_t> joints;
};
int main() {
    srand(17);
    SceneBuilder sb;
    const uint32_t matte = sb.add_material(SceneBuilder::make_material(RGB(0.5f), 0.5f, 0.04f, 0.0f));
    const uint32_t shaded = sb.add_mesh(grid(9, true)), bare = sb.add_mesh(grid(5, false));
    sb.add_model(shaded, matte, Transform(Vector3f(0, 0, 0)));
    sb.add_model(shaded, matte, Transform(Vector3f(2, 0, 0), Quaternionf::identity(), -1.0f));      // mirrored: index triples of its own
    sb.add_model(bare, matte, Transform(Vector3f(0, 2, 0)));
    sb.add_light(SceneBuilder::sphere_light(Vector3f(0, 2, 2), RGB(1.0f), 0.1f));
    sb.finalize();
    const uint32_t mesh_vertices[2] = {100, 36}, mesh_of[2] = {shaded, bare};
    uint32_t offsets[2];
    for (int m = 0; m < 2; ++m) { uint32_t r[5]; if (!sb.mesh_range(mesh_of[m], r) || r[1] != mesh_vertices[m]) return fail("mesh_range", -1); offsets[m] = r[0]; }
    unsigned long long posed_total = 0;
    for (int round = 0; round < 30; ++round) {
        // one rig per mesh over a random range; round 0 takes the pool's first vertex, round 1 its last
        std::vector<RigData> data(2);
        std::vector<SceneBuilder::RigDesc> rigs;
        std::vector<HiprRigDesc> pooled;
        std::vector<HiprRigPose> poses, other;
        for (int m = 0; m < 2; ++m) {
            const uint32_t n = mesh_vertices[m];
            uint32_t first = uint32_t(rand()) % n, count = 1 + uint32_t(rand()) % (n - first);
            if (round == 0 && m == 0) first = 0;
            if (round == 1 && m == 1) { first = n - 1; count = 1; }
            const uint32_t joint_choices[5] = {0, 1, 2, 320, 400};
            uint32_t joints = joint_choices[rand() % 5], targets = uint32_t(rand()) % 4;
            if (!joints && !targets) joints = 1;
            RigData& d = data[m];
            for (uint32_t v = 0; v < count; ++v) {
                for (int c = 0; c < 3; ++c) d.positions.push_back(unit() - 0.5f);
                if (m == 0) { d.normals.push_back(unit() - 0.5f); d.normals.push_back(unit() - 0.5f); d.normals.push_back(0.5f + unit()); }
                for (int s = 0; s < 4 && joints; ++s) { d.joints.push_back(uint16_t(uint32_t(rand()) % joints)); d.weights.push_back(s == 0 ? 0.5f : (rand() % 3 ? 0.0f : 0.5f * unit())); }
            }
            const bool target_normals = m == 0 && targets && rand() % 2;
            for (size_t i = 0; i < 3u * size_t(count) * targets; ++i) { d.target_positions.push_back(0.1f * (unit() - 0.5f)); if (target_normals) d.target_normals.push_back(unit() - 0.5f); }
            for (size_t i = 0; i < 12u * size_t(joints); ++i) { d.matrices.push_back(i % 5 == 0 ? 1.0f : 0.2f * (unit() - 0.5f)); d.other_matrices.push_back(unit()); }
            for (uint32_t t = 0; t < targets; ++t) { d.target_weights.push_back(rand() % 4 ? unit() : 0.0f); d.other_target_weights.push_back(-unit()); }
            if (joints && rand() % 6 == 0) std::fill(d.matrices.begin(), d.matrices.begin() + 12, 0.0f);      // a collapsed joint
            HiprRigDesc r = {first, count, joints, targets, d.positions.data(), m == 0 ? d.normals.data() : nullptr, joints ? d.joints.data() : nullptr, joints ? d.weights.data() : nullptr,
                             targets ? d.target_positions.data() : nullptr, target_normals ? d.target_normals.data() : nullptr};
            rigs.push_back({mesh_of[m], r});
            r.first_vertex += offsets[m];
            pooled.push_back(r);
            poses.push_back({uint32_t(m), 0u, joints ? d.matrices.data() : nullptr, targets ? d.target_weights.data() : nullptr});
            other.push_back({uint32_t(m), 0u, joints ? d.other_matrices.data() : nullptr, targets ? d.other_target_weights.data() : nullptr});
        }
        if (!sb.set_rigs(rigs)) return fail("set_rigs refused a sound list", round);
        const HiprSceneDesc& before = sb.desc();
        std::vector<HiprVertexGeometry> held(before.geometry, before.geometry + before.vertex_count);
        std::vector<uint8_t> marks(before.vertex_count, uint8_t(0));
        const uint32_t budgets[4] = {0, 1, 2, 320};
        const long long posed = vertex_pose_host_walk(pooled.data(), 2, poses.data(), 2, budgets[rand() % 4], held.data(), marks.data(), before.vertex_count);
        if (posed != (long long)(pooled[0].vertex_count + pooled[1].vertex_count)) return fail("the walk posed another number of vertices", round);
        posed_total += (unsigned long long)posed;
        if (round % 2 == 0) {
            bool refused = true;
            sb.pose_rigs(poses, 1e30, &refused);
            if (refused) return fail("pose_rigs refused sound poses", round);
        } else {
            std::vector<HiprRigPose> pool_poses;
            if (!sb.stage_rig_poses(other, pool_poses) || !sb.stage_rig_poses(poses, pool_poses) || pool_poses.size() != 4) return fail("stage_rig_poses", round);
            sb.apply_staged_transforms(1e30);
        }
        const HiprSceneDesc& after = sb.desc();
        if (std::memcmp(held.data(), after.geometry, held.size() * sizeof(HiprVertexGeometry))) return fail("the walk and the builder disagree in the geometry pool", round);
        for (int m = 0; m < 2; ++m) {
            std::vector<HiprVertexGeometry> rows(pooled[m].vertex_count);
            if (!SceneBuilder::posed_geometry(rigs[m].rig, poses[m], rows.data())) return fail("posed_geometry refused", round);
            if (std::memcmp(rows.data(), after.geometry + pooled[m].first_vertex, rows.size() * sizeof(HiprVertexGeometry))) return fail("posed_geometry and the builder disagree", round);
        }
    }
    // refusals: nothing may be touched
    {
        std::vector<float> positions(3 * 4, 0.25f), weights(4 * 4, 0.25f), matrices(12 * 2, 0.5f);
        std::vector<uint16_t> joints(4 * 4, uint16_t(1));
        HiprRigDesc good = {0, 4, 2, 0, positions.data(), nullptr, joints.data(), weights.data(), nullptr, nullptr};
        if (!sb.set_rigs({{bare, good}})) return fail("the sound rig", 99);
        HiprRigDesc bad = good;
        bad.vertex_count = 0;
        if (sb.set_rigs({{bare, bad}})) return fail("no vertices", 99);
        bad = good; bad.first_vertex = 33;
        if (sb.set_rigs({{bare, bad}})) return fail("past the mesh", 99);
        bad = good; bad.joint_count = 1;
        if (sb.set_rigs({{bare, bad}})) return fail("joint index", 99);
        bad = good; bad.weights = nullptr;
        if (sb.set_rigs({{bare, bad}})) return fail("null weights", 99);
        if (sb.set_rigs({{bare, good}, {bare, good}})) return fail("overlap", 99);
        weights[5] = NAN;
        if (sb.set_rigs({{bare, good}})) return fail("weight not finite", 99);
        weights[5] = 0.25f;
        bool refused = false;
        sb.pose_rigs({{1u, 0u, matrices.data(), nullptr}}, 1.5, &refused);
        if (!refused) return fail("unbound rig", 99);
        sb.pose_rigs({{0u, 0u, nullptr, nullptr}}, 1.5, &refused);
        if (!refused) return fail("null matrices", 99);
        matrices[7] = INFINITY;
        sb.pose_rigs({{0u, 0u, matrices.data(), nullptr}}, 1.5, &refused);
        if (!refused) return fail("matrix not finite", 99);
        matrices[7] = 0.5f;
        sb.pose_rigs({{0u, 0u, matrices.data(), nullptr}, {0u, 0u, matrices.data(), nullptr}}, 1.5, &refused);
        if (!refused) return fail("the same rig twice", 99);
        if (!sb.set_rigs({}) || sb.rig_count() != 0) return fail("removing the rigs", 99);
    }
    printf("vertex_pose_sanitize: 30 rounds, %llu vertices posed, the walk, pose_rigs, the staged path and posed_geometry agree; refusals touch nothing\n", posed_total);
    return 0;
}
