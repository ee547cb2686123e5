// VertexPoseHost.hip -- the pose kernel's body (csrc/vertex_pose.h), compiled for the HOST by hipcc's host pass (tests/native/libvertex_pose_host.so).
//
// Test infrastructure (tests/test_vertex_pose_on_host_cpu.py, tests/native/VertexPoseSanitize.cpp); nothing here is linked into or loaded by the product, which has
// no CPU path.
//
// check_rig_descs, pack_rig, check_rig_poses, plan_rig_poses and pose_vertex are host or __host__ __device__ functions; `hipcc --cuda-host-only -ffp-contract=off`
// yields an x86 build of exactly the statements hipr_set_scene_rigs, hipr_pose_scene_rigs and k_pose_vertices run. vertex_pose_host_walk runs them over a geometry
// pool in the kernel's shape -- the block table of the staging copy, blocks backwards, each with its matrices copied to a stand-in for the LDS when the rig fits
// the budget, threads backwards -- so that the CPU suite can hold the walk to SceneBuilder byte for byte without a GPU.
#define HIPR_VERTEX_POSE_HOST_ONLY 1      // not the kernel: this build holds host code only
#include "../../bifrost3d_amd/csrc/vertex_pose.h"

#include <vector>

using namespace hipr;

extern "C" {

// hipr_set_scene_rigs + hipr_pose_scene_rigs up to the pool writes, on host arrays: `geometry` (vertex_count rows, in place) and `marks` (a byte per pool vertex,
// set where a vertex was posed; may be null). lds_joints: the budget applied, at most POSE_LDS_CAPACITY. Returns the number of vertices posed, -1 when the rigs are
// refused, -2 when the poses are, -3 on a null array or a budget above the kernel's.
long long vertex_pose_host_walk(const HiprRigDesc* rigs, uint32_t rig_count, const HiprRigPose* poses, uint32_t pose_count, uint32_t lds_joints, HiprVertexGeometry* geometry, uint8_t* marks,
                                uint32_t vertex_count) {
    if (!geometry || lds_joints > POSE_LDS_CAPACITY) return -3;
    if (check_rig_descs(rigs, rig_count, vertex_count)) return -1;
    std::vector<uint32_t> words;
    std::vector<PoseRig> records(rig_count);
    std::vector<RigBook> books(rig_count);
    for (uint32_t k = 0; k < rig_count; ++k) pack_rig(rigs[k], words, records[k], books[k]);
    if (check_rig_poses(poses, pose_count, books.data(), books.size())) return -2;
    PosePlan plan;
    plan_rig_poses(poses, pose_count, books.data(), plan);
    const PoseBlock* blocks = reinterpret_cast<const PoseBlock*>(plan.staging.data());
    const PoseCall* calls = reinterpret_cast<const PoseCall*>(plan.staging.data() + plan.calls_at);
    const float* floats = reinterpret_cast<const float*>(plan.staging.data() + plan.floats_at);
    long long posed = 0;
    for (uint32_t b = plan.block_count; b-- > 0;) {
        const PoseBlock block = blocks[b];
        const PoseCall call = calls[block.call];
        const PoseRigView rig = view_of(records[call.rig], words.data());
        const float* matrices = floats + call.matrices;
        const bool in_lds = rig.joint_count && rig.joint_count <= lds_joints;
        std::vector<float> staged(size_t(POSE_LDS_CAPACITY) * POSE_LDS_STRIDE, -7.0e37f);      // the block's LDS: what is not staged holds nothing useful
        if (in_lds)
            for (uint32_t i = 12u * rig.joint_count; i-- > 0;) staged[(i / 12u) * POSE_LDS_STRIDE + i % 12u] = matrices[i];
        for (uint32_t thread = POSE_BLOCK; thread-- > 0;) {
            const uint32_t v = block.first + thread;
            if (v >= rig.vertex_count) continue;
            geometry[size_t(rig.first_vertex) + v] = in_lds ? pose_vertex(rig, v, staged.data(), POSE_LDS_STRIDE, floats + call.target_weights) : pose_vertex(rig, v, matrices, 12u, floats + call.target_weights);
            if (marks) marks[size_t(rig.first_vertex) + v] = uint8_t(1);
            ++posed;
        }
    }
    return posed;
}

// pose_encode_octahedral, the header's restatement of OctahedralNormal::encode_precise, for n normals.
void vertex_pose_host_encode(const float* normals_n3, uint32_t n, int16_t* out_n2) {
    for (uint32_t i = 0; i < n; ++i) pose_encode_octahedral(normals_n3 + 3u * size_t(i), out_n2 + 2u * size_t(i));
}

// The roundings the header counts for a position component, the LDS budget in joints that ships and the kernel's capacity.
uint32_t vertex_pose_host_roundings(uint32_t target_count) { return pose_roundings(target_count); }
uint32_t vertex_pose_host_lds_joints() { return POSE_LDS_JOINTS; }
uint32_t vertex_pose_host_lds_capacity() { return POSE_LDS_CAPACITY; }

}
