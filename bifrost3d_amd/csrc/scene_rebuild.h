// scene_rebuild.h -- the passes of hipr_rebuild_scene_trees that are not the two builds': the resident scene's trees rebuilt on the device, in place, from the
// triangles it holds (the reference asks OptiX for a "Trbvh" build, which runs on the GPU over the geometry the device holds, OR/Renderer.cpp:161-182,471-476; a
// moved node marks its acceleration dirty and the next launch rebuilds it there, OR/Renderer.cpp:472,1010-1041).
//
// The yardstick is BYTE EQUALITY with the host path: SceneBuilder::rebuild() followed by hipr_upload_scene on a fresh context. After a device refit the resident
// triangles are the host's world-space triangles byte for byte (wide8_refit.h pass 1), stored in the order of the OLD tree's leaves; the host builds over them in
// the order SceneBuilder::finalize flattens in -- instances in order, primitives in order -- and both builders' results depend on that order. So:
//   1  k_rebuild_count     the triangles of every instance counted: one integer atomic per wave and instance at most. The host prefix-sums instance_count words:
//                          first[i] = the flatten position of primitive 0 of instance i.
//   2  k_rebuild_scatter   every resident triangle and its class byte go to first[instance] + primitive_index of a flat scratch array. A claim word per position
//                          (an integer atomic add) raises the status flag when two triangles claim one position, or one lies outside its instance's range: the
//                          second claimant writes nothing, and the call refuses before anything resident is replaced.
//   -  the BVH2 build of bvh2_build.h over the flat array: its `order` is BvhBuildResult::order, position k <- flatten position order[k].
//   3  k_rebuild_levels    the hand-over to the collapse. The build creates its nodes level by level (BuildState::nodes, a level's nodes consecutive) and
//                          k_build_place gives each its depth-first place: place[] read in creation order IS the collapse's list of reachable nodes level by
//                          level, and the build's level sizes are the list's level boundaries. No host index walk and no re-upload. What w8_check_input asserts
//                          holds by construction for this library's own BVH2: children are placed after their parents inside the array, every node is placed
//                          exactly once, leaf ranges partition [0, count) and are met in ascending order depth first (the left child's range precedes the
//                          right's), and the build's levels are bounded by its depth limit, which the caller holds to W8_MAX_LEVELS. Within a level the list's
//                          order is the creation order, not the ascending one of w8_check_input: every pass of the collapse treats a level's nodes
//                          independently, so nothing of it reaches the output.
//   -  the collapse of wide8_build.h over the placed nodes, the flat array and `order`.
//   4  k_rebuild_gather    the new resident triangles and class bytes: position k <- flat[order[k]].
// All of it on the context's stream, launches in sequence: no block waits on another, nothing spins, integer atomics only.
//
// The routines are __host__ __device__ so that the CPU suite can walk them against SceneBuilder::rebuild() without a GPU.
#pragma once

#include "bvh2_build.h"

namespace hipr {

constexpr uint32_t REBUILD_STATUS_CLAIM = 0, REBUILD_STATUS_WORDS = 4;      // status[0]: a flatten position claimed twice, or a triangle outside its instance's range

struct RebuildArrays {
    const HiprTriangle* resident; const uint8_t* resident_class;      // the scene's triangles in the old tree's order, and their class bytes
    uint32_t triangle_count, instance_count;
    uint32_t* instance_counts;            // per instance: its triangles (pass 1)
    const uint32_t* first;                // instance_count + 1 words: the exclusive prefix sums of instance_counts (the host's)
    HiprTriangle* flat; uint8_t* flat_class; uint32_t* claim;      // per flatten position
    uint32_t* status;
};

// One whole 48-byte record: three 16-byte words on the device (every array here starts at an allocation's base, so a record is 16-byte aligned).
BHD void rebuild_copy_triangle(HiprTriangle* to, const HiprTriangle* from) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(sizeof(HiprTriangle) == 48, "three 16-byte words");
    const uint4* s = reinterpret_cast<const uint4*>(from);
    uint4* d = reinterpret_cast<uint4*>(to);
    const uint4 a = s[0], b = s[1], c = s[2];
    d[0] = a; d[1] = b; d[2] = c;
#else
    *to = *from;
#endif
}

// Pass 1, one triangle: the instance it counts for, BUILD_NONE (and the flag) for an instance index out of range.
BHD uint32_t rebuild_instance_of(const RebuildArrays& a, uint32_t t) {
    const uint32_t instance = a.resident[t].instance_index;
    if (instance < a.instance_count) return instance;
    a.status[REBUILD_STATUS_CLAIM] = 1u;      // every thread that gets here stores the same word
    return BUILD_NONE;
}
BHD void rebuild_count(const RebuildArrays& a, uint32_t t) {
    const uint32_t instance = rebuild_instance_of(a, t);
    if (instance != BUILD_NONE) build_atomic_add(a.instance_counts + instance, 1u);
}
// Pass 2, one triangle.
BHD void rebuild_scatter(const RebuildArrays& a, uint32_t t) {
    const HiprTriangle& triangle = a.resident[t];
    const uint32_t instance = triangle.instance_index, primitive = triangle.primitive_index;
    if (instance >= a.instance_count || primitive >= a.first[instance + 1] - a.first[instance]) { a.status[REBUILD_STATUS_CLAIM] = 1u; return; }
    const uint32_t position = a.first[instance] + primitive;      // < first[instance + 1] <= triangle_count: the host has checked the total
    if (build_atomic_add(a.claim + position, 1u) != 0u) { a.status[REBUILD_STATUS_CLAIM] = 1u; return; }
    rebuild_copy_triangle(a.flat + position, &triangle);
    a.flat_class[position] = a.resident_class[t];
}
// Pass 3, one node in creation order.
BHD void rebuild_level_node(const uint32_t* place, uint32_t* level_nodes, uint32_t node) { level_nodes[node] = place[node]; }
// Pass 4, one position of the new order.
BHD void rebuild_gather(const HiprTriangle* flat, const uint8_t* flat_class, const uint32_t* order, HiprTriangle* triangles, uint8_t* triangle_class, uint32_t k) {
    const uint32_t from = order[k];
    rebuild_copy_triangle(triangles + k, flat + from);
    triangle_class[k] = flat_class[from];
}

#if defined(__HIPCC__) && !defined(HIPR_REBUILD_HOST_ONLY)      // the kernels; a host build of the routines (tests/native/DeviceRebuildHost.hip) leaves them out

constexpr int REBUILD_BLOCK = 256;

// The lanes of a wave that count for one instance add once: in the old tree's order a wave's triangles belong to a handful of instances.
__global__ __launch_bounds__(REBUILD_BLOCK) void k_rebuild_count(RebuildArrays a) {
    const uint32_t t = blockIdx.x * uint32_t(REBUILD_BLOCK) + threadIdx.x;
    const uint32_t instance = t < a.triangle_count ? rebuild_instance_of(a, t) : BUILD_NONE;
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long todo = __ballot(instance != BUILD_NONE);      // wave-uniform: every lane runs every round
    while (todo) {
        const int leader = __ffsll(todo) - 1;
        const uint32_t which = uint32_t(__shfl(int(instance), leader, 64));
        const unsigned long long same = __ballot(instance == which);
        if (lane == uint32_t(leader)) atomicAdd(a.instance_counts + which, uint32_t(__popcll(same)));
        todo &= ~same;
    }
}
__global__ __launch_bounds__(REBUILD_BLOCK) void k_rebuild_scatter(RebuildArrays a) {
    const uint32_t t = blockIdx.x * uint32_t(REBUILD_BLOCK) + threadIdx.x;
    if (t < a.triangle_count) rebuild_scatter(a, t);
}
__global__ __launch_bounds__(REBUILD_BLOCK) void k_rebuild_levels(const uint32_t* __restrict__ place, uint32_t* __restrict__ level_nodes, uint32_t node_count) {
    const uint32_t k = blockIdx.x * uint32_t(REBUILD_BLOCK) + threadIdx.x;
    if (k < node_count) rebuild_level_node(place, level_nodes, k);
}
__global__ __launch_bounds__(REBUILD_BLOCK) void k_rebuild_gather(const HiprTriangle* __restrict__ flat, const uint8_t* __restrict__ flat_class, const uint32_t* __restrict__ order,
                                                                  HiprTriangle* __restrict__ triangles, uint8_t* __restrict__ triangle_class, uint32_t triangle_count) {
    const uint32_t k = blockIdx.x * uint32_t(REBUILD_BLOCK) + threadIdx.x;
    if (k < triangle_count) rebuild_gather(flat, flat_class, order, triangles, triangle_class, k);
}

#endif // the kernels

} // namespace hipr
