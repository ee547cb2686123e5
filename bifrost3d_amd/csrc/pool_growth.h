// pool_growth.h -- the device work of hipr_append_scene_pools: the resident pools grown at their tails, so that a model over a NEW mesh, material or texture can
// be created by hipr_edit_scene_instances without a flatten on the host and an upload of every pool (the reference loads a mesh, a texture or a material into
// buffers of its own and leaves the rest of the scene where it lives, OR/Renderer.cpp:92-136, :703-812). Every pool of the scene builder is append-only: growth
// is a tail.
//
// The yardstick is BYTE EQUALITY of every pool with SceneBuilder::add_mesh / add_material / add_texture (and the mirrored index copy of index_offset_for),
// rebuild() and hipr_upload_scene on a fresh context.
//   -  grow_pool           per pool: the new allocation when the resident one has no room, the device-to-device copy of the resident part, the host-to-device
//                          copy of the tail. A pool whose buffer has the room takes its tail in place.
//   -  k_mirror_triples    one thread per triple of a MIRROR segment of the index pool: the triple at `from + t` of the pool as it stands, written at `to + t`
//                          with the second and third corner exchanged (SceneBuilder::index_offset_for). `from + count <= to`: the host has checked the range
//                          against the pool as it stands when the segment is reached, so source and destination never overlap; earlier segments of the same
//                          call are read where the stream has put them. A mirror segment transfers nothing from the host.
// All of it on the context's stream, in sequence; plain vector loads and stores, no atomics, no LDS.
//
// mirror_triple is __host__ __device__ so that the CPU suite can walk it against the scene builder (tests/native/PoolGrowthHost.hip).
#pragma once

#include <cstddef>
#include <cstdint>

#ifndef BHD
#define BHD __host__ __device__ inline
#endif

namespace hipr {

constexpr int POOL_GROWTH_BLOCK = 256;

// Triple t of a mirror segment: indices[3 (to + t) ..] = (a, c, b) of indices[3 (from + t) ..].
BHD void mirror_triple(uint32_t* indices, uint32_t from, uint32_t to, uint32_t t) {
    const uint32_t* source = indices + 3 * size_t(from + t);
    uint32_t* target = indices + 3 * size_t(to + t);
    const uint32_t a = source[0], b = source[1], c = source[2];
    target[0] = a; target[1] = c; target[2] = b;
}

#if defined(__HIPCC__) && !defined(HIPR_REBUILD_HOST_ONLY)      // the kernel and the copies; a host build of the routine (tests/native/PoolGrowthHost.hip) leaves them out

__global__ __launch_bounds__(POOL_GROWTH_BLOCK) void k_mirror_triples(uint32_t* __restrict__ indices, uint32_t from, uint32_t to, uint32_t count) {
    const uint32_t t = blockIdx.x * uint32_t(POOL_GROWTH_BLOCK) + threadIdx.x;
    if (t < count) mirror_triple(indices, from, to, t);
}

// One pool's copies: the `keep` resident bytes into the new allocation (nothing when the pool grows in place, `grown` == `resident`), the tail behind them.
inline hipError_t queue_pool_growth(void* grown, const void* resident, size_t keep, const void* tail, size_t tail_bytes, hipStream_t stream) {
    if (grown != resident && keep)
        if (hipError_t e = hipMemcpyAsync(grown, resident, keep, hipMemcpyDeviceToDevice, stream)) return e;
    if (tail_bytes)
        if (hipError_t e = hipMemcpyAsync(static_cast<char*>(grown) + keep, tail, tail_bytes, hipMemcpyHostToDevice, stream)) return e;
    return hipSuccess;
}

// A mirror segment of `count` triples, queued behind whatever wrote [from, from + count).
inline void queue_mirror_triples(uint32_t* indices, uint32_t from, uint32_t to, uint32_t count, hipStream_t stream) {
    if (count) hipLaunchKernelGGL(k_mirror_triples, dim3((count + POOL_GROWTH_BLOCK - 1) / POOL_GROWTH_BLOCK), dim3(POOL_GROWTH_BLOCK), 0, stream, indices, from, to, count);
}

#endif

} // namespace hipr
