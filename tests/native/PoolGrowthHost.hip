// PoolGrowthHost.hip -- the mirror routine of hipr_append_scene_pools (csrc/pool_growth.h), compiled for the HOST by hipcc's host pass
// (tests/native/libpool_growth_host.so).
//
// Test infrastructure (tests/test_pool_growth_on_host_cpu.py, tests/native/PoolGrowthSanitize.cpp); nothing here is linked into or loaded by the product, which has
// no CPU path.
//
// grow_host_indices walks what ResidentScene::append_pools queues for the index pool, in its order: the host segments copied to their place in the tail, every
// mirror segment as its launch -- blocks of POOL_GROWTH_BLOCK threads, the threads of a launch taken BACKWARDS, those past the count doing nothing -- over the
// pool as it stands by then. The CPU suite holds the result to SceneBuilder::add_mesh / index_offset_for byte for byte.
#define HIPR_REBUILD_HOST_ONLY 1
#include <hip/hip_runtime.h>

#include "../../bifrost3d_amd/csrc/pool_growth.h"
#include "../../include/hiprenderer_c.h"

#include <cstring>

using namespace hipr;

extern "C" {

// One launch of k_mirror_triples over `indices`: (count + block - 1) / block blocks. Returns the threads that wrote.
uint32_t mirror_host_triples(uint32_t* indices, uint32_t from, uint32_t to, uint32_t count) {
    const uint32_t blocks = (count + POOL_GROWTH_BLOCK - 1) / POOL_GROWTH_BLOCK;
    uint32_t wrote = 0;
    for (uint32_t block = blocks; block-- > 0;)
        for (uint32_t thread = POOL_GROWTH_BLOCK; thread-- > 0;) {
            const uint32_t t = block * uint32_t(POOL_GROWTH_BLOCK) + thread;
            if (t < count) { mirror_triple(indices, from, to, t); ++wrote; }
        }
    return wrote;
}

// `pool`: room for `capacity` index words, of which the first `resident` are the pool before the call. The segments of `growth` are applied as
// hipr_append_scene_pools checks and applies them. Returns the words the pool holds afterwards, or -1 for what the entry point refuses (the pool is then untouched
// past `resident` only as far as the walk came: the caller compares nothing after a refusal).
long long grow_host_indices(uint32_t* pool, uint32_t resident, uint64_t capacity, const HiprPoolGrowth* growth) {
    if (!pool || !growth || (growth->segment_count && !growth->segments) || (growth->index_count && !growth->indices)) return -1;
    uint64_t position = resident, taken = 0;
    for (uint32_t k = 0; k < growth->segment_count; ++k) {      // check_pool_growth's walk, before anything is written
        const HiprIndexSegment& s = growth->segments[k];
        if (s.index_count % 3u) return -1;
        if (s.mirrored_from == HIPR_SEGMENT_FROM_HOST) taken += s.index_count;
        else if (3ull * s.mirrored_from + s.index_count > position) return -1;
        position += s.index_count;
        if (position > capacity || position > 0xFFFFFFFFull) return -1;
    }
    if (taken != growth->index_count) return -1;
    position = resident; taken = 0;
    for (uint32_t k = 0; k < growth->segment_count; ++k) {
        const HiprIndexSegment& s = growth->segments[k];
        if (s.mirrored_from == HIPR_SEGMENT_FROM_HOST) {
            if (s.index_count) std::memcpy(pool + position, growth->indices + taken, size_t(s.index_count) * 4);
            taken += s.index_count;
        } else if (mirror_host_triples(pool, s.mirrored_from, uint32_t(position / 3), s.index_count / 3) != s.index_count / 3) return -1;
        position += s.index_count;
    }
    return (long long)position;
}

}
