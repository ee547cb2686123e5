// vertex_update.h -- vertex edits of resident meshes applied to the resident scene on the device (hipr_update_scene_vertices): new positions, normals, texture
// coordinates, tints or emissions of vertices the device already holds are a copy into the four vertex pools plus what an upload DERIVES from vertex data -- the
// world-space corners of the triangles that read an edited position, the scene's bounds and the 8-wide tree's grid, the leaf records and the quantised boxes, the
// trace and shading records, and HIPR_TRIANGLE_OPAQUE of the triangles whose material leaves the decision to its coverage texture (covered_everywhere,
// material_rules.h) with everything that repeats it. (The reference's Meshes know "created" and "destroyed" only, Assets/Mesh.h: it cannot express the edit.)
//
// The yardstick is BYTE EQUALITY with the host path, SceneBuilder::update_vertices and a fresh upload. The passes, all on the context's stream, one after the other;
// no block waits on another, the reductions are min / max with the earliest corner winning, an integer AND and three counts -- all order independent:
//   pass 1  k_write_vertex_words       ONE launch whatever the number of edits, a thread per 4-byte word (every element -- 16, 8, 4, 12 bytes -- is a multiple of 4).
//                                      The host resolves the list order -- where two edits overlap the later one wins -- into DISJOINT segments (plan_vertex_edits), so
//                                      that no two threads write the same word, and packs their rows into the staging buffer in table order: a segment's source
//                                      word is its first thread word, and the table is (first word, pool and destination word), prefix-summed. A block of 256
//                                      words meets at most 256 segments (a segment has at least one word): it finds its first segment in the table, copies its
//                                      part of the table to LDS, and every lane of its waves searches that part. No byte outside a range is written. An edited
//                                      vertex is MARKED by a byte per pool vertex and kind (geometry, texcoords), zeroed per call and stored idempotently.
//   pass 2  k_refit_marked_triangles   the sibling of k_refit_triangles (wide8_refit.h): a triangle one of whose three pool vertices -- through its instance's own
//                                      index triple -- is marked gets its corners recomputed with refit_world_corner; every triangle feeds the bounds reduction
//                                      (refit_reduce_bounds, k_refit_bounds_final); the moved triangles are counted by a wave ballot and one atomic per wave.
//   then    the refit of the tree (k_refit_leaves, k_refit_nodes, k_refit_area) and the records (triangle_records.h), as they are.
//   pass 3  k_reflag_marked_triangles  the body of the material edit's pass (update_triangle_material, material_update.h) with `touched` set for a triangle that reads a
//                                      marked texture coordinate and whose instance's material leaves the decision to its coverage texture; counts as the texel
//                                      edit's (texel_update.h). Then k_update_leaf_flags (material_update.h, unchanged).
//
// The bodies are __host__ __device__ so that tests/native/VertexUpdateHost.hip can compile them for the host and the CPU suite can hold them to
// SceneBuilder::update_vertices without a GPU. This header includes material_rules.h: it must NEVER reach the fast-math shade unit (see there).
#pragma once

#include "material_update.h"
#include "wide8_refit.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

namespace hipr {

// The four vertex pools, in the order of HiprVertexEdit's pointers, and the 4-byte words of an element of each.
constexpr uint32_t VERTEX_POOL_GEOMETRY = 0, VERTEX_POOL_TEXCOORDS = 1, VERTEX_POOL_TINTS = 2, VERTEX_POOL_EMISSIONS = 3, VERTEX_POOLS = 4;
MRHD uint32_t vertex_pool_words(uint32_t pool) { return pool == VERTEX_POOL_GEOMETRY ? 4u : (pool == VERTEX_POOL_TEXCOORDS ? 2u : (pool == VERTEX_POOL_TINTS ? 1u : 3u)); }

// One disjoint range of destination words. Threads [first_word, the next segment's first_word) copy staging word = thread word to word `destination & MASK` + their
// offset of pool `destination >> 62`.
struct VertexSegment { uint64_t first_word, destination; };
constexpr uint64_t VERTEX_DESTINATION_MASK = (uint64_t(1) << 62) - 1u;

// What the host makes of an edit list (checked: hipr_update_scene_vertices' refusals): the table, the ranges of the callers' arrays that survive, in table order,
// and which pools are written at all.
struct VertexPlan {
    struct Piece { const uint8_t* source; uint64_t bytes; };
    std::vector<VertexSegment> table;
    std::vector<Piece> pieces;
    uint64_t word_count = 0;
    bool carries[VERTEX_POOLS] = {false, false, false, false};
};

inline void plan_vertex_edits(const HiprVertexEdit* edits, uint32_t edit_count, VertexPlan& plan) {
    plan = {};
    for (uint32_t pool = 0; pool < VERTEX_POOLS; ++pool) {
        const uint64_t words = vertex_pool_words(pool);
        std::map<uint64_t, uint64_t> covered;      // disjoint [begin, end) of vertices later edits write
        struct Range { uint64_t begin, end; const uint8_t* source; };      // source: of vertex `begin`
        std::vector<Range> kept;
        for (uint32_t k = edit_count; k-- > 0;) {
            const HiprVertexEdit& e = edits[k];
            const void* array = pool == VERTEX_POOL_GEOMETRY ? static_cast<const void*>(e.geometry) : (pool == VERTEX_POOL_TEXCOORDS ? static_cast<const void*>(e.texcoords)
                              : (pool == VERTEX_POOL_TINTS ? static_cast<const void*>(e.tints) : static_cast<const void*>(e.emissions)));
            if (!array) continue;
            plan.carries[pool] = true;
            const uint64_t begin = e.first_vertex, end = begin + e.vertex_count;
            // the parts of [begin, end) no later edit covers
            uint64_t at = begin;
            auto next = covered.upper_bound(begin);
            if (next != covered.begin() && std::prev(next)->second > at) at = std::prev(next)->second;
            for (; at < end; ++next) {
                const uint64_t stop = next != covered.end() && next->first < end ? next->first : end;
                if (stop > at) kept.push_back({at, stop, static_cast<const uint8_t*>(array) + (at - begin) * words * 4u});
                if (next == covered.end() || next->first >= end) break;
                at = std::max(at, next->second);
            }
            // ... and [begin, end) joins the covered ranges
            uint64_t lo = begin, hi = end;
            auto it = covered.lower_bound(begin);
            if (it != covered.begin() && std::prev(it)->second >= begin) --it;
            while (it != covered.end() && it->first <= hi) { lo = std::min(lo, it->first); hi = std::max(hi, it->second); it = covered.erase(it); }
            covered[lo] = hi;
        }
        std::sort(kept.begin(), kept.end(), [](const Range& a, const Range& b) { return a.begin < b.begin; });
        for (const Range& r : kept) {
            plan.table.push_back({plan.word_count, uint64_t(pool) << 62 | r.begin * words});
            plan.pieces.push_back({r.source, (r.end - r.begin) * words * 4u});
            plan.word_count += (r.end - r.begin) * words;
        }
    }
}
// The rows of a plan packed in table order: plan.word_count words at `data`.
inline void pack_vertex_rows(const VertexPlan& plan, uint8_t* data) {
    for (const VertexPlan::Piece& p : plan.pieces) { std::memcpy(data, p.source, size_t(p.bytes)); data += p.bytes; }
}

// The pools as words and the marks (a byte per pool vertex; null: that kind is not marked).
struct VertexPools { uint32_t* pool[VERTEX_POOLS]; uint8_t* marks[2]; };

// The last of table[0 .. count) whose first word is at most `word`; table[0].first_word <= word.
MRHD uint32_t find_vertex_segment(const VertexSegment* table, uint32_t count, uint64_t word) {
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (table[mid].first_word <= word) lo = mid; else hi = mid;
    }
    return lo;
}

// Pass 1 for thread word `word` of segment `s`: the word, and the mark of its vertex (the threads of one element store the same byte).
MRHD void write_vertex_word(const VertexSegment& s, uint64_t word, const uint32_t* data, const VertexPools& p) {
    const uint32_t pool = uint32_t(s.destination >> 62);
    const uint64_t at = (s.destination & VERTEX_DESTINATION_MASK) + (word - s.first_word);
    p.pool[pool][at] = data[word];
    if (pool == VERTEX_POOL_GEOMETRY && p.marks[0]) p.marks[0][at >> 2] = uint8_t(1);
    if (pool == VERTEX_POOL_TEXCOORDS && p.marks[1]) p.marks[1][at >> 1] = uint8_t(1);
}

// Does primitive `primitive_index` of `inst` read a marked pool vertex? Through the instance's own index triple: a mirrored instance has its own.
MRHD bool reads_marked_vertex(const HiprInstance& inst, uint32_t primitive_index, const uint32_t* indices, const uint8_t* marks) {
    const uint32_t* idx = indices + 3 * size_t(inst.index_offset + primitive_index);
    return (marks[size_t(inst.vertex_offset) + idx[0]] | marks[size_t(inst.vertex_offset) + idx[1]] | marks[size_t(inst.vertex_offset) + idx[2]]) != 0;
}

// Pass 2 for `tri` (a copy): false when it reads no marked vertex, otherwise its corners as SceneBuilder computes them.
MRHD bool refit_marked_triangle(HiprTriangle& tri, const HiprInstance* instances, const uint32_t* indices, const HiprVertexGeometry* geometry, const uint8_t* marks) {
    const HiprInstance& inst = instances[tri.instance_index];
    if (!reads_marked_vertex(inst, tri.primitive_index, indices, marks)) return false;
    const uint32_t* idx = indices + 3 * size_t(inst.index_offset + tri.primitive_index);
    float* corners[3] = {tri.v0, tri.v1, tri.v2};
    for (int k = 0; k < 3; ++k) refit_world_corner(inst.object_to_world, geometry[size_t(inst.vertex_offset) + idx[k]].position, corners[k]);
    return true;
}

// The words of passes 2 and 3: the AND of "opaque" (preset to 1), the triangles decided again, those whose flags changed, the triangles moved.
constexpr uint32_t VERTEX_WORD_OPAQUE = 0, VERTEX_WORD_DECIDED = 1, VERTEX_WORD_CHANGED = 2, VERTEX_WORD_MOVED = 3, VERTEX_SCRATCH_WORDS = 16;

// Pass 3 for triangle t. a.touched: a word per instance -- its material leaves its triangles' flags to a coverage texture and its mesh has texture coordinates.
MRHD void reflag_marked_triangle(const MaterialUpdateArrays& a, const uint8_t* marks, uint32_t t, bool& opaque, bool& decided, bool& changed) {
    const HiprTriangle& tri = a.triangles[t];
    const uint32_t before = tri.flags;
    decided = a.touched[tri.instance_index] != 0 && reads_marked_vertex(a.instances[tri.instance_index], tri.primitive_index, a.indices, marks);
    bool coated;
    update_triangle_material(a, t, decided, opaque, coated);
    changed = a.triangles[t].flags != before;
}

#if defined(__HIPCC__) && !defined(HIPR_MATERIAL_UPDATE_HOST_ONLY) && !defined(HIPR_REFIT_HOST_ONLY)      // the kernels; a host build of the bodies leaves them out

constexpr int VERTEX_UPDATE_BLOCK = 256;

// grid: word_count / block. table[0 .. segment_count), data[0 .. word_count).
__global__ __launch_bounds__(VERTEX_UPDATE_BLOCK) void k_write_vertex_words(const VertexSegment* __restrict__ table, uint32_t segment_count, const uint32_t* __restrict__ data, uint64_t word_count,
                                                                          VertexPools pools) {
    __shared__ VertexSegment part[VERTEX_UPDATE_BLOCK];
    const uint64_t block_word = uint64_t(blockIdx.x) * uint32_t(VERTEX_UPDATE_BLOCK);
    const uint32_t first = find_vertex_segment(table, segment_count, block_word);      // the same for every thread of the block
    const uint32_t count = segment_count - first < uint32_t(VERTEX_UPDATE_BLOCK) ? segment_count - first : uint32_t(VERTEX_UPDATE_BLOCK);
    if (threadIdx.x < count) part[threadIdx.x] = table[first + threadIdx.x];
    __syncthreads();
    const uint64_t word = block_word + threadIdx.x;
    if (word >= word_count) return;
    write_vertex_word(part[find_vertex_segment(part, count, word)], word, data, pools);
}

// words[VERTEX_WORD_MOVED] preset to 0. Every thread of the grid takes part in the reduction (threads past the end with neutral bounds).
__global__ __launch_bounds__(REFIT_BLOCK) void k_refit_marked_triangles(HiprTriangle* __restrict__ triangles, uint32_t triangle_count, const HiprInstance* __restrict__ instances,
                                                                        const uint8_t* __restrict__ marks, const uint32_t* __restrict__ indices, const HiprVertexGeometry* __restrict__ geometry,
                                                                        RefitBound* __restrict__ partial, uint32_t* __restrict__ words) {
    const uint32_t t = blockIdx.x * uint32_t(REFIT_BLOCK) + threadIdx.x;
    RefitBound bound[6];
    for (int k = 0; k < 6; ++k) bound[k] = {k < 3 ? FLT_MAX : -FLT_MAX, 0xFFFFFFFFu};
    bool moved = false;
    if (t < triangle_count) {
        HiprTriangle tri = triangles[t];
        moved = refit_marked_triangle(tri, instances, indices, geometry, marks);
        if (moved)
            for (int r = 0; r < 3; ++r) { triangles[t].v0[r] = tri.v0[r]; triangles[t].v1[r] = tri.v1[r]; triangles[t].v2[r] = tri.v2[r]; }
        const float* corners[3] = {tri.v0, tri.v1, tri.v2};
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) {
                const RefitBound p = {corners[k][a], 3u * t + uint32_t(k)};
                bound[a] = refit_lower(bound[a], p);
                bound[3 + a] = refit_upper(bound[3 + a], p);
            }
    }
    const unsigned long long have_moved = __ballot(moved);
    if ((threadIdx.x & 63u) == 0 && have_moved) atomicAdd(&words[VERTEX_WORD_MOVED], uint32_t(__popcll(have_moved)));
    refit_reduce_bounds(bound, partial);
}

// words[VERTEX_WORD_OPAQUE] preset to 1, the others to 0
__global__ __launch_bounds__(VERTEX_UPDATE_BLOCK) void k_reflag_marked_triangles(MaterialUpdateArrays a, const uint8_t* __restrict__ marks, uint32_t* __restrict__ words) {
    const uint32_t t = blockIdx.x * uint32_t(VERTEX_UPDATE_BLOCK) + threadIdx.x;
    bool opaque = true, decided = false, changed = false;      // neutral: the threads past the end
    if (t < a.triangle_count) reflag_marked_triangle(a, marks, t, opaque, decided, changed);
    const unsigned long long not_opaque = __ballot(!opaque), were_decided = __ballot(decided), have_changed = __ballot(changed);
    if ((threadIdx.x & 63u) == 0) {
        if (not_opaque) atomicAnd(&words[VERTEX_WORD_OPAQUE], 0u);
        if (were_decided) atomicAdd(&words[VERTEX_WORD_DECIDED], uint32_t(__popcll(were_decided)));
        if (have_changed) atomicAdd(&words[VERTEX_WORD_CHANGED], uint32_t(__popcll(have_changed)));
    }
}

#endif // the kernels

} // namespace hipr
