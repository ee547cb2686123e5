// hiprenderer.hip -- implementation of the C-ABI declared in include/hiprenderer_c.h.
//
// Host side of the MI355X wavefront path tracer: owns the device copies of the scene, the SoA
// path / hit / shadow queues and the f64 accumulation buffer, and drives the per-pass kernel loop
//   generate -> { trace_closest -> shade(+compact) -> trace_shadow } until no path is alive -> accumulate.
// Replaces the OptiX context + context->launch() of OR/Renderer.cpp:273-574,1250-1265.
// A pass (hipr_trace_pass) is begin_pass, start_wavefront for each wavefront, advance_wavefront round robin until none is left (or detach_tail, pipelined);
// a bounce is enqueue_bounce = launch_trace + launch_shade + the read-back of its sizes, and book_bounce keeps the counters of all of them. What tunes a
// context is in Knobs; drain() is where every queued pass has ended, on the device and in the books.
// There is no CPU fallback: every entry point that needs the GPU fails with a status code.
#include "kernels.h"
#ifndef HIPR_WIDE8_LOW_BUCKET
#define HIPR_WIDE8_LOW_BUCKET 0
#endif
#include "wide8_kernels.h"
#include "wide8_refit.h"
#include "material_update.h"
#include "bvh2_build.h"
#include "wide8_build.h"
#include "scene_rebuild.h"
#include "instance_edit.h"
#include "pool_growth.h"
#include "launch.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace hipr;

namespace {

thread_local std::string g_last_error;

int fail(int status, const char* fmt, ...) {
    char buf[512];
    va_list args;
    va_start(args, fmt);
    vsnprintf(buf, sizeof(buf), fmt, args);
    va_end(args);
    g_last_error = buf;
    fprintf(stderr, "hiprenderer: %s\n", buf);
    return status;
}

#define HIP_TRY(call)                                                                                          \
    do {                                                                                                       \
        hipError_t err__ = (call);                                                                             \
        if (err__ != hipSuccess)                                                                               \
            return fail(err__ == hipErrorOutOfMemory ? HIPR_ERROR_OUT_OF_MEMORY : HIPR_ERROR_HIP, "%s failed: %s (%s:%d)", #call, \
                        hipGetErrorString(err__), __FILE__, __LINE__);                                         \
    } while (0)

// Device memory that goes with its owner: movable, not copyable.
struct DeviceBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& other) noexcept : ptr(other.ptr), bytes(other.bytes) { other.ptr = nullptr; other.bytes = 0; }
    DeviceBuffer& operator=(DeviceBuffer&& other) noexcept { std::swap(ptr, other.ptr); std::swap(bytes, other.bytes); return *this; }
    ~DeviceBuffer() { release(); }
    int resize(size_t new_bytes) {
        if (new_bytes <= bytes && ptr) return HIPR_OK;
        if (ptr) { (void)hipFree(ptr); ptr = nullptr; bytes = 0; }
        if (new_bytes == 0) return HIPR_OK;
        HIP_TRY(hipMalloc(&ptr, new_bytes));
        bytes = new_bytes;
        return HIPR_OK;
    }
    int upload(const void* src, size_t n, hipStream_t stream) {
        if (n == 0) return HIPR_OK;
        if (int s = resize(n)) return s;
        HIP_TRY(hipMemcpyAsync(ptr, src, n, hipMemcpyHostToDevice, stream));
        return HIPR_OK;
    }
    void release() { if (ptr) (void)hipFree(ptr); ptr = nullptr; bytes = 0; }
    template <typename T> T* as() const { return static_cast<T*>(ptr); }
};

// A stream, an event or pinned host memory that goes with its owner; reads as the plain handle wherever one is expected.
template <typename T, hipError_t (*FREE)(T)>
struct Owned {
    T handle = nullptr;
    Owned() = default;
    Owned(Owned&& other) noexcept : handle(other.handle) { other.handle = nullptr; }
    Owned& operator=(Owned&& other) noexcept { std::swap(handle, other.handle); return *this; }
    ~Owned() { if (handle) (void)FREE(handle); }
    operator T() const { return handle; }
};
hipError_t free_pinned_words(uint32_t* words) { return hipHostFree(words); }
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
using PinnedWords = Owned<uint32_t*, free_pinned_words>;
// Each leaves the owner empty when HIP refuses: the caller checks the handle.
Stream make_stream() { Stream s; if (hipStreamCreateWithFlags(&s.handle, hipStreamNonBlocking) != hipSuccess) s.handle = nullptr; return s; }
Event make_event(unsigned flags = hipEventDisableTiming) { Event e; if (hipEventCreateWithFlags(&e.handle, flags) != hipSuccess) e.handle = nullptr; return e; }
PinnedWords make_pinned_words(size_t count) { PinnedWords p; if (hipHostMalloc((void**)&p.handle, count * sizeof(uint32_t)) != hipSuccess) p.handle = nullptr; return p; }

struct TimedLaunch { int kernel; hipEvent_t start, stop; };

// One independent wavefront of paths: its own queues, queue sizes and stream. A pass splits its path slots over the
// context's wavefronts; they advance through their bounces independently, so while one of them shades (few resident
// waves, waiting on gathers) the other one traces (many waves, latency bound) on the same CUs.
struct Wavefront {
    Stream own_stream;                  // first member: destroyed after the events and buffers below
    hipStream_t stream = nullptr;       // borrowed: wavefront 0 runs on the context stream, the others on their own
    Event shade_done[2], counts_copied[2], finished;   // by bounce parity: two bounces are in flight
    DeviceBuffer path[2][4], hits, shadow[3], queue_counts, order, nee_flags, sort_keys[2], sort_order, sort_temp;     // sort_*: ray_sort.hip (HIPR_COHERENCE_SORT=1)   // queue_counts: COUNT_LINES 64 B lines (see there); order: k_classify_hits' listing of a bounce's rays
    PinnedWords host_counts;            // pinned: {continuing paths, shadow rays} per bounce parity, [4] staging word
    uint32_t first_slot = 0, n_slots = 0;      // first_slot: the wavefront's phase in the round-robin deal of 64-slot groups (partition_path_slots)

    PathState path_state(int which) const {
        return {path[which][0].as<float4>(), path[which][1].as<float4>(), path[which][2].as<float4>(), path[which][3].as<uint2>()};
    }
    ShadowQueue shadow_queue() const { return {shadow[0].as<float4>(), shadow[1].as<float4>(), shadow[2].as<float4>()}; }
};
constexpr int MAX_WAVEFRONTS = 4;
constexpr int COUNT_PAIR_STRIDE = 16;   // uint32 words between the counters of a wavefront (one 64 B line each)
// A wavefront's counters: lines 0-2 the queue-size pairs {paths, shadow rays}, bounce k reads pair k % 3 and fills pair (k + 1) % 3. Nothing in the stream zeroes
// them between bounces: the shade kernel of bounce k zeroes pair (k + 2) % 3 -- read last by bounce k - 1, whose sizes the host has read back before it queues bounce k.
constexpr int COUNT_PAIRS = 3, COUNT_LINES = 3;
constexpr int HOST_COUNT_WORDS = 8 + COUNT_LINES * COUNT_PAIR_STRIDE;   // pinned: 2 x {paths, shadow rays} read back, [4..8) spare, then the image of the counters at the start of a pass

// What the argument checks of a description derive on their way (preflight_scene).
struct Preflight {
    uint32_t wide_stack_need = 0;       // worst-case stack need of the 4-wide tree: derived, not taken from the caller
    uint32_t wide8_height = 0;          // 0: the description brings no 8-wide tree
};

// The scene the device holds: the uploaded pools, what is derived from them, the argument blocks the kernels take and the host's copies of what later calls are
// checked against. Its writers -- upload() (hipr_upload_scene), update_geometry() (hipr_update_scene_geometry), refit_transforms() (hipr_refit_scene_transforms)
// update_materials() (hipr_update_scene_materials), install_rebuilt_trees() and append_pools() (hipr_append_scene_pools) -- are called once every refusal is behind the entry point and every queued pass has finished, and go: ready = false, device work, publish pointers, counts and
// flags, ready = true. One that fails on the way leaves a scene that answers HIPR_ERROR_NOT_READY until an upload succeeds, never one that names freed memory.
struct ResidentScene {
    DeviceBuffer nodes, wide_nodes, wide8_slots, triangles, instances, lights;                                     // what a geometry update brings again
    DeviceBuffer indices, geometry, texcoords, tints, emissions, materials, textures, texels, environment_PDF, environment_samples;      // ... and leaves in place
    DeviceBuffer shade_triangles, trace_triangles, trace_items;         // derived per triangle (derive_from_triangles)
    DeviceBuffer triangle_class;        // one byte per triangle for the listing pass (k_classify_hits): bit 0 = its material is coated
    DeviceScene args = {};              // also carries what is not the scene's: the tables, the sample offsets, the environment tint (hipr_create, hipr_upload_tables, hipr_set_scene_state)
    Wide8Scene wide8 = {};              // the 8-wide tree with leaf records: what the persistent kernels walk when the scene brings one
    uint32_t wide8_height = 0, wide_stack_entries = 0;
    int stack_size = 16;
    int shading_models = 7;             // bit mask of the shading models the scene's instances reference
    // Kernel instantiations picked by what the pools hold. A geometry update leaves the material, texture and environment pools in place, so these keep what
    // the UPLOAD decided: a refit description with other materials or texture formats must not switch the kernels over pools that still hold the old data.
    // Their second writer is update_materials(), which rewrites the material pool and derives them again from the host copies below.
    bool coverage_textures_r8 = false;  // every coverage texture is HIPR_TEXEL_R8 and linear: k_trace_wide8<..., COVERAGE_R8 = true>
    bool has_environment = true;        // an environment map, a presampled environment light or a float texture: k_shade<..., TEXTURES = 2>; 8-bit textures without those: TEXTURES = 1
    bool has_textures = true;           // a material references a texture, or has_environment: k_shade<..., TEXTURES = true>
    bool all_triangles_opaque = false;  // no triangle needs its material's coverage sampled (HIPR_TRIANGLE_OPAQUE on all): k_trace_wide8<..., COVERAGE = false>
    bool any_coated_triangle = false;
    // Host copies of what the device holds: a geometry update and a device refit are checked against THESE, and what they derive from the pools they leave in
    // place comes from these, not from their own description.
    std::vector<HiprMaterial> uploaded_materials;
    std::vector<uint32_t> uploaded_light_types;
    std::vector<HiprInstance> uploaded_instances;      // a device refit checks a new matrix's handedness against them
    std::vector<HiprTexture> uploaded_textures;        // small; a material edit derives the texture switches from it again
    bool uploaded_environment = false;                 // the upload brought an environment description
    uint32_t uploaded_texture_count = 0, uploaded_vertex_count = 0, uploaded_index_count = 0;
    uint32_t uploaded_mesh_attributes = 0;             // HIPR_MESH_TEXCOORDS | _TINTS | _EMISSIVE: the optional per-vertex pools the upload brought
    uint64_t uploaded_texel_bytes = 0;

    // device refit of the 8-wide tree (wide8_refit.h); filled at upload for scenes that bring the tree
    DeviceBuffer refit_leaf_slots, refit_node_slots, refit_exact, refit_moved, refit_partial, refit_scratch;
    std::vector<uint32_t> refit_level_begin;           // refit_node_slots[level_begin[l], level_begin[l + 1]) = the nodes l levels below the root
    uint32_t refit_leaf_count = 0;
    std::vector<uint32_t> refit_node_list, refit_node_words;      // host copy of refit_node_slots and each node's (base_valid, inner_mask) at the time: the topology the lists hold
    double uploaded_half_area = 0.0, current_half_area = 0.0;
    DeviceBuffer material_touched, material_scratch;   // update_materials: one word per instance; the two reduction words (material_update.h)
    bool tree_stale = false;            // a device refit left the BVH2 and 4-wide arrays behind: hipr_set_trace_variant refuses them until the next upload / geometry update

    bool ready = false;
    // The last writer was a device refit that reported needs_rebuild: the scene is not ready, but its pools and triangles are whole -- the one state besides `ready`
    // that rebuild_trees() accepts. Every writer clears it on its way in, so a scene a failed writer left behind is never taken for it.
    bool awaits_rebuild = false;
    void begin_write() { ready = false; awaits_rebuild = false; }
    // install_rebuilt_trees() replaced the BVH2 and the 8-wide tree and left the 4-wide array of the OLD tree behind: the next geometry update brings the new tree's,
    // whose size and stack need it takes instead of comparing them with the uploaded ones.
    bool wide4_awaits_geometry = false;
    // The search of the uploaded scene, fixed when it is uploaded (hipr_set_trace_variant / HIPR_TRACE_VARIANT name a request for the NEXT upload).
    int chosen_variant = HIPR_TRACE_BVH2;
    void choose_variant(int requested) {
        const bool large = args.node_count > 64;
        int v = requested;
        if (v < 0) v = large ? HIPR_TRACE_WIDE8_PERSISTENT : (args.triangle_count <= SMALL_SCENE_TRIANGLES ? HIPR_TRACE_EXHAUSTIVE : HIPR_TRACE_BVH2);
        if (v == HIPR_TRACE_WIDE8_PERSISTENT && wide8.slot_count == 0) v = HIPR_TRACE_WIDE_PERSISTENT;      // no 8-wide tree (none given, or higher than the LDS stacks)
        if (v == HIPR_TRACE_WIDE_PERSISTENT && args.wide_node_count == 0) v = HIPR_TRACE_BVH2;
        if (v == HIPR_TRACE_EXHAUSTIVE && args.trace_item_count == 0 && args.triangle_count != 0) v = HIPR_TRACE_BVH2;
        chosen_variant = v;
    }

    // `requested_variant`, `cull_backfaces`: the context's settings at the time of the call.
    int upload(const HiprSceneDesc* s, const Preflight& checked, int requested_variant, bool cull_backfaces, hipStream_t stream);
    int update_geometry(const HiprSceneDesc* s, const Preflight& checked, int requested_variant, bool cull_backfaces, hipStream_t stream);
    int refit_transforms(const HiprInstanceTransform* moved, uint32_t moved_count, const HiprLight* new_lights, uint32_t light_count, hipStream_t stream, HiprRefitResult* out);
    int update_materials(const HiprMaterialUpdate* changed, uint32_t changed_count, const HiprInstanceMaterial* assignments, uint32_t assignment_count, hipStream_t stream);
    int lights_keep_their_types(const char* who, const HiprLight* new_lights, uint32_t count) const;
    // What hipr_rebuild_scene_trees hands over once nothing can refuse any more: device arrays of the build's and the collapse's scratch, and the host's copy of the slots.
    struct RebuiltTrees {
        const HiprTriangle* flat; const uint8_t* flat_class; const uint32_t* order;      // the triangles in flatten order, and the new order over them
        const HiprBvhNode* nodes; uint32_t node_count, deepest;
        const HiprSlot8* slots; const HiprSlot8* host_slots; HiprWide8BuildResult wide8;
        // hipr_edit_scene_instances: another SET of triangles and instances comes in (null: the resident ones stay, as after hipr_rebuild_scene_trees)
        struct NewSet {
            uint32_t triangle_count; const HiprInstance* device_instances; const std::vector<HiprInstance>* instances;
            bool all_triangles_opaque, any_coated_triangle;      // reduced over the new set (k_edit_reduce)
        };
        const NewSet* new_set;
    };
    int install_rebuilt_trees(const RebuiltTrees& built, hipStream_t stream);
    // The device work of hipr_append_scene_pools, which has checked the description against the host copies (hipr_internal_check_pool_growth): the pools grown at their tails.
    int append_pools(const HiprPoolGrowth& growth, hipStream_t stream);
    double append_ms[3] = {0.0, 0.0, 0.0};      // of the last append_pools: the allocations (host clock), the device-to-device copies of the resident parts, the tails and the mirror segments (events)
    Event append_events[3];             // made by the first append_pools

private:
    int upload_pools(const HiprSceneDesc* s, bool all_pools, hipStream_t stream);
    void derive_from_pools(const HiprSceneDesc* s);
    void derive_switches_from_pools();
    int derive_from_triangles(const HiprSceneDesc* s, const Preflight& checked, bool new_topology, int requested_variant, bool cull_backfaces, hipStream_t stream);
    void queue_triangle_records(hipStream_t stream) const;
    int upload_wide8(const HiprSceneDesc* s, uint32_t height, bool cull_backfaces, hipStream_t stream);
    int prepare_refit(const HiprSceneDesc* s, bool new_topology, hipStream_t stream);
    template <bool WRITE> void queue_refit_tree(const float* grid_min, const float* grid_cell, hipStream_t stream) const;
};

// What tunes a context: read from the environment once, when the context is made (knobs_from_environment), and written by the setters of the C-ABI that are named here.
struct Knobs {
    int wavefront_limit = 0;            // hipr_set_wavefront_count / HIPR_WAVEFRONTS; 0 = by scene: see HiprContext::wavefronts_wanted()
    int trace_variant = -1;             // hipr_set_trace_variant / HIPR_TRACE_VARIANT: the search of the NEXT upload (HIPR_TRACE_*), -1: pick by BVH size
    int arithmetic = HIPR_ARITHMETIC_FAST;     // hipr_set_arithmetic / HIPR_ARITHMETIC=exact: which build of the shade unit the context launches (launch.h ShadeUnit)
    bool cull_backfaces = true;         // hipr_set_backface_culling / HIPR_BACKFACE_CULLING=0
    bool pipeline_passes = false;       // hipr_set_pass_pipelining / HIPR_PIPELINE_PASSES=1; off by default: measured slower
    int pipeline_spare_blocks = 1;      // HIPR_PIPELINE_SPARE_BLOCKS: blocks per CU a pipelined pass leaves to the other slot's tail
    bool lean_trace = true;             // HIPR_LEAN_TRACE=0: always the full kernel
    bool lean_shade = true;             // HIPR_LEAN_SHADE=0: always the full kernel
    bool coherence_sort = false;        // HIPR_COHERENCE_SORT=1: the rays of a fused trace launch are taken by (origin cell, octant), ray_sort.hip (built and measured in round 4: profiles/r04_ab_coherence_sort.txt); inert without HIPR_RAY_SORT
    bool shade_classes = false;         // HIPR_SHADE_CLASSES=1: coated surface hits listed apart (built and measured in round 4: no gain, profiles/r04_ab_shade_classes.txt)
    int blocks_per_cu_override = 0;     // HIPR_BLOCKS_PER_CU: persistent trace blocks per CU instead of what the occupancy query says
    int shade_blocks_per_cu = 0;        // persistent shade blocks per CU = waves per SIMD; 0: 3 (what the kernel is compiled for), 2 for all-Diffuse scenes (HIPR_SHADE_BLOCKS_PER_CU)
    uint32_t shade_ordered_from = 1u << 18;   // bounces with fewer paths than this are shaded in queue order (HIPR_SHADE_ORDERED_FROM); a listed bounce is dealt to the XCDs by chunks of 4096: under 8 chunks whole XCDs idle (shade_schedule.h)
    int refill_below = 40;              // persistent kernels refill a wave once fewer lanes than this are busy (HIPR_REFILL_BELOW)
    bool shade_split = false;           // HIPR_SHADE_SPLIT=1: the shade kernel as two, next event estimation and the rest (shade_kernel.h; measured)
    bool shade_ordered = true;          // k_classify_hits before k_shade (HIPR_SHADE_ORDERED=0: shade in queue order)
    bool shade_ordered_camera = false;  // ... also before shade(0) (HIPR_SHADE_ORDERED_CAMERA=1; measured: profiles/r04_ab_knobs.txt)
    bool trace_log = false;             // HIPR_TRACE_LOG=1: the occupancy queries and, with instrumentation on, every bounce on stderr
};

Knobs knobs_from_environment() {
    Knobs k;
    if (const char* v = getenv("HIPR_TRACE_VARIANT")) k.trace_variant = atoi(v);
    if (const char* v = getenv("HIPR_REFILL_BELOW")) k.refill_below = atoi(v);
    if (const char* v = getenv("HIPR_SHADE_ORDERED_FROM")) k.shade_ordered_from = uint32_t(atoll(v));
    if (const char* v = getenv("HIPR_SHADE_BLOCKS_PER_CU")) k.shade_blocks_per_cu = std::max(1, atoi(v));
    if (const char* v = getenv("HIPR_BLOCKS_PER_CU")) k.blocks_per_cu_override = atoi(v);
    if (const char* v = getenv("HIPR_WAVEFRONTS")) k.wavefront_limit = std::max(0, std::min(MAX_WAVEFRONTS, atoi(v)));
    if (const char* v = getenv("HIPR_TRACE_LOG")) k.trace_log = atoi(v) != 0;
    if (const char* v = getenv("HIPR_SHADE_CLASSES")) k.shade_classes = atoi(v) != 0;
    if (const char* v = getenv("HIPR_COHERENCE_SORT")) k.coherence_sort = HIPR_RAY_SORT && atoi(v) != 0;      // only in a build with the experiment linked in (tools/experiments/ray_sort.hip)
    if (const char* v = getenv("HIPR_LEAN_TRACE")) k.lean_trace = atoi(v) != 0;
    if (const char* v = getenv("HIPR_LEAN_SHADE")) k.lean_shade = atoi(v) != 0;
    if (const char* v = getenv("HIPR_SHADE_ORDERED")) k.shade_ordered = atoi(v) != 0;
    if (const char* v = getenv("HIPR_SHADE_ORDERED_CAMERA")) k.shade_ordered_camera = atoi(v) != 0;
    if (const char* v = getenv("HIPR_SHADE_SPLIT")) k.shade_split = atoi(v) != 0;
    if (const char* v = getenv("HIPR_ARITHMETIC")) k.arithmetic = (v[0] == 'e' || v[0] == 'E' || v[0] == '1') ? HIPR_ARITHMETIC_EXACT : HIPR_ARITHMETIC_FAST;
    if (const char* v = getenv("HIPR_BACKFACE_CULLING")) k.cull_backfaces = atoi(v) != 0;
    if (const char* v = getenv("HIPR_PIPELINE_PASSES")) k.pipeline_passes = atoi(v) != 0;
    if (const char* v = getenv("HIPR_PIPELINE_SPARE_BLOCKS")) k.pipeline_spare_blocks = std::max(0, atoi(v));
    return k;
}

// The device scratch of hipr_build_bvh2 (bvh2_build.h), about 240 B per triangle. Up to KEEP_BYTES (a build of a quarter of a million triangles) it stays with the
// context and the next build reuses it; a larger build gives its scratch back when it returns, whatever its outcome -- 2.4 GB at 10 M triangles are not held on a
// shared device between two edits that are seconds apart at best.
struct BuildScratch {
    static constexpr size_t KEEP_BYTES = size_t(128) << 20;
    DeviceBuffer triangles, boxes, centroids, order, seg, order_tmp, seg_tmp, ranges[2], acc, setup, split, scan_local, block_sums, nodes, sizes, place, out_nodes, status;
    double validate_ms = 0.0, upload_ms = 0.0, kernel_ms = 0.0, readback_ms = 0.0;      // of the last build
    uint32_t levels = 0;
    void release_if_large() {
        DeviceBuffer* all[] = {&triangles, &boxes, &centroids, &order, &seg, &order_tmp, &seg_tmp, &ranges[0], &ranges[1], &acc, &setup, &split, &scan_local, &block_sums, &nodes, &sizes, &place, &out_nodes, &status};
        size_t total = 0;
        for (const DeviceBuffer* b : all) total += b->bytes;
        if (total > KEEP_BYTES) for (DeviceBuffer* b : all) b->release();
    }
};
// Gives a large build's scratch back on every way out of hipr_build_bvh2.
struct BuildScratchGuard { BuildScratch& scratch; ~BuildScratchGuard() { scratch.release_if_large(); } };

// The device scratch of hipr_build_wide8 (wide8_build.h), by the same rule: the input (48 B per triangle, 64 B per BVH2 node), about 170 B per record for the tree, its
// tables and the records, 68 B per wide node and the slots.
struct CollapseScratch {
    DeviceBuffer nodes, triangles, order, level_nodes, counts, block_sums, partial, bounds, box, left, right, cost, split, roots_used, records, record_slot, wide_tree, wide_child, wide_all, wide_size,
        wide_base, wide_slot, slots, status;
    double validate_ms = 0.0, upload_ms = 0.0, kernel_ms = 0.0, readback_ms = 0.0;      // of the last collapse
    void release_if_large() {
        DeviceBuffer* all[] = {&nodes, &triangles, &order, &level_nodes, &counts, &block_sums, &partial, &bounds, &box, &left, &right, &cost, &split, &roots_used, &records, &record_slot, &wide_tree,
                               &wide_child, &wide_all, &wide_size, &wide_base, &wide_slot, &slots, &status};
        size_t total = 0;
        for (const DeviceBuffer* b : all) total += b->bytes;
        if (total > BuildScratch::KEEP_BYTES) for (DeviceBuffer* b : all) b->release();
    }
};
struct CollapseScratchGuard { CollapseScratch& scratch; ~CollapseScratchGuard() { scratch.release_if_large(); } };

// What hipr_rebuild_scene_trees needs beside the two builds' scratch (scene_rebuild.h), by the same rule: 9 B per triangle and a word per instance and BVH2 node. The
// flat triangle array itself is BuildScratch::triangles, where hipr_build_bvh2 keeps its input.
struct RebuildScratch {
    DeviceBuffer flat_class, claim, instance_counts, first, level_nodes, status;
    DeviceBuffer old_to_new, created, created_first, instances;      // hipr_edit_scene_instances (instance_edit.h): a word or a record per instance
    double flatten_ms = 0.0, bvh2_ms = 0.0, collapse_ms = 0.0, install_ms = 0.0, readback_ms = 0.0;      // of the last rebuild
    void release_if_large() {
        DeviceBuffer* all[] = {&flat_class, &claim, &instance_counts, &first, &level_nodes, &status, &old_to_new, &created, &created_first, &instances};
        size_t total = 0;
        for (const DeviceBuffer* b : all) total += b->bytes;
        if (total > BuildScratch::KEEP_BYTES) for (DeviceBuffer* b : all) b->release();
    }
};
struct RebuildScratchGuard { RebuildScratch& scratch; ~RebuildScratchGuard() { scratch.release_if_large(); } };

} // namespace

struct HiprContext {
    int device = 0;
    Stream own_stream, copy_stream;     // first members: destroyed last, after everything that was queued on them
    hipStream_t stream = nullptr;       // own_stream, or the one hipr_set_stream lent (never destroyed here)
    Event pass_start;
    Wavefront wavefronts[MAX_WAVEFRONTS];
    Knobs knobs;
    int wavefront_count = 1;                // set by partition_path_slots: small frames run as one wavefront
    int partitioned_for = 0;                // the wavefronts_wanted() the current partition was made for

    ResidentScene scene;                // the uploaded scene and the argument blocks the kernels take (scene.args, scene.wide8)
    const hipr::ShadeUnit& shade_unit() const { return knobs.arithmetic == HIPR_ARITHMETIC_EXACT ? hipr::shade_unit_exact() : hipr::shade_unit_fast(); }
    DeviceBuffer ggx_rho, dielectric_rho, alpha, sample_offsets, sobol_tables;
    bool tables_ready = false;

    // frame
    FrameInfo frame = {};
    bool frame_ready = false;
    uint32_t n_slots = 0;   // owned_tiles * 64 * samples_per_pass
    // Pass pipelining (scenes of the persistent kernels, one wavefront per pass): consecutive passes alternate between two SLOTS -- wavefronts[0] / [1] with
    // their queues and streams, `radiance` / `radiance_other`, two halves of the work-counter ring -- and a pass whose live paths have dwindled to a
    // sliver hands its remaining bounces to the GPU blindly (the kernels read their sizes on the device) and returns: the tail, a chain of launches that
    // each run as long as ONE traversal takes, drains on its stream while the next pass's full-size launches run on the other one.
    struct PassSlot {
        bool pending = false;           // a detached tail is (or may be) still running on the slot's stream
        uint32_t alive_at_detach = 0;   // paths that entered the first bounce of the tail
        uint32_t first_parity = 0;      // the first tail bounce's sizes come back through the wavefront's regular read-back pair of this parity
        uint32_t blind_bounces = 0;     // bounces after it, read back into `tail_counts`
        uint32_t next_bounce = 0;       // the bounce that would follow the tail
        PinnedWords tail_counts;        // pinned: {paths that continue, shadow rays queued} per blind bounce
        uint32_t work_index = 0;        // next unused claim-counter set of the slot's half of the ring
        HiprCameraState camera = {};    // of the pass that left the tail (finish_slot may have to queue more bounces)
    } pass_slots[2];
    int active_slot = 0;                // the slot whose pass is being queued (next_work_counter)
    int traced_slot = 0;                // the slot of the last hipr_trace_pass: what hipr_accumulate_samples folds
    int next_slot = 0;
    bool pipelining_now = false;        // the pass being queued is a pipelined one (Knobs::pipeline_passes, where the scene and the frame allow it)
    Event accumulated;                  // the last hipr_accumulate_samples: the next one (on the other slot's stream) folds after it
    bool accumulated_valid = false;
    DeviceBuffer radiance_other;        // the other slot's radiance (the two swap when the slots do)
    uint32_t traced_samples = 0;        // samples the radiance buffer holds since the last hipr_trace_pass
    float pass_depth_normalizer = 0.0f; // depth entry: far - near of the traced pass's camera
    DeviceBuffer radiance, accumulation, scratch_accumulation, counters, work_counters;
    bool use_scratch = false;
    int entry = HIPR_ENTRY_PATH_TRACING;
    DeviceBuffer& active_accumulation() { return use_scratch ? scratch_accumulation : accumulation; }
    uint32_t wide_stack_entries = 0;
    // persistent kernels walk the compressed 4-wide BVH; without one (HiprSceneDesc::wide_nodes == NULL) the plain BVH2 kernels serve every scene
    // Two half-frame wavefronts on two streams overlap one half's shading with the other's tracing. That pays where the trace kernels are short
    // and light (exhaustive search / BVH2: Cornell +9 % ... +27 %); the persistent wide-BVH kernels fill the register file on their own, the
    // other wavefront's blocks then wait for residency and nothing was gained with round 2's kernels (atrium 88.4 vs 88.8 ms, material 24.9 vs 25.1 ms
    // per step). With round 4's (profiles/r04_ab_wavefronts.txt) two wavefronts pay on every pass of tens of millions of paths -- atrium 63.4 -> 60.6 ms
    // per step, material 37.0 -> 35.7, 10 M triangles at 4K 91.8 -> 87.9: where one wavefront's launch drains, the other's blocks move in -- three and four do not
    // (62.0, 64.9), and a pass of 2 M paths (one accumulation per pass) loses 8 % to the halved launches: two from 2^24 path slots per pass on, else one.
    static constexpr uint64_t TWO_WAVEFRONTS_FROM_SLOTS = 1ull << 24;
    // `frame_is_set`: `frame` holds a valid description. hipr_set_frame partitions BEFORE it sets frame_ready (the first partition after an upload was
    // therefore always one wavefront with full-size queues, the first pass re-partitioned into two, and -- buffers never shrink -- wavefront 0 kept its full-size
    // queues next to wavefront 1's half: about 1.5x the queue memory of a 64-accumulation 1080p pass, plus a redundant allocation and synchronisation).
    int wavefronts_wanted(bool frame_is_set) const {
        if (knobs.wavefront_limit > 0) return knobs.wavefront_limit;
        if (scene.ready && use_persistent()) return frame_is_set && uint64_t(frame.owned_tiles) * 64u * frame.samples_per_pass >= TWO_WAVEFRONTS_FROM_SLOTS ? 2 : 1;
        return 2;
    }
    int wavefronts_wanted() const { return wavefronts_wanted(frame_ready); }
    bool use_wide8() const { return scene.chosen_variant == HIPR_TRACE_WIDE8_PERSISTENT; }
    bool use_wide4() const { return scene.chosen_variant == HIPR_TRACE_WIDE_PERSISTENT; }
    bool use_persistent() const { return use_wide8() || use_wide4(); }      // fused launches, one wavefront
    // tiny scenes: exhaustive search over the triangles (k_trace_*_small)
    bool use_exhaustive() const { return scene.chosen_variant == HIPR_TRACE_EXHAUSTIVE; }
    int active_trace_variant() const { return scene.chosen_variant; }
    int cu_count = 256;
    // resident blocks per CU of the persistent trace kernels, asked of the runtime at the first launch of each (persistent_launch)
    int persistent_blocks_per_cu[3][3] = {{0, 0, 0}, {0, 0, 0}};   // [shadow][stack bucket]
    int wide8_blocks_per_cu[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};   // [mode][stack bucket]

    // bookkeeping
    HiprCounters total = {};   // since hipr_reset_counters
    bool instrument = false;
    DeviceCounters trace_log_previous = {};
    bool timing = true;
    std::vector<Event> event_pool;
    size_t events_used = 0;
    std::vector<TimedLaunch> timed;
    HiprKernelTimes times = {};

    DeviceBuffer debug_a, debug_b, debug_c;
    BuildScratch build;                 // hipr_build_bvh2; nothing of the resident scene
    CollapseScratch collapse;           // hipr_build_wide8; likewise
    RebuildScratch rebuild;             // hipr_rebuild_scene_trees, which also runs over the two above

    hipEvent_t next_event() {
        if (events_used == event_pool.size()) {
            Event e = make_event(hipEventDefault);
            if (!e) return nullptr;
            event_pool.push_back(std::move(e));
        }
        return event_pool[events_used++];
    }
    // An event in a stream costs the command processor about 6 us between two kernels -- a tenth of a bounce of a few thousand paths -- so launches that
    // follow each other on a stream share the event between them: the stop of the one is the start of the next (until break_chain()).
    struct Chain { hipStream_t stream; hipEvent_t event; } chains[MAX_WAVEFRONTS + 1] = {};
    Chain& chain_of(hipStream_t on) {
        for (Chain& ch : chains) if (ch.stream == on) return ch;
        for (Chain& ch : chains) if (!ch.event) { ch.stream = on; return ch; }
        chains[0] = {on, nullptr};
        return chains[0];
    }
    void break_chain(hipStream_t on) { chain_of(on).event = nullptr; }     // something other than a timed launch was queued on the stream
    void begin_timed(int kernel, hipStream_t on) {
        if (!timing) return;
        Chain& ch = chain_of(on);
        TimedLaunch t = {kernel, ch.event ? ch.event : next_event(), next_event()};
        if (!t.start || !t.stop) return;
        if (!ch.event) (void)hipEventRecord(t.start, on);
        ch.event = nullptr;
        timed.push_back(t);
    }
    // Returns the event recorded behind the launch (nullptr with timing off).
    hipEvent_t end_timed(hipStream_t on) {
        if (!timing || timed.empty()) return nullptr;
        (void)hipEventRecord(timed.back().stop, on);
        chain_of(on).event = timed.back().stop;
        return timed.back().stop;
    }
    // Requires the stream to be idle (called after a synchronize).
    void collect_times() {
        for (const TimedLaunch& t : timed) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, t.start, t.stop) == hipSuccess) {
                times.milliseconds[t.kernel] += ms;
                times.launches[t.kernel] += 1;
            }
        }
        timed.clear();
        events_used = 0;
        for (Chain& ch : chains) ch.event = nullptr;
    }
};

namespace {

uint32_t grid_for(uint32_t items, uint32_t block, uint32_t max_blocks) {
    uint32_t blocks = (items + block - 1) / block;
    blocks = std::max(1u, std::min(blocks, max_blocks));
    return (blocks + 7u) & ~7u;   // multiple of 8: xcd_chunk() needs every XCD to own the same number of chunks
}

// Items of the exhaustive search (kernels.h "Exhaustive-search items"): every triangle in order, except that a triangle (a, b, c)
// and a LATER one of the same instance and flags that is (a, c, d) in some rotation, with bit-identical shared corners and
// d = a + (c - b) within 1e-6 of the longest edge component, are merged into the parallelogram item (a, b - a, d - a) at the first
// one's place. Only scenes of at most SMALL_SCENE_TRIANGLES triangles -- the ones searched exhaustively by default -- are paired: above
// that an exhaustive search (HIPR_TRACE_VARIANT) stays per triangle and bit-identical to the BVH searches.
constexpr uint32_t PAIRING_LIMIT = SMALL_SCENE_TRIANGLES;
void build_trace_items(const HiprTriangle* triangles, uint32_t count, std::vector<float>& items) {
    auto corner = [&](uint32_t t, int k) -> const float* { const HiprTriangle& tri = triangles[t]; return k % 3 == 0 ? tri.v0 : (k % 3 == 1 ? tri.v1 : tri.v2); };
    auto same = [](const float* p, const float* q) { return std::memcmp(p, q, 12) == 0; };
    auto bits = [](uint32_t v) { float f; std::memcpy(&f, &v, 4); return f; };
    std::vector<bool> merged(count, false);
    items.clear();
    for (uint32_t i = 0; i < count; ++i) {
        if (merged[i]) continue;
        int ra = 0, rb = 0;
        uint32_t partner = UINT32_MAX;
        for (uint32_t j = i + 1; count <= PAIRING_LIMIT && j < count && partner == UINT32_MAX; ++j) {
            if (merged[j] || triangles[j].instance_index != triangles[i].instance_index || triangles[j].flags != triangles[i].flags) continue;
            for (int x = 0; x < 3 && partner == UINT32_MAX; ++x)
                for (int y = 0; y < 3 && partner == UINT32_MAX; ++y) {
                    const float *a = corner(i, x), *b = corner(i, x + 1), *c = corner(i, x + 2), *a2 = corner(j, y), *c2 = corner(j, y + 1), *d = corner(j, y + 2);
                    if (!same(a, a2) || !same(c, c2)) continue;
                    float longest = 0.0f, off = 0.0f;
                    for (int k = 0; k < 3; ++k) {
                        longest = std::fmax(longest, std::fmax(std::fabs(b[k] - a[k]), std::fabs(d[k] - a[k])));
                        off = std::fmax(off, std::fabs(d[k] - (a[k] + (c[k] - b[k]))));
                    }
                    if (off <= 1e-6f * longest) { partner = j; ra = x; rb = y; }
                }
        }
        const float *a = corner(i, ra), *b = corner(i, ra + 1), *d = partner == UINT32_MAX ? corner(i, ra + 2) : corner(partner, rb + 2);
        // stored vertex k of a triangle is corner (k - rotation) mod 3 of its half: u = weight of vertex 1, v = weight of vertex 2
        const uint32_t selectors = partner == UINT32_MAX ? 0u : uint32_t((4 - ra) % 3) | uint32_t((5 - ra) % 3) << 2 | uint32_t((4 - rb) % 3) << 4 | uint32_t((5 - rb) % 3) << 6;
        const float item[16] = {a[0], a[1], a[2], b[0] - a[0], b[1] - a[1], b[2] - a[2], d[0] - a[0], d[1] - a[1], d[2] - a[2],
                                bits(triangles[i].instance_index), bits(triangles[i].primitive_index), bits(triangles[i].flags | (partner == UINT32_MAX ? 0u : HIPR_ITEM_QUAD)),
                                bits(i), bits(partner == UINT32_MAX ? i : partner), bits(partner == UINT32_MAX ? triangles[i].primitive_index : triangles[partner].primitive_index),
                                bits(selectors)};
        items.insert(items.end(), item, item + 16);
        if (partner != UINT32_MAX) merged[partner] = true;
    }
}

constexpr uint32_t WORK_SETS = 256;                                       // launches served before the ring is re-zeroed
constexpr uint32_t WORK_SET_WORDS = TRACE_SHARDS * TRACE_SHARD_STRIDE;   // one claim counter per shard, 64 B apart
constexpr uint32_t WORK_COUNTERS = WORK_SETS * WORK_SET_WORDS;

// Hands out a zeroed work counter for one persistent launch; re-zeroes the ring when it wraps (stream ordered).
// Each pass slot has its own half of the buffer (two passes may be in flight, each re-zeroing its own sets at its start on its own stream).
uint32_t* next_work_counter(HiprContext* c) {
    uint32_t& index = c->pass_slots[c->active_slot].work_index;
    uint32_t* ring = c->work_counters.as<uint32_t>() + size_t(c->active_slot) * WORK_COUNTERS;
    if (index >= WORK_SETS) {   // out of sets inside a pass (the used prefix is re-zeroed at every pass start): drain and re-zero
        for (int g = 0; g < MAX_WAVEFRONTS; ++g) if (c->wavefronts[g].stream) (void)hipStreamSynchronize(c->wavefronts[g].stream);
        (void)hipMemsetAsync(ring, 0, WORK_COUNTERS * sizeof(uint32_t), c->stream);
        (void)hipStreamSynchronize(c->stream);
        index = 0;
    }
    return ring + size_t(index++) * WORK_SET_WORDS;
}

// The rays of one trace launch.
struct TraceWork {
    PathState in;                       // the path queue: the closest-hit rays
    const uint32_t* closest_count;      // on the device: the entries of `in`; nullptr in a launch over the shadow queue alone
    const uint32_t* shadow_count;       // on the device: the entries of the wavefront's shadow queue; nullptr in a launch over the path queue alone
    uint32_t upper_bound;               // of the rays of the launch: sizes the grid
    const uint32_t* sorted = nullptr;   // ray_sort.hip's listing of the launch's rays (HIPR_RAY_SORT builds)
};

// Every instantiation of a kernel family has the family's type: picking a kernel is picking a pointer.
using Wide8Kernel = void (*)(DeviceScene, Wide8Scene, PathState, float4*, ShadowQueue, float4*, const uint32_t*, const uint32_t*, uint32_t*, int, DeviceCounters*, const uint32_t*);
using Wide4Kernel = void (*)(DeviceScene, PathState, float4*, ShadowQueue, float4*, const uint32_t*, const uint32_t*, uint32_t*, int, DeviceCounters*);
using ClosestKernel = void (*)(DeviceScene, PathState, float4*, const uint32_t*, DeviceCounters*);
using ShadowKernel = void (*)(DeviceScene, ShadowQueue, float4*, const uint32_t*, DeviceCounters*);

// The grid and the claim counters of one persistent launch. The grid: the blocks that stay resident -- asked of the runtime once per family, mode and stack
// bucket (`per_cu`), HIPR_BLOCKS_PER_CU instead where set -- less `spare_per_cu` of them per CU, and no more than the rays of the launch can occupy.
struct PersistentLaunch { uint32_t grid; uint32_t* work_counter; };
template <typename Kernel>
PersistentLaunch persistent_launch(HiprContext* c, Kernel kernel, const char* family, int stack, int mode, int& per_cu, int spare_per_cu, uint32_t upper_bound) {
    if (per_cu == 0) {
        int blocks = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kernel, TRACE_BLOCK, 0) != hipSuccess || blocks <= 0) blocks = 4;
        if (c->knobs.trace_log) fprintf(stderr, "[hipr] %s<%d, %d>: occupancy query says %d blocks of %d threads per CU\n", family, stack, mode, blocks, TRACE_BLOCK);
        if (c->knobs.blocks_per_cu_override > 0) blocks = c->knobs.blocks_per_cu_override;
        per_cu = blocks;
    }
    const uint32_t waves_per_block = TRACE_BLOCK / 64;
    const uint32_t grid = uint32_t(c->cu_count) * uint32_t(per_cu > 2 ? per_cu - spare_per_cu : per_cu);
    return {std::max(1u, std::min(grid, (upper_bound + 63u) / 64u / waves_per_block + 1u)), next_work_counter(c)};
}

// One persistent launch over the 8-wide tree (wide8_kernels.h).
template <int STACK, int MODE, bool INSTRUMENT>
void launch_wide8(HiprContext* c, const Wavefront& w, const TraceWork& work, int bucket) {
    Wide8Kernel kernel = k_trace_wide8<STACK, MODE, INSTRUMENT>;      // the one with all the code: its occupancy sizes the grid of the lean ones below too
    // pipelined passes: one block slot per CU stays free, so that the other slot's tail launches find room next to this pass's persistent blocks
    const PersistentLaunch p = persistent_launch(c, kernel, "k_trace_wide8", STACK, MODE, c->wide8_blocks_per_cu[MODE][bucket], c->pipelining_now ? c->knobs.pipeline_spare_blocks : 0, work.upper_bound);
    // The lean instantiations serve launches that can reach the coverage code and count nothing: without that code for scenes whose triangles are all statically
    // opaque, with the sampler for 8-bit single-channel textures only where every coverage texture is one.
    const bool opaque = c->scene.all_triangles_opaque, lean = c->knobs.lean_trace && !INSTRUMENT && MODE != TRACE_CLOSEST && !work.sorted;
#if HIPR_RAY_SORT
    if constexpr (MODE == TRACE_FUSED && !INSTRUMENT) if (work.sorted) kernel = opaque && c->knobs.lean_trace ? k_trace_wide8<STACK, MODE, INSTRUMENT, false, true> : k_trace_wide8<STACK, MODE, INSTRUMENT, true, true>;
#endif
    if constexpr (!INSTRUMENT && MODE != TRACE_CLOSEST) if (lean && !opaque && c->scene.coverage_textures_r8) kernel = k_trace_wide8<STACK, MODE, INSTRUMENT, true, false, true>;
    if (lean && opaque) kernel = k_trace_wide8<STACK, MODE, INSTRUMENT, false>;
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(TRACE_BLOCK), 0, w.stream, c->scene.args, c->scene.wide8, work.in, w.hits.as<float4>(), w.shadow_queue(), c->radiance.as<float4>(),
                       work.closest_count, work.shadow_count, p.work_counter, c->knobs.refill_below, c->counters.as<DeviceCounters>(), work.sorted);
}

// One persistent launch over the 4-wide tree (kernels.h).
template <int STACK, int MODE, bool INSTRUMENT, bool OVERFLOW>
void launch_wide4(HiprContext* c, const Wavefront& w, const TraceWork& work, int bucket) {
    const Wide4Kernel kernel = k_trace_persistent<STACK, MODE, INSTRUMENT, OVERFLOW>;
    const PersistentLaunch p = persistent_launch(c, kernel, "k_trace_persistent", STACK, MODE, c->persistent_blocks_per_cu[MODE][bucket], 0, work.upper_bound);
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(TRACE_BLOCK), 0, w.stream, c->scene.args, work.in, w.hits.as<float4>(), w.shadow_queue(), c->radiance.as<float4>(),
                       work.closest_count, work.shadow_count, p.work_counter, c->knobs.refill_below, c->counters.as<DeviceCounters>());
}

// One ray per lane: the exhaustive search of tiny scenes, or the BVH2 kernel with the LDS stack the tree's depth asks for.
template <bool INSTRUMENT> ClosestKernel closest_kernel(const HiprContext* c) {
    if (c->use_exhaustive()) return k_trace_closest_small<INSTRUMENT>;
    if (c->scene.stack_size == 16) return k_trace_closest<16, INSTRUMENT>;
    if (c->scene.stack_size == 32) return k_trace_closest<32, INSTRUMENT>;
    return k_trace_closest<64, INSTRUMENT>;
}
template <bool INSTRUMENT> ShadowKernel shadow_kernel(const HiprContext* c) {
    if (c->use_exhaustive()) return k_trace_shadow_small<INSTRUMENT>;
    if (c->scene.stack_size == 16) return k_trace_shadow<16, INSTRUMENT>;
    if (c->scene.stack_size == 32) return k_trace_shadow<32, INSTRUMENT>;
    return k_trace_shadow<64, INSTRUMENT>;
}

#ifndef HIPR_STACK_MID
#define HIPR_STACK_MID 16
#endif
// One trace launch on the wavefront's stream, over its path queue (TRACE_CLOSEST), its shadow queue (TRACE_SHADOW) or both (TRACE_FUSED: the closest-hit rays of a
// bounce and the shadow rays the previous bounce queued; persistent kernels only). Scenes whose whole BVH sits in the L1 / scalar cache (a few dozen nodes) are
// VALU-issue bound and run fastest one ray per lane; everything larger wants a persistent kernel (measured: profiles/).
template <int MODE, bool INSTRUMENT>
void launch_trace(HiprContext* c, const Wavefront& w, TraceWork work) {
    if (c->use_wide8()) {       // the LDS stack by the tree's height h: a ray keeps at most one group per level, so at most h - 1 groups wait on the stack
#if HIPR_RAY_SORT
        if constexpr (MODE == TRACE_FUSED && !INSTRUMENT) if (c->knobs.coherence_sort && w.sort_order.ptr) {
            const ShadowQueue q = w.shadow_queue();
            hipr::RaySortLaunch a = {w.stream, work.in.o_tmin, work.in.d_pdf, q.o_tmax, q.d_slot, work.closest_count, work.shadow_count, std::min(work.upper_bound, 2u * std::max(w.n_slots, 64u)), {}, {},
                                     w.sort_keys[0].as<uint16_t>(), w.sort_keys[1].as<uint16_t>(), w.sort_order.as<uint32_t>(), w.sort_temp.ptr, w.sort_temp.bytes};
            for (int k = 0; k < 3; ++k) { a.grid_min[k] = c->scene.wide8.grid_min[k]; a.cells_per_unit[k] = 16.0f / (c->scene.wide8.grid_cell[k] * 2097152.0f); }
            if (hipr::launch_ray_sort(a) == 0) work.sorted = w.sort_order.as<uint32_t>();
        }
#endif
        const uint32_t height = c->scene.wide8_height;
#if HIPR_WIDE8_LOW_BUCKET
        if (height <= 9u) launch_wide8<8, MODE, INSTRUMENT>(c, w, work, 3);
        else
#endif
        if (height <= uint32_t(WIDE8_STACK_SHALLOW) + 1u) launch_wide8<WIDE8_STACK_SHALLOW, MODE, INSTRUMENT>(c, w, work, 0);
        else if (height <= 17u) launch_wide8<16, MODE, INSTRUMENT>(c, w, work, 1);
        else launch_wide8<32, MODE, INSTRUMENT>(c, w, work, 2);
    } else if (c->use_wide4()) {
        // LDS stack entries by the worst case of the 4-wide tree. Trees that need up to 32 entries run with 16 in LDS and the rest in a per-lane scratch
        // array (traversals rarely get past 16): 4 KB of LDS per wave instead of 8 lets a sixth wave per SIMD stay resident, and the kernel is bound by
        // the latency of its dependent gathers (atrium, 260 k triangles: 61.0 -> 57.7 ms of trace time per step). Deeper trees (the 10 M triangle
        // atrium) spill often enough that 32 LDS entries + scratch is the faster split (116.7 vs 119.9 ms).
        if (c->scene.wide_stack_entries <= 16) launch_wide4<16, MODE, INSTRUMENT, false>(c, w, work, 0);
        else if (c->scene.wide_stack_entries <= 32) launch_wide4<HIPR_STACK_MID, MODE, INSTRUMENT, true>(c, w, work, 1);
        else launch_wide4<32, MODE, INSTRUMENT, true>(c, w, work, 2);
    } else if constexpr (MODE != TRACE_FUSED) {
        const uint32_t block = c->use_exhaustive() ? 256u : uint32_t(TRACE_BLOCK), grid = grid_for(work.upper_bound, block, 256u * 16u);
        if constexpr (MODE == TRACE_CLOSEST) hipLaunchKernelGGL(closest_kernel<INSTRUMENT>(c), dim3(grid), dim3(block), 0, w.stream, c->scene.args, work.in, w.hits.as<float4>(), work.closest_count, c->counters.as<DeviceCounters>());
        else hipLaunchKernelGGL(shadow_kernel<INSTRUMENT>(c), dim3(grid), dim3(block), 0, w.stream, c->scene.args, w.shadow_queue(), c->radiance.as<float4>(), work.shadow_count, c->counters.as<DeviceCounters>());
    } else (void)fail(HIPR_ERROR_UNSUPPORTED, "a fused trace launch needs a persistent kernel");      // not reached: enqueue_bounce fuses only where use_persistent()
}

// The one place where the context's instrumentation flag becomes the kernels' template argument.
template <int MODE>
void trace_rays(HiprContext* c, const Wavefront& w, const TraceWork& work) {
    if (c->instrument) launch_trace<MODE, true>(c, w, work);
    else launch_trace<MODE, false>(c, w, work);
}

// The listing pass of a bounce (kernels.h k_classify_hits): `order` chunk by chunk [plain surface hits | coated surface hits | everything else]. `grid` 0: one block
// per chunk up to eight per CU.
void classify_hits(HiprContext* c, hipStream_t stream, const float4* hits, const uint32_t* count, uint32_t upper_bound, uint32_t* order, bool classes, uint32_t grid) {
    if (!grid) grid = grid_for(upper_bound, 256u * CLASSIFY_ROUNDS, uint32_t(c->cu_count) * 8u);
    if (classes) hipLaunchKernelGGL(k_classify_hits<true>, dim3(grid), dim3(256), 0, stream, hits, count, order, c->scene.triangle_class.as<unsigned char>());
    else hipLaunchKernelGGL(k_classify_hits<false>, dim3(grid), dim3(256), 0, stream, hits, count, order, (const unsigned char*)nullptr);
}

void launch_shade(HiprContext* c, const Wavefront& w, const HiprCameraState& camera, int cur, uint32_t alive, const uint32_t* in_count, uint32_t* out_counts, uint32_t* zero_pair, bool camera_rays) {
    // The rays of the bounce listed by kind (kernels.h k_classify_hits): the shade kernel's batches then hold surface hits only, or none.
    const uint32_t* order = nullptr;
    // Pays where a good share of a bounce's rays did not hit a surface (the atrium's open roof: shade 23.3 -> 21.4 ms per step) and costs a pass over the hits
    // where nearly all did (the closed Cornell box: +7 %): on for the scenes of the persistent kernels, which are the large ones.
    // A bounce of a few thousand paths runs one wave per SIMD at most: the order they are taken in changes nothing, the listing pass would cost a launch.
    // Camera rays need no listing: a wave of them is one pixel's samples (or an 8 x 8 tile's pixels) -- they hit a surface, or miss, together (HIPR_SHADE_ORDERED_CAMERA=1 lists them anyway).
    if (c->knobs.shade_ordered && c->use_persistent() && c->entry == HIPR_ENTRY_PATH_TRACING && alive >= c->knobs.shade_ordered_from && (!camera_rays || c->knobs.shade_ordered_camera)) {
        classify_hits(c, w.stream, w.hits.as<float4>(), in_count, alive, w.order.as<uint32_t>(), c->knobs.shade_classes && c->scene.any_coated_triangle, 0u);
        order = w.order.as<uint32_t>();
    }
    // persistent blocks: three per CU stay resident (3 waves per SIMD), each walks the queue with a grid stride, one batch ahead on its inputs
    // measured: the Default / Transmissive kernels gain from a third wave per SIMD (atrium 29.4 -> 25.9 ms of shading per step), the lighter all-Diffuse
    // kernel loses (Cornell 18 390 -> 17 194 Mrays/s)
    const bool split = c->knobs.shade_split && c->entry == HIPR_ENTRY_PATH_TRACING && c->scene.args.light_count != 0 && w.nee_flags.ptr;
    const uint32_t blocks_per_cu = c->knobs.shade_blocks_per_cu > 0 ? uint32_t(c->knobs.shade_blocks_per_cu) : (split ? uint32_t(HIPR_SHADE_SPLIT_WAVES) : (c->scene.shading_models == 2 ? 2u : uint32_t(c->shade_unit().waves_per_simd)));
    PathState shaded = w.path_state(cur);
    if (camera_rays) shaded.thr_bounces = nullptr;      // k_generate's queue: throughput 1, no bounce yet -- not stored
    ShadeLaunch a = {grid_for(alive, SHADE_BLOCK, uint32_t(c->cu_count) * blocks_per_cu), w.stream, c->scene.args, camera, c->frame, c->entry, shaded, w.hits.as<float4>(), order, w.path_state(1 - cur),
                     w.shadow_queue(), c->radiance.as<float4>(), in_count, reinterpret_cast<unsigned long long*>(out_counts), reinterpret_cast<unsigned long long*>(zero_pair), split ? w.nee_flags.as<unsigned char>() : nullptr,
                     c->counters.as<DeviceCounters>(), c->scene.has_textures || !c->knobs.lean_shade, c->scene.has_environment || !c->knobs.lean_shade};
    c->shade_unit().shade(c->scene.shading_models, a);
}

// Splits the path slots of a pass (owned tiles x 64 x samples_per_pass) over the wavefronts on a tile (= wave) boundary and sizes the
// queues and the per-sample radiance buffer; small passes stay one wavefront. Buffers only ever grow. The accumulation is not touched.
int partition_path_slots(HiprContext* c) {
    const FrameInfo& fi = c->frame;
    const uint64_t slots = uint64_t(fi.owned_tiles) * 64u * fi.samples_per_pass;
    c->n_slots = uint32_t(slots);
    c->traced_samples = 0;   // the radiance buffer may move and its sample layout changes: nothing traced before can be folded any more
    int r = 0;
    c->partitioned_for = c->wavefronts_wanted(true);      // every caller has put a valid description into c->frame
    c->wavefront_count = int(std::max<uint64_t>(1, std::min<uint64_t>(uint64_t(c->partitioned_for), slots / 65536u)));
    // The slots are dealt to the wavefronts in groups of 64 (one wave of camera rays), round robin: with the pixel-major slot order every wavefront then
    // covers the whole frame evenly -- contiguous halves would be the top and the bottom of the image, one of them done with its deep bounces long before
    // the other (material scene: +2.3 % step time with halves). Queue entry i of wavefront g is slot ((i / 64) * G + g) * 64 + i % 64 (k_generate).
    const uint64_t groups = slots / 64u;      // owned_tiles * 64 * samples: a multiple of 64
    for (int g = 0; g < MAX_WAVEFRONTS; ++g) {
        Wavefront& w = c->wavefronts[g];
        w.first_slot = uint32_t(g);           // the wavefront's phase in the deal
        w.n_slots = g >= c->wavefront_count ? 0u : uint32_t((groups + uint64_t(c->wavefront_count) - 1u - uint64_t(g)) / uint64_t(c->wavefront_count) * 64u);
        const bool second_slot = g == 1 && c->wavefront_count == 1 && c->knobs.pipeline_passes && c->partitioned_for == 1;    // the other pass slot: a copy of wavefront 0's share
        if (second_slot) { w.first_slot = c->wavefronts[0].first_slot; w.n_slots = c->wavefronts[0].n_slots; }
        const size_t bytes = size_t(std::max(w.n_slots, 64u)) * 16;
        if (g >= c->wavefront_count && !second_slot) {   // queues of wavefronts this pass size does not use go back to the allocator
            for (auto& buffers : w.path) for (DeviceBuffer& b : buffers) b.release();
            w.hits.release(); w.order.release(); w.nee_flags.release();
            w.sort_keys[0].release(); w.sort_keys[1].release(); w.sort_order.release(); w.sort_temp.release();
            for (DeviceBuffer& b : w.shadow) b.release();
            continue;
        }
        for (int i = 0; i < 2; ++i) for (int j = 0; j < 4; ++j) r |= w.path[i][j].resize(j == 3 ? bytes / 2 : bytes);      // [3]: the 8-byte meta records
        r |= w.hits.resize(bytes);
        r |= w.order.resize(bytes / 4);
        if (c->knobs.shade_split) r |= w.nee_flags.resize(bytes / 16);
#if HIPR_RAY_SORT
        if (c->knobs.coherence_sort) {      // both queues of a fused launch: 2 x n_slots entries
            const size_t entries = bytes / 16 * 2;
            r |= w.sort_keys[0].resize(entries * 2); r |= w.sort_keys[1].resize(entries * 2); r |= w.sort_order.resize(entries * 4);
            r |= w.sort_temp.resize(hipr::ray_sort_temp_bytes(uint32_t(entries)));
        }
#endif
        for (int j = 0; j < 3; ++j) r |= w.shadow[j].resize(bytes);
    }
    const bool two_slots = c->wavefront_count == 1 && c->knobs.pipeline_passes && c->partitioned_for == 1;
    if (!two_slots) {
        if (c->traced_slot == 1 && c->radiance_other.ptr) std::swap(c->radiance, c->radiance_other);      // the slots are gone: `radiance` is wavefront 0's again
        c->radiance_other.release();
        c->traced_slot = c->next_slot = c->active_slot = 0;
    }
    r |= c->radiance.resize(slots * 16);
    if (two_slots) r |= c->radiance_other.resize(slots * 16);
    return r;
}

void set_frame_divisors(FrameInfo& f) { f.by_samples_per_pass = make_divisor(f.samples_per_pass); f.by_tiles_x = make_divisor(f.tiles_x); }

int check_context(HiprContext* c) {
    if (!c) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null context");
    HIP_TRY(hipSetDevice(c->device));
    return HIPR_OK;
}

// Bounce k of a wavefront = trace stage + shade(k). The trace stage serves the closest-hit rays of bounce k AND the shadow rays
// shade(k - 1) queued (they are independent; radiance slots are still updated in the order shade(0), shadow(0), shade(1), ...):
// one fused persistent launch for big scenes, two plain launches otherwise. All queue sizes stay on the device; the host only
// needs them to stop. `bound`: an upper bound of the bounce's rays (sizes the launches); `host_sizes`: where the sizes the bounce
// produced -- {paths that continue, shadow rays queued} -- are read back to (nullptr: the wavefront's regular pair of the bounce's parity).
int enqueue_bounce(HiprContext* c, Wavefront& w, const HiprCameraState& camera, uint32_t k, uint32_t bound, uint32_t* host_sizes = nullptr) {
    const bool fused = c->use_persistent();
    if (!host_sizes) host_sizes = w.host_counts + 2 * (k & 1u);

    // Queue sizes live in three 8-byte pairs, 64 B apart (COUNT_PAIRS): pair[k % 3] = {paths of bounce k, shadow rays shade(k - 1) queued}.
    // shade(k) fills pair[(k + 1) % 3] with one 64-bit atomic per block and zeroes pair[(k + 2) % 3] for shade(k + 1).
    uint32_t* counts = w.queue_counts.as<uint32_t>();
    const int parity = int(k & 1u);
    uint32_t* in_count = counts + COUNT_PAIR_STRIDE * (k % COUNT_PAIRS);
    uint32_t* shadow_in = in_count + 1;
    uint32_t* out_count = counts + COUNT_PAIR_STRIDE * ((k + 1u) % COUNT_PAIRS);
    uint32_t* zero_pair = counts + COUNT_PAIR_STRIDE * ((k + 2u) % COUNT_PAIRS);
    const size_t first_timed = c->timed.size();
    // a bounce queued blindly (pipelined passes) is not behind the host's read of the sizes of bounce k - 2, which sit in the pair its shade kernel zeroes
    if (host_sizes != w.host_counts + 2 * (k & 1u) && k >= 2) {
        HIP_TRY(hipStreamWaitEvent(w.stream, w.counts_copied[parity], 0));
        c->break_chain(w.stream);
    }

    c->begin_timed(HIPR_KERNEL_TRACE_CLOSEST, w.stream);
    if (k > 0 && fused) trace_rays<TRACE_FUSED>(c, w, {w.path_state(parity), in_count, shadow_in, 2u * bound});
    else trace_rays<TRACE_CLOSEST>(c, w, {w.path_state(parity), in_count, nullptr, bound});
    c->end_timed(w.stream);
    if (k > 0 && !fused) {
        c->begin_timed(HIPR_KERNEL_TRACE_SHADOW, w.stream);
        trace_rays<TRACE_SHADOW>(c, w, {PathState{}, nullptr, shadow_in, bound});
        c->end_timed(w.stream);
    }

    c->begin_timed(HIPR_KERNEL_SHADE, w.stream);
    launch_shade(c, w, camera, parity, bound, in_count, out_count, zero_pair, k == 0);
    hipEvent_t shaded = c->end_timed(w.stream);
    if (!shaded) {
        shaded = w.shade_done[parity];
        HIP_TRY(hipEventRecord(shaded, w.stream));
    }
    HIP_TRY(hipStreamWaitEvent(c->copy_stream, shaded, 0));
    HIP_TRY(hipMemcpyAsync(host_sizes, out_count, 8, hipMemcpyDeviceToHost, c->copy_stream));     // {paths that continue, shadow rays}
    HIP_TRY(hipEventRecord(w.counts_copied[parity], c->copy_stream));

    if (c->instrument && c->knobs.trace_log) {   // diagnostic (HIPR_TRACE_LOG=1): per-bounce counters and kernel times; serialises the pass
        HIP_TRY(hipStreamSynchronize(w.stream));
        HIP_TRY(hipStreamSynchronize(c->copy_stream));
        DeviceCounters dc;
        HIP_TRY(hipMemcpy(&dc, c->counters.ptr, sizeof(dc), hipMemcpyDeviceToHost));
        const DeviceCounters& p = c->trace_log_previous;
        fprintf(stderr, "[hipr] wavefront %d bounce %u: <= %u closest rays: nodes %llu tris %llu | shadow rays of the previous bounce: nodes %llu tris %llu | kernels",
                int(&w - c->wavefronts), k, bound, dc.closest_nodes - p.closest_nodes, dc.closest_triangles - p.closest_triangles, dc.shadow_nodes - p.shadow_nodes,
                dc.shadow_triangles - p.shadow_triangles);
        for (size_t i = first_timed; i < c->timed.size(); ++i) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, c->timed[i].start, c->timed[i].stop);
            fprintf(stderr, " %s %.1f us", c->timed[i].kernel == HIPR_KERNEL_SHADE ? "shade" : (c->timed[i].kernel == HIPR_KERNEL_TRACE_SHADOW ? "shadow" : "trace"), ms * 1e3f);
        }
        fprintf(stderr, " -> %u paths continue, %u shadow rays\n", w.host_counts[2 * parity], w.host_counts[2 * parity + 1]);
        if (dc.node_iterations != p.node_iterations) {
            const double ni = double(dc.node_iterations - p.node_iterations), ti = double(dc.triangle_iterations - p.triangle_iterations);
            fprintf(stderr, "[hipr]     wave iterations: %.0f node (%.1f lanes working) + %.0f triangle (%.1f lanes working); %.1f lanes busy on average; %llu refills\n", ni,
                    double(dc.node_lanes - p.node_lanes) / ni, ti, ti > 0 ? double(dc.triangle_lanes - p.triangle_lanes) / ti : 0.0,
                    double(dc.busy_lanes - p.busy_lanes) / (ni + ti), dc.refills - p.refills);
            const double rc = double(dc.record_iterations_closest - p.record_iterations_closest), rs = double(dc.record_iterations_shadow - p.record_iterations_shadow),
                         rm = double(dc.record_iterations_mixed - p.record_iterations_mixed);
            if (rc + rs + rm > 0)      // fused launches over the 8-wide tree: a record iteration with one kind of ray branches over the other kind's code
                fprintf(stderr, "[hipr]     triangle iterations by the rays on the records: %.0f closest-hit only (%.1f %%) + %.0f shadow only (%.1f %%) + %.0f both (%.1f %%)\n", rc,
                        100.0 * rc / (rc + rs + rm), rs, 100.0 * rs / (rc + rs + rm), rm, 100.0 * rm / (rc + rs + rm));
            const double pushes = double(dc.pushes - p.pushes);
            if (pushes > 0)
                fprintf(stderr, "[hipr]     stack pushes: %.0f, of which %.3f %% onto entry 16 or deeper and %.3f %% onto entry 24 or deeper\n", pushes,
                        100.0 * double(dc.pushes_past_16 - p.pushes_past_16) / pushes, 100.0 * double(dc.pushes_past_24 - p.pushes_past_24) / pushes);
        }
        c->trace_log_previous = dc;
    }
    return HIPR_OK;
}

// The books of a pass, kept here and nowhere else: bounce k of a wavefront, which `alive` paths entered and which left `sizes` = {paths that continue, shadow rays
// queued}, is added to `books`, and `alive` becomes what enters bounce k + 1. A wavefront that is still going after RUNAWAY_BOUNCES is an error.
constexpr uint32_t RUNAWAY_BOUNCES = 8192;
int book_bounce(HiprCounters& books, uint32_t k, uint32_t& alive, const uint32_t* sizes) {
    books.closest_rays += alive;
    books.shadow_rays += sizes[1];
    books.iterations += 1;
    alive = sizes[0];
    return k > RUNAWAY_BOUNCES ? fail(HIPR_ERROR_HIP, "wavefront loop did not terminate") : HIPR_OK;
}

// One step of a wavefront: queues bounce `queued`, sized by the paths alive now, waits for the sizes bounce `awaited` produced and books that bounce. A pass runs
// with queued = awaited + 1 -- the next bounce is queued speculatively (at most `alive` paths continue), so the GPU never idles on the read-back; a wavefront whose
// paths all ended has, with that last speculative bounce, also traced its last shadow rays. A bounce that no path entered traces shadow rays only and is not booked.
int advance_wavefront(HiprContext* c, Wavefront& w, const HiprCameraState& camera, uint32_t queued, uint32_t awaited, uint32_t& alive, HiprCounters& books) {
    if (int s = enqueue_bounce(c, w, camera, queued, std::max(alive, 1u))) return s;
    HIP_TRY(hipEventSynchronize(w.counts_copied[awaited & 1u]));
    return alive == 0 ? HIPR_OK : book_bounce(books, awaited, alive, w.host_counts + 2 * (awaited & 1u));
}

// Brings the books of a pass slot up to date: waits for the tail its last pass left on the slot's stream and adds the rays of the tail's bounces to the
// totals (their queue sizes were read back bounce by bounce into pinned memory). Should paths have outlived the blind bounces (hits that keep being
// rejected and retraced do not count as bounces), the pass is finished here bounce by bounce.
int finish_slot(HiprContext* c, int slot_index) {
    HiprContext::PassSlot& slot = c->pass_slots[slot_index];
    if (!slot.pending) return HIPR_OK;
    Wavefront& w = c->wavefronts[slot_index];
    HIP_TRY(hipStreamSynchronize(w.stream));
    HIP_TRY(hipStreamSynchronize(c->copy_stream));
    slot.pending = false;
    const uint32_t first_bounce = slot.next_bounce - slot.blind_bounces - 1u;      // of the tail
    uint32_t in = slot.alive_at_detach, shadows = 0;
    for (uint32_t t = 0; t <= slot.blind_bounces && in > 0; ++t) {
        const uint32_t* sizes = t == 0 ? w.host_counts + 2 * slot.first_parity : slot.tail_counts + 2 * (t - 1);
        shadows = sizes[1];
        if (int s = book_bounce(c->total, first_bounce + t, in, sizes)) return s;
    }
    if (in == 0 && shadows == 0) return HIPR_OK;
    // the last blind bounce left paths (or only shadow rays): carry on the ordinary way
    const int saved_slot = c->active_slot;
    c->active_slot = slot_index;
    const bool swap = slot_index != c->traced_slot;     // launches write the radiance of the pass being finished
    if (swap) std::swap(c->radiance, c->radiance_other);
    int status = HIPR_OK;
    uint32_t k = slot.next_bounce, entered;
    do {      // nothing is queued ahead here; the last turn is the bounce no path entered: it traces the last shadow rays
        entered = in;
        status = advance_wavefront(c, w, slot.camera, k, k, in, c->total);
        ++k;
    } while (status == HIPR_OK && entered > 0);
    if (swap) std::swap(c->radiance, c->radiance_other);
    c->active_slot = saved_slot;
    if (status == HIPR_OK) HIP_TRY(hipStreamSynchronize(w.stream));
    return status;
}

// Every pass queued so far is complete on the device and in the books (the entry points that read results, change the frame or the scene, or collect
// timings start here).
int finish_all(HiprContext* c) {
    for (int slot = 0; slot < 2; ++slot)
        if (int s = finish_slot(c, slot)) return s;
    for (int g = 0; g < MAX_WAVEFRONTS; ++g) if (c->wavefronts[g].stream) HIP_TRY(hipStreamSynchronize(c->wavefronts[g].stream));
    HIP_TRY(hipStreamSynchronize(c->copy_stream));
    return HIPR_OK;
}

// finish_all, and the timed launches of the passes that finished with it are added to the kernel times.
int drain(HiprContext* c) {
    if (int s = finish_all(c)) return s;
    c->collect_times();
    return HIPR_OK;
}

// The camera rays of a pass: the pixel-samples inside the frame (edge tiles may hang over it).
uint64_t camera_rays_of(const FrameInfo& f) {
    if (f.tile_stride == 1) return uint64_t(f.width) * f.height * f.samples_per_pass;
    uint64_t valid_pixels = 0;
    for (uint32_t t = f.tile_phase; t < f.tiles_total; t += f.tile_stride) {
        const uint32_t tx = t % f.tiles_x, ty = t / f.tiles_x;
        valid_pixels += uint64_t(std::min(8u, f.width - tx * 8)) * std::min(8u, f.height - ty * 8);
    }
    return valid_pixels * f.samples_per_pass;
}

// What the depth entry point divides by: the distance between the near and far plane centres (SimpleRGPs.cu:247-255).
float depth_range_of(const HiprCameraState& camera) {
    const float* ip = camera.inverse_projection_matrix;
    const float near_z = (ip[8] * 0.0f + ip[9] * 0.0f + ip[10] * -1.0f + ip[11]) / (ip[12] * 0.0f + ip[13] * 0.0f + ip[14] * -1.0f + ip[15]);
    const float far_z = (ip[8] * 0.0f + ip[9] * 0.0f + ip[10] * 1.0f + ip[11]) / (ip[12] * 0.0f + ip[13] * 0.0f + ip[14] * 1.0f + ip[15]);
    return far_z - near_z;
}

// Begins a pass on a pass slot (0 for a pass that is not pipelined): what ran on the slot before -- every pass, where this one is not pipelined -- is finished,
// `radiance` becomes the slot's buffer, the claim counters the slot's previous pass used are zeroed again, and the streams of the other wavefronts get their start.
int begin_pass(HiprContext* c, int slot, bool pipelined) {
    c->pipelining_now = pipelined;
    if (pipelined) {
        if (int s = finish_slot(c, slot)) return s;
        c->next_slot = 1 - slot;
    } else if (int s = finish_all(c)) return s;
    if (slot != c->traced_slot) std::swap(c->radiance, c->radiance_other);      // `radiance` is the buffer of the pass being traced / last traced
    c->traced_slot = c->active_slot = slot;
    HiprContext::PassSlot& ps = c->pass_slots[slot];
    if (ps.work_index > 0) {   // the slot's stream is ordered behind its previous pass
        HIP_TRY(hipMemsetAsync(c->work_counters.as<uint32_t>() + size_t(slot) * WORK_COUNTERS, 0, size_t(std::min(ps.work_index, WORK_SETS)) * WORK_SET_WORDS * sizeof(uint32_t),
                               c->wavefronts[slot].stream));
        ps.work_index = 0;
    }
    if (!pipelined) HIP_TRY(hipEventRecord(c->pass_start, c->stream));
    return HIPR_OK;
}

// Starts a wavefront's share of a pass: its counters, the camera rays and bounce 0.
int start_wavefront(HiprContext* c, Wavefront& w, const HiprCameraState& camera, bool pipelined) {
    if (!pipelined && &w != c->wavefronts) HIP_TRY(hipStreamWaitEvent(w.stream, c->pass_start, 0));
    // the counters at the start of a pass: pair 0 = {paths, 0 shadow rays}, all others zero (pinned image, rewritten only after the syncs of the next pass)
    memset(w.host_counts + 8, 0, COUNT_LINES * COUNT_PAIR_STRIDE * sizeof(uint32_t));
    w.host_counts[8] = w.n_slots;
    HIP_TRY(hipMemcpyAsync(w.queue_counts.as<uint32_t>(), w.host_counts + 8, COUNT_LINES * COUNT_PAIR_STRIDE * sizeof(uint32_t), hipMemcpyHostToDevice, w.stream));
    c->break_chain(w.stream);
    c->begin_timed(HIPR_KERNEL_GENERATE, w.stream);
    hipLaunchKernelGGL(k_generate, dim3((w.n_slots + 255) / 256), dim3(256), 0, w.stream, c->frame, camera, w.path_state(0), c->radiance.as<float4>(), w.first_slot, uint32_t(pipelined ? 1 : c->wavefront_count), w.n_slots);
    c->end_timed(w.stream);
    return enqueue_bounce(c, w, camera, 0, w.n_slots);
}

// Hands the rest of a pipelined pass to the GPU once bounce k left a sliver of `alive` paths (bounce k + 1 is queued for them already): every bounce that can
// follow is queued now, sized by this count and reading its own on the device -- those the camera's bounce limit allows, one more for the last shadow rays, and a
// reserve for hits that get rejected and retraced without counting as a bounce (finish_slot() takes over if that reserve runs out).
int detach_tail(HiprContext* c, Wavefront& w, HiprContext::PassSlot& ps, const HiprCameraState& camera, uint32_t k, uint32_t alive) {
    const uint32_t reserve = 8u;
    const uint32_t blind = std::min(120u, (camera.max_bounce_count + 2u > k ? camera.max_bounce_count + 2u - k : 1u) + reserve);
    for (uint32_t t = 0; t < blind; ++t)
        if (int s = enqueue_bounce(c, w, camera, k + 2 + t, alive, ps.tail_counts + 2 * t)) return s;
    ps.pending = true;
    ps.alive_at_detach = alive;
    ps.first_parity = (k + 1) & 1u;
    ps.blind_bounces = blind;
    ps.next_bounce = k + 2 + blind;
    ps.camera = camera;
    return HIPR_OK;
}

// O(n) check of everything the kernels dereference through an index of the description (the header is public: a bad ID must be an
// error code, not an out-of-bounds read on the GPU). Also derives the worst-case stack need of the wide tree instead of trusting
// the caller's figure. Returns nullptr when the scene is sound, a message otherwise.
// What makes ONE material unusable against a texture pool of `texture_count` entries: a texture ID outside it, an unknown shading model. The check of
// validate_scene for every material of a description, and of hipr_update_scene_materials for every slot it is given. Returns nullptr when sound.
const char* invalid_material(const HiprMaterial& m, uint32_t index, uint32_t texture_count, char* message, size_t message_size) {
    const int32_t ids[4] = {m.tint_roughness_texture_ID, m.roughness_texture_ID, m.metallic_texture_ID, m.coverage_texture_ID};
    for (int32_t id : ids)
        if (id < 0 || (id > 0 && uint32_t(id) >= texture_count)) { snprintf(message, message_size, "material %u references texture %d of %u", index, id, texture_count); return message; }
    if (m.shading_model > HIPR_SHADING_TRANSMISSIVE) { snprintf(message, message_size, "material %u has the unknown shading model %u", index, unsigned(m.shading_model)); return message; }
    return nullptr;
}

// What makes ONE texture unusable against a texel pool of `texel_bytes`: an unknown format, an empty extent, texels that do not lie inside the pool or start off
// their alignment. The check of validate_scene for every texture of a description, and of hipr_append_scene_pools for every texture it brings, against the grown pool.
const char* invalid_texture(const HiprTexture& t, uint32_t index, uint64_t texel_bytes, char* message, size_t message_size) {
    const uint64_t size = t.format == HIPR_TEXEL_R8 ? 1u : (t.format == HIPR_TEXEL_RGBA8 ? 4u : (t.format == HIPR_TEXEL_R32F ? 4u : (t.format == HIPR_TEXEL_RGBA32F ? 16u : 0u)));
    if (size == 0) { snprintf(message, message_size, "texture %u has the unknown texel format %u", index, unsigned(t.format)); return message; }
    if (t.width == 0 || t.height == 0) { snprintf(message, message_size, "texture %u is %u x %u", index, t.width, t.height); return message; }
    const uint64_t bytes = uint64_t(t.width) * t.height * size;
    if (t.texel_offset > texel_bytes || bytes > texel_bytes - t.texel_offset || t.texel_offset % (size == 16 ? 16 : 4) != 0) {
        snprintf(message, message_size, "texture %u (%u x %u, offset %llu) does not fit the %llu byte texel pool", index, t.width, t.height, (unsigned long long)t.texel_offset, (unsigned long long)texel_bytes);
        return message;
    }
    return nullptr;
}

const char* validate_scene(const HiprSceneDesc* s, uint32_t& wide_stack_need, char* message, size_t message_size) {
#define INVALID(...) do { snprintf(message, message_size, __VA_ARGS__); return message; } while (0)
    wide_stack_need = 0;
    if (s->texture_count && !s->textures) INVALID("texture_count is %u but textures is null", s->texture_count);
    if (s->light_count && !s->lights) INVALID("light_count is %u but lights is null", s->light_count);
    if (s->texel_bytes && !s->texels) INVALID("texel_bytes is %llu but texels is null", (unsigned long long)s->texel_bytes);
    for (uint32_t i = 1; i < s->texture_count; ++i)   // slot 0 = none
        if (invalid_texture(s->textures[i], i, s->texel_bytes, message, message_size)) return message;
    for (uint32_t i = 0; i < s->material_count; ++i)
        if (invalid_material(s->materials[i], i, s->texture_count, message, message_size)) return message;
    const uint32_t primitive_total = s->index_count / 3;
    for (uint32_t i = 0; i < s->instance_count; ++i) {
        const HiprInstance& inst = s->instances[i];
        if (inst.material_index < 0 || uint32_t(inst.material_index) >= s->material_count) INVALID("instance %u references material %d of %u", i, inst.material_index, s->material_count);
        if (inst.index_offset > primitive_total || inst.vertex_offset > s->vertex_count) INVALID("instance %u starts outside the index / vertex pools", i);
    }
    for (uint32_t t = 0; t < s->triangle_count; ++t) {
        const HiprTriangle& tri = s->triangles[t];
        if (tri.instance_index >= s->instance_count) INVALID("triangle %u references instance %u of %u", t, tri.instance_index, s->instance_count);
        const HiprInstance& inst = s->instances[tri.instance_index];
        if (tri.primitive_index >= primitive_total - inst.index_offset) INVALID("triangle %u references primitive %u beyond the index pool", t, tri.primitive_index);
        if (tri.flags & HIPR_TRIANGLE_ONE_SIDED) {      // the traversal may step over hits on its back: only where the hit program would refuse them
            const HiprMaterial& m = s->materials[inst.material_index];
            if ((m.flags & (HIPR_MATERIAL_CUTOUT | HIPR_MATERIAL_THIN_WALLED)) || m.shading_model == HIPR_SHADING_TRANSMISSIVE)
                INVALID("triangle %u is flagged HIPR_TRIANGLE_ONE_SIDED but material %d is thin-walled, a cut-out or transmissive", t, inst.material_index);
        }
        const uint32_t* idx = s->indices + 3 * size_t(inst.index_offset + tri.primitive_index);
        for (int k = 0; k < 3; ++k)
            if (idx[k] >= s->vertex_count - inst.vertex_offset) INVALID("triangle %u: vertex index %u is beyond the vertex pool", t, idx[k]);
    }
    auto leaf_ok = [&](int32_t ref) { const uint32_t code = uint32_t(~ref); return uint64_t(code >> 3) + (code & 7u) + 1u <= s->triangle_count; };
    if (s->triangle_count && s->node_count == 0) INVALID("a scene with triangles needs a BVH");
    for (uint32_t n = 0; n < s->node_count; ++n)
        for (int k = 0; k < 2; ++k) {
            const int32_t ref = s->nodes[n].child[k];
            if (ref >= 0 ? uint32_t(ref) >= s->node_count : !leaf_ok(ref)) INVALID("BVH node %u: child %d is out of range", n, ref);
        }
    if (s->wide_nodes && s->wide_node_count) {
        // need(node) = (children - 1) + max need(child): iterative post-order; a node reached twice or a cycle is an error
        std::vector<uint32_t> need(s->wide_node_count, 0u);
        std::vector<uint8_t> state(s->wide_node_count, 0);   // 0 unseen, 1 open, 2 done
        std::vector<uint32_t> stack = {0u};
        while (!stack.empty()) {
            const uint32_t n = stack.back();
            const HiprWideNode& w = s->wide_nodes[n];
            if (state[n] == 0) {
                state[n] = 1;
                for (int k = 0; k < 4; ++k) {
                    const int32_t ref = w.child[k];
                    if (ref == HIPR_WIDE_EMPTY) continue;
                    if (ref < 0) { if (!leaf_ok(ref)) INVALID("wide BVH node %u: leaf %d is out of range", n, ref); continue; }
                    if (uint32_t(ref) >= s->wide_node_count || state[ref] != 0) INVALID("wide BVH node %u: child %d is out of range or shared", n, ref);
                    stack.push_back(uint32_t(ref));
                }
            } else {
                uint32_t children = 0, below = 0;
                for (int k = 0; k < 4; ++k) {
                    const int32_t ref = w.child[k];
                    if (ref == HIPR_WIDE_EMPTY) continue;
                    ++children;
                    if (ref >= 0) below = std::max(below, need[ref]);
                }
                need[n] = (children ? children - 1u : 0u) + below;
                state[n] = 2;
                stack.pop_back();
            }
        }
        wide_stack_need = need[0];
    }
    return nullptr;
#undef INVALID
}

// The 8-wide tree of a description: every slot reached at most once from the root, child ranges inside the array, leaf records referencing triangles
// of the description, finite grid. Derives the height (the stack need of the traversal). Returns nullptr when sound.
const char* validate_wide8(const HiprSceneDesc* s, uint32_t& height, char* message, size_t message_size) {
#define INVALID(...) do { snprintf(message, message_size, __VA_ARGS__); return message; } while (0)
    height = 0;
    if (!s->wide8_slots || s->wide8_slot_count == 0) return nullptr;
    if (s->wide8_slot_count > 0x1000000u) INVALID("the 8-wide tree has %u slots, more than 2^24", s->wide8_slot_count);
    for (int a = 0; a < 3; ++a)
        if (!(s->wide8_grid_cell[a] > 0.0f) || !std::isfinite(s->wide8_grid_cell[a]) || !std::isfinite(s->wide8_grid_min[a])) INVALID("the 8-wide tree's grid is not finite");
    std::vector<uint8_t> seen(s->wide8_slot_count, 0);
    struct Visit { uint32_t slot, depth; };
    std::vector<Visit> stack = {{0u, 1u}};
    seen[0] = 1;
    while (!stack.empty()) {
        const Visit v = stack.back();
        stack.pop_back();
        height = std::max(height, v.depth);
        const HiprNode8& n = s->wide8_slots[v.slot].node;
        const uint32_t base = n.base_valid & 0xFFFFFFu, valid = n.base_valid >> 24;
        const uint32_t children = uint32_t(__builtin_popcount(valid));
        if (children == 0 || uint64_t(base) + children > s->wide8_slot_count) INVALID("8-wide node in slot %u: children [%u, %u) outside the %u slots", v.slot, base, base + children, s->wide8_slot_count);
        if (n.inner_mask & ~valid) INVALID("8-wide node in slot %u marks an empty position as an inner node", v.slot);
        uint32_t rank = 0;
        for (uint32_t position = 0; position < 8; ++position) {
            if (!(valid >> position & 1u)) continue;
            const uint32_t child = base + rank++;
            if (seen[child]) INVALID("slot %u of the 8-wide tree is reached twice", child);
            seen[child] = 1;
            if (n.inner_mask >> position & 1u) stack.push_back({child, v.depth + 1u});
            else {
                const HiprLeaf8& leaf = s->wide8_slots[child].leaf;
                if (leaf.triangle[0] >= s->triangle_count || (leaf.triangle[1] != HIPR_LEAF8_NONE && leaf.triangle[1] >= s->triangle_count))
                    INVALID("leaf record in slot %u references triangles %u / %u of %u", child, leaf.triangle[0], leaf.triangle[1], s->triangle_count);
                for (int shift = 8; shift < 16; shift += 2)
                    if (((leaf.flags >> shift) & 3u) == 3u) INVALID("leaf record in slot %u has an invalid corner selector", child);
                for (int which = 0; which < 2; ++which) {
                    if (leaf.triangle[which] == HIPR_LEAF8_NONE) continue;
                    const bool one_sided = (s->triangles[leaf.triangle[which]].flags & HIPR_TRIANGLE_ONE_SIDED) != 0;
                    if ((leaf.flags >> (2 + which) & 1u) && !one_sided) INVALID("leaf record in slot %u marks triangle %u one-sided, the triangle is not", child, leaf.triangle[which]);
                }
                if ((leaf.flags & 12u) && !(leaf.facing_margin >= 0.0f && std::isfinite(leaf.facing_margin))) INVALID("leaf record in slot %u has no valid facing margin", child);
            }
        }
    }
    return nullptr;
#undef INVALID
}

// Bit mask of the shading models that instances reference; `materials`: the pool the DEVICE holds (a geometry update brings instances, not materials).
int shading_model_mask(const HiprInstance* instances, uint32_t count, const HiprMaterial* materials) {
    int models = 0;
    for (uint32_t i = 0; i < count; ++i) models |= 1 << std::min<int>(materials[instances[i].material_index].shading_model, 2);
    return models ? models : 7;
}
// Everything hipr_upload_scene and hipr_update_scene_geometry refuse a description for by looking at it alone, and what the checks derive on the way. Pure host
// code -- no context, no HIP call: hipr_validate_scene is exactly this, and the two uploads run it before they touch the device. `who`: the entry point, for the message.
int preflight_scene(const char* who, const HiprSceneDesc* s, Preflight& out) {
    if (!s) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null scene", who);
    if (s->triangle_count && (!s->nodes || !s->triangles || !s->instances || !s->indices || !s->geometry || !s->materials))
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: missing geometry arrays", who);
    char invalid[256];
    if (validate_scene(s, out.wide_stack_need, invalid, sizeof(invalid)) || validate_wide8(s, out.wide8_height, invalid, sizeof(invalid)))
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: %s", who, invalid);
    for (uint32_t i = 0; i < s->instance_count; ++i)
        if ((s->instances[i].mesh_flags & HIPR_MESH_TEXCOORDS && !s->texcoords) || (s->instances[i].mesh_flags & HIPR_MESH_TINTS && !s->tints) ||
            (s->instances[i].mesh_flags & HIPR_MESH_EMISSIVE && !s->emissions))
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: instance %u flags an attribute whose pool is null", who, i);
    if (const HiprEnvironment* env = s->environment)
        if (env->environment_map_ID <= 0 || uint32_t(env->environment_map_ID) >= s->texture_count || !env->per_pixel_PDF || !env->samples || env->sample_count == 0 ||
            env->pdf_width == 0 || env->pdf_height == 0)
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: incomplete environment description", who);
    return HIPR_OK;
}

// The pools of a checked description, queued on `stream`: all of them (an upload), or those a geometry update brings again.
int ResidentScene::upload_pools(const HiprSceneDesc* s, bool all_pools, hipStream_t stream) {
    int r = 0;
    r |= nodes.upload(s->nodes, size_t(s->node_count) * sizeof(HiprBvhNode), stream);
    if (s->wide_nodes && s->wide_node_count) r |= wide_nodes.upload(s->wide_nodes, size_t(s->wide_node_count) * sizeof(HiprWideNode), stream);
    r |= triangles.upload(s->triangles, size_t(s->triangle_count) * sizeof(HiprTriangle), stream);
    r |= instances.upload(s->instances, size_t(s->instance_count) * sizeof(HiprInstance), stream);
    r |= lights.upload(s->lights, size_t(s->light_count) * sizeof(HiprLight), stream);
    if (all_pools) {
        r |= indices.upload(s->indices, size_t(s->index_count) * 4, stream);
        r |= geometry.upload(s->geometry, size_t(s->vertex_count) * sizeof(HiprVertexGeometry), stream);
        if (s->texcoords) r |= texcoords.upload(s->texcoords, size_t(s->vertex_count) * 8, stream);
        if (s->tints) r |= tints.upload(s->tints, size_t(s->vertex_count) * 4, stream);
        if (s->emissions) r |= emissions.upload(s->emissions, size_t(s->vertex_count) * 12, stream);
        r |= materials.upload(s->materials, size_t(s->material_count) * sizeof(HiprMaterial), stream);
        r |= textures.upload(s->textures, size_t(s->texture_count) * sizeof(HiprTexture), stream);
        r |= texels.upload(s->texels, s->texel_bytes, stream);
        if (const HiprEnvironment* env = s->environment) {
            r |= environment_PDF.upload(env->per_pixel_PDF, size_t(env->pdf_width) * env->pdf_height * sizeof(float), stream);
            r |= environment_samples.upload(env->samples, size_t(env->sample_count) * sizeof(HiprLightSample), stream);
        }
    }
    if (r) return r < 0 ? r : HIPR_ERROR_HIP;
    HIP_TRY(hipStreamSynchronize(stream));      // the caller's arrays are read
    return HIPR_OK;
}

// Uploads (or re-uploads, after a refit) the 8-wide tree of a validated description; trees higher than the largest LDS stack are left to the 4-wide kernels.
int ResidentScene::upload_wide8(const HiprSceneDesc* s, uint32_t height, bool cull_backfaces, hipStream_t stream) {
    wide8 = {};
    wide8_height = 0;
    if (!s->wide8_slots || s->wide8_slot_count == 0 || height > 33u) return HIPR_OK;
    if (int r = wide8_slots.upload(s->wide8_slots, size_t(s->wide8_slot_count) * sizeof(HiprSlot8), stream)) return r;
    HIP_TRY(hipStreamSynchronize(stream));
    wide8.slots = wide8_slots.as<uint4>();
    wide8.slot_count = s->wide8_slot_count;
    for (int a = 0; a < 3; ++a) { wide8.grid_min[a] = s->wide8_grid_min[a]; wide8.grid_cell[a] = s->wide8_grid_cell[a]; }
    wide8.cull_backfaces = cull_backfaces ? 1u : 0u;
    wide8_height = height;
    return HIPR_OK;
}

unsigned short to_unorm16(float v) { return (unsigned short)(v * 65535 + 0.5f); }

// Reverse Halton offsets of OR/Renderer.cpp:323-336 (OR/RNG.h:196-231): primes 2, 3, 5, 7, digits d -> p - d, f64 inside.
float reverse_halton(int prime, int i) {
    double h = 0.0, f = 1.0 / double(prime), fct = f;
    while (i > 0) {
        int digit = i % prime;
        h += (digit == 0 ? 0 : prime - digit) * fct;
        i /= prime;
        fct *= f;
    }
    return float(h);
}

// What an upload derives from the material, texture and light pools it brings: the host copies later calls are checked against, and the kernel instantiations
// the pools allow (ResidentScene: a geometry update keeps them).
void ResidentScene::derive_from_pools(const HiprSceneDesc* s) {
    uploaded_materials.assign(s->materials, s->materials + s->material_count);
    uploaded_textures.assign(s->textures, s->textures + s->texture_count);
    uploaded_environment = s->environment != nullptr;
    uploaded_light_types.resize(s->light_count);
    for (uint32_t l = 0; l < s->light_count; ++l) uploaded_light_types[l] = s->lights[l].flags & HIPR_LIGHT_TYPE_MASK;
    uploaded_texture_count = s->texture_count; uploaded_vertex_count = s->vertex_count; uploaded_index_count = s->index_count; uploaded_texel_bytes = s->texel_bytes;
    uploaded_mesh_attributes = (s->texcoords ? HIPR_MESH_TEXCOORDS : 0u) | (s->tints ? HIPR_MESH_TINTS : 0u) | (s->emissions ? HIPR_MESH_EMISSIVE : 0u);
    derive_switches_from_pools();
}

// The kernel instantiations the material, texture and light pools allow, from the host copies of what the device holds: after an upload, and after a material
// edit (update_materials) has rewritten slots of the material pool.
void ResidentScene::derive_switches_from_pools() {
    has_textures = has_environment = uploaded_environment;
    for (const HiprMaterial& material : uploaded_materials)
        has_textures = has_textures || material.tint_roughness_texture_ID || material.roughness_texture_ID || material.metallic_texture_ID || material.coverage_texture_ID;
    for (uint32_t type : uploaded_light_types) has_environment = has_environment || type == HIPR_LIGHT_PRESAMPLED_ENVIRONMENT;
    for (size_t t = 1; t < uploaded_textures.size(); ++t)       // float textures take the generic samplers: TEXTURES = 2 as well
        has_environment = has_environment || uploaded_textures[t].format == HIPR_TEXEL_R32F || uploaded_textures[t].format == HIPR_TEXEL_RGBA32F;
    has_textures = has_textures || has_environment;
    coverage_textures_r8 = true;
    for (const HiprMaterial& material : uploaded_materials)
        if (const int32_t id = material.coverage_texture_ID)
            coverage_textures_r8 = coverage_textures_r8 && uint32_t(id) < uploaded_textures.size() && uploaded_textures[id].format == HIPR_TEXEL_R8 && !uploaded_textures[id].is_sRGB;
}

// The shade and trace records of every triangle (k_build_shade_triangles: the per-hit attribute chain flattened; k_build_trace_triangles: the vertex + edges form
// the trace kernels test), from the pools and the triangles the device holds at the time.
void ResidentScene::queue_triangle_records(hipStream_t stream) const {
    hipLaunchKernelGGL(k_build_shade_triangles, dim3((args.triangle_count + 255) / 256), dim3(256), 0, stream, args, shade_triangles.as<float4>());
    hipLaunchKernelGGL(k_build_trace_triangles, dim3((args.triangle_count + 255) / 256), dim3(256), 0, stream, args.triangles, args.triangle_count, trace_triangles.as<float4>());
}

// What an upload and a geometry update derive from the triangles, instances and trees they bring -- over the material pool the device HOLDS (uploaded_materials): the
// per-triangle records, the listing pass's classes, the exhaustive search's items (build_trace_items), the 8-wide tree and the device refit's lists.
// `new_topology`: an upload; a geometry update keeps the tree the upload took (or left).
int ResidentScene::derive_from_triangles(const HiprSceneDesc* s, const Preflight& checked, bool new_topology, int requested_variant, bool cull_backfaces, hipStream_t stream) {
    shading_models = shading_model_mask(s->instances, s->instance_count, uploaded_materials.data());
    uploaded_instances.assign(s->instances, s->instances + s->instance_count);
    any_coated_triangle = false;
    all_triangles_opaque = true;
    args.trace_items = nullptr;
    args.trace_item_count = 0;
    if (s->triangle_count) {
        if (int r = shade_triangles.resize(size_t(s->triangle_count) * SHADE_TRIANGLE_QUADS * sizeof(float4))) return r;
        if (int r = trace_triangles.resize(size_t(s->triangle_count) * 3 * sizeof(float4))) return r;
        args.shade_triangles = shade_triangles.as<float4>();
        args.trace_triangles = trace_triangles.as<float4>();
        queue_triangle_records(stream);
        HIP_TRY(hipGetLastError());
        std::vector<unsigned char> classes(s->triangle_count, 0);      // k_classify_hits: bit 0 = the material of its instance carries a coat
        for (uint32_t t = 0; t < s->triangle_count; ++t) {
            all_triangles_opaque = all_triangles_opaque && (s->triangles[t].flags & HIPR_TRIANGLE_OPAQUE) != 0;
            classes[t] = uploaded_materials[s->instances[s->triangles[t].instance_index].material_index].coat != 0 ? 1 : 0;
            any_coated_triangle = any_coated_triangle || classes[t] != 0;
        }
        if (int r = triangle_class.upload(classes.data(), classes.size(), stream)) return r;
        HIP_TRY(hipStreamSynchronize(stream));      // `classes` is read
        if (s->triangle_count <= SMALL_SCENE_TRIANGLES || requested_variant == HIPR_TRACE_EXHAUSTIVE) {
            std::vector<float> items;
            build_trace_items(s->triangles, s->triangle_count, items);
            if (int r = trace_items.upload(items.data(), items.size() * sizeof(float), stream)) return r;
            HIP_TRY(hipStreamSynchronize(stream));
            args.trace_items = trace_items.as<float4>();
            args.trace_item_count = uint32_t(items.size() / 16);
        }
    }
    if (new_topology || wide8.slot_count)
        if (int r = upload_wide8(s, checked.wide8_height, cull_backfaces, stream)) return r;
    return prepare_refit(s, new_topology, stream);
}

// ---- device refit (wide8_refit.h) -------------------------------------------------------------------------------------------------------------------------
// refit_scratch: [0, 48) the six reduced bounds, [48, 52) the rebuild flag, [64, 72) the area sum.
constexpr size_t REFIT_SCRATCH_FLAG = 48, REFIT_SCRATCH_AREA = 64, REFIT_SCRATCH_BYTES = 128;

// Queues passes 2 - 4. WRITE = false: exact boxes and area only (the slots stay as uploaded).
template <bool WRITE>
void ResidentScene::queue_refit_tree(const float* grid_min, const float* grid_cell, hipStream_t st) const {
    HiprSlot8* slots = wide8_slots.as<HiprSlot8>();
    RefitBox* exact = refit_exact.as<RefitBox>();
    char* scratch = refit_scratch.as<char>();
    const uint32_t slot_count = wide8.slot_count;
    if (refit_leaf_count)
        hipLaunchKernelGGL((k_refit_leaves<WRITE>), dim3((refit_leaf_count + REFIT_BLOCK - 1) / REFIT_BLOCK), dim3(REFIT_BLOCK), 0, st, slots, refit_leaf_slots.as<uint32_t>(), refit_leaf_count,
                           triangles.as<HiprTriangle>(), exact, reinterpret_cast<uint32_t*>(scratch + REFIT_SCRATCH_FLAG));
    for (size_t level = refit_level_begin.size() - 1; level-- > 0;) {      // deepest first: a launch per level is the only ordering there is
        const uint32_t begin = refit_level_begin[level], count = refit_level_begin[level + 1] - begin;
        if (!count) continue;
        hipLaunchKernelGGL((k_refit_nodes<WRITE>), dim3((count + REFIT_BLOCK - 1) / REFIT_BLOCK), dim3(REFIT_BLOCK), 0, st, slots, refit_node_slots.as<uint32_t>() + begin, count, exact,
                           grid_min[0], grid_min[1], grid_min[2], grid_cell[0], grid_cell[1], grid_cell[2]);
    }
    const uint32_t blocks = (slot_count + REFIT_BLOCK - 1) / REFIT_BLOCK;
    hipLaunchKernelGGL(k_refit_area, dim3(blocks), dim3(REFIT_BLOCK), 0, st, exact, slot_count, refit_partial.as<double>());
    hipLaunchKernelGGL(k_refit_area_final, dim3(1), dim3(REFIT_BLOCK), 0, st, refit_partial.as<double>(), blocks, reinterpret_cast<double*>(scratch + REFIT_SCRATCH_AREA));
}

// After an upload (`new_topology`) or a geometry update of a scene with the 8-wide tree: the slot lists by kind and level and the
// half area the tree starts with, taken by the kernels that take it after a refit.
int ResidentScene::prepare_refit(const HiprSceneDesc* s, bool new_topology, hipStream_t st) {
    tree_stale = false;
    if (wide8.slot_count == 0) {
        refit_level_begin.clear();
        refit_node_list.clear();
        refit_node_words.clear();
        refit_leaf_count = 0;
        uploaded_half_area = current_half_area = 0.0;
        return HIPR_OK;
    }
    const uint32_t slot_count = wide8.slot_count;
    // A geometry update promises the uploaded topology, and hipr_update_scene_geometry has only compared counts and heights: the lists are kept when every node they
    // name carries the topology words they were made from -- from the root down that is the same tree, slot for slot -- and made again otherwise, so that the
    // leaf kernel never takes a node slot for a leaf record.
    if (!new_topology) {
        new_topology = refit_node_list.empty() || refit_node_words.size() != refit_node_list.size() * 2;
        for (size_t i = 0; i < refit_node_list.size() && !new_topology; ++i) {
            const HiprNode8& n = s->wide8_slots[refit_node_list[i]].node;
            new_topology = n.base_valid != refit_node_words[2 * i] || n.inner_mask != refit_node_words[2 * i + 1];
        }
    }
    if (new_topology) {
        std::vector<uint32_t> nodes = {0u}, leaves;
        nodes.reserve(slot_count / 4 + 1);
        leaves.reserve(slot_count);
        refit_level_begin.assign(1, 0u);
        for (size_t begin = 0; begin < nodes.size();) {      // the tree was validated: every child slot is in range and has one parent
            const size_t end = nodes.size();
            refit_level_begin.push_back(uint32_t(end));
            for (size_t i = begin; i < end; ++i) {
                const HiprNode8& n = s->wide8_slots[nodes[i]].node;
                const uint32_t base = n.base_valid & 0xFFFFFFu, valid = n.base_valid >> 24;
                uint32_t rank = 0;
                for (int p = 0; p < 8; ++p) {
                    if (!(valid >> p & 1u)) continue;
                    const uint32_t child = base + rank++;
                    if (n.inner_mask >> p & 1u) nodes.push_back(child); else leaves.push_back(child);
                }
            }
            begin = end;
        }
        refit_leaf_count = uint32_t(leaves.size());
        refit_node_list.clear();      // the host copies describe what the device holds: set together, once the uploads below are through
        refit_node_words.clear();
        const size_t triangle_blocks = (size_t(s->triangle_count) + REFIT_BLOCK - 1) / REFIT_BLOCK, slot_blocks = (size_t(slot_count) + REFIT_BLOCK - 1) / REFIT_BLOCK;
        int r = 0;
        r |= refit_node_slots.upload(nodes.data(), nodes.size() * 4, st);
        r |= refit_leaf_slots.upload(leaves.data(), leaves.size() * 4, st);
        r |= refit_exact.resize(size_t(slot_count) * sizeof(RefitBox));
        r |= refit_moved.resize(std::max<size_t>(s->instance_count, 1) * 4);
        r |= refit_partial.resize(std::max(triangle_blocks * 6 * sizeof(RefitBound), slot_blocks * sizeof(double)));
        r |= refit_scratch.resize(REFIT_SCRATCH_BYTES);
        if (r) return r < 0 ? r : HIPR_ERROR_HIP;
        HIP_TRY(hipStreamSynchronize(st));      // the upload reads the lists
        refit_node_words.resize(nodes.size() * 2);
        for (size_t i = 0; i < nodes.size(); ++i) {
            refit_node_words[2 * i] = s->wide8_slots[nodes[i]].node.base_valid;
            refit_node_words[2 * i + 1] = s->wide8_slots[nodes[i]].node.inner_mask;
        }
        refit_node_list = std::move(nodes);
    }
    queue_refit_tree<false>(wide8.grid_min, wide8.grid_cell, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&uploaded_half_area, refit_scratch.as<char>() + REFIT_SCRATCH_AREA, sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    current_half_area = uploaded_half_area;
    return HIPR_OK;
}

int ResidentScene::upload(const HiprSceneDesc* s, const Preflight& checked, int requested_variant, bool cull_backfaces, hipStream_t stream) {
    begin_write();
    wide4_awaits_geometry = false;
    if (int r = upload_pools(s, true, stream)) return r;
    const HiprEnvironment* env = s->environment;
    args.nodes = nodes.as<float4>();
    args.node_count = s->node_count;
    args.wide_nodes = s->wide_nodes && s->wide_node_count ? wide_nodes.as<uint4>() : nullptr;
    args.wide_node_count = s->wide_nodes ? s->wide_node_count : 0u;
    args.triangles = triangles.as<float4>();
    args.triangle_count = s->triangle_count;
    args.instances = instances.as<HiprInstance>();
    args.indices = indices.as<uint32_t>();
    args.geometry = geometry.as<float4>();
    args.texcoords = texcoords.as<float2>();
    args.tints = tints.as<uint32_t>();
    args.emissions = emissions.as<float>();
    args.materials = materials.as<HiprMaterial>();
    args.lights = lights.as<HiprLight>();
    args.light_count = s->light_count;
    args.textures = textures.as<HiprTexture>();
    args.texels = texels.as<uint8_t>();
    args.env_map_ID = env ? env->environment_map_ID : 0;
    args.env_per_pixel_PDF = env ? environment_PDF.as<float>() : nullptr;
    args.env_samples = env ? environment_samples.as<float4>() : nullptr;
    args.env_pdf_width = env ? env->pdf_width : 0u; args.env_pdf_height = env ? env->pdf_height : 0u; args.env_sample_count = env ? env->sample_count : 0u;
    wide_stack_entries = checked.wide_stack_need;
    stack_size = s->bvh_max_depth <= 16 ? 16 : (s->bvh_max_depth <= 32 ? 32 : 64);
    derive_from_pools(s);
    if (int r = derive_from_triangles(s, checked, true, requested_variant, cull_backfaces, stream)) return r;
    choose_variant(requested_variant);
    ready = true;
    return HIPR_OK;
}

// The pools it brings again have the uploaded sizes (hipr_update_scene_geometry has compared them): no buffer moves, the pointers and counts in `args` stay.
int ResidentScene::update_geometry(const HiprSceneDesc* s, const Preflight& checked, int requested_variant, bool cull_backfaces, hipStream_t stream) {
    begin_write();
    if (int r = upload_pools(s, false, stream)) return r;
    if (wide4_awaits_geometry) {      // the 4-wide array of the rebuilt tree: the buffer may have moved and its size has changed
        args.wide_nodes = s->wide_nodes && s->wide_node_count ? wide_nodes.as<uint4>() : nullptr;
        args.wide_node_count = s->wide_nodes ? s->wide_node_count : 0u;
        wide_stack_entries = checked.wide_stack_need;
        wide4_awaits_geometry = false;
    }
    if (int r = derive_from_triangles(s, checked, false, requested_variant, cull_backfaces, stream)) return r;      // also ends the state a device refit left
    ready = true;
    return HIPR_OK;
}

// The lights ARE brought again by a geometry update and a device refit (they move), but the kernels were instantiated for the kinds of light the upload brought --
// environment code or not -- and the environment's own data is not part of either: a light may move, not change its type.
int ResidentScene::lights_keep_their_types(const char* who, const HiprLight* new_lights, uint32_t count) const {
    for (uint32_t l = 0; l < count; ++l)
        if ((new_lights[l].flags & HIPR_LIGHT_TYPE_MASK) != uploaded_light_types[l])
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: light %u changes its type (%u -> %u); upload the scene instead", who, l, uploaded_light_types[l], new_lights[l].flags & HIPR_LIGHT_TYPE_MASK);
    return HIPR_OK;
}

// The device work of hipr_refit_scene_transforms, which has checked the arguments against uploaded_instances and uploaded_light_types.
int ResidentScene::refit_transforms(const HiprInstanceTransform* moved, uint32_t moved_count, const HiprLight* new_lights, uint32_t light_count, hipStream_t st, HiprRefitResult* out) {
    begin_write();
    *out = {};
    if (new_lights && light_count) {
        if (int r = lights.upload(new_lights, size_t(light_count) * sizeof(HiprLight), st)) return r;
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (moved_count) {
        std::vector<uint32_t> flags(uploaded_instances.size(), 0u);
        std::vector<HiprInstance> moved_instances = uploaded_instances;      // becomes the host copy once the device holds it (after the last synchronise)
        for (uint32_t k = 0; k < moved_count; ++k) {
            std::memcpy(moved_instances[moved[k].instance_index].object_to_world, moved[k].object_to_world, sizeof(moved[k].object_to_world));
            flags[moved[k].instance_index] = 1u;
        }
        HIP_TRY(hipMemcpyAsync(instances.ptr, moved_instances.data(), moved_instances.size() * sizeof(HiprInstance), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(refit_moved.ptr, flags.data(), flags.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(refit_scratch.ptr, 0, REFIT_SCRATCH_BYTES, st));
        // pass 1: world-space triangles and the scene's bounds
        const uint32_t blocks = (args.triangle_count + REFIT_BLOCK - 1) / REFIT_BLOCK;
        hipLaunchKernelGGL(k_refit_triangles, dim3(blocks), dim3(REFIT_BLOCK), 0, st, triangles.as<HiprTriangle>(), args.triangle_count, instances.as<HiprInstance>(), refit_moved.as<uint32_t>(),
                           indices.as<uint32_t>(), geometry.as<HiprVertexGeometry>(), refit_partial.as<RefitBound>());
        hipLaunchKernelGGL(k_refit_bounds_final, dim3(1), dim3(REFIT_BLOCK), 0, st, refit_partial.as<RefitBound>(), blocks, refit_scratch.as<RefitBound>());
        HIP_TRY(hipGetLastError());
        RefitBound bounds[6];
        HIP_TRY(hipMemcpyAsync(bounds, refit_scratch.ptr, sizeof(bounds), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));      // `flags` and the instances are read by now as well
        const float lo[3] = {bounds[0].v, bounds[1].v, bounds[2].v}, hi[3] = {bounds[3].v, bounds[4].v, bounds[5].v};
        float grid_min[3], grid_cell[3];
        refit_grid(lo, hi, grid_min, grid_cell);      // the moved scene's bounds: node origins must not be clamped at the ends of a stale grid
        // passes 2 - 4, then the records derived from the triangles
        queue_refit_tree<true>(grid_min, grid_cell, st);
        queue_triangle_records(st);
        HIP_TRY(hipGetLastError());
        struct { uint32_t flag; uint32_t pad[3]; double area; } tail = {};
        static_assert(REFIT_SCRATCH_AREA - REFIT_SCRATCH_FLAG == 16, "the flag and the area are read back together");
        HIP_TRY(hipMemcpyAsync(&tail, refit_scratch.as<char>() + REFIT_SCRATCH_FLAG, sizeof(tail), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        uploaded_instances.swap(moved_instances);
        tree_stale = true;
        for (int a = 0; a < 3; ++a) { wide8.grid_min[a] = grid_min[a]; wide8.grid_cell[a] = grid_cell[a]; }
        current_half_area = tail.area;
        out->needs_rebuild = tail.flag ? 1 : 0;      // a pair parted: this tree cannot hold the scene any more
    }
    out->child_half_area = current_half_area;
    out->uploaded_half_area = uploaded_half_area;
    for (int a = 0; a < 3; ++a) { out->grid_min[a] = wide8.grid_min[a]; out->grid_cell[a] = wide8.grid_cell[a]; }
    ready = !out->needs_rebuild;
    awaits_rebuild = !ready;
    return HIPR_OK;
}

// The device work of hipr_update_scene_materials, which has checked every index against uploaded_materials, uploaded_instances and uploaded_textures.
int ResidentScene::update_materials(const HiprMaterialUpdate* changed, uint32_t changed_count, const HiprInstanceMaterial* assignments, uint32_t assignment_count, hipStream_t st) {
    begin_write();
    // the host copies as they will be once the device holds them (after the last synchronise); the copies below read from them
    std::vector<HiprMaterial> new_materials = uploaded_materials;
    std::vector<HiprInstance> new_instances = uploaded_instances;
    std::vector<bool> rewritten(new_materials.size(), false);
    std::vector<uint32_t> touched(std::max<size_t>(new_instances.size(), 1), 0u);
    for (uint32_t k = 0; k < changed_count; ++k) { new_materials[changed[k].material_index] = changed[k].material; rewritten[changed[k].material_index] = true; }
    for (uint32_t k = 0; k < assignment_count; ++k) { new_instances[assignments[k].instance_index].material_index = assignments[k].material_index; touched[assignments[k].instance_index] = 1u; }
    for (size_t i = 0; i < new_instances.size(); ++i)
        if (rewritten[size_t(new_instances[i].material_index)]) touched[i] = 1u;
    // 1. the changed slots and words
    for (uint32_t k = 0; k < changed_count; ++k) {
        const size_t at = changed[k].material_index;
        HIP_TRY(hipMemcpyAsync(materials.as<HiprMaterial>() + at, &new_materials[at], sizeof(HiprMaterial), hipMemcpyHostToDevice, st));
    }
    for (uint32_t k = 0; k < assignment_count; ++k) {
        const size_t at = assignments[k].instance_index;
        HIP_TRY(hipMemcpyAsync(&instances.as<HiprInstance>()[at].material_index, &new_instances[at].material_index, sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    uint32_t reduction[2] = {1u, 0u};      // all opaque, none coated: the result for a scene without triangles
    if (args.triangle_count) {
        // 2. the two passes
        if (int r = material_touched.upload(touched.data(), touched.size() * 4, st)) return r;
        if (int r = material_scratch.resize(64)) return r;
        uint32_t* words = material_scratch.as<uint32_t>();
        HIP_TRY(hipMemsetAsync(words, 0, 64, st));
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(words), 1, 1, st));
        const MaterialUpdateArrays a = {triangles.as<HiprTriangle>(), args.triangle_count, instances.as<HiprInstance>(), materials.as<HiprMaterial>(), indices.as<uint32_t>(),
                                        reinterpret_cast<const float*>(args.texcoords), textures.as<HiprTexture>(), uint32_t(uploaded_textures.size()), texels.as<uint8_t>(),
                                        material_touched.as<uint32_t>(), trace_triangles.as<uint32_t>(), shade_triangles.as<uint32_t>(), triangle_class.as<uint8_t>()};
        hipLaunchKernelGGL(k_update_triangle_materials, dim3((args.triangle_count + MATERIAL_UPDATE_BLOCK - 1) / MATERIAL_UPDATE_BLOCK), dim3(MATERIAL_UPDATE_BLOCK), 0, st, a, words);
        if (wide8.slot_count && refit_leaf_count)
            hipLaunchKernelGGL(k_update_leaf_flags, dim3((refit_leaf_count + MATERIAL_UPDATE_BLOCK - 1) / MATERIAL_UPDATE_BLOCK), dim3(MATERIAL_UPDATE_BLOCK), 0, st, wide8_slots.as<HiprSlot8>(),
                               refit_leaf_slots.as<uint32_t>(), refit_leaf_count, triangles.as<HiprTriangle>());
        HIP_TRY(hipGetLastError());
        // 3. the eight reduction bytes
        HIP_TRY(hipMemcpyAsync(reduction, words, sizeof(reduction), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));      // `touched`, new_materials and new_instances are read by now as well
    // 4., 5. the host copies in step, and what is derived from them
    uploaded_materials.swap(new_materials);
    uploaded_instances.swap(new_instances);
    shading_models = shading_model_mask(uploaded_instances.data(), uint32_t(uploaded_instances.size()), uploaded_materials.data());
    derive_switches_from_pools();
    all_triangles_opaque = reduction[0] != 0;
    any_coated_triangle = reduction[1] != 0;
    ready = true;
    return HIPR_OK;
}

// The device work of hipr_append_scene_pools (pool_growth.h). Every new buffer is allocated BEFORE the scene is touched: a failed allocation frees what it got and
// leaves the scene as found. A pool whose buffer has the room (a larger scene was uploaded before) takes its tail in place; the others get a buffer of exactly the
// new size -- no headroom: what it is worth has not been measured (the pools of the 10 M atrium are 152 MB and copy in 0.1 ms; a texel pool can be gigabytes). Then, as the other writers: not ready,
// the copies and the mirror kernel on the stream, the new pointers in `args`, the host copies, the switches -- and the state the call found, ready or awaiting a
// rebuild: no tree, triangle or instance references a tail, so nothing derived from them changes.
int ResidentScene::append_pools(const HiprPoolGrowth& g, hipStream_t st) {
    struct Pool { DeviceBuffer* pool; size_t keep, tail_bytes; const void* tail; DeviceBuffer fresh; };
    const size_t vertices = uploaded_vertex_count;
    // an attribute pool the device holds takes its tail; one it does not hold comes whole (or not at all)
    auto attribute = [&](DeviceBuffer* pool, uint32_t bit, const void* array, uint32_t covered, size_t stride) -> Pool {
        return {pool, uploaded_mesh_attributes & bit ? vertices * stride : 0u, size_t(covered) * stride, array, DeviceBuffer()};
    };
    size_t segment_words = 0;
    for (uint32_t k = 0; k < g.segment_count; ++k) segment_words += g.segments[k].index_count;
    Pool pools[] = {
        {&indices, size_t(uploaded_index_count) * 4, segment_words * 4, nullptr, DeviceBuffer()},      // its tail is the segments'
        {&geometry, vertices * sizeof(HiprVertexGeometry), size_t(g.vertex_count) * sizeof(HiprVertexGeometry), g.geometry, DeviceBuffer()},
        attribute(&texcoords, HIPR_MESH_TEXCOORDS, g.texcoords, g.texcoord_vertices, 8),
        attribute(&tints, HIPR_MESH_TINTS, g.tints, g.tint_vertices, 4),
        attribute(&emissions, HIPR_MESH_EMISSIVE, g.emissions, g.emission_vertices, 12),
        {&materials, uploaded_materials.size() * sizeof(HiprMaterial), size_t(g.material_count) * sizeof(HiprMaterial), g.materials, DeviceBuffer()},
        {&textures, uploaded_textures.size() * sizeof(HiprTexture), size_t(g.texture_count) * sizeof(HiprTexture), g.textures, DeviceBuffer()},
        {&texels, size_t(uploaded_texel_bytes), size_t(g.texel_bytes), g.texels, DeviceBuffer()},
    };
    const auto t0 = std::chrono::steady_clock::now();
    for (Pool& p : pools)
        if (p.tail_bytes && !(p.pool->ptr && p.pool->bytes >= p.keep + p.tail_bytes))
            if (p.fresh.resize(p.keep + p.tail_bytes)) {
                (void)hipGetLastError();      // the failed allocation's error is answered here: it must not meet the next call's check
                return HIPR_ERROR_OUT_OF_MEMORY;      // `pools` goes, and with it what the others got
            }
    const auto t1 = std::chrono::steady_clock::now();
    const bool was_ready = ready, awaited_rebuild = awaits_rebuild;
    begin_write();
    // the resident parts into the new allocations first; events around them tell their time from the tails' without a synchronise of their own
    for (Event& e : append_events)
        if (!e) e = make_event(hipEventDefault);
    const bool timed = append_events[0] && append_events[1] && append_events[2];
    if (timed) HIP_TRY(hipEventRecord(append_events[0], st));
    for (Pool& p : pools)
        if (p.tail_bytes && p.fresh.ptr) HIP_TRY(queue_pool_growth(p.fresh.ptr, p.pool->ptr, p.keep, nullptr, 0u, st));
    if (timed) HIP_TRY(hipEventRecord(append_events[1], st));
    for (Pool& p : pools) {
        if (!p.tail_bytes) continue;
        void* grown = p.fresh.ptr ? p.fresh.ptr : p.pool->ptr;
        HIP_TRY(queue_pool_growth(grown, grown, p.keep, p.tail, p.tail ? p.tail_bytes : 0u, st));
        if (p.pool != &indices) continue;
        // the segments in order: a mirror reads what the stream has put there by then, earlier segments of this call included
        uint32_t* words = static_cast<uint32_t*>(grown);
        size_t position = uploaded_index_count, taken = 0;
        for (uint32_t k = 0; k < g.segment_count; ++k) {
            const HiprIndexSegment& s = g.segments[k];
            if (s.mirrored_from == HIPR_SEGMENT_FROM_HOST) {
                if (s.index_count) HIP_TRY(hipMemcpyAsync(words + position, g.indices + taken, size_t(s.index_count) * 4, hipMemcpyHostToDevice, st));
                taken += s.index_count;
            } else queue_mirror_triples(words, s.mirrored_from, uint32_t(position / 3), s.index_count / 3, st);
            position += s.index_count;
        }
        HIP_TRY(hipGetLastError());
    }
    if (timed) HIP_TRY(hipEventRecord(append_events[2], st));
    HIP_TRY(hipStreamSynchronize(st));      // the caller's arrays are read; the old buffers are free to go
    float copies_ms = 0.0f, tails_ms = 0.0f;
    if (timed) { HIP_TRY(hipEventElapsedTime(&copies_ms, append_events[0], append_events[1])); HIP_TRY(hipEventElapsedTime(&tails_ms, append_events[1], append_events[2])); }
    append_ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count(); append_ms[1] = copies_ms; append_ms[2] = tails_ms;
    for (Pool& p : pools)
        if (p.fresh.ptr) std::swap(*p.pool, p.fresh);      // the old buffer goes with `pools`
    args.indices = indices.as<uint32_t>();
    args.geometry = geometry.as<float4>();
    args.texcoords = texcoords.as<float2>();
    args.tints = tints.as<uint32_t>();
    args.emissions = emissions.as<float>();
    args.materials = materials.as<HiprMaterial>();
    args.textures = textures.as<HiprTexture>();
    args.texels = texels.as<uint8_t>();
    uploaded_materials.insert(uploaded_materials.end(), g.materials, g.materials + g.material_count);
    uploaded_textures.insert(uploaded_textures.end(), g.textures, g.textures + g.texture_count);
    uploaded_texture_count = uint32_t(uploaded_textures.size());
    uploaded_vertex_count += g.vertex_count;
    uploaded_index_count += uint32_t(segment_words);
    uploaded_mesh_attributes |= (g.texcoord_vertices ? HIPR_MESH_TEXCOORDS : 0u) | (g.tint_vertices ? HIPR_MESH_TINTS : 0u) | (g.emission_vertices ? HIPR_MESH_EMISSIVE : 0u);
    uploaded_texel_bytes += g.texel_bytes;
    derive_switches_from_pools();
    ready = was_ready;
    awaits_rebuild = awaited_rebuild;
    return HIPR_OK;
}

// The last step of hipr_rebuild_scene_trees, which has refused everything it refuses: the new resident arrays, and what an upload derives from them. The pools, the
// instances and the lights stay; all_triangles_opaque, any_coated_triangle and the other switches cannot change under a permutation of the triangles and stay. The
// 4-wide array is not rebuilt: tree_stale stays set until the next upload or geometry update, as after the refit.
// After hipr_edit_scene_instances (`built.new_set`) the set of triangles and the instance list are other ones: every per-triangle and per-instance array takes the new
// size, the instance array and its host copy become the new list, and the switches that follow the triangles and the instances are the ones reduced over the new set.
// The pools stay, and with them the switches derived from them.
int ResidentScene::install_rebuilt_trees(const RebuiltTrees& built, hipStream_t st) {
    begin_write();
    if (const RebuiltTrees::NewSet* set = built.new_set) {
        const size_t t = set->triangle_count, i = set->instances->size();
        int r = 0;
        r |= triangles.resize(t * sizeof(HiprTriangle));
        r |= triangle_class.resize(t);
        r |= shade_triangles.resize(t * SHADE_TRIANGLE_QUADS * sizeof(float4));
        r |= trace_triangles.resize(t * 3 * sizeof(float4));
        r |= instances.resize(i * sizeof(HiprInstance));
        if (r) return r < 0 ? r : HIPR_ERROR_HIP;
        HIP_TRY(hipMemcpyAsync(instances.ptr, set->device_instances, i * sizeof(HiprInstance), hipMemcpyDeviceToDevice, st));
        args.triangles = triangles.as<float4>();
        args.triangle_count = set->triangle_count;
        args.shade_triangles = shade_triangles.as<float4>();
        args.trace_triangles = trace_triangles.as<float4>();
        args.instances = instances.as<HiprInstance>();
        uploaded_instances = *set->instances;
        shading_models = shading_model_mask(uploaded_instances.data(), uint32_t(uploaded_instances.size()), uploaded_materials.data());
        all_triangles_opaque = set->all_triangles_opaque;
        any_coated_triangle = set->any_coated_triangle;
    }
    const uint32_t triangle_count = args.triangle_count;
    hipLaunchKernelGGL(k_rebuild_gather, dim3((triangle_count + REBUILD_BLOCK - 1) / REBUILD_BLOCK), dim3(REBUILD_BLOCK), 0, st, built.flat, built.flat_class, built.order,
                       triangles.as<HiprTriangle>(), triangle_class.as<uint8_t>(), triangle_count);
    HIP_TRY(hipGetLastError());
    if (int r = nodes.resize(size_t(built.node_count) * sizeof(HiprBvhNode))) return r;
    if (int r = wide8_slots.resize(size_t(built.wide8.slot_count) * sizeof(HiprSlot8))) return r;
    HIP_TRY(hipMemcpyAsync(nodes.ptr, built.nodes, size_t(built.node_count) * sizeof(HiprBvhNode), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(wide8_slots.ptr, built.slots, size_t(built.wide8.slot_count) * sizeof(HiprSlot8), hipMemcpyDeviceToDevice, st));
    args.nodes = nodes.as<float4>();
    args.node_count = built.node_count;
    wide8.slots = wide8_slots.as<uint4>();
    wide8.slot_count = built.wide8.slot_count;
    for (int a = 0; a < 3; ++a) { wide8.grid_min[a] = built.wide8.grid_min[a]; wide8.grid_cell[a] = built.wide8.grid_cell[a]; }
    wide8_height = built.wide8.height;
    const uint32_t bvh_max_depth = built.deepest + 1u;      // BvhBuildResult::max_depth
    stack_size = bvh_max_depth <= 16 ? 16 : (bvh_max_depth <= 32 ? 32 : 64);
    queue_triangle_records(st);
    HIP_TRY(hipGetLastError());
    HiprSceneDesc lists = {};      // what prepare_refit reads of a description
    lists.wide8_slots = built.host_slots; lists.wide8_slot_count = built.wide8.slot_count;
    lists.triangle_count = triangle_count; lists.instance_count = uint32_t(uploaded_instances.size());
    if (int r = prepare_refit(&lists, true, st)) return r;      // the slot lists by kind and level with their host copies, and uploaded_half_area by the kernels that take it at upload
    tree_stale = true;
    wide4_awaits_geometry = true;
    ready = true;
    return HIPR_OK;
}

} // namespace

extern "C" {

const char* hipr_last_error(void) { return g_last_error.c_str(); }
// Not part of the public header: group.hip hands the message of a member that failed on a worker thread to the calling thread.
void hipr_internal_set_last_error(const char* message) { g_last_error = message ? message : ""; }

int hipr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int hipr_create(int device_id, HiprContext** out_context) {
    if (!out_context) return fail(HIPR_ERROR_INVALID_ARGUMENT, "out_context is null");
    *out_context = nullptr;
    int n = hipr_device_count();
    if (n == 0) return fail(HIPR_ERROR_NO_DEVICE, "no HIP device available");
    if (device_id < 0 || device_id >= n) return fail(HIPR_ERROR_INVALID_ARGUMENT, "device %d out of range [0, %d)", device_id, n);
    HIP_TRY(hipSetDevice(device_id));
    std::unique_ptr<HiprContext, int (*)(HiprContext*)> owner(new HiprContext(), hipr_destroy);      // the one failure exit: whichever return below is taken before release()
    HiprContext* c = owner.get();
    c->device = device_id;
    c->own_stream = make_stream(); c->copy_stream = make_stream();
    c->pass_start = make_event(); c->accumulated = make_event();
    bool ok = c->own_stream && c->copy_stream && c->pass_start && c->accumulated;
    for (auto& slot : c->pass_slots) { slot.tail_counts = make_pinned_words(2 * 128); ok = ok && slot.tail_counts; }
    c->stream = c->own_stream;
    for (int g = 0; ok && g < MAX_WAVEFRONTS; ++g) {
        Wavefront& w = c->wavefronts[g];
        if (g > 0) { w.own_stream = make_stream(); ok = ok && w.own_stream; }
        w.stream = g == 0 ? c->stream : w.own_stream;
        for (int i = 0; i < 2; ++i) { w.shade_done[i] = make_event(); w.counts_copied[i] = make_event(); ok = ok && w.shade_done[i] && w.counts_copied[i]; }
        w.finished = make_event();
        w.host_counts = make_pinned_words(HOST_COUNT_WORDS);
        ok = ok && w.finished && w.host_counts && w.queue_counts.resize(COUNT_LINES * COUNT_PAIR_STRIDE * sizeof(uint32_t)) == 0;
    }
    if (!ok) return fail(HIPR_ERROR_HIP, "stream / event / pinned allocation failed");
    if (int s = c->counters.resize(sizeof(DeviceCounters))) return s;
    if (int s = c->work_counters.resize(2 * WORK_COUNTERS * sizeof(uint32_t))) return s;
    c->pass_slots[0].work_index = c->pass_slots[1].work_index = WORK_SETS;   // forces the first launch of either slot to zero its ring
    hipDeviceProp_t props;
    if (hipGetDeviceProperties(&props, device_id) == hipSuccess && props.multiProcessorCount > 0) c->cu_count = props.multiProcessorCount;
    c->knobs = knobs_from_environment();
    HIP_TRY(hipMemsetAsync(c->counters.ptr, 0, sizeof(DeviceCounters), c->stream));

    float offsets[256 * 4];
    const int primes[4] = {2, 3, 5, 7};
    for (int i = 0; i < 256; ++i)
        for (int d = 0; d < 4; ++d) offsets[4 * i + d] = reverse_halton(primes[d], i);
    if (int s = c->sample_offsets.upload(offsets, sizeof(offsets), c->stream)) return s;
    // Byte-indexed Sobol tables: entry [d][k][b] = XOR of the direction numbers of dimension d + 1 selected by byte k = b.
    std::vector<uint32_t> sobol(SOBOL_TABLE_WORDS);
    for (int d = 0; d < 3; ++d)
        for (int k = 0; k < 4; ++k)
            for (int b = 0; b < 256; ++b) {
                uint32_t v = 0;
                for (int j = 0; j < 8; ++j)
                    if (b & (1 << j)) v ^= SOBOL_DIRECTIONS[d][8 * k + j];
                sobol[(d * 4 + k) * 256 + b] = v;
            }
    if (int s = c->sobol_tables.upload(sobol.data(), sobol.size() * 4, c->stream)) return s;
    if (int finish_status = finish_all(c)) return finish_status;
    c->scene.args.sobol_tables = c->sobol_tables.as<uint32_t>();
    c->scene.args.sample_offsets = c->sample_offsets.as<float4>();
    c->scene.args.next_event_sample_count = 3;   // OR/Renderer.cpp:479
    *out_context = owner.release();
    return HIPR_OK;
}

int hipr_destroy(HiprContext* c) {
    if (!c) return HIPR_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();      // nothing is freed before this; the members then go in reverse order, the context's streams last
    delete c;
    return HIPR_OK;
}

int hipr_set_stream(HiprContext* c, void* hip_stream) {
    if (int s = check_context(c)) return s;
    if (int s = drain(c)) return s;
    c->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->own_stream;
    c->wavefronts[0].stream = c->stream;
    return HIPR_OK;
}

int hipr_upload_tables(HiprContext* c, const HiprTables* t) {
    if (int s = check_context(c)) return s;
    if (!t || !t->ggx_with_fresnel_rho || !t->ggx_rho || !t->dielectric_light_rho || !t->dielectric_dense_rho || !t->ggx_alpha_from_max_PDF)
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_upload_tables: null table");
    std::vector<unsigned short> rho(2 * 32 * 32), diel(2 * 32 * 16 * 16), alpha(32 * 32);
    for (int i = 0; i < 32 * 32; ++i) {
        rho[2 * i] = to_unorm16(t->ggx_with_fresnel_rho[i]);   // F0 = 0
        rho[2 * i + 1] = to_unorm16(t->ggx_rho[i]);            // F0 = 1
        alpha[i] = to_unorm16(t->ggx_alpha_from_max_PDF[i]);
    }
    const int per_medium = 16 * 16 * 16;
    for (int i = 0; i < 2 * per_medium; ++i) {
        diel[i] = to_unorm16(t->dielectric_light_rho[i]);
        diel[2 * per_medium + i] = to_unorm16(t->dielectric_dense_rho[i]);
    }
    if (int s = c->ggx_rho.upload(rho.data(), rho.size() * 2, c->stream)) return s;
    if (int s = c->dielectric_rho.upload(diel.data(), diel.size() * 2, c->stream)) return s;
    if (int s = c->alpha.upload(alpha.data(), alpha.size() * 2, c->stream)) return s;
    if (int finish_status = finish_all(c)) return finish_status;
    c->scene.args.tables = {c->ggx_rho.as<ushort2>(), c->dielectric_rho.as<ushort2>(), c->alpha.as<unsigned short>()};
    c->tables_ready = true;
    return HIPR_OK;
}

int hipr_validate_scene(const HiprSceneDesc* s) {
    Preflight checked;
    return preflight_scene("hipr_validate_scene", s, checked);
}

int hipr_upload_scene(HiprContext* c, const HiprSceneDesc* s) {
    if (int st = check_context(c)) return st;
    Preflight checked;
    if (int st = preflight_scene("hipr_upload_scene", s, checked)) return st;
    // what the kernels cannot serve (a description hipr_validate_scene finds sound may still meet these)
    if (s->bvh_max_depth > 64) return fail(HIPR_ERROR_UNSUPPORTED, "BVH depth %u exceeds the 64 entry LDS stack", s->bvh_max_depth);
    if (checked.wide_stack_need > 32u + uint32_t(TRACE_SPILL_ENTRIES))
        return fail(HIPR_ERROR_UNSUPPORTED, "the wide BVH needs %u stack entries, more than the %u the traversal kernels provide", checked.wide_stack_need, 32u + uint32_t(TRACE_SPILL_ENTRIES));
    if (s->environment) {
        const uint8_t format = s->textures[s->environment->environment_map_ID].format;
        if (format != HIPR_TEXEL_RGBA8 && format != HIPR_TEXEL_RGBA32F)
            return fail(HIPR_ERROR_UNSUPPORTED, "only environments with 4 channels are supported (OptiXRenderer/Renderer.cpp:1141-1158)");
    }
    if (int finish_status = finish_all(c)) return finish_status;
    return c->scene.upload(s, checked, c->knobs.trace_variant, c->knobs.cull_backfaces, c->stream);
}

int hipr_update_scene_geometry(HiprContext* c, const HiprSceneDesc* s) {
    if (int st = check_context(c)) return st;
    Preflight checked;
    if (int st = preflight_scene("hipr_update_scene_geometry", s, checked)) return st;
    const ResidentScene& r = c->scene;
    if (!r.ready) return fail(HIPR_ERROR_NOT_READY, "hipr_update_scene_geometry: no scene uploaded");
    // Meshes, materials and textures stay on the device as uploaded: the description was validated against ITS pools, so those must be the
    // uploaded ones in size -- an index that is in range for a larger pool of the description would read out of bounds on the device.
    if (s->material_count != r.uploaded_materials.size() || s->texture_count != r.uploaded_texture_count || s->vertex_count != r.uploaded_vertex_count ||
        s->index_count != r.uploaded_index_count || s->texel_bytes != r.uploaded_texel_bytes)
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_geometry: material, texture, vertex, index and texel pool sizes must equal the uploaded scene's (those pools are not re-uploaded)");
    const bool wide4_follows = r.wide4_awaits_geometry;      // after hipr_rebuild_scene_trees the 4-wide tree is a new one: it is taken, not compared
    if (s->node_count != r.args.node_count || s->triangle_count != r.args.triangle_count || (!wide4_follows && (s->wide_nodes ? s->wide_node_count : 0u) != r.args.wide_node_count) ||
        s->light_count != r.args.light_count || s->instance_count != r.uploaded_instances.size())
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_geometry: node, triangle, instance and light counts must equal the uploaded scene's (a refit keeps the topology)");
    if (!wide4_follows && checked.wide_stack_need != r.wide_stack_entries) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_geometry: the wide BVH's topology changed");
    if (wide4_follows && (checked.wide_stack_need > 32u + uint32_t(TRACE_SPILL_ENTRIES) || s->bvh_max_depth > 64))
        return fail(HIPR_ERROR_UNSUPPORTED, "hipr_update_scene_geometry: the rebuilt scene's trees need more stack than the traversal kernels provide");
    if (r.wide8.slot_count && (s->wide8_slot_count != r.wide8.slot_count || checked.wide8_height != r.wide8_height))
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_geometry: the 8-wide tree's topology changed");
    if (int st = r.lights_keep_their_types("hipr_update_scene_geometry", s->lights, s->light_count)) return st;
    if (int finish_status = finish_all(c)) return finish_status;      // pipelined passes included: no pending pass may go on over the new geometry
    return c->scene.update_geometry(s, checked, c->knobs.trace_variant, c->knobs.cull_backfaces, c->stream);
}

int hipr_refit_scene_transforms(HiprContext* c, const HiprInstanceTransform* moved, uint32_t moved_count, const HiprLight* lights, uint32_t light_count, HiprRefitResult* out) {
    if (int st = check_context(c)) return st;
    if (!out || (moved_count && !moved)) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_refit_scene_transforms: null argument");
    const ResidentScene& r = c->scene;
    if (!r.ready) return fail(HIPR_ERROR_NOT_READY, "hipr_refit_scene_transforms: no scene uploaded");
    // Scenes that are not traced through the 8-wide tree have at most 64 BVH2 nodes (or a tree too high for the kernels, or a search forced for an experiment): the
    // host path costs nothing there, and the arrays their search walks are the ones this call leaves stale. The exhaustive search's items are built on the host.
    if (r.wide8.slot_count == 0 || !c->use_wide8() || r.args.trace_item_count != 0 || r.args.triangle_count > 0x55555555u)
        return fail(HIPR_ERROR_UNSUPPORTED, "hipr_refit_scene_transforms: the uploaded scene is not traced through the 8-wide tree; refit on the host and call hipr_update_scene_geometry");
    for (uint32_t k = 0; k < moved_count; ++k) {
        if (moved[k].instance_index >= r.uploaded_instances.size())
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_refit_scene_transforms: instance %u of %zu", moved[k].instance_index, r.uploaded_instances.size());
        for (int e = 0; e < 12; ++e)
            if (!std::isfinite(moved[k].object_to_world[e])) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_refit_scene_transforms: the matrix of instance %u is not finite", moved[k].instance_index);
        // A mirrored instance is drawn from index triples of its own (two corners exchanged): that changes the triangle array, which stays the host path's business.
        if (refit_mirrors(moved[k].object_to_world) != refit_mirrors(r.uploaded_instances[moved[k].instance_index].object_to_world))
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_refit_scene_transforms: the matrix of instance %u changes its handedness; refit on the host", moved[k].instance_index);
    }
    if (lights) {
        if (light_count != r.args.light_count) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_refit_scene_transforms: %u lights given, the uploaded scene has %u", light_count, r.args.light_count);
        if (int st = r.lights_keep_their_types("hipr_refit_scene_transforms", lights, light_count)) return st;
    }
    if (int finish_status = finish_all(c)) return finish_status;      // no pending pass may go on over the new geometry
    return c->scene.refit_transforms(moved, moved_count, lights, light_count, c->stream, out);
}

// Not part of the public header: every refusal of hipr_update_scene_materials, and nothing else -- the device and the books stay as they are. The group asks
// every member before any member writes.
int hipr_internal_check_material_update(HiprContext* c, const HiprMaterialUpdate* materials, uint32_t material_count, const HiprInstanceMaterial* assignments, uint32_t assignment_count) {
    if (int st = check_context(c)) return st;
    const ResidentScene& r = c->scene;
    if (!r.ready) return fail(HIPR_ERROR_NOT_READY, "hipr_update_scene_materials: no scene uploaded");
    if ((material_count && !materials) || (assignment_count && !assignments)) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_materials: null array with a non-zero count");
    for (uint32_t k = 0; k < material_count; ++k) {
        if (materials[k].material_index >= r.uploaded_materials.size())
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_materials: material %u of %zu (the material pool does not grow; upload the scene instead)", materials[k].material_index, r.uploaded_materials.size());
        char invalid[256];
        if (invalid_material(materials[k].material, materials[k].material_index, uint32_t(r.uploaded_textures.size()), invalid, sizeof(invalid)))
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_materials: %s", invalid);
    }
    for (uint32_t k = 0; k < assignment_count; ++k) {
        if (assignments[k].instance_index >= r.uploaded_instances.size())
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_materials: instance %u of %zu", assignments[k].instance_index, r.uploaded_instances.size());
        if (assignments[k].material_index < 0 || size_t(assignments[k].material_index) >= r.uploaded_materials.size())
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_update_scene_materials: instance %u is given material %d of %zu", assignments[k].instance_index, assignments[k].material_index, r.uploaded_materials.size());
    }
    // The exhaustive search's items pair triangles of equal flags (build_trace_items): there a material edit changes a topology, which only the host builds.
    if (r.args.trace_item_count != 0)
        return fail(HIPR_ERROR_UNSUPPORTED, "hipr_update_scene_materials: the uploaded scene carries the exhaustive search's items, which pair triangles by their flags; upload the scene instead");
    return HIPR_OK;
}

int hipr_update_scene_materials(HiprContext* c, const HiprMaterialUpdate* materials, uint32_t material_count, const HiprInstanceMaterial* assignments, uint32_t assignment_count) {
    if (int st = hipr_internal_check_material_update(c, materials, material_count, assignments, assignment_count)) return st;
    if (int finish_status = finish_all(c)) return finish_status;      // no pending pass may go on over the new materials
    return c->scene.update_materials(materials, material_count, assignments, assignment_count, c->stream);
}

// What the device work of a BVH2 build leaves beside the context's BuildScratch (out_nodes, order, place, status): the nodes, and the nodes created per level.
struct Bvh2Built { uint32_t node_count = 1; std::vector<uint32_t> level_nodes; };
// The device-to-device core hipr_build_bvh2 and hipr_rebuild_scene_trees share: scratch, kernels and the words read per level, on the context's stream, ending
// synchronised. `host_triangles` are uploaded into the scratch first (`uploaded` is the time after that); otherwise the build runs over `device_triangles` where they
// lie. `who` names the entry point in the messages. The caller holds the BuildScratchGuard and has checked count and corners.
static int build_bvh2_on_the_device(HiprContext* c, const char* who, const HiprTriangle* host_triangles, const HiprTriangle* device_triangles, uint32_t count, uint32_t depth_limit, Bvh2Built& built,
                                    std::chrono::steady_clock::time_point& uploaded) {
    const uint32_t max_levels = std::min(depth_limit, count) + 2u;      // a range's depth grows by one per level and never passes the limit
    const size_t n = count, max_open = n / 4 + 2, max_long = n / BUILD_SHORT_RANGE + 2, blocks = (n + BUILD_BLOCK - 1) / BUILD_BLOCK;
    const size_t status_words = STATUS_LEVELS + 2 * size_t(max_levels + 2);
    BuildScratch& b = c->build;
    hipStream_t stream = c->stream;
    if (b.boxes.resize(n * sizeof(BuildBox)) | b.centroids.resize(n * 12) | b.order.resize(n * 4) | b.seg.resize(n * 4) | b.order_tmp.resize(n * 4) | b.seg_tmp.resize(n * 4) |
        b.ranges[0].resize(max_open * sizeof(BuildRange)) | b.ranges[1].resize(max_open * sizeof(BuildRange)) | b.acc.resize(max_long * ACC_WORDS * 4) | b.setup.resize(max_long * sizeof(BuildSetup)) |
        b.split.resize(max_long * sizeof(BuildSplit)) | b.scan_local.resize(n * 4) | b.block_sums.resize(blocks * 4) | b.nodes.resize(n * sizeof(HiprBvhNode)) | b.sizes.resize(n * 4) |
        b.place.resize(n * 4) | b.out_nodes.resize(n * sizeof(HiprBvhNode)) | b.status.resize(status_words * 4))
        return HIPR_ERROR_OUT_OF_MEMORY;
    if (host_triangles) {
        if (int st = b.triangles.upload(host_triangles, n * sizeof(HiprTriangle), stream)) return st;
        HIP_TRY(hipStreamSynchronize(stream));
    }
    uploaded = std::chrono::steady_clock::now();

    BuildState S = {};
    S.triangles = host_triangles ? b.triangles.as<HiprTriangle>() : device_triangles; S.count = count; S.depth_limit = depth_limit;
    S.boxes = b.boxes.as<BuildBox>(); S.centroids = b.centroids.as<float>();
    S.order = b.order.as<uint32_t>(); S.seg = b.seg.as<uint32_t>(); S.order_tmp = b.order_tmp.as<uint32_t>(); S.seg_tmp = b.seg_tmp.as<uint32_t>();
    S.acc = b.acc.as<uint32_t>(); S.setup = b.setup.as<BuildSetup>(); S.split = b.split.as<BuildSplit>();
    S.scan_local = b.scan_local.as<uint32_t>(); S.block_sums = b.block_sums.as<uint32_t>();
    S.nodes = b.nodes.as<HiprBvhNode>(); S.sizes = b.sizes.as<uint32_t>(); S.place = b.place.as<uint32_t>(); S.out_nodes = b.out_nodes.as<HiprBvhNode>();
    S.status = b.status.as<uint32_t>();

    std::vector<uint32_t> status(status_words, 0u);
    status[STATUS_DECLINE] = status[STATUS_DECLINE + 1] = 0xFFFFFFFFu;
    status[STATUS_LEVELS] = 1u;
    status[STATUS_LEVELS + 1] = count > BUILD_SHORT_RANGE ? 1u : 0u;
    HIP_TRY(hipMemcpyAsync(S.status, status.data(), status_words * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(S.nodes, 0, n * sizeof(HiprBvhNode), stream));
    HIP_TRY(hipMemsetAsync(S.place, 0, 4, stream));
    const dim3 block(BUILD_BLOCK), per_position{uint32_t(blocks)};
    hipLaunchKernelGGL(k_build_prepare, per_position, block, 0, stream, S);
    std::vector<uint32_t>& level_nodes = built.level_nodes;      // the open ranges = new nodes of every level
    level_nodes.clear();
    uint32_t node_count = 1;
    if (count <= BUILD_LEAF_MAX) hipLaunchKernelGGL(k_build_single_leaf, dim3(1), block, 0, stream, S);
    else {
        const BuildRange root = {0u, count, 1u, BUILD_NONE, count > BUILD_SHORT_RANGE ? 0u : BUILD_NONE, 0u};
        HIP_TRY(hipMemcpyAsync(b.ranges[0].ptr, &root, sizeof(root), hipMemcpyHostToDevice, stream));
        uint32_t open = 1, long_ranges = root.long_index == BUILD_NONE ? 0u : 1u, node_base = 0;
        for (uint32_t level = 0; open; ++level) {
            if (level >= max_levels || node_base + open > count - 1u || open > max_open - 2 || long_ranges > max_long - 2)
                return fail(HIPR_ERROR_HIP, "%s: the build left its bounds at level %u (%u open ranges, %u nodes)", who, level, open, node_base);
            const BuildLevel L = {b.ranges[level & 1u].as<BuildRange>(), b.ranges[(level + 1u) & 1u].as<BuildRange>(), open, node_base, level};
            const dim3 per_range((open + BUILD_BLOCK - 1) / BUILD_BLOCK);
            if (long_ranges) {
                const uint64_t words = uint64_t(long_ranges) * ACC_WORDS;
                hipLaunchKernelGGL(k_build_acc_init, dim3(uint32_t((words + BUILD_BLOCK - 1) / BUILD_BLOCK)), block, 0, stream, S.acc, words);
                hipLaunchKernelGGL(k_build_bounds, per_position, block, 0, stream, S, L);
                hipLaunchKernelGGL(k_build_range_setup, per_range, block, 0, stream, S, L);
                hipLaunchKernelGGL(k_build_bins, per_position, block, 0, stream, S, L);
                hipLaunchKernelGGL(k_build_split, per_range, block, 0, stream, S, L, 1);
                hipLaunchKernelGGL(k_build_scan_local, per_position, block, 0, stream, S, L);
                hipLaunchKernelGGL(k_build_scan_sums, dim3(1), block, 0, stream, S.block_sums, uint32_t(blocks));
                hipLaunchKernelGGL(k_build_scatter, per_position, block, 0, stream, S, L);
                hipLaunchKernelGGL(k_build_copy_back, per_position, block, 0, stream, S, L);
                hipLaunchKernelGGL(k_build_leaves, per_range, block, 0, stream, S, L);
            }
            hipLaunchKernelGGL(k_build_split, per_range, block, 0, stream, S, L, 0);
            HIP_TRY(hipMemcpyAsync(status.data(), S.status, (STATUS_LEVELS + 2 * size_t(level + 2)) * 4, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (status[STATUS_DECLINE] != 0xFFFFFFFFu) {
                b.levels = level + 1;
                return fail(HIPR_ERROR_UNSUPPORTED, "%s: the range [%u, %u) of %u triangles at level %u takes the median path (the depth budget, or coincident centroids) and is longer than the %u a lane sorts; build on the host",
                            who, status[STATUS_DECLINE + 1], status[STATUS_DECLINE], status[STATUS_DECLINE] - status[STATUS_DECLINE + 1], level, BUILD_MEDIAN_LANE_LIMIT);
            }
            level_nodes.push_back(open);
            node_base += open;
            open = status[STATUS_LEVELS + 2 * (level + 1)];
            long_ranges = status[STATUS_LEVELS + 2 * (level + 1) + 1];
        }
        node_count = node_base;
        std::vector<uint32_t> first(level_nodes.size());
        for (size_t l = 0, at = 0; l < level_nodes.size(); at += level_nodes[l++]) first[l] = uint32_t(at);
        for (size_t l = level_nodes.size(); l-- > 0;) hipLaunchKernelGGL(k_build_count, dim3((level_nodes[l] + BUILD_BLOCK - 1) / BUILD_BLOCK), block, 0, stream, S, first[l], level_nodes[l]);
        for (size_t l = 0; l < level_nodes.size(); ++l) hipLaunchKernelGGL(k_build_place, dim3((level_nodes[l] + BUILD_BLOCK - 1) / BUILD_BLOCK), block, 0, stream, S, first[l], level_nodes[l]);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    built.node_count = node_count;
    b.levels = uint32_t(level_nodes.size());
    return HIPR_OK;
}

// The BVH2 of host/BvhBuilder.cpp built by the kernels of bvh2_build.h. Nothing of the resident scene is read or written; the outputs are written only once the
// whole build has succeeded.
int hipr_build_bvh2(HiprContext* c, const HiprTriangle* triangles, uint32_t count, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t node_capacity, uint32_t* out_node_count,
                    uint32_t* out_order, uint32_t* out_deepest) {
    if (int st = check_context(c)) return st;
    const auto t_validate = std::chrono::steady_clock::now();
    if (!triangles || !count || !out_nodes || !out_node_count || !out_order || !out_deepest) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_build_bvh2: null argument or no triangles");
    if (count > BUILD_MAX_TRIANGLES) return fail(HIPR_ERROR_UNSUPPORTED, "hipr_build_bvh2: %u triangles, a leaf reference holds %u", count, BUILD_MAX_TRIANGLES);
    if (node_capacity < std::max(std::max(count, 1u) - 1u, 1u)) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_build_bvh2: room for %u nodes, %u triangles can need %u", node_capacity, count, std::max(count - 1u, 1u));
    for (uint32_t i = 0; i < count; ++i)
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(triangles[i].v0[k]) || !std::isfinite(triangles[i].v1[k]) || !std::isfinite(triangles[i].v2[k]))
                return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_build_bvh2: triangle %u has a corner that is not finite", i);
    const uint32_t depth_limit = std::max(max_depth, 8u);
    const size_t n = count;
    BuildScratch& b = c->build;
    const BuildScratchGuard guard{b};
    hipStream_t stream = c->stream;
    c->break_chain(stream);
    const auto t0 = std::chrono::steady_clock::now();
    Bvh2Built built;
    std::chrono::steady_clock::time_point t1;
    if (int st = build_bvh2_on_the_device(c, "hipr_build_bvh2", triangles, nullptr, count, depth_limit, built, t1)) return st;
    const uint32_t node_count = built.node_count;
    uint32_t status[STATUS_LEVELS] = {};
    const auto t2 = std::chrono::steady_clock::now();
    if (node_count > node_capacity) return fail(HIPR_ERROR_HIP, "hipr_build_bvh2: %u nodes built, room for %u", node_count, node_capacity);
    HIP_TRY(hipMemcpyAsync(status, b.status.ptr, STATUS_LEVELS * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out_nodes, b.out_nodes.ptr, size_t(node_count) * sizeof(HiprBvhNode), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(out_order, b.order.ptr, n * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *out_node_count = node_count;
    *out_deepest = status[STATUS_DEEPEST];
    const auto t3 = std::chrono::steady_clock::now();
    b.validate_ms = std::chrono::duration<double, std::milli>(t0 - t_validate).count();
    b.upload_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    b.kernel_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    b.readback_ms = std::chrono::duration<double, std::milli>(t3 - t2).count();
    if (std::getenv("HIPR_BVH_TIMING"))
        fprintf(stderr, "[hipr] hipr_build_bvh2: %u triangles, %u nodes, %u levels: argument checks %.3f ms, allocation + upload %.3f ms, kernels %.3f ms, read-back %.3f ms (transfers %.0f %% of %.3f ms)\n", count, node_count, b.levels,
                b.validate_ms, b.upload_ms, b.kernel_ms, b.readback_ms, 100.0 * (b.upload_ms + b.readback_ms) / (b.validate_ms + b.upload_ms + b.kernel_ms + b.readback_ms),
                b.validate_ms + b.upload_ms + b.kernel_ms + b.readback_ms);
    return HIPR_OK;
}

int hipr_debug_build_times(HiprContext* c, double* out4_ms) {
    if (!c || !out4_ms) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_build_times: null argument");
    out4_ms[0] = c->build.validate_ms; out4_ms[1] = c->build.upload_ms; out4_ms[2] = c->build.kernel_ms; out4_ms[3] = c->build.readback_ms;
    return HIPR_OK;
}

// The device-to-device core hipr_build_wide8 and hipr_rebuild_scene_trees share: the passes of wide8_build.h over a BVH2, its triangles, their order and the level lists
// the device already holds (W8State's input members, the scratch of collapse_scratch_for cleared), on the context's stream, ending synchronised with the slots in
// CollapseScratch::slots. `level_first`: level l is level_nodes[level_first[l] .. level_first[l + 1]). `who` names the entry point in the messages. The caller holds
// the CollapseScratchGuard.
static int collapse_on_the_device(HiprContext* c, const char* who, W8State& S, const std::vector<uint32_t>& level_first, uint32_t slot_capacity, HiprWide8BuildResult& result) {
    CollapseScratch& b = c->collapse;
    hipStream_t stream = c->stream;
    const uint32_t triangle_count = S.triangle_count, node_count = S.node_count, reachable = S.reachable, bvh_levels = uint32_t(level_first.size()) - 1u;
    const size_t T = triangle_count, N = node_count, scan_blocks = (T + W8_BLOCK - 1) / W8_BLOCK;
    const dim3 block(W8_BLOCK), per_triangle{uint32_t(scan_blocks)}, per_reference((2u * reachable + W8_BLOCK - 1) / W8_BLOCK);
    auto blocks_for = [](uint32_t threads) { return dim3((threads + W8_BLOCK - 1) / W8_BLOCK); };
    // 1, 2: the bounds and the record numbers; the host reads both together
    hipLaunchKernelGGL(k_w8_bounds, per_triangle, block, 0, stream, S.triangles, triangle_count, b.partial.as<RefitBound>(), S.status);
    hipLaunchKernelGGL(k_refit_bounds_final, dim3(1), block, 0, stream, b.partial.as<RefitBound>(), uint32_t(scan_blocks), b.bounds.as<RefitBound>());
    hipLaunchKernelGGL(k_w8_count_leaf, per_reference, block, 0, stream, S);
    hipLaunchKernelGGL(k_w8_scan_local, per_triangle, block, 0, stream, S);
    hipLaunchKernelGGL(k_build_scan_sums, dim3(1), block, 0, stream, S.block_sums, uint32_t(scan_blocks + 1));
    RefitBound bounds[6];
    uint32_t record_total = 0, not_finite = 0;
    HIP_TRY(hipMemcpyAsync(bounds, b.bounds.ptr, sizeof(bounds), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&record_total, S.block_sums + scan_blocks, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&not_finite, S.status + W8_STATUS_NOT_FINITE, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (not_finite) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: a triangle corner or a child box is not finite", who);
    if (record_total == 0 || record_total > triangle_count) return fail(HIPR_ERROR_HIP, "%s: %u records of %u triangles", who, record_total, triangle_count);
    result = {};
    {
        const float lo[3] = {bounds[0].v, bounds[1].v, bounds[2].v}, hi[3] = {bounds[3].v, bounds[4].v, bounds[5].v};
        refit_grid(lo, hi, result.grid_min, result.grid_cell);
        for (int a = 0; a < 3; ++a) { S.grid_min[a] = result.grid_min[a]; S.grid_cell[a] = result.grid_cell[a]; }
    }
    // 3, 4: the tree over the records and its dynamic program
    const size_t R = record_total, inner = N + R, wide_capacity = R;
    if (b.box.resize((inner + R) * sizeof(RefitBox)) | b.left.resize(inner * 4) | b.right.resize(inner * 4) | b.cost.resize(inner * 28) | b.split.resize(inner * 7) | b.roots_used.resize(inner * 7) |
        b.records.resize(R * sizeof(HiprLeaf8)) | b.record_slot.resize(R * 4) | b.wide_tree.resize(wide_capacity * 4) | b.wide_child.resize(wide_capacity * 32) | b.wide_all.resize(wide_capacity * sizeof(RefitBox)) |
        b.wide_size.resize(wide_capacity * 4) | b.wide_base.resize(wide_capacity * 4) | b.wide_slot.resize(wide_capacity * 4))
        return HIPR_ERROR_OUT_OF_MEMORY;
    S.record_total = record_total; S.leaf_base = uint32_t(inner); S.wide_capacity = uint32_t(wide_capacity);
    S.box = b.box.as<RefitBox>(); S.left = b.left.as<int32_t>(); S.right = b.right.as<int32_t>(); S.cost = b.cost.as<float>(); S.split = b.split.as<uint8_t>(); S.roots_used = b.roots_used.as<uint8_t>();
    S.records = b.records.as<HiprLeaf8>(); S.record_slot = b.record_slot.as<uint32_t>();
    S.wide_tree = b.wide_tree.as<uint32_t>(); S.wide_child = b.wide_child.as<int32_t>(); S.wide_all = b.wide_all.as<RefitBox>();
    S.wide_size = b.wide_size.as<uint32_t>(); S.wide_base = b.wide_base.as<uint32_t>(); S.wide_slot = b.wide_slot.as<uint32_t>();
    hipLaunchKernelGGL(k_w8_leaf, per_reference, block, 0, stream, S);
    if (!S.single_leaf)
        for (uint32_t l = bvh_levels; l-- > 0;) {
            const uint32_t first = level_first[l], count = level_first[l + 1] - first;
            hipLaunchKernelGGL(k_w8_optimise, blocks_for(count), block, 0, stream, S, first, count);
        }
    // 5: the wide nodes, level by level
    std::vector<uint32_t> wide_first, wide_count;
    uint32_t status[W8_STATUS_WORDS] = {};
    for (uint32_t level = 0, first = 0, count = 1; count; ++level) {
        if (level >= W8_MAX_WIDE_LEVELS || size_t(first) + count > wide_capacity) return fail(HIPR_ERROR_HIP, "%s: the collapse left its bounds at wide level %u (%u nodes from %u, room for %zu)", who, level, count, first, wide_capacity);
        hipLaunchKernelGGL(k_w8_prepare, blocks_for(count), block, 0, stream, S, first, count, level);
        HIP_TRY(hipMemcpyAsync(status, S.status, (W8_STATUS_LEVELS + level + 2) * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (status[W8_STATUS_OVERFLOW]) return fail(HIPR_ERROR_HIP, "%s: more wide nodes than a tree over %u records holds", who, record_total);
        wide_first.push_back(first); wide_count.push_back(count);
        first += count;
        count = status[W8_STATUS_LEVELS + level + 1];
    }
    const uint32_t wide_total = wide_first.back() + wide_count.back(), wide_levels = uint32_t(wide_first.size());
    // 6: the sizes; the slots needed are known before one is written
    for (uint32_t l = wide_levels; l-- > 0;) hipLaunchKernelGGL(k_w8_size, blocks_for(wide_count[l]), block, 0, stream, S, wide_first[l], wide_count[l]);
    uint32_t size_below_root = 0;
    HIP_TRY(hipMemcpyAsync(&size_below_root, S.wide_size, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint64_t slot_count = 1ull + size_below_root;
    if (slot_count != uint64_t(wide_total) + record_total) return fail(HIPR_ERROR_HIP, "%s: %llu slots below the root, %u nodes and %u records", who, (unsigned long long)slot_count, wide_total, record_total);
    if (slot_count > W8_MAX_SLOTS) return fail(HIPR_ERROR_UNSUPPORTED, "%s: the tree needs %llu slots, a node addresses %u", who, (unsigned long long)slot_count, W8_MAX_SLOTS);
    if (slot_count > slot_capacity) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the tree needs %llu slots, room for %u", who, (unsigned long long)slot_count, slot_capacity);
    if (b.slots.resize(size_t(slot_count) * sizeof(HiprSlot8))) return HIPR_ERROR_OUT_OF_MEMORY;
    S.slots = b.slots.as<HiprSlot8>();
    // 7, 8: the places, then the slots
    const uint32_t root_place[2] = {0u, 1u};
    HIP_TRY(hipMemcpyAsync(S.wide_slot, &root_place[0], 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(S.wide_base, &root_place[1], 4, hipMemcpyHostToDevice, stream));
    for (uint32_t l = 0; l < wide_levels; ++l) hipLaunchKernelGGL(k_w8_place, blocks_for(wide_count[l]), block, 0, stream, S, wide_first[l], wide_count[l]);
    hipLaunchKernelGGL(k_w8_emit_nodes, blocks_for(wide_total), block, 0, stream, S, wide_total);
    hipLaunchKernelGGL(k_w8_emit_leaves, blocks_for(record_total), block, 0, stream, S);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    result.slot_count = uint32_t(slot_count);
    result.height = wide_levels;
    result.node_count = wide_total; result.leaf_count = record_total; result.paired_leaves = status[W8_STATUS_PAIRED];
    return HIPR_OK;
}
// The scratch every collapse starts from, sized and cleared (queued on `stream`).
static int collapse_scratch_for(CollapseScratch& b, size_t T, hipStream_t stream) {
    const size_t scan_blocks = (T + W8_BLOCK - 1) / W8_BLOCK;
    if (b.counts.resize(T * 4) | b.block_sums.resize((scan_blocks + 1) * 4) | b.partial.resize(scan_blocks * 6 * sizeof(RefitBound)) | b.bounds.resize(6 * sizeof(RefitBound)) | b.status.resize(W8_STATUS_WORDS * 4))
        return HIPR_ERROR_OUT_OF_MEMORY;
    HIP_TRY(hipMemsetAsync(b.counts.ptr, 0, T * 4, stream));
    HIP_TRY(hipMemsetAsync(b.block_sums.ptr, 0, (scan_blocks + 1) * 4, stream));
    HIP_TRY(hipMemsetAsync(b.status.ptr, 0, W8_STATUS_WORDS * 4, stream));
    return HIPR_OK;
}

// The 8-wide tree of host/Wide8Builder.cpp collapsed from a BVH2 by the kernels of wide8_build.h. Nothing of the resident scene is read or written; the outputs are
// written only once the whole collapse has succeeded.
int hipr_build_wide8(HiprContext* c, const HiprBvhNode* nodes, uint32_t node_count, const HiprTriangle* triangles, const uint32_t* order, uint32_t triangle_count, HiprSlot8* out_slots,
                     uint32_t slot_capacity, HiprWide8BuildResult* out) {
    if (int st = check_context(c)) return st;
    const auto t_validate = std::chrono::steady_clock::now();
    if (!nodes || !node_count || !triangles || !triangle_count || !out_slots || !out) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_build_wide8: null argument, no nodes or no triangles");
    if (triangle_count > BUILD_MAX_TRIANGLES || node_count > BUILD_MAX_TRIANGLES) return fail(HIPR_ERROR_UNSUPPORTED, "hipr_build_wide8: %u triangles and %u nodes, a leaf reference holds %u", triangle_count, node_count, BUILD_MAX_TRIANGLES);
    W8Input input;
    char reason[256] = "";
    if (const int refused = w8_check_input(nodes, node_count, order, triangle_count, input, reason, sizeof(reason)))
        return fail(refused == W8_INPUT_DECLINED ? HIPR_ERROR_UNSUPPORTED : HIPR_ERROR_INVALID_ARGUMENT, "hipr_build_wide8: %s", reason);
    const uint32_t reachable = uint32_t(input.level_nodes.size()), bvh_levels = uint32_t(input.level_first.size()) - 1u;
    CollapseScratch& b = c->collapse;
    const CollapseScratchGuard guard{b};
    hipStream_t stream = c->stream;
    c->break_chain(stream);
    const auto t0 = std::chrono::steady_clock::now();
    const size_t T = triangle_count, N = node_count, scan_blocks = (T + W8_BLOCK - 1) / W8_BLOCK;
    if (b.counts.resize(T * 4) | b.block_sums.resize((scan_blocks + 1) * 4) | b.partial.resize(scan_blocks * 6 * sizeof(RefitBound)) | b.bounds.resize(6 * sizeof(RefitBound)) | b.status.resize(W8_STATUS_WORDS * 4))
        return HIPR_ERROR_OUT_OF_MEMORY;
    if (int st = b.nodes.upload(nodes, N * sizeof(HiprBvhNode), stream)) return st;
    if (int st = b.triangles.upload(triangles, T * sizeof(HiprTriangle), stream)) return st;
    if (order) if (int st = b.order.upload(order, T * 4, stream)) return st;
    if (int st = b.level_nodes.upload(input.level_nodes.data(), size_t(reachable) * 4, stream)) return st;
    HIP_TRY(hipMemsetAsync(b.counts.ptr, 0, T * 4, stream));
    HIP_TRY(hipMemsetAsync(b.block_sums.ptr, 0, (scan_blocks + 1) * 4, stream));
    HIP_TRY(hipMemsetAsync(b.status.ptr, 0, W8_STATUS_WORDS * 4, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const auto t1 = std::chrono::steady_clock::now();

    W8State S = {};
    S.nodes = b.nodes.as<HiprBvhNode>(); S.node_count = node_count;
    S.triangles = b.triangles.as<HiprTriangle>(); S.order = order ? b.order.as<uint32_t>() : nullptr; S.triangle_count = triangle_count;
    S.level_nodes = b.level_nodes.as<uint32_t>(); S.reachable = reachable; S.single_leaf = input.single_leaf ? 1u : 0u;
    S.counts = b.counts.as<uint32_t>(); S.block_sums = b.block_sums.as<uint32_t>(); S.status = b.status.as<uint32_t>();
    HiprWide8BuildResult result = {};
    if (int st = collapse_on_the_device(c, "hipr_build_wide8", S, input.level_first, slot_capacity, result)) return st;
    const uint32_t record_total = result.leaf_count,wide_total = result.node_count, wide_levels = result.height;
    const uint64_t slot_count = result.slot_count;
    const auto t2 = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpyAsync(out_slots, S.slots, size_t(slot_count) * sizeof(HiprSlot8), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *out = result;
    const auto t3 = std::chrono::steady_clock::now();
    b.validate_ms = std::chrono::duration<double, std::milli>(t0 - t_validate).count();
    b.upload_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    b.kernel_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    b.readback_ms = std::chrono::duration<double, std::milli>(t3 - t2).count();
    if (std::getenv("HIPR_BVH_TIMING"))
        fprintf(stderr, "[hipr] hipr_build_wide8: %u triangles, %u BVH2 nodes on %u levels, %u records, %u wide nodes on %u levels, %u slots: index walk %.3f ms, allocation + upload %.3f ms, kernels %.3f ms, read-back %.3f ms\n",
                triangle_count, node_count, bvh_levels, record_total, wide_total, wide_levels, result.slot_count, b.validate_ms, b.upload_ms, b.kernel_ms, b.readback_ms);
    return HIPR_OK;
}

int hipr_debug_collapse_times(HiprContext* c, double* out4_ms) {
    if (!c || !out4_ms) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_collapse_times: null argument");
    out4_ms[0] = c->collapse.validate_ms; out4_ms[1] = c->collapse.upload_ms; out4_ms[2] = c->collapse.kernel_ms; out4_ms[3] = c->collapse.readback_ms;
    return HIPR_OK;
}

// The trees of the resident scene rebuilt on the device, in place, from the triangles it holds (scene_rebuild.h): flatten order, the BVH2 build, the hand-over, the
// collapse -- all in scratch, where every refusal still leaves the scene as the call found it -- and then ResidentScene::install_rebuilt_trees.
//
// hipr_edit_scene_instances is the same call with another instance list going in and another triangle count coming out: `edit`, which its entry point has checked
// (check_instance_edit), names the new list. The count per OLD instance is taken as without it; the flat array is then the NEW list's -- kept triangles through
// the old-to-new table, new ones made in place (instance_edit.h) -- and everything from the BVH2 build on runs over the new count.
struct InstanceEdit {
    std::vector<HiprInstance> instances;      // the new list: kept entries as the device holds them, new ones as given
    std::vector<uint32_t> source;             // per entry of the new list: the resident instance kept, BUILD_NONE for a new one
    std::vector<uint32_t> primitive_count;    // per entry of the new list: a new instance's count (kept ones: filled from the count pass)
    std::vector<uint32_t> old_to_new;         // per resident instance: its new index, BUILD_NONE when removed
    uint32_t order_capacity = 0;
    uint32_t triangle_count = 0;              // out: of the new set
};
static int rebuild_trees_on_the_device(HiprContext* c, const char* who, InstanceEdit* edit, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t node_capacity, uint32_t* out_order,
                                       HiprSlot8* out_slots, uint32_t slot_capacity, HiprSceneRebuildResult* out) {
    if (int st = check_context(c)) return st;
    ResidentScene& r = c->scene;
    if (!r.ready && !r.awaits_rebuild) return fail(HIPR_ERROR_NOT_READY, "%s: no scene uploaded, or one a failed call left behind", who);
    const uint32_t count = r.args.triangle_count, instance_count = uint32_t(r.uploaded_instances.size());
    // the conditions hipr_refit_scene_transforms refuses on: the arrays another search walks are the ones this call leaves stale, and the exhaustive search's items are the host's
    if (r.wide8.slot_count == 0 || !c->use_wide8() || r.args.trace_item_count != 0 || count > 0x55555555u || count == 0)
        return fail(HIPR_ERROR_UNSUPPORTED, "%s: the resident scene is not traced through the 8-wide tree; rebuild on the host and call hipr_upload_scene", who);
    if (count > BUILD_MAX_TRIANGLES) return fail(HIPR_ERROR_UNSUPPORTED, "%s: %u triangles, a leaf reference holds %u", who, count, BUILD_MAX_TRIANGLES);
    if (!out) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null result", who);
    // the room the outputs need for `triangles` triangles; an edit knows its count once the kept instances are counted, and is checked there
    auto outputs_fit = [&](uint32_t triangles) {
        const uint32_t nodes_needed = std::max(std::max(triangles, 1u) - 1u, 1u), slots_needed = uint32_t(std::min<uint64_t>(2ull * triangles, W8_MAX_SLOTS));
        if (out_nodes && node_capacity < nodes_needed) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: room for %u nodes, %u triangles can need %u", who, node_capacity, triangles, nodes_needed);
        if (out_slots && slot_capacity < slots_needed) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: room for %u slots, %u triangles can need %u", who, slot_capacity, triangles, slots_needed);
        if (edit && out_order && edit->order_capacity < triangles) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: room for %u order words, the new list has %u triangles", who, edit->order_capacity, triangles);
        return int(HIPR_OK);
    };
    if (!edit)
        if (int st = outputs_fit(count)) return st;
    if (int finish_status = finish_all(c)) return finish_status;      // no pending pass may go on over the new trees
    const uint32_t depth_limit = std::max(max_depth, 8u);
    BuildScratch& b = c->build;
    CollapseScratch& w = c->collapse;
    RebuildScratch& x = c->rebuild;
    const BuildScratchGuard build_guard{b};
    const CollapseScratchGuard collapse_guard{w};
    const RebuildScratchGuard rebuild_guard{x};
    hipStream_t stream = c->stream;
    c->break_chain(stream);
    const auto t0 = std::chrono::steady_clock::now();

    // the flatten order: the triangles per resident instance ...
    if (x.instance_counts.resize(size_t(instance_count) * 4) | x.status.resize(REBUILD_STATUS_WORDS * 4)) return HIPR_ERROR_OUT_OF_MEMORY;
    HIP_TRY(hipMemsetAsync(x.instance_counts.ptr, 0, size_t(instance_count) * 4, stream));
    HIP_TRY(hipMemsetAsync(x.status.ptr, 0, REBUILD_STATUS_WORDS * 4, stream));
    RebuildArrays a = {r.triangles.as<HiprTriangle>(), r.triangle_class.as<uint8_t>(), count, instance_count, x.instance_counts.as<uint32_t>(), nullptr, nullptr, nullptr, nullptr, x.status.as<uint32_t>()};
    const dim3 block(REBUILD_BLOCK), per_triangle((count + REBUILD_BLOCK - 1) / REBUILD_BLOCK);
    hipLaunchKernelGGL(k_rebuild_count, per_triangle, block, 0, stream, a);      // reads the resident triangles, writes the counts and the flag
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> counted(size_t(instance_count) + 1, 0u);
    HIP_TRY(hipMemcpyAsync(counted.data(), x.instance_counts.ptr, size_t(instance_count) * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    uint64_t total = 0;
    for (uint32_t i = 0; i < instance_count; ++i) total += counted[i];
    if (total != count) return fail(HIPR_ERROR_UNSUPPORTED, "%s: %llu of %u resident triangles belong to one of the %u instances", who, (unsigned long long)total, count, instance_count);
    // ... and first[] of the list the flat array is made for: the resident instances, or the edit's
    const uint32_t list_count = edit ? uint32_t(edit->instances.size()) : instance_count;
    std::vector<uint32_t> first(size_t(list_count) + 1, 0u), created, created_first(1, 0u);
    total = 0;
    for (uint32_t i = 0; i < list_count; ++i) {
        if (edit && edit->source[i] != BUILD_NONE) edit->primitive_count[i] = counted[edit->source[i]];
        if (edit && edit->source[i] == BUILD_NONE) { created.push_back(i); created_first.push_back(created_first.back() + edit->primitive_count[i]); }      // below 2^32: each count is inside the index pool, checked against the total next
        total += edit ? edit->primitive_count[i] : counted[i];
        if (total > BUILD_MAX_TRIANGLES) return fail(HIPR_ERROR_UNSUPPORTED, "%s: the new list has more than %u triangles, what a leaf reference holds", who, BUILD_MAX_TRIANGLES);
        first[i + 1] = uint32_t(total);
    }
    const size_t n = size_t(total);
    const uint32_t new_count = uint32_t(total);
    if (edit) {
        if (new_count == 0) return fail(HIPR_ERROR_UNSUPPORTED, "%s: the new list yields no triangle", who);
        if (int st = outputs_fit(new_count)) return st;
    }
    if (b.triangles.resize(n * sizeof(HiprTriangle)) | x.flat_class.resize(n) | x.claim.resize(n * 4) | x.first.resize((size_t(list_count) + 1) * 4)) return HIPR_ERROR_OUT_OF_MEMORY;
    HIP_TRY(hipMemsetAsync(x.claim.ptr, 0, n * 4, stream));
    HIP_TRY(hipMemcpyAsync(x.first.ptr, first.data(), first.size() * 4, hipMemcpyHostToDevice, stream));
    a.first = x.first.as<uint32_t>(); a.flat = b.triangles.as<HiprTriangle>(); a.flat_class = x.flat_class.as<uint8_t>(); a.claim = x.claim.as<uint32_t>();
    if (!edit) hipLaunchKernelGGL(k_rebuild_scatter, per_triangle, block, 0, stream, a);
    else {
        const uint32_t created_count = uint32_t(created.size()), created_triangles = created_first.back();
        if (x.old_to_new.upload(edit->old_to_new.data(), edit->old_to_new.size() * 4, stream) | x.created.upload(created.data(), created.size() * 4, stream) |
            x.created_first.upload(created_first.data(), created_first.size() * 4, stream) | x.instances.upload(edit->instances.data(), edit->instances.size() * sizeof(HiprInstance), stream))
            return HIPR_ERROR_OUT_OF_MEMORY;
        const EditArrays e = {a.resident, a.resident_class, count, instance_count, x.old_to_new.as<uint32_t>(), a.first, list_count, new_count, x.created.as<uint32_t>(), x.created_first.as<uint32_t>(),
                              created_count, created_triangles, x.instances.as<HiprInstance>(), r.materials.as<HiprMaterial>(), r.indices.as<uint32_t>(), r.geometry.as<HiprVertexGeometry>(),
                              r.uploaded_vertex_count, r.uploaded_mesh_attributes & HIPR_MESH_TEXCOORDS ? reinterpret_cast<const float*>(r.args.texcoords) : nullptr, r.textures.as<HiprTexture>(), uint32_t(r.uploaded_textures.size()), r.texels.as<uint8_t>(),
                              a.flat, a.flat_class, a.claim, a.status};
        hipLaunchKernelGGL(k_edit_scatter, per_triangle, block, 0, stream, e);
        if (created_triangles) hipLaunchKernelGGL(k_edit_new_triangles, dim3((created_triangles + REBUILD_BLOCK - 1) / REBUILD_BLOCK), block, 0, stream, e);
        hipLaunchKernelGGL(k_edit_reduce, dim3((new_count + REBUILD_BLOCK - 1) / REBUILD_BLOCK), block, 0, stream, e.flat, e.flat_class, e.claim, e.status, new_count);
    }
    HIP_TRY(hipGetLastError());
    uint32_t flatten_status[REBUILD_STATUS_WORDS] = {};
    HIP_TRY(hipMemcpyAsync(flatten_status, x.status.ptr, sizeof(flatten_status), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));      // the host's lists are read by now as well
    if (edit && flatten_status[EDIT_STATUS_INDEX]) return fail(HIPR_ERROR_UNSUPPORTED, "%s: an index triple of a new instance points outside the vertex pool", who);
    if (edit && flatten_status[REBUILD_STATUS_CLAIM]) return fail(HIPR_ERROR_UNSUPPORTED, "%s: a flatten position (instance, primitive) is claimed twice or not at all; rebuild on the host", who);
    if (flatten_status[REBUILD_STATUS_CLAIM]) return fail(HIPR_ERROR_UNSUPPORTED, "%s: two resident triangles claim one flatten position (instance, primitive); rebuild on the host", who);
    const auto t1 = std::chrono::steady_clock::now();

    // the BVH2 over the flat array
    Bvh2Built built;
    std::chrono::steady_clock::time_point unused;
    if (int st = build_bvh2_on_the_device(c, who, nullptr, b.triangles.as<HiprTriangle>(), new_count, depth_limit, built, unused)) return st;
    uint32_t build_status[STATUS_LEVELS] = {};
    HIP_TRY(hipMemcpyAsync(build_status, b.status.ptr, STATUS_LEVELS * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint32_t node_count = built.node_count, deepest = build_status[STATUS_DEEPEST];
    const uint32_t bvh_levels = std::max<uint32_t>(uint32_t(built.level_nodes.size()), 1u);
    if (bvh_levels > W8_MAX_LEVELS || deepest + 1u > 64u)
        return fail(HIPR_ERROR_UNSUPPORTED, "%s: the new BVH2 has %u levels of nodes and its deepest leaf at %u, the kernels walk 64", who, bvh_levels, deepest);
    // a fresh upload of so small a scene would choose another search (ResidentScene::choose_variant) and build other arrays: the host path serves it
    if (edit && node_count <= 64u) return fail(HIPR_ERROR_UNSUPPORTED, "%s: the new BVH2 has %u nodes, the 8-wide search serves more than 64; rebuild on the host and call hipr_upload_scene", who, node_count);
    const auto t2 = std::chrono::steady_clock::now();

    // the hand-over and the collapse
    if (x.level_nodes.resize(size_t(node_count) * 4)) return HIPR_ERROR_OUT_OF_MEMORY;
    if (int st = collapse_scratch_for(w, n, stream)) return st;
    hipLaunchKernelGGL(k_rebuild_levels, dim3((node_count + REBUILD_BLOCK - 1) / REBUILD_BLOCK), block, 0, stream, b.place.as<uint32_t>(), x.level_nodes.as<uint32_t>(), node_count);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> level_first(size_t(bvh_levels) + 1, 0u);
    if (built.level_nodes.empty()) level_first[1] = 1u;      // at most three triangles: the root references one leaf twice
    else for (uint32_t l = 0; l < bvh_levels; ++l) level_first[l + 1] = level_first[l] + built.level_nodes[l];
    W8State S = {};
    S.nodes = b.out_nodes.as<HiprBvhNode>(); S.node_count = node_count;
    S.triangles = b.triangles.as<HiprTriangle>(); S.order = b.order.as<uint32_t>(); S.triangle_count = new_count;
    S.level_nodes = x.level_nodes.as<uint32_t>(); S.reachable = node_count; S.single_leaf = built.level_nodes.empty() ? 1u : 0u;
    S.counts = w.counts.as<uint32_t>(); S.block_sums = w.block_sums.as<uint32_t>(); S.status = w.status.as<uint32_t>();
    HiprWide8BuildResult wide8 = {};
    if (int st = collapse_on_the_device(c, who, S, level_first, 0xFFFFFFFFu, wide8)) return st == HIPR_ERROR_INVALID_ARGUMENT ? HIPR_ERROR_UNSUPPORTED : st;
    if (wide8.height > 33u) return fail(HIPR_ERROR_UNSUPPORTED, "%s: the new 8-wide tree is %u levels high, the kernels' stacks hold 33; rebuild on the host", who, wide8.height);
    if ((out_nodes && node_count > node_capacity) || (out_slots && wide8.slot_count > slot_capacity)) return fail(HIPR_ERROR_HIP, "%s: %u nodes and %u slots built, more than the bounds checked", who, node_count, wide8.slot_count);
    std::vector<HiprSlot8> host_slots(wide8.slot_count);      // the refit's lists are made from the host's copy, as at upload
    HIP_TRY(hipMemcpyAsync(host_slots.data(), S.slots, host_slots.size() * sizeof(HiprSlot8), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const auto t3 = std::chrono::steady_clock::now();

    // nothing refuses from here on: the new resident arrays
    const ResidentScene::RebuiltTrees::NewSet new_set = {new_count, x.instances.as<HiprInstance>(), edit ? &edit->instances : nullptr, flatten_status[EDIT_STATUS_NOT_OPAQUE] == 0,
                                                         flatten_status[EDIT_STATUS_COATED] != 0};
    const ResidentScene::RebuiltTrees trees = {b.triangles.as<HiprTriangle>(), x.flat_class.as<uint8_t>(), b.order.as<uint32_t>(), b.out_nodes.as<HiprBvhNode>(), node_count, deepest,
                                               S.slots, host_slots.data(), wide8, edit ? &new_set : nullptr};
    if (int st = r.install_rebuilt_trees(trees, stream)) return st;
    if (edit) edit->triangle_count = new_count;
    const auto t4 = std::chrono::steady_clock::now();
    if (out_nodes) HIP_TRY(hipMemcpyAsync(out_nodes, b.out_nodes.ptr, size_t(node_count) * sizeof(HiprBvhNode), hipMemcpyDeviceToHost, stream));
    if (out_order) HIP_TRY(hipMemcpyAsync(out_order, b.order.ptr, n * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (out_slots) std::memcpy(out_slots, host_slots.data(), host_slots.size() * sizeof(HiprSlot8));
    out->node_count = node_count; out->deepest = deepest; out->wide8 = wide8; out->half_area = r.uploaded_half_area;
    const auto t5 = std::chrono::steady_clock::now();
    auto ms = [](std::chrono::steady_clock::time_point from, std::chrono::steady_clock::time_point to) { return std::chrono::duration<double, std::milli>(to - from).count(); };
    x.flatten_ms = ms(t0, t1); x.bvh2_ms = ms(t1, t2); x.collapse_ms = ms(t2, t3); x.install_ms = ms(t3, t4); x.readback_ms = ms(t4, t5);
    if (std::getenv("HIPR_BVH_TIMING"))
        fprintf(stderr, "[hipr] %s: %u triangles, %u nodes, %u slots: flatten order %.3f ms, BVH2 %.3f ms, collapse + slots to the host %.3f ms, new resident arrays %.3f ms, read-back %.3f ms\n", who, new_count, node_count,
                wide8.slot_count, x.flatten_ms, x.bvh2_ms, x.collapse_ms, x.install_ms, x.readback_ms);
    return HIPR_OK;
}

int hipr_rebuild_scene_trees(HiprContext* c, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t node_capacity, uint32_t* out_order, HiprSlot8* out_slots, uint32_t slot_capacity,
                             HiprSceneRebuildResult* out) {
    return rebuild_trees_on_the_device(c, "hipr_rebuild_scene_trees", nullptr, max_depth, out_nodes, node_capacity, out_order, out_slots, slot_capacity, out);
}

// Every refusal of hipr_edit_scene_instances that looks at the list and the host's books alone, and the new list with its tables on the way: no HIP call.
static int check_instance_edit(const ResidentScene& r, const HiprInstanceEdit* edits, uint32_t edit_count, InstanceEdit& plan) {
    const char* who = "hipr_edit_scene_instances";
    if (!edits) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null list", who);
    const uint32_t resident = uint32_t(r.uploaded_instances.size()), primitive_total = r.uploaded_index_count / 3;
    plan.instances.resize(edit_count);
    plan.source.assign(edit_count, BUILD_NONE);
    plan.primitive_count.assign(edit_count, 0u);
    plan.old_to_new.assign(resident, BUILD_NONE);
    for (uint32_t i = 0; i < edit_count; ++i) {
        const HiprInstanceEdit& e = edits[i];
        if (e.source != HIPR_EDIT_NEW_INSTANCE) {
            if (e.source >= resident) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: entry %u keeps instance %u of %u", who, i, e.source, resident);
            if (plan.old_to_new[e.source] != BUILD_NONE) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: entry %u names instance %u, which entry %u keeps already", who, i, e.source, plan.old_to_new[e.source]);
            plan.old_to_new[e.source] = i;
            plan.source[i] = e.source;
            plan.instances[i] = r.uploaded_instances[e.source];
            continue;
        }
        const HiprInstance& inst = e.instance;
        if (inst.index_offset > primitive_total || e.primitive_count > primitive_total - inst.index_offset || inst.vertex_offset > r.uploaded_vertex_count)
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: entry %u (index offset %u, %u primitives, vertex offset %u) lies outside the uploaded pools of %u triples and %u vertices", who, i, inst.index_offset,
                        e.primitive_count, inst.vertex_offset, primitive_total, r.uploaded_vertex_count);
        if (inst.material_index < 0 || size_t(inst.material_index) >= r.uploaded_materials.size())
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: entry %u references material %d of %zu", who, i, inst.material_index, r.uploaded_materials.size());
        char invalid[256];
        if (invalid_material(r.uploaded_materials[size_t(inst.material_index)], uint32_t(inst.material_index), uint32_t(r.uploaded_textures.size()), invalid, sizeof(invalid)))
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: entry %u: %s", who, i, invalid);
        if (inst.mesh_flags & (HIPR_MESH_TEXCOORDS | HIPR_MESH_TINTS | HIPR_MESH_EMISSIVE) & ~r.uploaded_mesh_attributes)
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: entry %u flags an attribute whose pool was not uploaded", who, i);
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(inst.object_to_world[k])) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the matrix of entry %u is not finite", who, i);
        plan.instances[i] = inst;
        plan.primitive_count[i] = e.primitive_count;
    }
    return HIPR_OK;
}

// Models added and removed on the device (instance_edit.h): the list checked on the host, then the rebuild's core over the new list.
int hipr_edit_scene_instances(HiprContext* c, const HiprInstanceEdit* edits, uint32_t edit_count, uint32_t max_depth, HiprBvhNode* out_nodes, uint32_t node_capacity, uint32_t* out_order,
                              uint32_t order_capacity, HiprSlot8* out_slots, uint32_t slot_capacity, HiprSceneEditResult* out) {
    const char* who = "hipr_edit_scene_instances";
    if (int st = check_context(c)) return st;
    const ResidentScene& r = c->scene;
    if (!r.ready && !r.awaits_rebuild) return fail(HIPR_ERROR_NOT_READY, "%s: no scene uploaded, or one a failed call left behind", who);
    if (!out) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null result", who);
    InstanceEdit plan;
    plan.order_capacity = order_capacity;
    if (int st = check_instance_edit(r, edits, edit_count, plan)) return st;
    if (edit_count == 0) return fail(HIPR_ERROR_UNSUPPORTED, "%s: an empty list; a scene without models is the host path's", who);
    HiprSceneRebuildResult trees = {};
    if (int st = rebuild_trees_on_the_device(c, who, &plan, max_depth, out_nodes, node_capacity, out_order, out_slots, slot_capacity, &trees)) return st;
    *out = {};
    out->triangle_count = plan.triangle_count; out->instance_count = edit_count;
    out->node_count = trees.node_count; out->deepest = trees.deepest; out->wide8 = trees.wide8; out->half_area = trees.half_area;
    return HIPR_OK;
}

// Not part of the public header: every refusal of hipr_append_scene_pools that is not a failed allocation, and nothing else -- no HIP call, the device and the
// books stay as they are. The group asks every member before any member writes.
int hipr_internal_check_pool_growth(HiprContext* c, const HiprPoolGrowth* g) {
    const char* who = "hipr_append_scene_pools";
    if (int st = check_context(c)) return st;
    const ResidentScene& r = c->scene;
    if (!r.ready && !r.awaits_rebuild) return fail(HIPR_ERROR_NOT_READY, "%s: no scene uploaded, or one a failed call left behind", who);
    if (!g) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null description", who);
    if ((g->vertex_count && !g->geometry) || (g->texcoord_vertices && !g->texcoords) || (g->tint_vertices && !g->tints) || (g->emission_vertices && !g->emissions) || (g->index_count && !g->indices) ||
        (g->segment_count && !g->segments) || (g->material_count && !g->materials) || (g->texture_count && !g->textures) || (g->texel_bytes && !g->texels))
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: null array with a non-zero count", who);
    const uint64_t limit = 0xFFFFFFFFull, vertices = uint64_t(r.uploaded_vertex_count) + g->vertex_count;
    if (vertices > limit) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: %u + %u vertices do not fit 32 bits", who, r.uploaded_vertex_count, g->vertex_count);
    const struct { const char* name; uint32_t bit, covered; } attributes[3] = {{"texcoords", HIPR_MESH_TEXCOORDS, g->texcoord_vertices}, {"tints", HIPR_MESH_TINTS, g->tint_vertices},
                                                                               {"emissions", HIPR_MESH_EMISSIVE, g->emission_vertices}};
    for (const auto& a : attributes) {
        if (r.uploaded_mesh_attributes & a.bit) {
            if (a.covered != g->vertex_count)
                return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the %s pool is resident and takes its tail, %u entries; %u given", who, a.name, g->vertex_count, a.covered);
        } else if (a.covered != 0 && a.covered != vertices)
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the %s pool is not resident and comes whole, %llu entries, or not at all; %u given", who, a.name, (unsigned long long)vertices, a.covered);
    }
    if (g->segment_count && r.uploaded_index_count % 3u) return fail(HIPR_ERROR_UNSUPPORTED, "%s: the uploaded index pool of %u words is not one of whole triples", who, r.uploaded_index_count);
    uint64_t position = r.uploaded_index_count, from_host = 0;
    for (uint32_t k = 0; k < g->segment_count; ++k) {
        const HiprIndexSegment& s = g->segments[k];
        if (s.index_count % 3u) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: segment %u has %u index words, not whole triples", who, k, s.index_count);
        if (s.mirrored_from == HIPR_SEGMENT_FROM_HOST) from_host += s.index_count;
        else if (3ull * s.mirrored_from + s.index_count > position)
            return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: segment %u mirrors %u triples from triple %u on, the pool holds %llu there", who, k, s.index_count / 3u, s.mirrored_from, (unsigned long long)(position / 3u));
        position += s.index_count;
        if (position > limit) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the grown index pool does not fit 32 bits", who);
    }
    if (from_host != g->index_count) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the host segments take %llu index words, %u given", who, (unsigned long long)from_host, g->index_count);
    const uint64_t material_total = uint64_t(r.uploaded_materials.size()) + g->material_count, texture_total = uint64_t(r.uploaded_textures.size()) + g->texture_count;
    if (material_total > limit || texture_total > limit || g->texel_bytes > ~0ull - r.uploaded_texel_bytes) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: the grown material, texture or texel pool does not fit its count", who);
    char invalid[256];
    for (uint32_t k = 0; k < g->texture_count; ++k)
        if (invalid_texture(g->textures[k], uint32_t(r.uploaded_textures.size()) + k, r.uploaded_texel_bytes + g->texel_bytes, invalid, sizeof(invalid))) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: %s", who, invalid);
    for (uint32_t k = 0; k < g->material_count; ++k)
        if (invalid_material(g->materials[k], uint32_t(r.uploaded_materials.size()) + k, uint32_t(texture_total), invalid, sizeof(invalid))) return fail(HIPR_ERROR_INVALID_ARGUMENT, "%s: %s", who, invalid);
    return HIPR_OK;
}

// The resident pools grown at their tails (pool_growth.h): the description checked on the host, then ResidentScene::append_pools.
int hipr_append_scene_pools(HiprContext* c, const HiprPoolGrowth* g) {
    if (int st = hipr_internal_check_pool_growth(c, g)) return st;
    if (!g->vertex_count && !g->texcoord_vertices && !g->tint_vertices && !g->emission_vertices && !g->segment_count && !g->material_count && !g->texture_count && !g->texel_bytes) return HIPR_OK;
    if (int finish_status = finish_all(c)) return finish_status;      // no pending pass may go on over buffers that are about to move
    c->break_chain(c->stream);
    return c->scene.append_pools(*g, c->stream);
}

int hipr_debug_append_times(HiprContext* c, double* out3_ms) {
    if (!c || !out3_ms) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_append_times: null argument");
    for (int k = 0; k < 3; ++k) out3_ms[k] = c->scene.append_ms[k];
    return HIPR_OK;
}

int hipr_debug_rebuild_times(HiprContext* c, double* out5_ms) {
    if (!c || !out5_ms) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_rebuild_times: null argument");
    const RebuildScratch& x = c->rebuild;
    out5_ms[0] = x.flatten_ms; out5_ms[1] = x.bvh2_ms; out5_ms[2] = x.collapse_ms; out5_ms[3] = x.install_ms; out5_ms[4] = x.readback_ms;
    return HIPR_OK;
}

// Where the device holds scene array `which`, and how many bytes of it the scene's counts make readable; false for an unknown array.
static bool scene_buffer(const ResidentScene& r, int which, const void*& from, uint64_t& bytes) {
    const uint64_t triangles = r.args.triangle_count, vertices = r.uploaded_vertex_count;
    auto attribute = [&](const DeviceBuffer& pool, uint32_t bit, uint64_t stride) { from = pool.ptr; bytes = r.uploaded_mesh_attributes & bit ? vertices * stride : 0u; };      // an absent pool: zero bytes
    if (which == HIPR_SCENE_BUFFER_TRIANGLES) { from = r.triangles.ptr; bytes = triangles * sizeof(HiprTriangle); }
    else if (which == HIPR_SCENE_BUFFER_WIDE8_SLOTS) { from = r.wide8_slots.ptr; bytes = uint64_t(r.wide8.slot_count) * sizeof(HiprSlot8); }
    else if (which == HIPR_SCENE_BUFFER_TRACE_TRIANGLES) { from = r.trace_triangles.ptr; bytes = triangles * 3 * sizeof(float4); }
    else if (which == HIPR_SCENE_BUFFER_SHADE_TRIANGLES) { from = r.shade_triangles.ptr; bytes = triangles * SHADE_TRIANGLE_QUADS * sizeof(float4); }
    else if (which == HIPR_SCENE_BUFFER_TRIANGLE_CLASS) { from = r.triangle_class.ptr; bytes = triangles; }
    else if (which == HIPR_SCENE_BUFFER_MATERIALS) { from = r.materials.ptr; bytes = uint64_t(r.uploaded_materials.size()) * sizeof(HiprMaterial); }
    else if (which == HIPR_SCENE_BUFFER_INSTANCES) { from = r.instances.ptr; bytes = uint64_t(r.uploaded_instances.size()) * sizeof(HiprInstance); }
    else if (which == HIPR_SCENE_BUFFER_NODES) { from = r.nodes.ptr; bytes = uint64_t(r.args.node_count) * sizeof(HiprBvhNode); }
    else if (which == HIPR_SCENE_BUFFER_INDICES) { from = r.indices.ptr; bytes = uint64_t(r.uploaded_index_count) * 4; }
    else if (which == HIPR_SCENE_BUFFER_GEOMETRY) { from = r.geometry.ptr; bytes = vertices * sizeof(HiprVertexGeometry); }
    else if (which == HIPR_SCENE_BUFFER_TEXCOORDS) attribute(r.texcoords, HIPR_MESH_TEXCOORDS, 8);
    else if (which == HIPR_SCENE_BUFFER_TINTS) attribute(r.tints, HIPR_MESH_TINTS, 4);
    else if (which == HIPR_SCENE_BUFFER_EMISSIONS) attribute(r.emissions, HIPR_MESH_EMISSIVE, 12);
    else if (which == HIPR_SCENE_BUFFER_TEXTURES) { from = r.textures.ptr; bytes = uint64_t(r.uploaded_textures.size()) * sizeof(HiprTexture); }
    else if (which == HIPR_SCENE_BUFFER_TEXELS) { from = r.texels.ptr; bytes = r.uploaded_texel_bytes; }
    else return false;
    return true;
}

int hipr_debug_read_scene_buffer(HiprContext* c, int which, void* out, uint64_t capacity_bytes) {
    if (int st = check_context(c)) return st;
    if (!out) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_read_scene_buffer: null output");
    if (c->scene.args.triangle_count == 0 && c->scene.wide8.slot_count == 0) return fail(HIPR_ERROR_NOT_READY, "hipr_debug_read_scene_buffer: no scene uploaded");
    const void* from = nullptr;
    uint64_t bytes = 0;
    if (!scene_buffer(c->scene, which, from, bytes)) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_read_scene_buffer: unknown buffer %d", which);
    if (capacity_bytes < bytes) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_read_scene_buffer: %llu bytes needed, %llu given", (unsigned long long)bytes, (unsigned long long)capacity_bytes);
    if (int finish_status = finish_all(c)) return finish_status;
    if (bytes) HIP_TRY(hipMemcpy(out, from, bytes, hipMemcpyDeviceToHost));
    return HIPR_OK;
}

int hipr_debug_scene_buffer_bytes(HiprContext* c, int which, uint64_t* out_bytes) {
    if (int st = check_context(c)) return st;
    if (!out_bytes) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_scene_buffer_bytes: null output");
    if (c->scene.args.triangle_count == 0 && c->scene.wide8.slot_count == 0) return fail(HIPR_ERROR_NOT_READY, "hipr_debug_scene_buffer_bytes: no scene uploaded");
    const void* from = nullptr;
    if (!scene_buffer(c->scene, which, from, *out_bytes)) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_scene_buffer_bytes: unknown buffer %d", which);
    return HIPR_OK;
}

int hipr_set_scene_state(HiprContext* c, const HiprSceneState* state) {
    if (int s = check_context(c)) return s;
    if (!state) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null scene state");
    for (int i = 0; i < 3; ++i) c->scene.args.env_tint[i] = state->environment_tint[i];
    c->scene.args.next_event_sample_count = std::min(std::max(state->next_event_sample_count, 0), 256);
    return HIPR_OK;
}

int hipr_set_frame(HiprContext* c, const HiprFrameDesc* f) {
    if (int s = check_context(c)) return s;
    if (!f || f->width == 0 || f->height == 0 || f->tile_stride == 0 || f->tile_phase >= f->tile_stride || f->samples_per_pass == 0)
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_set_frame: bad frame description");
    FrameInfo fi;
    fi.width = f->width; fi.height = f->height;
    fi.tiles_x = (f->width + 7) / 8;
    fi.tiles_total = fi.tiles_x * ((f->height + 7) / 8);
    fi.tile_phase = f->tile_phase; fi.tile_stride = f->tile_stride;
    fi.owned_tiles = (fi.tiles_total + f->tile_stride - 1 - f->tile_phase) / f->tile_stride;
    fi.samples_per_pass = f->samples_per_pass;
    set_frame_divisors(fi);
    const uint64_t slots = uint64_t(fi.owned_tiles) * 64u * fi.samples_per_pass;
    if (slots == 0 || slots > 0x7FFFFFFFull) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_set_frame: %llu path slots per pass", (unsigned long long)slots);
    if (int finish_status = finish_all(c)) return finish_status;
    c->frame_ready = false;      // a failure below leaves HIPR_ERROR_NOT_READY, not the earlier frame's flag over this frame's buffers
    c->frame = fi;
    int r = partition_path_slots(c);
    const size_t acc_bytes = size_t(fi.owned_tiles) * 64 * sizeof(double4);
    c->accumulation.release();
    c->scratch_accumulation.release();
    c->use_scratch = false;
    r |= c->accumulation.resize(acc_bytes);
    if (r) return HIPR_ERROR_OUT_OF_MEMORY;
    HIP_TRY(hipMemsetAsync(c->accumulation.ptr, 0, acc_bytes, c->stream));
    if (int finish_status = finish_all(c)) return finish_status;
    c->traced_samples = 0;
    c->frame_ready = true;
    return HIPR_OK;
}

int hipr_set_entry_point(HiprContext* c, int entry) {
    if (!c) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null context");
    switch (entry) {
    case HIPR_ENTRY_PATH_TRACING: case HIPR_ENTRY_DEPTH: case HIPR_ENTRY_ALBEDO: case HIPR_ENTRY_TINT: case HIPR_ENTRY_ROUGHNESS:
    case HIPR_ENTRY_SHADING_NORMAL: case HIPR_ENTRY_PRIMITIVE_ID: case HIPR_ENTRY_DENOISER_ALBEDO:
        c->entry = entry;
        return HIPR_OK;
    case 1: case 2:
        return fail(HIPR_ERROR_UNSUPPORTED, "entry point %d is one of the two launches of the reference's AIDenoisedBackend command list; here that backend is a path tracing pass, "
                    "a HIPR_ENTRY_DENOISER_ALBEDO pass and hipr_denoiser_process (include/hipr_denoiser_c.h)", entry);
    }
    return fail(HIPR_ERROR_INVALID_ARGUMENT, "unknown entry point %d", entry);
}

int hipr_use_scratch_accumulation(HiprContext* c, int enable) {
    if (int s = check_context(c)) return s;
    if (!c->frame_ready) return fail(HIPR_ERROR_NOT_READY, "no frame set");
    if (int s = drain(c)) return s;
    if (enable) {
        const size_t bytes = size_t(c->frame.owned_tiles) * 64 * sizeof(double4);
        const bool keep = enable == 2 && c->scratch_accumulation.ptr && c->scratch_accumulation.bytes >= bytes;   // a running mean kept across calls
        if (int s = c->scratch_accumulation.resize(bytes)) return s;
        if (!keep) HIP_TRY(hipMemset(c->scratch_accumulation.ptr, 0, bytes));
    }
    c->use_scratch = enable != 0;
    return HIPR_OK;
}

int hipr_owned_pixel_count(HiprContext* c, uint32_t* out_count) {
    if (!c || !out_count) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null argument");
    if (!c->frame_ready) return fail(HIPR_ERROR_NOT_READY, "no frame set");
    *out_count = c->frame.owned_tiles * 64u;
    return HIPR_OK;
}

int hipr_set_samples_per_pass(HiprContext* c, uint32_t samples_per_pass) {
    if (int s = check_context(c)) return s;
    if (!c->frame_ready) return fail(HIPR_ERROR_NOT_READY, "no frame set");
    const uint64_t slots = uint64_t(c->frame.owned_tiles) * 64u * samples_per_pass;
    if (samples_per_pass == 0 || slots > 0x7FFFFFFFull) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_set_samples_per_pass: %llu path slots per pass", (unsigned long long)slots);
    if (samples_per_pass == c->frame.samples_per_pass) return HIPR_OK;
    if (int s = drain(c)) return s;      // the queues may move
    c->frame.samples_per_pass = samples_per_pass;
    set_frame_divisors(c->frame);
    if (partition_path_slots(c)) return HIPR_ERROR_OUT_OF_MEMORY;
    return HIPR_OK;
}

int hipr_render_pass(HiprContext* c, const HiprCameraState* camera, void* out_half4_device, uint32_t out_pitch_pixels, int synchronize) {
    if (int s = hipr_trace_pass(c, camera)) return s;
    return hipr_accumulate_samples(c, 0, c->frame.samples_per_pass, camera->accumulations, out_half4_device, out_pitch_pixels, synchronize);
}

int hipr_trace_pass(HiprContext* c, const HiprCameraState* camera) {
    if (int s = check_context(c)) return s;
    if (!camera) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null camera");
    if (!c->tables_ready || !c->scene.ready || !c->frame_ready) return fail(HIPR_ERROR_NOT_READY, "tables, scene and frame must be set before rendering");
    if (c->partitioned_for != c->wavefronts_wanted()) {      // the scene uploaded since hipr_set_frame wants another split of the path slots
        if (int s = drain(c)) return s;
        if (partition_path_slots(c)) return HIPR_ERROR_OUT_OF_MEMORY;
    }
    // Pipelined passes (HiprContext::PassSlot): this pass takes the slot the pass before the last one used, whose tail has long drained.
    const bool pipelined = c->knobs.pipeline_passes && c->use_persistent() && c->wavefront_count == 1 && c->radiance_other.ptr && !c->instrument;
    const int slot = pipelined ? c->next_slot : 0;
    if (int s = begin_pass(c, slot, pipelined)) return s;
    const int first_wavefront = pipelined ? slot : 0, end_wavefront = pipelined ? slot + 1 : c->wavefront_count;

    HiprCounters pass = {};
    pass.camera_rays = camera_rays_of(c->frame);
    pass.closest_rays -= c->n_slots - uint32_t(std::min<uint64_t>(c->n_slots, pass.camera_rays));   // dead lanes of partial tiles are queued but never traced
    uint32_t alive[MAX_WAVEFRONTS] = {}, bounce[MAX_WAVEFRONTS] = {};      // alive: the paths of the wavefront's current bounce; 0: it has ended
    for (int g = first_wavefront; g < end_wavefront; ++g) {
        if (int s = start_wavefront(c, c->wavefronts[g], *camera, pipelined)) return s;
        alive[g] = c->wavefronts[g].n_slots;
    }
    // Round robin over the wavefronts, one bounce of each at a time, until all have ended or the pass's tail is detached.
    bool detached = false;
    for (int remaining = end_wavefront - first_wavefront; remaining > 0 && !detached;) {
        for (int g = first_wavefront; g < end_wavefront && !detached; ++g) {
            if (alive[g] == 0) continue;
            Wavefront& w = c->wavefronts[g];
            const uint32_t k = bounce[g]++;
            if (int s = advance_wavefront(c, w, *camera, k + 1, k, alive[g], pass)) return s;
            if (alive[g] == 0) {
                --remaining;
                if (!pipelined && g > 0) {
                    HIP_TRY(hipEventRecord(w.finished, w.stream));
                    HIP_TRY(hipStreamWaitEvent(c->stream, w.finished, 0));
                }
            } else if (pipelined && k >= 1 && uint64_t(alive[g]) * 64u < w.n_slots) {      // a sliver of the paths is left
                if (int s = detach_tail(c, w, c->pass_slots[slot], *camera, k, alive[g])) return s;
                detached = true;
            }
        }
    }

    c->pass_depth_normalizer = c->entry == HIPR_ENTRY_DEPTH ? depth_range_of(*camera) : 0.0f;
    HIP_TRY(hipGetLastError());
    c->traced_samples = c->frame.samples_per_pass;
    c->total.camera_rays += pass.camera_rays;
    c->total.closest_rays += pass.closest_rays;
    c->total.shadow_rays += pass.shadow_rays;
    c->total.iterations += pass.iterations;
    if (c->instrument || c->timed.size() > 2048)
        if (int s = drain(c)) return s;
    return HIPR_OK;
}

int hipr_accumulate_samples(HiprContext* c, uint32_t first_sample, uint32_t sample_count, uint32_t first_accumulation, void* out_half4_device, uint32_t out_pitch_pixels,
                            int synchronize) {
    if (int s = check_context(c)) return s;
    if (!c->frame_ready) return fail(HIPR_ERROR_NOT_READY, "no frame set");
    if (sample_count == 0 || uint64_t(first_sample) + sample_count > c->traced_samples)
        return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_accumulate_samples: samples [%u, %u) of a traced pass of %u", first_sample, first_sample + sample_count, c->traced_samples);
    if (out_half4_device && c->frame.tile_stride == 1 && out_pitch_pixels < c->frame.width) return fail(HIPR_ERROR_INVALID_ARGUMENT, "output pitch smaller than the frame width");
    const FrameInfo& f = c->frame;
    // The fold runs on the stream of the slot that traced the samples, behind that pass's tail; two consecutive folds may be on different streams and
    // both update the running mean and the frame: the later one waits for the earlier one.
    hipStream_t stream = c->wavefronts[c->traced_slot].stream;
    if (c->accumulated_valid) HIP_TRY(hipStreamWaitEvent(stream, c->accumulated, 0));
    c->break_chain(stream);
    c->begin_timed(HIPR_KERNEL_ACCUMULATE, stream);
    hipLaunchKernelGGL(k_accumulate, dim3((f.owned_tiles * 64 + 255) / 256), dim3(256), 0, stream, f, first_sample, sample_count, first_accumulation, c->radiance.as<float4>(),
                       c->active_accumulation().as<double4>(), static_cast<ushort4*>(out_half4_device), out_pitch_pixels, c->pass_depth_normalizer);
    c->end_timed(stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->accumulated, stream));
    c->accumulated_valid = true;
    if (synchronize || c->instrument || c->timed.size() > 2048) {
        if (int s = drain(c)) return s;
    }
    return HIPR_OK;
}

int hipr_synchronize(HiprContext* c) {
    if (int s = check_context(c)) return s;
    if (int s = drain(c)) return s;
    return HIPR_OK;
}

int hipr_get_counters(HiprContext* c, HiprCounters* out) {
    if (int s = check_context(c)) return s;
    if (!out) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null counters");
    if (int s = drain(c)) return s;
    DeviceCounters dc;
    HIP_TRY(hipMemcpy(&dc, c->counters.ptr, sizeof(dc), hipMemcpyDeviceToHost));
    *out = c->total;
    out->shaded_hits = dc.shaded_hits;
    out->closest_nodes = dc.closest_nodes;
    out->closest_triangles = dc.closest_triangles;
    out->shadow_nodes = dc.shadow_nodes;
    out->shadow_triangles = dc.shadow_triangles;
    return HIPR_OK;
}

int hipr_reset_counters(HiprContext* c) {
    if (int s = check_context(c)) return s;
    if (int s = drain(c)) return s;
    HIP_TRY(hipMemset(c->counters.ptr, 0, sizeof(DeviceCounters)));
    c->total = {};
    c->trace_log_previous = {};
    return HIPR_OK;
}

int hipr_set_wavefront_count(HiprContext* c, int count) {
    if (!c) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null context");
    if (count < 0 || count > MAX_WAVEFRONTS) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_set_wavefront_count: %d is outside [0, %d]", count, MAX_WAVEFRONTS);
    c->knobs.wavefront_limit = count;   // 0: by scene; takes effect with the next pass
    return HIPR_OK;
}

int hipr_get_wavefront_count(HiprContext* c, int* out_count) {
    if (!c || !out_count) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_get_wavefront_count: null argument");
    // what the NEXT pass runs as: the partition is redone at its start when the rule's answer changed (scene uploaded, limit set since hipr_set_frame)
    const uint64_t slots = uint64_t(c->frame.owned_tiles) * 64u * c->frame.samples_per_pass;
    *out_count = c->frame_ready ? int(std::max<uint64_t>(1, std::min<uint64_t>(uint64_t(c->wavefronts_wanted()), slots / 65536u))) : 0;
    return HIPR_OK;
}

int hipr_get_trace_variant(HiprContext* c, int* out_variant) {
    if (!c || !out_variant) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_get_trace_variant: null argument");
    *out_variant = c->scene.ready ? c->active_trace_variant() : HIPR_TRACE_BVH2;
    return HIPR_OK;
}

int hipr_set_trace_variant(HiprContext* c, int variant) {
    if (!c) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null context");
    if (variant < -1 || variant > HIPR_TRACE_WIDE8_PERSISTENT) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_set_trace_variant: unknown variant %d", variant);
    if (c->scene.tree_stale && (variant == HIPR_TRACE_BVH2 || variant == HIPR_TRACE_WIDE_PERSISTENT))
        return fail(HIPR_ERROR_UNSUPPORTED, "hipr_set_trace_variant: the BVH2 and 4-wide arrays are stale after hipr_refit_scene_transforms; call hipr_update_scene_geometry or hipr_upload_scene first");
    c->knobs.trace_variant = variant;     // the exhaustive search's items are built at upload: upload the scene after this call
    return HIPR_OK;
}

int hipr_set_backface_culling(HiprContext* c, int enable) {
    if (int s = check_context(c)) return s;
    if (int s = finish_all(c)) return s;
    c->knobs.cull_backfaces = enable != 0;
    c->scene.wide8.cull_backfaces = c->knobs.cull_backfaces ? 1u : 0u;
    return HIPR_OK;
}

int hipr_set_arithmetic(HiprContext* c, int arithmetic) {
    if (int s = check_context(c)) return s;
    if (arithmetic != HIPR_ARITHMETIC_FAST && arithmetic != HIPR_ARITHMETIC_EXACT) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_set_arithmetic: unknown mode %d", arithmetic);
    if (int s = finish_all(c)) return s;
    c->knobs.arithmetic = arithmetic;
    return HIPR_OK;
}

int hipr_get_arithmetic(HiprContext* c) {
    if (int s = check_context(c)) return s;      // statuses are negative
    return c->knobs.arithmetic;
}

int hipr_set_pass_pipelining(HiprContext* c, int enable) {
    if (int s = check_context(c)) return s;
    if (int s = finish_all(c)) return s;
    c->knobs.pipeline_passes = enable != 0;
    if (c->frame_ready && partition_path_slots(c)) return HIPR_ERROR_OUT_OF_MEMORY;      // the second slot's queues come and go with the setting
    return HIPR_OK;
}

int hipr_set_instrumentation(HiprContext* c, int count_traversal_steps) {
    if (!c) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null context");
    c->instrument = count_traversal_steps != 0;
    return HIPR_OK;
}

int hipr_reset_timers(HiprContext* c) {
    if (int s = check_context(c)) return s;
    if (int s = drain(c)) return s;
    c->times = {};
    return HIPR_OK;
}

int hipr_get_kernel_times(HiprContext* c, HiprKernelTimes* out) {
    if (int s = check_context(c)) return s;
    if (!out) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null output");
    if (int s = drain(c)) return s;
    *out = c->times;
    return HIPR_OK;
}

int hipr_read_accumulation(HiprContext* c, double* out_rgba, uint64_t capacity_pixels) {
    if (int s = check_context(c)) return s;
    if (!c->frame_ready) return fail(HIPR_ERROR_NOT_READY, "no frame set");
    const FrameInfo& f = c->frame;
    const uint64_t owned = uint64_t(f.owned_tiles) * 64;
    const uint64_t needed = f.tile_stride == 1 ? uint64_t(f.width) * f.height : owned;
    if (!out_rgba || capacity_pixels < needed) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_read_accumulation: need room for %llu pixels", (unsigned long long)needed);
    if (int s = drain(c)) return s;
    if (f.tile_stride != 1) {
        HIP_TRY(hipMemcpy(out_rgba, c->active_accumulation().ptr, owned * 32, hipMemcpyDeviceToHost));
        return HIPR_OK;
    }
    std::vector<double> compact(owned * 4);
    HIP_TRY(hipMemcpy(compact.data(), c->active_accumulation().ptr, owned * 32, hipMemcpyDeviceToHost));
    for (uint32_t y = 0; y < f.height; ++y)
        for (uint32_t x = 0; x < f.width; ++x) {
            const uint64_t k = (uint64_t(y >> 3) * f.tiles_x + (x >> 3)) * 64 + ((x & 7) + ((y & 7) << 3));
            std::memcpy(out_rgba + 4 * (uint64_t(y) * f.width + x), compact.data() + 4 * k, 32);
        }
    return HIPR_OK;
}

int hipr_scatter_tiles(HiprContext* c, const void* compact, uint64_t rank_stride, uint32_t rank_count, uint32_t width, uint32_t height, void* out,
                       uint32_t out_pitch) {
    if (int s = check_context(c)) return s;
    if (!compact || !out || rank_count == 0 || out_pitch < width) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_scatter_tiles: bad argument");
    hipLaunchKernelGGL(k_scatter_tiles, dim3((width + 15) / 16, (height + 15) / 16), dim3(256), 0, c->stream, static_cast<const ushort4*>(compact),
                       (unsigned long long)rank_stride, rank_count, width, height, static_cast<ushort4*>(out), out_pitch);
    HIP_TRY(hipGetLastError());
    return HIPR_OK;
}

// ------------------------------------------------------------------------------------------- presentation side
int hipr_device_malloc(HiprContext* c, uint64_t bytes, void** out_device_pointer) {
    if (int s = check_context(c)) return s;
    if (!out_device_pointer || bytes == 0) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_device_malloc: bad argument");
    HIP_TRY(hipMalloc(out_device_pointer, bytes));
    return HIPR_OK;
}

int hipr_device_free(HiprContext* c, void* device_pointer) {
    if (int s = check_context(c)) return s;
    if (!device_pointer) return HIPR_OK;
    if (int finish_status = finish_all(c)) return finish_status;
    HIP_TRY(hipFree(device_pointer));
    return HIPR_OK;
}

int hipr_device_memset(HiprContext* c, void* device_pointer, int byte_value, uint64_t bytes) {
    if (int s = check_context(c)) return s;
    if (!device_pointer) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_device_memset: null pointer");
    HIP_TRY(hipMemsetAsync(device_pointer, byte_value, bytes, c->stream));
    return HIPR_OK;
}

int hipr_copy_to_host(HiprContext* c, void* host, const void* device_pointer, uint64_t bytes) {
    if (int s = check_context(c)) return s;
    if (!host || !device_pointer) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_copy_to_host: bad argument");
    HIP_TRY(hipMemcpyAsync(host, device_pointer, bytes, hipMemcpyDeviceToHost, c->stream));
    if (int finish_status = finish_all(c)) return finish_status;
    return HIPR_OK;
}

int hipr_present_flipped(HiprContext* c, const void* pixels, uint32_t pitch, uint32_t width, uint32_t height, void* backbuffer, uint32_t backbuffer_pitch) {
    if (int s = check_context(c)) return s;
    if (!pixels || !backbuffer || pitch < width || backbuffer_pitch < width) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_present_flipped: bad argument");
    if (width == 0 || height == 0) return HIPR_OK;
    hipLaunchKernelGGL(k_present_flipped, dim3((width + 63) / 64, (height + 3) / 4), dim3(256), 0, c->stream, static_cast<const ushort4*>(pixels), pitch, width,
                       height, static_cast<ushort4*>(backbuffer), backbuffer_pitch);
    HIP_TRY(hipGetLastError());
    return HIPR_OK;
}

// ------------------------------------------------------------------------------------------- debug / parity entry points
int hipr_debug_generate(HiprContext* c, const HiprCameraState* camera, uint32_t accumulation, float* out_origin_tmin, float* out_direction, uint32_t* out_pixel) {
    if (int s = check_context(c)) return s;
    if (!camera || !c->frame_ready) return fail(HIPR_ERROR_NOT_READY, "hipr_debug_generate needs a camera and a frame");
    FrameInfo f = c->frame;
    f.samples_per_pass = 1;
    set_frame_divisors(f);
    const uint32_t n = f.owned_tiles * 64;
    HiprCameraState cam = *camera;
    cam.accumulations = accumulation;
    DeviceBuffer bo, bd, bt, bm, br;
    if (bo.resize(size_t(n) * 16) | bd.resize(size_t(n) * 16) | bt.resize(size_t(n) * 16) | bm.resize(size_t(n) * 16) | br.resize(size_t(n) * 16)) return HIPR_ERROR_OUT_OF_MEMORY;
    const PathState out = {bo.as<float4>(), bd.as<float4>(), bt.as<float4>(), bm.as<uint2>()};
    hipLaunchKernelGGL(k_generate, dim3((n + 255) / 256), dim3(256), 0, c->stream, f, cam, out, br.as<float4>(), 0u, 1u, n);
    if (int finish_status = finish_all(c)) return finish_status;
    if (out_origin_tmin) HIP_TRY(hipMemcpy(out_origin_tmin, bo.ptr, size_t(n) * 16, hipMemcpyDeviceToHost));
    if (out_direction) HIP_TRY(hipMemcpy(out_direction, bd.ptr, size_t(n) * 16, hipMemcpyDeviceToHost));
    if (out_pixel) {
        for (uint32_t k = 0; k < n; ++k) {
            uint32_t tile = (k >> 6) * f.tile_stride + f.tile_phase, lane = k & 63;
            uint32_t x = (tile % f.tiles_x) * 8 + (lane & 7), y = (tile / f.tiles_x) * 8 + (lane >> 3);
            out_pixel[k] = (tile < f.tiles_total && x < f.width && y < f.height) ? (x | (y << 16)) : 0xFFFFFFFFu;
        }
    }
    return HIPR_OK;
}

int hipr_debug_shading(HiprContext* c, int shading_model, const float* params10, const float* wo_n3, const float* in_n3, uint32_t n, int mode, float* out_n7) {
    if (int s = check_context(c)) return s;
    if (!c->tables_ready) return fail(HIPR_ERROR_NOT_READY, "hipr_debug_shading needs the tables");
    if (!params10 || !wo_n3 || !in_n3 || !out_n7 || shading_model < 0 || shading_model > 2 || mode < 0 || mode > 1) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_shading: bad argument");
    if (n == 0) return HIPR_OK;
    DeviceBuffer bp, bw, bi, bo;
    int r = bp.upload(params10, 10 * 4, c->stream) | bw.upload(wo_n3, size_t(n) * 12, c->stream) | bi.upload(in_n3, size_t(n) * 12, c->stream) | bo.resize(size_t(n) * 28);
    if (r) return HIPR_ERROR_OUT_OF_MEMORY;
    c->shade_unit().debug_shading(c->stream, c->scene.args.tables, shading_model, bp.as<float>(), bw.as<float>(), bi.as<float>(), int(n), mode, bo.as<float>());
    HIP_TRY(hipGetLastError());
    if (int finish_status = finish_all(c)) return finish_status;
    HIP_TRY(hipMemcpy(out_n7, bo.ptr, size_t(n) * 28, hipMemcpyDeviceToHost));
    return HIPR_OK;
}

int hipr_debug_shade(HiprContext* c, const HiprCameraState* camera, uint32_t n, const float* rays_n8, const float* throughput_bounces_n4, const float* hits_n4, const uint32_t* last_triangle,
                     const uint32_t* pixel_hash, const uint32_t* accumulation, float* out_n32) {
    if (int s = check_context(c)) return s;
    if (!c->tables_ready || !c->scene.ready) return fail(HIPR_ERROR_NOT_READY, "hipr_debug_shade needs the tables and a scene");
    if (!camera || !rays_n8 || !throughput_bounces_n4 || !hits_n4 || !last_triangle || !pixel_hash || !accumulation || !out_n32) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_shade: null argument");
    if (n == 0) return HIPR_OK;
    for (uint32_t i = 0; i < n; ++i) {      // the entries name triangles and lights of the uploaded scene
        uint32_t id;
        std::memcpy(&id, hits_n4 + 4 * size_t(i) + 3, 4);
        if (id == HIPR_HIT_MISS) continue;
        if ((id & HIPR_HIT_LIGHT) ? (id & ~HIPR_HIT_LIGHT) >= c->scene.args.light_count : id >= c->scene.args.triangle_count) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_shade: entry %u names hit %u outside the scene", i, id);
    }
    DeviceBuffer br, bt, bh, bl, bp, ba, bo;
    if (br.upload(rays_n8, size_t(n) * 32, c->stream) | bt.upload(throughput_bounces_n4, size_t(n) * 16, c->stream) | bh.upload(hits_n4, size_t(n) * 16, c->stream) |
        bl.upload(last_triangle, size_t(n) * 4, c->stream) | bp.upload(pixel_hash, size_t(n) * 4, c->stream) | ba.upload(accumulation, size_t(n) * 4, c->stream) | bo.resize(size_t(n) * 128))
        return HIPR_ERROR_OUT_OF_MEMORY;
    c->shade_unit().debug_shade(c->stream, c->scene.args, *camera, n, br.as<float4>(), bt.as<float4>(), bh.as<float4>(), bl.as<uint32_t>(), bp.as<uint32_t>(), ba.as<uint32_t>(), bo.as<float>());
    HIP_TRY(hipGetLastError());
    if (int finish_status = finish_all(c)) return finish_status;
    HIP_TRY(hipMemcpy(out_n32, bo.ptr, size_t(n) * 128, hipMemcpyDeviceToHost));
    return HIPR_OK;
}

int hipr_debug_math(HiprContext* c, int function, uint32_t n, const float* x, const float* y, float* out) {
    if (int s = check_context(c)) return s;
    if (!x || !out || function < 0 || function > 2 || (function == 2 && !y)) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_math: bad argument");
    if (n == 0) return HIPR_OK;
    DeviceBuffer bx, by, bo;
    if (bx.upload(x, size_t(n) * 4, c->stream) | by.upload(y ? y : x, size_t(n) * 4, c->stream) | bo.resize(size_t(n) * 4)) return HIPR_ERROR_OUT_OF_MEMORY;
    c->shade_unit().debug_math(c->stream, function, int(n), bx.as<float>(), by.as<float>(), bo.as<float>());
    HIP_TRY(hipGetLastError());
    if (int finish_status = finish_all(c)) return finish_status;
    HIP_TRY(hipMemcpy(out, bo.ptr, size_t(n) * 4, hipMemcpyDeviceToHost));
    return HIPR_OK;
}

int hipr_debug_light(HiprContext* c, const HiprLight* light, const float* position3, const float* in_n3, uint32_t n, int mode, float* out_n8) {
    if (int s = check_context(c)) return s;
    if (!light || !position3 || !in_n3 || !out_n8 || mode < 0 || mode > 1) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_light: bad argument");
    if (mode == 1 && (light->flags & HIPR_LIGHT_TYPE_MASK) != HIPR_LIGHT_SPOT) return fail(HIPR_ERROR_UNSUPPORTED, "hipr_debug_light: evaluate / pdf by direction is exposed for spot lights only");
    if (n == 0) return HIPR_OK;
    DeviceBuffer bp, bi, bo;
    if (bp.upload(position3, 3 * 4, c->stream) | bi.upload(in_n3, size_t(n) * 12, c->stream) | bo.resize(size_t(n) * 32)) return HIPR_ERROR_OUT_OF_MEMORY;
    c->shade_unit().debug_light(c->stream, *light, bp.as<float>(), bi.as<float>(), int(n), mode, bo.as<float>());
    HIP_TRY(hipGetLastError());
    if (int finish_status = finish_all(c)) return finish_status;
    HIP_TRY(hipMemcpy(out_n8, bo.ptr, size_t(n) * 32, hipMemcpyDeviceToHost));
    return HIPR_OK;
}

int hipr_debug_sobol(HiprContext* c, const uint32_t* triples, uint32_t n, uint32_t* out_uint4) {
    if (int s = check_context(c)) return s;
    if (!triples || !out_uint4) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return HIPR_OK;
    if (int s = c->debug_a.upload(triples, size_t(n) * 12, c->stream)) return s;
    if (int s = c->debug_b.resize(size_t(n) * 16)) return s;
    hipLaunchKernelGGL(k_debug_sobol, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->debug_a.as<uint32_t>(), n, c->debug_b.as<uint32_t>(), c->sobol_tables.as<uint32_t>());
    if (int finish_status = finish_all(c)) return finish_status;
    HIP_TRY(hipMemcpy(out_uint4, c->debug_b.ptr, size_t(n) * 16, hipMemcpyDeviceToHost));
    return HIPR_OK;
}

// ---- the VALU roof, measured -----------------------------------------------------------------------------------------------------------------------
#define HIPR_RATE_KERNEL(NAME, INSTR)                                                                                              \
    __global__ __launch_bounds__(256) void NAME(uint32_t* out, const uint32_t* in, int iterations) {                                \
        uint32_t a0 = in[threadIdx.x & 7], a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7; \
        const uint32_t m = in[8 + (threadIdx.x & 1)], k = in[10 + (threadIdx.x & 1)];                                               \
        for (int it = 0; it < iterations; ++it)                                                                                     \
            asm volatile(INSTR(0) INSTR(1) INSTR(2) INSTR(3) INSTR(4) INSTR(5) INSTR(6) INSTR(7)                                    \
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(m), "v"(k));        \
        out[blockIdx.x * blockDim.x + threadIdx.x] = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;                                         \
    }
#define HIPR_RATE_FMA(k) "v_fma_f32 %" #k ", %" #k ", %8, %9\n"
#define HIPR_RATE_MAX(k) "v_max_f32 %" #k ", %" #k ", %8\n"
#define HIPR_RATE_CVT(k) "v_cvt_f32_ubyte1 %" #k ", %" #k "\n"
HIPR_RATE_KERNEL(k_rate_fma, HIPR_RATE_FMA)
HIPR_RATE_KERNEL(k_rate_max, HIPR_RATE_MAX)
HIPR_RATE_KERNEL(k_rate_cvt, HIPR_RATE_CVT)

int hipr_debug_valu_issue_rates(HiprContext* c, double* out3) {
    if (int s = check_context(c)) return s;
    if (!out3) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null argument");
    if (int finish_status = finish_all(c)) return finish_status;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, c->device));
    const int blocks = prop.multiProcessorCount * 8, threads = 256, iterations = 4096;      // 8 blocks of 4 waves per CU: 8 waves per SIMD
    const uint32_t seed[12] = {0x3f800000u, 0x3f810000u, 0x3f820000u, 0x3f830000u, 0x3f840000u, 0x3f850000u, 0x3f860000u, 0x3f870000u, 0x3f7fff00u, 0x3f7ffe00u, 0x33800000u, 0x33900000u};
    if (int s = c->debug_a.upload(seed, sizeof(seed), c->stream)) return s;
    if (int s = c->debug_b.resize(size_t(blocks) * threads * 4)) return s;
    const Event e0 = make_event(hipEventDefault), e1 = make_event(hipEventDefault);
    if (!e0 || !e1) return fail(HIPR_ERROR_HIP, "hipEventCreate failed");
    typedef void (*RateKernel)(uint32_t*, const uint32_t*, int);
    const RateKernel kernels[3] = {k_rate_fma, k_rate_max, k_rate_cvt};
    for (int which = 0; which < 3; ++which) {
        float best = 1e30f;
        for (int repeat = 0; repeat < 4; ++repeat) {      // the first launch warms the clocks up
            HIP_TRY(hipEventRecord(e0, c->stream));
            hipLaunchKernelGGL(kernels[which], dim3(blocks), dim3(threads), 0, c->stream, c->debug_b.as<uint32_t>(), c->debug_a.as<uint32_t>(), iterations);
            HIP_TRY(hipEventRecord(e1, c->stream));
            HIP_TRY(hipEventSynchronize(e1));
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
            if (repeat > 0) best = std::min(best, ms);
        }
        out3[which] = double(blocks) * (threads / 64) * double(iterations) * 8.0 / (double(best) * 1e-3);
    }
    return HIPR_OK;
}

int hipr_debug_sample_offsets(HiprContext* c, float* out_256x4) {
    if (int s = check_context(c)) return s;
    if (!out_256x4) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null argument");
    if (int finish_status = finish_all(c)) return finish_status;
    HIP_TRY(hipMemcpy(out_256x4, c->sample_offsets.ptr, 256 * 4 * sizeof(float), hipMemcpyDeviceToHost));
    return HIPR_OK;
}

static void debug_prepare_rays(const float* rays, uint32_t n, std::vector<float>& o, std::vector<float>& d) {
    o.resize(size_t(n) * 4);
    d.resize(size_t(n) * 4);
    for (uint32_t i = 0; i < n; ++i) {
        std::memcpy(&o[4 * i], rays + 8 * size_t(i), 16);
        std::memcpy(&d[4 * i], rays + 8 * size_t(i) + 4, 16);
    }
}

int hipr_debug_trace_closest(HiprContext* c, const float* rays, const uint32_t* skip, uint32_t n, float* out_hits) {
    if (int s = check_context(c)) return s;
    if (!c->scene.ready) return fail(HIPR_ERROR_NOT_READY, "no scene uploaded");
    if (!rays || !out_hits) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return HIPR_OK;
    if (int s = drain(c)) return s;      // the tail of a pipelined pass may still be running: nothing of the context is touched before it has ended
    std::vector<float> o, d;
    debug_prepare_rays(rays, n, o, d);
    std::vector<uint32_t> meta(size_t(n) * 2);
    for (uint32_t i = 0; i < n; ++i) { meta[2 * i] = i; meta[2 * i + 1] = skip ? skip[i] : HIPR_NO_TRIANGLE; }
    DeviceBuffer bo, bd, bm, bh, bc;
    int r = bo.upload(o.data(), o.size() * 4, c->stream) | bd.upload(d.data(), d.size() * 4, c->stream) | bm.upload(meta.data(), meta.size() * 4, c->stream) |
            bh.resize(size_t(n) * 16) | bc.upload(&n, 4, c->stream);
    if (r) return HIPR_ERROR_OUT_OF_MEMORY;
    HIP_TRY(hipMemsetAsync(c->counters.ptr, 0, sizeof(DeviceCounters), c->stream));
    PathState in = {bo.as<float4>(), bd.as<float4>(), nullptr, bm.as<uint2>()};
    Wavefront w;
    w.stream = c->stream;
    w.hits = std::move(bh);
    trace_rays<TRACE_CLOSEST>(c, w, {in, bc.as<uint32_t>(), nullptr, n});
    if (int finish_status = finish_all(c)) return finish_status;
    HIP_TRY(hipMemcpy(out_hits, w.hits.ptr, size_t(n) * 16, hipMemcpyDeviceToHost));
    c->total = {};
    c->total.closest_rays = n;
    return HIPR_OK;
}

int hipr_debug_trace_shadow(HiprContext* c, const float* rays, uint32_t n, float* out_transmittance) {
    if (int s = check_context(c)) return s;
    if (!c->scene.ready) return fail(HIPR_ERROR_NOT_READY, "no scene uploaded");
    if (!rays || !out_transmittance) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return HIPR_OK;
    if (int s = drain(c)) return s;      // as in hipr_debug_trace_closest: the swap of `radiance` below must not meet a pass that is still running
    std::vector<float> o(size_t(n) * 4), d(size_t(n) * 4), rad(size_t(n) * 4, 0.0f), ones(size_t(n) * 4, 1.0f);
    for (uint32_t i = 0; i < n; ++i) {
        std::memcpy(&o[4 * i], rays + 8 * size_t(i), 12);
        o[4 * i + 3] = rays[8 * size_t(i) + 7];               // tmax
        std::memcpy(&d[4 * i], rays + 8 * size_t(i) + 4, 12);
        std::memcpy(&d[4 * i + 3], &i, 4);                    // slot
    }
    DeviceBuffer bo, bd, br, bacc, bc;
    int r = bo.upload(o.data(), o.size() * 4, c->stream) | bd.upload(d.data(), d.size() * 4, c->stream) | br.upload(ones.data(), ones.size() * 4, c->stream) |
            bacc.upload(rad.data(), rad.size() * 4, c->stream) | bc.upload(&n, 4, c->stream);
    if (r) return HIPR_ERROR_OUT_OF_MEMORY;
    HIP_TRY(hipMemsetAsync(c->counters.ptr, 0, sizeof(DeviceCounters), c->stream));
    Wavefront w;
    w.stream = c->stream;
    w.shadow[0] = std::move(bo); w.shadow[1] = std::move(bd); w.shadow[2] = std::move(br);
    std::swap(c->radiance, bacc);      // the launch writes the context's radiance buffer: this call's, for its duration
    trace_rays<TRACE_SHADOW>(c, w, {PathState{}, nullptr, bc.as<uint32_t>(), n});
    std::swap(c->radiance, bacc);
    if (int finish_status = finish_all(c)) return finish_status;
    std::vector<float> result(size_t(n) * 4);
    HIP_TRY(hipMemcpy(result.data(), bacc.ptr, result.size() * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i) out_transmittance[i] = result[4 * i];
    c->total = {};
    c->total.shadow_rays = n;
    return HIPR_OK;
}

// The listing pass (kernels.h k_classify_hits) on given hits, through the launch path of a pass (classify_hits).
int hipr_debug_classify_hits(HiprContext* c, const float* hits_n4, uint32_t n, int coat_classes, uint32_t grid, uint32_t* out_order) {
    if (int s = check_context(c)) return s;
    if (!hits_n4 || !out_order) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null argument");
    if (grid > 65536u) return fail(HIPR_ERROR_INVALID_ARGUMENT, "grid");
    if (n == 0) return HIPR_OK;
    if (coat_classes) {      // the kernel reads one class byte per surface hit: every id must name a triangle of the resident scene
        if (!c->scene.ready || !c->scene.triangle_class.ptr) return fail(HIPR_ERROR_NOT_READY, "no scene uploaded");
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t id;
            std::memcpy(&id, hits_n4 + 4 * size_t(i) + 3, 4);
            if (id != HIPR_HIT_MISS && !(id & HIPR_HIT_LIGHT) && id >= c->scene.args.triangle_count) return fail(HIPR_ERROR_INVALID_ARGUMENT, "a hit names a triangle the scene does not hold");
        }
    }
    if (int s = drain(c)) return s;
    DeviceBuffer bh, bc, bo;
    if (bh.upload(hits_n4, size_t(n) * 16, c->stream) | bc.upload(&n, 4, c->stream) | bo.resize(size_t(n) * 4)) return HIPR_ERROR_OUT_OF_MEMORY;
    HIP_TRY(hipMemsetAsync(bo.ptr, 0xFF, size_t(n) * 4, c->stream));      // a place the pass leaves out shows as 0xFFFFFFFF
    classify_hits(c, c->stream, bh.as<float4>(), bc.as<uint32_t>(), n, bo.as<uint32_t>(), coat_classes != 0, grid);
    HIP_TRY(hipGetLastError());
    if (int finish_status = finish_all(c)) return finish_status;
    HIP_TRY(hipMemcpy(out_order, bo.ptr, size_t(n) * 4, hipMemcpyDeviceToHost));
    return HIPR_OK;
}

// Both of the above in ONE fused launch, as a bounce of a pass makes it for the scenes of the persistent kernels: the closest-hit rays first, the shadow rays behind
// them in one index space. Same ray layouts as the two entries above; either queue may be empty.
int hipr_debug_trace_fused(HiprContext* c, const float* closest_rays, const uint32_t* skip, uint32_t n_closest, const float* shadow_rays, uint32_t n_shadow, float* out_hits,
                           float* out_transmittance) {
    if (int s = check_context(c)) return s;
    if (!c->scene.ready) return fail(HIPR_ERROR_NOT_READY, "no scene uploaded");
    if ((n_closest && (!closest_rays || !out_hits)) || (n_shadow && (!shadow_rays || !out_transmittance))) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null argument");
    if (n_closest > 0x7FFFFFFFu || n_shadow > 0x7FFFFFFFu) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_trace_fused: more than 2^31 rays of a kind");
    if (!c->use_persistent()) return fail(HIPR_ERROR_UNSUPPORTED, "a fused trace launch needs a persistent kernel");
    if (n_closest + n_shadow == 0) return HIPR_OK;
    if (int s = drain(c)) return s;      // as in hipr_debug_trace_closest
    const size_t nc = std::max(n_closest, 1u), ns = std::max(n_shadow, 1u);      // an empty queue still has its buffers
    std::vector<float> o(nc * 4, 0.0f), d(nc * 4, 0.0f), so(ns * 4, 0.0f), sd(ns * 4, 0.0f), rad(ns * 4, 0.0f), ones(ns * 4, 1.0f);
    std::vector<uint32_t> meta(nc * 2, 0u);
    if (n_closest) debug_prepare_rays(closest_rays, n_closest, o, d);
    for (uint32_t i = 0; i < n_closest; ++i) { meta[2 * i] = i; meta[2 * i + 1] = skip ? skip[i] : HIPR_NO_TRIANGLE; }
    for (uint32_t i = 0; i < n_shadow; ++i) {
        std::memcpy(&so[4 * i], shadow_rays + 8 * size_t(i), 12);
        so[4 * i + 3] = shadow_rays[8 * size_t(i) + 7];       // tmax
        std::memcpy(&sd[4 * i], shadow_rays + 8 * size_t(i) + 4, 12);
        std::memcpy(&sd[4 * i + 3], &i, 4);                   // slot
    }
    const uint32_t counts[2] = {n_closest, n_shadow};
    DeviceBuffer bo, bd, bm, bh, bso, bsd, br, bacc, bc;
    int r = bo.upload(o.data(), o.size() * 4, c->stream) | bd.upload(d.data(), d.size() * 4, c->stream) | bm.upload(meta.data(), meta.size() * 4, c->stream) | bh.resize(nc * 16) |
            bso.upload(so.data(), so.size() * 4, c->stream) | bsd.upload(sd.data(), sd.size() * 4, c->stream) | br.upload(ones.data(), ones.size() * 4, c->stream) |
            bacc.upload(rad.data(), rad.size() * 4, c->stream) | bc.upload(counts, 8, c->stream);
    if (r) return HIPR_ERROR_OUT_OF_MEMORY;
    HIP_TRY(hipMemsetAsync(c->counters.ptr, 0, sizeof(DeviceCounters), c->stream));
    PathState in = {bo.as<float4>(), bd.as<float4>(), nullptr, bm.as<uint2>()};
    Wavefront w;
    w.stream = c->stream;
    w.hits = std::move(bh);
    w.shadow[0] = std::move(bso); w.shadow[1] = std::move(bsd); w.shadow[2] = std::move(br);
    std::swap(c->radiance, bacc);      // the launch writes the context's radiance buffer: this call's, for its duration
    trace_rays<TRACE_FUSED>(c, w, {in, bc.as<uint32_t>(), bc.as<uint32_t>() + 1, n_closest + n_shadow});
    std::swap(c->radiance, bacc);
    if (int finish_status = finish_all(c)) return finish_status;
    if (n_closest) HIP_TRY(hipMemcpy(out_hits, w.hits.ptr, size_t(n_closest) * 16, hipMemcpyDeviceToHost));
    if (n_shadow) {
        std::vector<float> result(size_t(n_shadow) * 4);
        HIP_TRY(hipMemcpy(result.data(), bacc.ptr, result.size() * 4, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n_shadow; ++i) out_transmittance[i] = result[4 * i];
    }
    c->total = {};
    c->total.closest_rays = n_closest;
    c->total.shadow_rays = n_shadow;
    return HIPR_OK;
}

} // extern "C"
