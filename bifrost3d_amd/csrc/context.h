// context.h -- what the two host units of the renderer share: the context (HiprContext) with the types its members are of, and the few functions
// one unit calls in the other. hiprenderer.hip is the render pass and everything about a context that is not its scene; scene.hip is the resident scene
// (ResidentScene) with its checks, its device edits and the device tree builds. Internal: not installed, included by those two units only.
// The types live in namespace hipr, not in an unnamed one: HiprContext is ONE type in both units only if its members' types are.
#pragma once

#include "kernels.h"
#include "wide8_kernels.h"
#include "launch.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <vector>

namespace hipr {

// Sets the calling thread's hipr_last_error() message, prints it and returns `status`. Defined once, in hiprenderer.hip, next to the message it sets.
int fail(int status, const char* fmt, ...);

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
inline hipError_t free_pinned_words(uint32_t* words) { return hipHostFree(words); }
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
using PinnedWords = Owned<uint32_t*, free_pinned_words>;
// Each leaves the owner empty when HIP refuses: the caller checks the handle.
inline Stream make_stream() { Stream s; if (hipStreamCreateWithFlags(&s.handle, hipStreamNonBlocking) != hipSuccess) s.handle = nullptr; return s; }
inline Event make_event(unsigned flags = hipEventDisableTiming) { Event e; if (hipEventCreateWithFlags(&e.handle, flags) != hipSuccess) e.handle = nullptr; return e; }
inline PinnedWords make_pinned_words(size_t count) { PinnedWords p; if (hipHostMalloc((void**)&p.handle, count * sizeof(uint32_t)) != hipSuccess) p.handle = nullptr; return p; }

struct TimedLaunch { int kernel; hipEvent_t start, stop; };

// One independent wavefront of paths: its own queues, queue sizes and stream. A pass splits its path slots over the
// context's wavefronts; they advance through their bounces independently, so while one of them shades (few resident
// waves, waiting on gathers) the other one traces (many waves, latency bound) on the same CUs.
struct Wavefront {
    Stream own_stream;                  // first member: destroyed after the events and buffers below
    hipStream_t stream = nullptr;       // borrowed: wavefront 0 runs on the context stream, the others on their own
    Event shade_done[2], counts_copied[2], finished;   // by bounce parity: two bounces are in flight
    DeviceBuffer path[2][4], hits, shadow[3], queue_counts, order, nee_flags, sort_keys[2], sort_order, sort_temp;     // sort_*: ray_sort.hip (HIPR_COHERENCE_SORT=1)   // queue_counts: COUNT_LINES 64 B lines (see there); order: k_classify_hits' listing of a bounce's rays
    DeviceBuffer camera_hints;          // the hint table of the wavefront's camera rays (wide8_kernels.h): one word per 64 queue entries, zeroed when the slots are partitioned
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
struct LightingScratch;      // below, with the other scratches
struct TexelScratch;
struct VertexScratch;
struct PoseScratch;

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
    // The generation of the 8-wide tree, 1 ... 255: wide8.hint_tag carries it in its top byte, and so does every entry of a hint table that names a record slot of
    // this tree (wide8_kernels.h hint_start). new_wide8_tree() is the one place that bumps it, called wherever the slot array is replaced or the kind of a slot can
    // change (upload_wide8: upload and geometry update, host adoption included; install_rebuilt_trees: device rebuild, instance edits, pool growth). A refit keeps the
    // kinds and the generation. hint_wraps counts the times the generation started over: the context clears its tables before the next pass (begin_pass).
    uint32_t hint_generation = 0, hint_wraps = 0;
    void new_wide8_tree() {
        if (++hint_generation > 255u) { hint_generation = 1u; ++hint_wraps; }
        wide8.hint_tag = hint_generation << 24;
    }
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
    // The device work of hipr_update_scene_lighting, which has checked its arguments against the host copies (hipr_internal_check_lighting_update): the light list
    // replaced, the environment kept, removed or rebuilt from the resident texels (environment_build.h).
    int update_lighting(const HiprLight* new_lights, uint32_t light_count, int environment_action, const HiprEnvironmentBuild* build, float* out_per_pixel_PDF, HiprLightSample* out_samples,
                        LightingScratch& scratch, hipStream_t stream, HiprLightingResult* out);
    // The device work of hipr_update_scene_texels, which has checked every rectangle against uploaded_textures (hipr_internal_check_texel_update): the rectangles
    // written into the texel pool and the flags that follow texels decided again (texel_update.h).
    int update_texels(const HiprTexelEdit* edits, uint32_t edit_count, TexelScratch& scratch, hipStream_t stream, HiprTexelUpdateResult* out);
    // The device work of hipr_update_scene_vertices, which has checked every range against the host copies (hipr_internal_check_vertex_update): the ranges written
    // into the vertex pools and everything an upload derives from vertex data brought along (vertex_update.h).
    int update_vertices(const HiprVertexEdit* edits, uint32_t edit_count, VertexScratch& scratch, hipStream_t stream, HiprVertexUpdateResult* out);
    // The rigs hipr_set_scene_rigs bound (vertex_pose.h): a record per rig and the rest data of all of them on the device, and the host's book the poses are checked
    // against. upload() drops them; every other writer keeps them (none moves a pool vertex).
    DeviceBuffer rig_records, rig_data;
    struct Rig { uint32_t first_vertex, vertex_count, joint_count, target_count, flags; };      // vertex_pose.h RigBook, which this unit's includes do not reach: scene.hip asserts the layout
    std::vector<Rig> rigs;
    uint32_t pose_lds_joints = 32;      // POSE_LDS_JOINTS (scene.hip asserts it); hipr_debug_set_pose_lds_joints sets it
    // The device work of hipr_set_scene_rigs, which has checked the list (check_rig_descs): the new set allocated and copied, then the old one let go.
    int set_rigs(const HiprRigDesc* descs, uint32_t count, hipStream_t stream);
    // The device work of hipr_pose_scene_rigs, which has checked the poses (hipr_internal_check_rig_poses): the pose kernel, then queue_refit_of_marked and finish_vertex_writes.
    int pose_rigs(const HiprRigPose* poses, uint32_t pose_count, PoseScratch& scratch, VertexScratch& vertex_scratch, hipStream_t stream, HiprVertexUpdateResult* out);
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
    // What follows writes into the geometry pool whose vertices are marked in `marks` (a byte per pool vertex), shared by update_vertices and pose_rigs: the moved
    // triangles (words[VERTEX_WORD_MOVED]) with the bounds, the grid and the refit of the tree, queued on the stream after ONE synchronise for the bounds.
    int queue_refit_of_marked(const uint8_t* marks, uint32_t* words, float* grid_min, float* grid_cell, hipStream_t stream);
    // ... and the end of both calls once everything is queued: the read-backs, the state refit_transforms leaves, `out` filled. all-opaque and the two counts of the
    // flag pass are the caller's (decides_flags false: none ran).
    int finish_vertex_writes(bool moves, bool decides_flags, const uint32_t* device_words, const float* grid_min, const float* grid_cell, hipStream_t stream, HiprVertexUpdateResult* out);
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

// The device scratch of the tree builds. Up to KEEP_BYTES (a build of a quarter of a million triangles) a scratch stays with the context and the next build reuses
// it; a larger build gives its scratch back when it returns, whatever its outcome -- 2.4 GB at 10 M triangles are not held on a shared device between two edits
// that are seconds apart at best. Each scratch is judged alone. BUFFERS is a struct of DeviceBuffers and of nothing else (the books of a scratch stand in the
// struct derived from this one): the struct itself is then the list of what is summed and given back, and a buffer added to it cannot be forgotten there.
template <typename BUFFERS>
struct Scratch : BUFFERS {
    static constexpr size_t KEEP_BYTES = size_t(128) << 20;
    static_assert(std::is_standard_layout<BUFFERS>::value && sizeof(BUFFERS) % sizeof(DeviceBuffer) == 0 && alignof(BUFFERS) == alignof(DeviceBuffer), "a scratch's buffers are DeviceBuffers only");
    void release_if_large() {
        DeviceBuffer* const all = reinterpret_cast<DeviceBuffer*>(static_cast<BUFFERS*>(this));
        const size_t count = sizeof(BUFFERS) / sizeof(DeviceBuffer);
        size_t total = 0;
        for (size_t i = 0; i < count; ++i) total += all[i].bytes;
        if (total > KEEP_BYTES) for (size_t i = 0; i < count; ++i) all[i].release();
    }
};
// Gives a large build's scratch back on every way out of the call that holds it.
template <typename SCRATCH>
struct ScratchGuard {
    SCRATCH& scratch;
    explicit ScratchGuard(SCRATCH& held) : scratch(held) {}
    ~ScratchGuard() { scratch.release_if_large(); }
};

// The device scratch of hipr_build_bvh2 (bvh2_build.h), about 240 B per triangle.
struct BuildBuffers { DeviceBuffer triangles, boxes, centroids, order, seg, order_tmp, seg_tmp, ranges[2], acc, setup, split, scan_local, block_sums, nodes, sizes, place, out_nodes, status; };
struct BuildScratch : Scratch<BuildBuffers> {
    double validate_ms = 0.0, upload_ms = 0.0, kernel_ms = 0.0, readback_ms = 0.0;      // of the last build
    uint32_t levels = 0;
};

// The device scratch of hipr_build_wide8 (wide8_build.h): the input (48 B per triangle, 64 B per BVH2 node), about 170 B per record for the tree, its
// tables and the records, 68 B per wide node and the slots.
struct CollapseBuffers {
    DeviceBuffer nodes, triangles, order, level_nodes, counts, block_sums, partial, bounds, box, left, right, cost, split, roots_used, records, record_slot, wide_tree, wide_child, wide_all, wide_size,
        wide_base, wide_slot, slots, status;
};
struct CollapseScratch : Scratch<CollapseBuffers> {
    double validate_ms = 0.0, upload_ms = 0.0, kernel_ms = 0.0, readback_ms = 0.0;      // of the last collapse
};

// The device scratch of hipr_build_wide4 (wide4_build.h): the input (64 B per BVH2 node and its place in the level lists), a word of binary_need per node, and per wide
// node -- at most one per BVH2 node -- 20 B of frontier and layout words and the node twice, in frontier order and in place.
struct Collapse4Buffers { DeviceBuffer nodes, level_nodes, need, wide_root, wide_budget, made, wide_size, wide_stack, wide_at, out, status; };
struct Collapse4Scratch : Scratch<Collapse4Buffers> {
    double validate_ms = 0.0, upload_ms = 0.0, kernel_ms = 0.0, readback_ms = 0.0;      // of the last collapse
};

// What hipr_rebuild_scene_trees needs beside the two builds' scratch (scene_rebuild.h): 9 B per triangle and a word per instance and BVH2 node. The
// flat triangle array itself is BuildScratch::triangles, where hipr_build_bvh2 keeps its input.
struct RebuildBuffers {
    DeviceBuffer flat_class, claim, instance_counts, first, level_nodes, status;
    DeviceBuffer old_to_new, created, created_first, instances;      // hipr_edit_scene_instances (instance_edit.h): a word or a record per instance
};
struct RebuildScratch : Scratch<RebuildBuffers> {
    double flatten_ms = 0.0, bvh2_ms = 0.0, collapse_ms = 0.0, install_ms = 0.0, readback_ms = 0.0;      // of the last rebuild
};

// The device scratch of hipr_update_scene_lighting's environment build (environment_build.h): the three tables, then per PDF texel the importance, its blurred
// copy and the conditional sums (a word more per row) -- about three PDF images -- and a few words per row.
struct LightingBuffers { DeviceBuffer row_sines, srgb_decode, draw_points, importance, blurred, conditional, marginal_raw, marginal, totals, integral; };
struct LightingScratch : Scratch<LightingBuffers> {
    double upload_ms = 0.0, kernel_ms = 0.0, finish_ms = 0.0, readback_ms = 0.0;      // of the last lighting update
    Event events[4];                    // around the kernels before and after the integral is read; made by the first build
};

// The device scratch of hipr_update_scene_texels (texel_update.h): the rectangles' rows packed, a word per instance and the flag pass's few words.
struct TexelBuffers { DeviceBuffer staging, touched, words; };
struct TexelScratch : Scratch<TexelBuffers> {
    double staging_ms = 0.0, write_ms = 0.0, coverage_ms = 0.0, leaf_ms = 0.0;      // of the last texel update
    Event events[4];                    // around the rectangle writes, the flag pass and the leaf pass; made by the first update
};

// The device scratch of hipr_update_scene_vertices (vertex_update.h): the segment table, a word per instance and the ranges' rows packed, a byte per pool vertex
// for each kind of mark, and the passes' few words.
struct VertexBuffers { DeviceBuffer staging, marks_geometry, marks_texcoords, words; };
struct VertexScratch : Scratch<VertexBuffers> {
    double staging_ms = 0.0, write_ms = 0.0, refit_ms = 0.0, flag_ms = 0.0;      // of the last vertex update
    Event events[4];                    // around the pool writes, the refit passes with the records, the flag pass with the leaf pass; made by the first update
};

// The device scratch of hipr_pose_scene_rigs (vertex_pose.h): the block table, the calls, the matrices and the target weights packed. The marks and the passes'
// words are the vertex update's (VertexScratch): the continuation is shared.
struct PoseBuffers { DeviceBuffer staging; };
struct PoseScratch : Scratch<PoseBuffers> {
    double staging_ms = 0.0, pose_ms = 0.0, refit_ms = 0.0;      // of the last pose
    Event events[3];                    // around the pose kernel, the refit passes with the records; made by the first pose
};

// The context; HiprContext, the C-ABI's opaque type, is this and nothing else.
struct Context {
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
    DeviceBuffer occluder_hints;        // the hint table of the shadow rays shade(0) queues (wide8_kernels.h): one word per 64 radiance slots, zeroed when the slots are partitioned
    uint32_t hint_wraps_seen = 0;       // ResidentScene::hint_wraps when the hint tables were last cleared
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
    Collapse4Scratch collapse4;         // hipr_build_wide4; likewise
    RebuildScratch rebuild;             // hipr_rebuild_scene_trees, which also runs over the two above
    LightingScratch lighting;           // hipr_update_scene_lighting's environment build
    TexelScratch texel_update;          // hipr_update_scene_texels
    VertexScratch vertex_update;        // hipr_update_scene_vertices
    PoseScratch vertex_pose;            // hipr_pose_scene_rigs

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

} // namespace hipr

struct HiprContext : hipr::Context {};

namespace hipr {

// hiprenderer.hip, for the entry points of scene.hip: the context is there and its device current; every pass queued so far is complete on the device and in the books.
int check_context(HiprContext* c);
int finish_all(HiprContext* c);

} // namespace hipr
