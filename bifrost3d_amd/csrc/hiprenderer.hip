// hiprenderer.hip -- implementation of the C-ABI declared in include/hiprenderer_c.h: the context and the render pass. The scene a context holds -- its checks,
// its upload and every edit of it on the device -- is scene.hip's; context.h is what the two units share.
//
// Host side of the MI355X wavefront path tracer: owns the SoA
// path / hit / shadow queues and the f64 accumulation buffer, and drives the per-pass kernel loop
//   generate -> { trace_closest -> shade(+compact) -> trace_shadow } until no path is alive -> accumulate.
// Replaces the OptiX context + context->launch() of OR/Renderer.cpp:273-574,1250-1265.
// A pass (hipr_trace_pass) is begin_pass, start_wavefront for each wavefront, advance_wavefront round robin until none is left (or detach_tail, pipelined);
// a bounce is enqueue_bounce = launch_trace + launch_shade + the read-back of its sizes, and book_bounce keeps the counters of all of them. What tunes a
// context is in Knobs; drain() is where every queued pass has ended, on the device and in the books.
// There is no CPU fallback: every entry point that needs the GPU fails with a status code.
#ifndef HIPR_WIDE8_LOW_BUCKET
#define HIPR_WIDE8_LOW_BUCKET 0
#endif
#include "context.h"

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

} // namespace

int hipr::fail(int status, const char* fmt, ...) {
    char buf[512];
    va_list args;
    va_start(args, fmt);
    vsnprintf(buf, sizeof(buf), fmt, args);
    va_end(args);
    g_last_error = buf;
    fprintf(stderr, "hiprenderer: %s\n", buf);
    return status;
}

namespace {

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

uint32_t grid_for(uint32_t items, uint32_t block, uint32_t max_blocks) {
    uint32_t blocks = (items + block - 1) / block;
    blocks = std::max(1u, std::min(blocks, max_blocks));
    return (blocks + 7u) & ~7u;   // multiple of 8: xcd_chunk() needs every XCD to own the same number of chunks
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
    uint32_t* hints = nullptr;          // the launch's hint table (wide8_kernels.h): one word per 64 entries of `in` (closest-only) or per 64 radiance slots (the others); nullptr: no hints
};

// Every instantiation of a kernel family has the family's type: picking a kernel is picking a pointer.
using Wide8Kernel = void (*)(DeviceScene, Wide8Scene, PathState, float4*, ShadowQueue, float4*, const uint32_t*, const uint32_t*, uint32_t*, int, DeviceCounters*, const uint32_t*, uint32_t*);
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
                       work.closest_count, work.shadow_count, p.work_counter, c->knobs.refill_below, c->counters.as<DeviceCounters>(), work.sorted,
                       INSTRUMENT || work.sorted ? nullptr : work.hints);      // the counting and the sorted instantiations have no code for hints: their counters and order are the oracle's
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

// The hint tables of the trace launches (wide8_kernels.h) start empty: an all-zero word names no tree. Called where nothing is queued: when the slots are partitioned
// (new buffers, and entries that stand for other pixels) and when the scene's tree generation has wrapped (begin_pass).
int clear_hint_tables(HiprContext* c) {
    for (Wavefront& w : c->wavefronts) if (w.camera_hints.ptr) HIP_TRY(hipMemsetAsync(w.camera_hints.ptr, 0, w.camera_hints.bytes, c->stream));
    if (c->occluder_hints.ptr) HIP_TRY(hipMemsetAsync(c->occluder_hints.ptr, 0, c->occluder_hints.bytes, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));      // the wavefronts' own streams are not ordered behind the context's
    c->hint_wraps_seen = c->scene.hint_wraps;
    return HIPR_OK;
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
            w.hits.release(); w.order.release(); w.nee_flags.release(); w.camera_hints.release();
            w.sort_keys[0].release(); w.sort_keys[1].release(); w.sort_order.release(); w.sort_temp.release();
            for (DeviceBuffer& b : w.shadow) b.release();
            continue;
        }
        for (int i = 0; i < 2; ++i) for (int j = 0; j < 4; ++j) r |= w.path[i][j].resize(j == 3 ? bytes / 2 : bytes);      // [3]: the 8-byte meta records
        r |= w.hits.resize(bytes);
        r |= w.order.resize(bytes / 4);
        r |= w.camera_hints.resize(bytes / 16 / 64 * sizeof(uint32_t));      // one word per 64 queue entries (bytes / 16 entries, a multiple of 64)
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
    r |= c->occluder_hints.resize(std::max<uint64_t>(slots, 64u) / 64u * sizeof(uint32_t));      // one word per 64 radiance slots
    return r ? r : clear_hint_tables(c);
}

void set_frame_divisors(FrameInfo& f) { f.by_samples_per_pass = make_divisor(f.samples_per_pass); f.by_tiles_x = make_divisor(f.tiles_x); }

} // namespace

int hipr::check_context(HiprContext* c) {
    if (!c) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null context");
    HIP_TRY(hipSetDevice(c->device));
    return HIPR_OK;
}

namespace {

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
    // Hints (wide8_kernels.h): the camera rays start on the record their pixel's samples hit in the last pass, the shadow rays shade(0) queued on the record that
    // stopped their pixel's last. From bounce 1 on (closest hits) and bounce 2 on (shadow rays) neighbouring entries have nothing in common any more: measured
    // worthless there (profiles/ab_trace_hints.txt section 0), so those launches get no table.
    const bool hinted = c->use_wide8();
    if (k > 0 && fused) trace_rays<TRACE_FUSED>(c, w, {w.path_state(parity), in_count, shadow_in, 2u * bound, nullptr, hinted && k == 1 ? c->occluder_hints.as<uint32_t>() : nullptr});
    else trace_rays<TRACE_CLOSEST>(c, w, {w.path_state(parity), in_count, nullptr, bound, nullptr, hinted && k == 0 ? w.camera_hints.as<uint32_t>() : nullptr});
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

} // namespace

// Every pass queued so far is complete on the device and in the books (the entry points that read results, change the frame or the scene, or collect
// timings start here).
int hipr::finish_all(HiprContext* c) {
    for (int slot = 0; slot < 2; ++slot)
        if (int s = finish_slot(c, slot)) return s;
    for (int g = 0; g < MAX_WAVEFRONTS; ++g) if (c->wavefronts[g].stream) HIP_TRY(hipStreamSynchronize(c->wavefronts[g].stream));
    HIP_TRY(hipStreamSynchronize(c->copy_stream));
    return HIPR_OK;
}

namespace {

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
    if (c->hint_wraps_seen != c->scene.hint_wraps)      // the tree generation started over: an old entry could carry a new tree's tag. A scene writer has drained every pass since.
        if (int s = clear_hint_tables(c)) return s;
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

// The launches of the three entries above over the 8-wide tree, each GIVEN A HINT TABLE (wide8_kernels.h): `mode` 0 = closest-only (n_shadow must be 0; the table is
// keyed by ray index / 64), 1 = shadow-only (n_closest must be 0), 2 = fused (both keyed by shadow ray index / 64: the radiance slot of ray i is i). `hints` holds
// `hint_words` words -- at least one per 64 rays of the keyed kind -- that the launch reads and writes; they are returned as the launch left them. An entry that carries the
// resident tree's tag (*out_tag, when asked for) must name a leaf record: anything else in such an entry is refused here, since the kernel would read a node as a record.
int hipr_debug_trace_hinted(HiprContext* c, int mode, const float* closest_rays, const uint32_t* skip, uint32_t n_closest, const float* shadow_rays, uint32_t n_shadow, uint32_t* hints,
                            uint32_t hint_words, float* out_hits, float* out_transmittance, uint32_t* out_tag) {
    if (int s = check_context(c)) return s;
    if (!c->scene.ready) return fail(HIPR_ERROR_NOT_READY, "no scene uploaded");
    if (!c->use_wide8()) return fail(HIPR_ERROR_UNSUPPORTED, "hipr_debug_trace_hinted: hints are the 8-wide kernel's");
    const uint32_t tag = c->scene.wide8.hint_tag;
    if (out_tag) *out_tag = tag;
    if (mode < 0 || mode > 2 || (mode == TRACE_CLOSEST && n_shadow) || (mode == TRACE_SHADOW && n_closest)) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_trace_hinted: mode %d with %u + %u rays", mode, n_closest, n_shadow);
    if ((n_closest && (!closest_rays || !out_hits)) || (n_shadow && (!shadow_rays || !out_transmittance))) return fail(HIPR_ERROR_INVALID_ARGUMENT, "null argument");
    if (n_closest > 0x7FFFFFFFu || n_shadow > 0x7FFFFFFFu) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_trace_hinted: more than 2^31 rays of a kind");
    if (n_closest + n_shadow == 0) return HIPR_OK;
    const uint32_t keyed = mode == TRACE_CLOSEST ? n_closest : n_shadow;
    if (!hints || uint64_t(hint_words) * 64u < keyed) return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_trace_hinted: %u hint words for %u rays", hint_words, keyed);
    if (int s = drain(c)) return s;
    {      // which slots are leaf records: the refit's list (made at upload and by every tree install)
        std::vector<uint32_t> leaves(c->scene.refit_leaf_count);
        if (!leaves.empty()) HIP_TRY(hipMemcpy(leaves.data(), c->scene.refit_leaf_slots.ptr, leaves.size() * 4, hipMemcpyDeviceToHost));
        std::vector<bool> is_record(c->scene.wide8.slot_count, false);
        for (uint32_t slot : leaves) if (slot < is_record.size()) is_record[slot] = true;
        for (uint32_t i = 0; i < hint_words; ++i)
            if ((hints[i] ^ tag) < (1u << 24) && ((hints[i] & 0xFFFFFFu) >= is_record.size() || !is_record[hints[i] & 0xFFFFFFu]))
                return fail(HIPR_ERROR_INVALID_ARGUMENT, "hipr_debug_trace_hinted: entry %u carries the tree's tag and names slot %u, which is no leaf record", i, hints[i] & 0xFFFFFFu);
    }
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
    DeviceBuffer bo, bd, bm, bh, bso, bsd, br, bacc, bc, bhints;
    int r = bo.upload(o.data(), o.size() * 4, c->stream) | bd.upload(d.data(), d.size() * 4, c->stream) | bm.upload(meta.data(), meta.size() * 4, c->stream) | bh.resize(nc * 16) |
            bso.upload(so.data(), so.size() * 4, c->stream) | bsd.upload(sd.data(), sd.size() * 4, c->stream) | br.upload(ones.data(), ones.size() * 4, c->stream) |
            bacc.upload(rad.data(), rad.size() * 4, c->stream) | bc.upload(counts, 8, c->stream) | bhints.upload(hints, size_t(hint_words) * 4, c->stream);
    if (r) return HIPR_ERROR_OUT_OF_MEMORY;
    HIP_TRY(hipMemsetAsync(c->counters.ptr, 0, sizeof(DeviceCounters), c->stream));
    PathState in = {bo.as<float4>(), bd.as<float4>(), nullptr, bm.as<uint2>()};
    Wavefront w;
    w.stream = c->stream;
    w.hits = std::move(bh);
    w.shadow[0] = std::move(bso); w.shadow[1] = std::move(bsd); w.shadow[2] = std::move(br);
    std::swap(c->radiance, bacc);      // the launch writes the context's radiance buffer: this call's, for its duration
    if (mode == TRACE_CLOSEST) trace_rays<TRACE_CLOSEST>(c, w, {in, bc.as<uint32_t>(), nullptr, n_closest, nullptr, bhints.as<uint32_t>()});
    else if (mode == TRACE_SHADOW) trace_rays<TRACE_SHADOW>(c, w, {PathState{}, nullptr, bc.as<uint32_t>() + 1, n_shadow, nullptr, bhints.as<uint32_t>()});
    else trace_rays<TRACE_FUSED>(c, w, {in, bc.as<uint32_t>(), bc.as<uint32_t>() + 1, n_closest + n_shadow, nullptr, bhints.as<uint32_t>()});
    std::swap(c->radiance, bacc);
    if (int finish_status = finish_all(c)) return finish_status;
    if (n_closest) HIP_TRY(hipMemcpy(out_hits, w.hits.ptr, size_t(n_closest) * 16, hipMemcpyDeviceToHost));
    if (n_shadow) {
        std::vector<float> result(size_t(n_shadow) * 4);
        HIP_TRY(hipMemcpy(result.data(), bacc.ptr, result.size() * 4, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n_shadow; ++i) out_transmittance[i] = result[4 * i];
    }
    HIP_TRY(hipMemcpy(hints, bhints.ptr, size_t(hint_words) * 4, hipMemcpyDeviceToHost));
    c->total = {};
    c->total.closest_rays = n_closest;
    c->total.shadow_rays = n_shadow;
    return HIPR_OK;
}

} // extern "C"
