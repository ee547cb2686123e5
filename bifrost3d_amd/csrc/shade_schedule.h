// shade_schedule.h -- which batch of a bounce's shading order a persistent block of k_shade takes in which round (shade_kernel.h).
//
// The listing pass (kernels.h k_classify_hits) orders the queue entries CHUNK by chunk: places [c * 4096, (c + 1) * 4096) of `order` hold chunk c's own entries as
// [plain surface hits | coated surface hits | everything else]. A batch is 256 consecutive places, a chunk 16 batches. The entries of a chunk share their queue
// lines -- the kinds are interleaved entry by entry, a 128 B line holds 8 or 16 records -- so every line of a chunk is wanted by its hit batches AND by its other
// batches. The schedule below lets all 16 batches of a chunk be taken by blocks of ONE XCD (one L2), in the same round or the next: the second reader of a line
// finds it in that L2 instead of fetching it again.
//
// Blocks are dealt to the eight XCDs round robin (block b runs on XCD b % 8; the trace kernel's shard start relies on the same). Chunk c belongs to XCD c % 8. The
// batches of an XCD's chunks, in chunk order, are dealt in order to its blocks: place s = round * (grid / 8) + block / 8 of that sequence is batch s % 16 of the
// XCD's chunk s / 16. Inside a chunk the batches are rotated by the round the chunk starts in: with grid / 8 a multiple of 16 a block would otherwise take the same
// batch of every chunk it meets -- always hits (thousands of instructions) or always others (tens) -- and the blocks of the cheap batches would leave the rest behind.
// Grids that are no multiple of 8 (or hold fewer than 8 blocks) take the batches with the plain grid stride. The host sizes every launch to a multiple of 8 blocks
// (hiprenderer.hip grid_for), so a listed bounce of a pass always takes the schedule by XCD.
//
// A chunk is the unit that is dealt to the XCDs: a bounce of fewer than 8 chunks (32 768 rays) leaves the blocks of whole XCDs without a batch, and one of a few
// dozen chunks loads the XCDs unevenly by a chunk, where the plain stride gave every block its share. The listing starts at 2^18 rays per bounce (64 chunks;
// hiprenderer.hip shade_ordered_from), where that is a sixth of a round at most; HIPR_SHADE_ORDERED_FROM set lower buys the listing of small bounces at that price.
//
// Pure 32-bit integer arithmetic (a queue holds fewer than 2^32 entries, so every place and batch index stays below 2^25), host and device: tests/native/ShadeScheduleHost.hip compiles it for the CPU suite (tests/test_shade_schedule_cpu.py).
#pragma once

#include <cstdint>

// A macro of this header's own: device_math.h's HD is device-only in the product's units and must not be decided here by the order of two includes.
#define SHADE_SCHEDULE_HD __host__ __device__ __forceinline__

namespace hipr {

constexpr uint32_t SHADE_XCDS = 8;                   // XCDs of the device; blocks are dealt to them round robin
constexpr uint32_t SHADE_CHUNK_BATCHES = 16;         // batches of a listing chunk: CLASSIFY_ROUNDS * 256 / SHADE_BLOCK (asserted in kernels.h)
constexpr uint32_t SHADE_NO_BATCH = 0xFFFFFFFFu;

SHADE_SCHEDULE_HD bool shade_schedule_by_xcd(uint32_t grid) { return grid >= SHADE_XCDS && grid % SHADE_XCDS == 0u; }

// The plain grid stride: batch round * grid + block.
SHADE_SCHEDULE_HD uint32_t shade_rounds_strided(uint32_t block, uint32_t grid, uint32_t batches) { return block < batches ? (batches - block + grid - 1u) / grid : 0u; }
SHADE_SCHEDULE_HD uint32_t shade_batch_strided(uint32_t block, uint32_t round, uint32_t grid, uint32_t batches) {
    const uint32_t b = round * grid + block;
    return b < batches ? b : SHADE_NO_BATCH;
}

// The rounds block `block` of `grid` runs over `batches` batches: every batch it takes lies in a round below this (a round below it may still hold none for the
// block: the rotated batches of the last, partial chunk), and no round from this on holds one.
SHADE_SCHEDULE_HD uint32_t shade_rounds(uint32_t block, uint32_t grid, uint32_t batches) {
    if (!shade_schedule_by_xcd(grid)) return shade_rounds_strided(block, grid, batches);
    const uint32_t per_xcd = grid / SHADE_XCDS, xcd = block % SHADE_XCDS, k = block / SHADE_XCDS;
    const uint32_t chunks = (batches + SHADE_CHUNK_BATCHES - 1u) / SHADE_CHUNK_BATCHES;
    const uint32_t places = xcd < chunks ? ((chunks - xcd + SHADE_XCDS - 1u) / SHADE_XCDS) * SHADE_CHUNK_BATCHES : 0u;      // of this XCD's sequence, the partial chunk counted whole
    return k < places ? (places - k + per_xcd - 1u) / per_xcd : 0u;
}

// The batch block `block` of `grid` takes in round `round`, of `batches` batches in all; SHADE_NO_BATCH for none. Over all blocks and rounds every batch comes exactly once.
SHADE_SCHEDULE_HD uint32_t shade_batch(uint32_t block, uint32_t round, uint32_t grid, uint32_t batches) {
    if (!shade_schedule_by_xcd(grid)) return shade_batch_strided(block, round, grid, batches);
    const uint32_t per_xcd = grid / SHADE_XCDS, xcd = block % SHADE_XCDS;
    const uint32_t place = round * per_xcd + block / SHADE_XCDS;
    const uint32_t local_chunk = place / SHADE_CHUNK_BATCHES;
    const uint32_t rotation = local_chunk * SHADE_CHUNK_BATCHES / per_xcd;      // the round the chunk starts in: a function of the chunk alone, so the 16 places still hold 16 different batches
    const uint32_t b = (local_chunk * SHADE_XCDS + xcd) * SHADE_CHUNK_BATCHES + (place + rotation) % SHADE_CHUNK_BATCHES;
    return b < batches ? b : SHADE_NO_BATCH;
}

} // namespace hipr
