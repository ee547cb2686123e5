// ShadeScheduleHost.hip -- the batch schedule of the shade kernel (csrc/shade_schedule.h), compiled for the HOST by hipcc's host pass
// (tests/native/libshade_schedule_host.so).
//
// Test infrastructure (tests/test_shade_schedule_cpu.py); nothing here is linked into or loaded by the product, which has no CPU path.
//
// shade_batch and shade_rounds are __host__ __device__ functions of 32-bit integer arithmetic: the x86 build runs exactly the statements k_shade runs.
#include <hip/hip_runtime.h>

#include "../../bifrost3d_amd/csrc/shade_schedule.h"

using namespace hipr;

extern "C" {

// The whole schedule of a launch: out[block * rounds + round] = the batch the block takes in that round (0xFFFFFFFF: none), for every block of `grid` and every
// round below `rounds`; rounds_of_block[block] = shade_rounds, the rounds the kernel's loop runs for the block.
void shade_schedule_host(uint32_t grid, uint32_t batches, uint32_t rounds, uint32_t* out, uint32_t* rounds_of_block) {
    for (uint32_t block = 0; block < grid; ++block) {
        rounds_of_block[block] = shade_rounds(block, grid, batches);
        for (uint32_t round = 0; round < rounds; ++round) out[size_t(block) * rounds + round] = shade_batch(block, round, grid, batches);
    }
}

uint32_t shade_schedule_host_chunk_batches() { return SHADE_CHUNK_BATCHES; }
uint32_t shade_schedule_host_xcds() { return SHADE_XCDS; }

}
