"""The batch schedule of the shade kernel (csrc/shade_schedule.h: which batch of the shading order a persistent block of k_shade takes in which round) WITHOUT a GPU:
shade_batch and shade_rounds are __host__ __device__ functions of 32-bit integer arithmetic, compiled for the host by tests/native/ShadeScheduleHost.hip.

Every batch is taken exactly once, inside the rounds the kernel's loop runs; on grids that are multiples of 8 all 16 batches of a listing chunk go to blocks of one
XCD (the same blockIdx % 8), in the same round or two neighbouring rounds.

On that last property. An XCD of p blocks takes p batches of its sequence per round, and chunk number l of that sequence stands at places 16 l ... 16 l + 15 of it: it is
taken in rounds floor(16 l / p) ... floor((16 l + 15) / p), every one of them. The test holds every chunk to exactly those rounds, and the grids of the list to what
follows from them: grid 768 (96 blocks per XCD, a multiple of 16) ONE round; grid 96 (12 blocks) two neighbouring rounds, never more; grid 8 -- one block per XCD, which
takes one batch per round -- exactly 16 consecutive rounds, the fewest in which one block can take 16 batches at all. Grid 8 is the one grid of the list that cannot
meet "the same round or two neighbouring rounds"; the kernel's own grids hold 128 blocks or more."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

LIB_PATH = Path(__file__).resolve().parent / "native" / "libshade_schedule_host.so"
GRIDS = (1, 7, 8, 9, 96, 768, 771)
BATCH_COUNTS = (0, 1, 15, 16, 17, 1000, 5401)
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(str(LIB_PATH))
    lib.shade_schedule_host.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.shade_schedule_host.restype = None
    lib.shade_schedule_host_chunk_batches.restype = C.c_uint32
    lib.shade_schedule_host_xcds.restype = C.c_uint32
    return lib


def schedule(lib, grid, batches):
    """(grid, rounds) batch per block and round, with three rounds more than any block can need, and the rounds of the kernel's loop per block."""
    rounds = (batches + grid - 1) // grid + 16 + 3      # the plain stride's rounds, a chunk more for the XCD schedule's uneven deal, the kernel's look-ahead of two
    table = np.zeros((grid, rounds), np.uint32)
    loop = np.zeros(grid, np.uint32)
    up = C.POINTER(C.c_uint32)
    lib.shade_schedule_host(grid, batches, rounds, table.ctypes.data_as(up), loop.ctypes.data_as(up))
    return table, loop


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("batches", BATCH_COUNTS)
def test_every_batch_is_taken_exactly_once_inside_the_loop_of_its_block(lib, grid, batches):
    table, loop = schedule(lib, grid, batches)
    taken = table[table != NONE]
    assert np.array_equal(np.sort(taken), np.arange(batches, dtype=np.uint32))
    rounds = np.arange(table.shape[1])[None, :]
    assert (table[rounds >= loop[:, None]] == NONE).all()      # nothing at or behind the end of a block's loop (the look-ahead of two rounds reads there)
    assert loop.max(initial=0) < table.shape[1] - 2
    # rounds of a block's loop without a batch: only the places of the last, partial chunk that hold none (its batches are rotated, so they may lie among the others)
    idle = int(sum((table[block, :loop[block]] == NONE).sum() for block in range(grid)))
    chunk = lib.shade_schedule_host_chunk_batches()
    assert idle == ((-batches) % chunk if grid % 8 == 0 else 0)


ROUNDS_OF_A_WHOLE_CHUNK = {8: (16, 16), 96: (2, 2), 768: (1, 1)}      # grid: (fewest, most) rounds a chunk of 16 batches lies in


@pytest.mark.parametrize("grid", [g for g in GRIDS if g % 8 == 0])
@pytest.mark.parametrize("batches", BATCH_COUNTS)
def test_the_batches_of_a_chunk_go_to_one_xcd_in_neighbouring_rounds(lib, grid, batches):
    table, _ = schedule(lib, grid, batches)
    chunk, xcds = lib.shade_schedule_host_chunk_batches(), lib.shade_schedule_host_xcds()
    assert (chunk, xcds) == (16, 8)
    per_xcd = grid // xcds
    fewest, most = ROUNDS_OF_A_WHOLE_CHUNK[grid]
    blocks, rounds = np.nonzero(table != NONE)
    chunks = table[blocks, rounds] // chunk
    for c in range(-(-batches // chunk)):
        mine = chunks == c
        held = min(chunk, batches - c * chunk)
        assert mine.sum() == held
        assert len(set(blocks[mine] % xcds)) == 1 and blocks[mine][0] % xcds == c % xcds
        local = c // xcds                                      # the chunk's number in its XCD's sequence
        first, last = local * chunk // per_xcd, (local * chunk + chunk - 1) // per_xcd
        taken_in = set(rounds[mine].tolist())
        assert taken_in <= set(range(first, last + 1)), (c, sorted(taken_in), first, last)
        span = max(taken_in) - min(taken_in) + 1
        assert span <= most, (c, span)
        if held == chunk:                                      # a whole chunk: every round of its stretch, no gap
            assert taken_in == set(range(first, last + 1)) and fewest <= span <= most, (c, sorted(taken_in))
        if grid >= 96:
            assert span <= 2                                   # the same round or two neighbouring ones


@pytest.mark.parametrize("grid", [g for g in GRIDS if g % 8 != 0])
def test_other_grids_take_the_plain_stride(lib, grid):
    table, loop = schedule(lib, grid, 1000)
    for block in range(grid):
        expected = np.arange(block, 1000, grid, dtype=np.uint32)
        assert loop[block] == len(expected) and np.array_equal(table[block, :len(expected)], expected)


def test_a_block_meets_every_batch_of_a_chunk_in_turn(lib):
    """With 96 blocks per XCD (grid 768) a block stands at the same place of every chunk it meets; the rotation by the chunk's first round makes it take a different
    batch of the chunk each time, so that no block is left with the hit batches (or the cheap ones) alone."""
    table, loop = schedule(lib, 768, 768 * 40)
    for block in (0, 5, 100, 767):
        inside = table[block, :loop[block]] % 16
        assert len(set(inside[:16].tolist())) == 16
