"""The two fetch stages of the shade kernel (csrc/shade_kernel.h: shade_fetch_inputs, then shade_fetch_by_kind once the hit has arrived) WITHOUT a GPU: the routines
are __host__ __device__ functions of loads and integer compares, compiled for the host by tests/native/ShadeFetchHost.hip.

An entry fetches what its kind of hit reads and nothing else. After both stages its inputs hold:

    kind                              origin field                   direction field
    surface hit                       zero                           loaded
    light hit                         loaded                         loaded
    miss under a constant sky         the path's radiance[slot]      zero
    miss under an environment map     the path's radiance[slot]      loaded
    AOV entries, any live entry       loaded                         loaded
    dead slot, or past the end        untouched                      untouched

Every array holds a pattern of its own, so a field says which array it was loaded from; "zero" is what the first stage leaves, and a second run that fills both
fields with a mark between the stages shows that a field the table calls zero or untouched is not written by the second stage at all. Queues of 1, 63, 64 and 257
entries hold the four kinds in rotation (every rotation, so that the queue of one entry is each kind in turn), in the queue's own order and in a listed one, with and
without the throughput array (camera rays carry none); the places go on past the end of the queue to the end of the last batch of 256 and one batch more.
"""
import ctypes as C
import itertools
from pathlib import Path

import numpy as np
import pytest

LIB_PATH = Path(__file__).resolve().parent / "native" / "libshade_fetch_host.so"
MISS, LIGHT = 0xFFFFFFFF, 0x80000000
SURFACE, LIGHT_HIT, MISSED, DEAD = range(4)
KIND_NAMES = ("surface hit", "light hit", "miss", "dead slot")
SIZES = (1, 63, 64, 257)
SLOTS = 1024
MARK = np.array([-11, -12, -13, -14, -21, -22, -23, -24], np.float32)


@pytest.fixture(scope="module")
def lib():
    lib = C.CDLL(str(LIB_PATH))
    f, u = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    lib.shade_fetch_host.argtypes = [C.c_uint32, C.c_uint32, u, C.c_int, C.c_int, f, f, f, u, f, f, f, f, f]
    lib.shade_fetch_host.restype = None
    lib.shade_fetch_host_record_words.restype = C.c_uint32
    lib.shade_fetch_host_dead_slot.restype = C.c_uint32
    assert lib.shade_fetch_host_record_words() == 19
    return lib


def pattern(base, count):
    """(count, 4) floats, every one different from every float of a pattern with another base (exact in f32: below 2^24)."""
    return (base + np.arange(4 * count, dtype=np.float32)).reshape(count, 4)


def make_queue(n, rotation, dead_slot):
    """A queue of n entries whose kinds rotate; slots are scattered over the radiance array and differ from the entry numbers."""
    kinds = (np.arange(n) + rotation) % 4
    o_tmin, d_pdf, thr = pattern(100_000, n), pattern(200_000, n), pattern(300_000, n)
    hits = pattern(400_000, n)
    ids = np.select([kinds == SURFACE, kinds == LIGHT_HIT], [np.arange(n) * 5 + 3, LIGHT | (np.arange(n) % 3)], MISS).astype(np.uint32)      # a dead slot's hit is a miss (k_trace_closest)
    hits[:, 3] = ids.view(np.float32)
    meta = np.zeros((n, 2), np.uint32)
    meta[:, 0] = (np.arange(n) * 37 + 11) % SLOTS      # 37 and 1024 are coprime: no slot twice
    meta[:, 1] = np.arange(n) + 9000
    meta[kinds == DEAD, 0] = dead_slot
    radiance = pattern(500_000, SLOTS)
    return kinds, o_tmin, d_pdf, thr, meta, hits, radiance


def run(lib, n, places, order, aov, environment, queue, with_throughput, mark):
    kinds, o_tmin, d_pdf, thr, meta, hits, radiance = queue
    f, u = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    first, second = np.full((places, 19), np.nan, np.float32), np.full((places, 19), np.nan, np.float32)
    lib.shade_fetch_host(n, places, order.ctypes.data_as(u) if order is not None else None, int(aov), int(environment), o_tmin.ctypes.data_as(f), d_pdf.ctypes.data_as(f),
                         thr.ctypes.data_as(f) if with_throughput else None, meta.ctypes.data_as(u), hits.ctypes.data_as(f), radiance.ctypes.data_as(f),
                         mark.ctypes.data_as(f) if mark is not None else None, first.ctypes.data_as(f), second.ctypes.data_as(f))
    return first, second


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


CASES = list(itertools.product(SIZES, (False, True), (False, True)))


@pytest.mark.parametrize("n,aov,environment", CASES, ids=[f"{n}-{'aov' if a else 'plain'}-{'map' if e else 'sky'}" for n, a, e in CASES])
def test_every_kind_of_entry_fetches_what_it_reads_and_nothing_else(lib, n, aov, environment):
    dead_slot = lib.shade_fetch_host_dead_slot()
    places = -(-n // 256) * 256 + 256                      # to the end of the last batch, and a batch of places that hold no entry
    zero = np.zeros(4, np.float32)
    rng = np.random.default_rng(n)
    checked = set()
    for rotation, listed, with_throughput in itertools.product(range(4), (False, True), (False, True)):
        queue = make_queue(n, rotation, dead_slot)
        kinds, o_tmin, d_pdf, thr, meta, hits, radiance = queue
        order = rng.permutation(n).astype(np.uint32) if listed else None
        first, second = run(lib, n, places, order, aov, environment, queue, with_throughput, None)
        _, marked = run(lib, n, places, order, aov, environment, queue, with_throughput, MARK)
        for j in range(places):
            where = (n, rotation, listed, with_throughput, j)
            a, b, m = first[j], second[j], marked[j]
            if j >= n:                                     # past the end: no entry, nothing read, nothing written by the second stage
                assert bits(a[0:3]).tolist() == [dead_slot, dead_slot, 0] and np.array_equal(a[3:15], np.zeros(12, np.float32)), where
                assert bits(a[15:19]).tolist() == [0, 0, 0, MISS], where
                assert np.array_equal(bits(b[1:]), bits(a[1:])) and bits(b[0:1])[0] == 0, where
                assert np.array_equal(m[3:11], MARK), where
                checked.add("past the end")
                continue
            e = int(order[j]) if listed else j
            kind = int(kinds[e])
            # the first stage: entry, slot and last triangle, throughput (camera rays: ones and bounce 0), hit; origin and direction fields zero
            assert bits(a[0:3]).tolist() == [e, int(meta[e, 0]), int(meta[e, 1])], where
            assert np.array_equal(a[3:11], np.zeros(8, np.float32)), where
            assert np.array_equal(bits(a[11:15]), bits(thr[e]) if with_throughput else bits(np.array([1, 1, 1, 0], np.float32))), where
            assert np.array_equal(bits(a[15:19]), bits(hits[e])), where
            # the second stage leaves everything but the two fields as it was
            assert np.array_equal(bits(b[1:3]), bits(a[1:3])) and np.array_equal(bits(b[11:19]), bits(a[11:19])), where
            slot = int(meta[e, 0])
            if kind == DEAD:
                origin, direction, origin_marked, direction_marked, holds = zero, zero, MARK[:4], MARK[4:], 0
            elif aov:
                origin, direction, origin_marked, direction_marked, holds = o_tmin[e], d_pdf[e], o_tmin[e], d_pdf[e], 0
            elif kind == SURFACE:
                origin, direction, origin_marked, direction_marked, holds = zero, d_pdf[e], MARK[:4], d_pdf[e], 0
            elif kind == LIGHT_HIT:
                origin, direction, origin_marked, direction_marked, holds = o_tmin[e], d_pdf[e], o_tmin[e], d_pdf[e], 0
            else:
                direction = d_pdf[e] if environment else zero
                origin, origin_marked, direction_marked, holds = radiance[slot], radiance[slot], d_pdf[e] if environment else MARK[4:], 1
            assert np.array_equal(b[3:7], origin) and np.array_equal(b[7:11], direction), (where, KIND_NAMES[kind])
            assert np.array_equal(m[3:7], origin_marked) and np.array_equal(m[7:11], direction_marked), (where, KIND_NAMES[kind])
            assert bits(b[0:1])[0] == holds == bits(m[0:1])[0], (where, KIND_NAMES[kind])      # k_shade adds to the origin field of a miss outside the AOV entries only
            checked.add(KIND_NAMES[kind])
    assert checked == set(KIND_NAMES) | {"past the end"}
