"""The start state of a hinted ray of k_trace_wide8 (csrc/wide8_kernels.h), on the host build of the header's routines (tests/native/TraceHintStartHost.hip).

A ray with a valid hint starts on the record the hint names, with the root as a group of its own whose one child is still pending: gx = 1 << 24 (base 0, no valid
bits), gy = (1 << octant) | (1 << 8). The traversal loop has no code for that: its next-item step (next_item_of_group, the text the loop expands in place) must then

  * yield the root -- slot 0, an inner node -- for every octant, and leave (gx, gy) = (1 << 24, 1 << 8), the state in which an unhinted ray starts;
  * from there yield exactly the items an unhinted ray takes: checked on groups of the atrium's real nodes, every octant and every subset of pending children,
    against a plain restatement of the visiting order (position = pending bit ^ octant, slot = base + valid children in lower positions).

And hint_start must refuse every entry that does not carry the tree's generation in its top byte -- all 255 other values of that byte, the empty entry among them --
and every slot outside the tree, leaving the unhinted start untouched.
"""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from bifrost3d_amd.host import Scene
from device_refit_bindings import decode_tree

LIB_PATH = Path(__file__).resolve().parent / "native" / "libtrace_hint_start_host.so"
ITEM_RECORD, ITEM_FINISHED = 0x80000000, 0xFFFFFFFE
ROOT_GX, ROOT_GY = 1 << 24, 1 << 8
_up = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def lib():
    library = C.CDLL(str(LIB_PATH))
    library.trace_hint_start_host_start.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _up]
    library.trace_hint_start_host_start.restype = None
    library.trace_hint_start_host_items.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _up, _up]
    library.trace_hint_start_host_items.restype = C.c_uint32
    return library


def start(lib, hint, tag, slot_count, octant):
    out = (C.c_uint32 * 3)()
    lib.trace_hint_start_host_start(hint, tag, slot_count, octant, out)
    return bool(out[0]), int(out[1]), int(out[2])


def items(lib, gx, gy, octant):
    """([items], [gy after each]) of the group until it is empty."""
    taken, groups = (C.c_uint32 * 16)(), (C.c_uint32 * 16)()
    n = lib.trace_hint_start_host_items(gx, gy, octant, 16, taken, groups)
    return list(taken[:n]), list(groups[:n])


def expected_items(gx, gy, octant):
    """The visiting order as the kernel's header states it, written out plainly."""
    base, valid, pending, inner = gx & 0xFFFFFF, gx >> 24, gy & 0xFF, (gy >> 8) & 0xFF
    out = []
    for p in range(8):
        if pending >> p & 1:
            position = p ^ octant
            slot = base + bin(valid & ((1 << position) - 1)).count("1")
            out.append(slot if inner >> position & 1 else slot | ITEM_RECORD)
    return out + [ITEM_FINISHED]


@pytest.mark.parametrize("octant", range(8))
def test_the_hinted_start_yields_the_root_and_then_the_unhinted_start_state(lib, octant):
    tag, slot_count, record = 7 << 24, 1000, 123
    accepted, item, gy = start(lib, tag | record, tag, slot_count, octant)
    assert accepted and item == record | ITEM_RECORD and gy == (1 << octant) | (1 << 8)
    taken, groups = items(lib, ROOT_GX, gy, octant)
    assert taken == [0, ITEM_FINISHED]               # the root, an inner node; nothing else was pending
    assert groups[0] == ROOT_GY                      # ... and after it the group is the one an unhinted ray starts with, its root already taken
    # an unhinted ray: item 0 and the same group, so from here on the two rays are one
    accepted, item, gy = start(lib, 0, tag, slot_count, octant)
    assert not accepted and item == 0 and gy == ROOT_GY
    # the octant's upper bits are not read (the closest-only kernel keeps the record of the best hit there)
    assert items(lib, ROOT_GX, (1 << octant) | (1 << 8), octant | 0x12345600) == (taken, groups)


def test_the_step_takes_the_items_of_real_nodes_in_the_stated_order(lib):
    slots = Scene("atrium", param0=20000, param1=3).wide8_slots()
    is_node, _ = decode_tree(slots)
    nodes = np.nonzero(is_node)[0]
    rng = np.random.default_rng(5)
    checked = 0
    for slot in rng.choice(nodes, 200, replace=False):
        gx, inner = int(slots[slot, 3]), int(slots[slot, 2]) >> 24
        valid = gx >> 24
        for octant in range(8):
            for _ in range(4):
                hit = int(rng.integers(0, 256)) & valid                                                 # the children the ray hits, by position
                pending = sum(1 << (position ^ octant) for position in range(8) if hit >> position & 1)      # ... by pending bit
                gy = pending | inner << 8
                taken, _ = items(lib, gx, gy, octant)
                assert taken == expected_items(gx, gy, octant)
                kinds = [bool(is_node[t & 0xFFFFFF]) == (t & ITEM_RECORD == 0) for t in taken[:-1]]
                assert all(kinds)                                                                     # a node item names a node, a record item a record
                checked += len(taken) - 1
    assert checked > 10000


def test_the_tag_compare_refuses_every_other_generation_and_every_slot_outside_the_tree(lib):
    slot_count = 5000
    for generation in (1, 2, 128, 255):
        tag = generation << 24
        for other in range(256):
            accepted, item, gy = start(lib, other << 24 | 17, tag, slot_count, 3)
            assert accepted == (other == generation)
            if not accepted:
                assert (item, gy) == (0, ROOT_GY)      # the unhinted start, untouched
        for slot, inside in ((0, True), (slot_count - 1, True), (slot_count, False), (0xFFFFFF, False)):
            assert start(lib, tag | slot, tag, slot_count, 0)[0] == inside
    assert start(lib, 0, 1 << 24, slot_count, 0)[0] is False                   # the empty entry
    assert start(lib, 1 << 24 | 1, 1 << 24, 0, 0) == (False, ITEM_FINISHED, ROOT_GY)      # no tree: nothing to start on
