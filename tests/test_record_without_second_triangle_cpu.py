"""A leaf record of ONE triangle cannot be hit through its absent second triangle, and the retire's two-step light test is the whole test.

The shadow lanes of k_trace_wide8's lean instantiations (csrc/wide8_kernels.h: no coverage code, no counters) never load a record's fourth quad -- triangle ids, flags,
facing margin -- and take "is there a B" from e3 instead. That rests on two facts, held here on the host build of the routines (tests/native/LeanRecordsHost.hip):

  * both record writers (host/Wide8Builder.cpp make_record, csrc/wide8_refit.h refit_make_record) store e3 = +0 in every component of a record without a B, and a
    B that is there has e3 != 0 in some component;
  * with e3 == 0, triangle_inside(a, e2, e3, o, d) is false for EVERY ray: p = d x e3 holds products with a zero only, so det = e2 . p is +-0 or NaN, and the test
    refuses both. Random rays, rays with zero components, rays with infinite and NaN components.

And the closest-hit lanes' retire takes the analytic light test in two steps (analytic_light_reachable, analytic_light_distance_of): the value is
analytic_light_distance's bit for bit, NaN where that is NaN, for a sphere and for a disk, on rays that hit, graze and miss.
"""
import ctypes as C
import itertools
from pathlib import Path

import numpy as np
import pytest

from bifrost3d_amd import capi
from bifrost3d_amd.host import Scene
from device_refit_bindings import decode_tree, refit_leaf

LIB_PATH = Path(__file__).resolve().parent / "native" / "liblean_records_host.so"
NONE = 0xFFFFFFFF
_fp, _up, _bp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def lib():
    library = C.CDLL(str(LIB_PATH))
    library.lean_records_host_inside.argtypes = [_up, _up, _fp, _fp, C.c_uint32, C.c_int, _bp, _up]
    library.lean_records_host_inside.restype = C.c_uint32
    library.lean_records_host_light.argtypes = [C.POINTER(capi.HiprLight), _fp, _fp, C.c_uint32, _fp, _fp, _bp]
    library.lean_records_host_light.restype = None
    return library


@pytest.fixture(scope="module")
def atrium():
    return Scene("atrium", param0=20000, param1=3)


@pytest.fixture(scope="module")
def records(atrium):
    """(the atrium's leaf records as the host builder wrote them, the same rebuilt by refit_make_record), 16 words each."""
    slots, triangles = atrium.wide8_slots(), atrium.triangles()
    is_node, _ = decode_tree(slots)
    built = slots[~is_node]
    rebuilt = np.zeros_like(built)
    for k, stored in enumerate(built):
        ok, rebuilt[k], _ = refit_leaf(triangles, stored)
        assert ok
    assert np.array_equal(built, rebuilt)      # the two writers agree (tests/test_device_refit_on_host_cpu.py holds them to each other at length)
    for array in (built, rebuilt):
        array.setflags(write=False)
    return built, rebuilt


def inside(lib, records, record_of, origins, directions, which):
    records = np.ascontiguousarray(records, np.uint32)
    record_of = np.ascontiguousarray(record_of, np.uint32)
    origins, directions = np.ascontiguousarray(origins, np.float32), np.ascontiguousarray(directions, np.float32)
    n = len(record_of)
    assert origins.shape == directions.shape == (n, 3) and record_of.max() < len(records)
    hit, det = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    count = lib.lean_records_host_inside(records.ctypes.data_as(_up), record_of.ctypes.data_as(_up), origins.ctypes.data_as(_fp), directions.ctypes.data_as(_fp), n, which,
                                         hit.ctypes.data_as(_bp), det.ctypes.data_as(_up))
    assert count == int(hit.sum())
    return hit.astype(bool), det.view(np.float32)


def test_a_record_of_one_triangle_holds_plus_zero_for_e3_and_a_pair_does_not(atrium, records):
    for which in records:
        single = which[:, 13] == NONE
        assert 100 < single.sum() < len(which) - 100          # the atrium has plenty of both kinds of record
        assert (which[:, 12] != NONE).all()                   # A is always there
        assert (which[single, 9:12] == 0).all()               # the bits of +0, in all three components
        assert ((which[~single, 9:12] & 0x7FFFFFFF) != 0).any(axis=1).all()      # the kernel's test for "B is there": some component of e3 is not a zero


def test_the_absent_second_triangle_refuses_every_ray(lib, atrium, records):
    _, rebuilt = records                                      # the records refit_make_record made, index_b == HIPR_LEAF8_NONE
    single = rebuilt[rebuilt[:, 13] == NONE]
    rng = np.random.default_rng(11)
    n = 100000
    record_of = rng.integers(0, len(single), n).astype(np.uint32)
    a = single[record_of, 0:3].view(np.float32)
    e1, e2 = single[record_of, 3:6].view(np.float32), single[record_of, 6:9].view(np.float32)
    # half of the rays aimed at a point inside triangle A (the solve of B shares a and e2 with it), half anywhere in the hall
    u, v = rng.uniform(0, 1, (2, n, 1)).astype(np.float32)
    flip = (u + v) > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    target = a + u * e1 + v * e2
    origins = rng.uniform(-14.0, 14.0, (n, 3)).astype(np.float32)
    directions = target - origins
    directions[n // 2:] = rng.normal(size=(n - n // 2, 3))
    directions = (directions / np.linalg.norm(directions, axis=1, keepdims=True)).astype(np.float32)
    hit_a, _ = inside(lib, single, record_of, origins, directions, 0)
    assert hit_a[:n // 2].mean() > 0.9                        # the shim does find triangles: the aimed rays are inside A
    hit_b, det = inside(lib, single, record_of, origins, directions, 1)
    assert not hit_b.any()
    assert (det == 0).all()                                   # finite rays: the determinant is a zero of either sign

    # rays with zero components of either sign, and with components that are not finite, in every combination
    values = np.array([0.0, -0.0, 1.0, -2.5, np.inf, -np.inf, np.nan], np.float32)
    triples = np.array(list(itertools.product(values, repeat=3)), np.float32)
    pairs = np.array(list(itertools.product(range(len(triples)), repeat=2)))
    origins, directions = triples[pairs[:, 0]], triples[pairs[:, 1]]
    record_of = (np.arange(len(pairs)) % len(single)).astype(np.uint32)
    hit_b, det = inside(lib, single, record_of, origins, directions, 1)
    assert len(pairs) == 7 ** 6 and not hit_b.any()
    assert ((det == 0) | np.isnan(det)).all() and np.isnan(det).any() and (det == 0).any()


def light(kind, position, radius, direction=(0.0, -1.0, 0.0)):
    l = capi.HiprLight()
    l.data[0:3] = [10.0, 9.0, 8.0]
    l.data[3:6] = list(position)
    l.data[6] = radius
    l.data[7:10] = list(direction)
    l.data[10] = 0.8
    l.flags = kind
    return l


@pytest.mark.parametrize("kind,name", [(1, "sphere"), (5, "spot")])      # include/hiprenderer_c.h HIPR_LIGHT_SPHERE, HIPR_LIGHT_SPOT
def test_the_two_step_light_test_is_the_whole_test(lib, kind, name):
    centre, radius = np.array([1.0, 4.0, 0.5], np.float32), np.float32(1.5)
    normal = np.array([0.0, -1.0, 0.0], np.float32)
    l = light(kind, centre, radius, normal)
    rng = np.random.default_rng(3)
    n = 60000
    origins = rng.uniform(-12.0, 12.0, (n, 3)).astype(np.float32)
    # aimed at points around the light, out to 1.2 radii (hits and near misses); a third at its very rim (grazing); a third anywhere
    target = centre + rng.uniform(-1.2, 1.2, (n, 3)).astype(np.float32) * radius
    rim = rng.normal(size=(n, 3)).astype(np.float32)
    if kind == 5: rim[:, 1] = 0.0                             # the disk's rim lies in its plane
    rim = centre + radius * rim / np.linalg.norm(rim, axis=1, keepdims=True) * rng.choice(np.array([1 - 1e-6, 1.0, 1 + 1e-6], np.float32), (n, 1))
    target[n // 3:2 * n // 3] = rim[n // 3:2 * n // 3]
    directions = target - origins
    if kind == 1:                                             # a sphere is grazed by the rays of its tangent cone: sin(angle to the centre) = radius / distance
        to_centre = (centre - origins).astype(np.float64)
        distance = np.linalg.norm(to_centre, axis=1, keepdims=True)
        along = to_centre / distance
        across = np.cross(along, rng.normal(size=(n, 3)))
        across /= np.linalg.norm(across, axis=1, keepdims=True)
        sine = np.minimum(1.0, radius * rng.choice([1 - 1e-6, 1.0, 1 + 1e-6], (n, 1)) / distance)
        tangent = np.sqrt(1.0 - sine * sine) * along + sine * across
        directions[n // 3:2 * n // 3] = tangent[n // 3:2 * n // 3]
    directions[2 * n // 3:] = rng.normal(size=(n - 2 * n // 3, 3))
    directions = (directions / np.linalg.norm(directions, axis=1, keepdims=True)).astype(np.float32)
    # ... and the rays of zero, infinite and NaN components
    values = np.array([0.0, -0.0, 1.0, -2.5, np.inf, np.nan], np.float32)
    triples = np.array(list(itertools.product(values, repeat=3)), np.float32)
    pairs = np.array(list(itertools.product(range(len(triples)), repeat=2)))
    origins = np.ascontiguousarray(np.concatenate([origins, triples[pairs[:, 0]]]), np.float32)
    directions = np.ascontiguousarray(np.concatenate([directions, triples[pairs[:, 1]]]), np.float32)
    total = len(origins)
    whole, two_step, reachable = np.zeros(total, np.float32), np.zeros(total, np.float32), np.zeros(total, np.uint8)
    lib.lean_records_host_light(C.byref(l), origins.ctypes.data_as(_fp), directions.ctypes.data_as(_fp), total, whole.ctypes.data_as(_fp), two_step.ctypes.data_as(_fp),
                                reachable.ctypes.data_as(_bp))
    # NaN is NaN (the compare with the ray's bounds refuses every one of them); everything else bit for bit
    assert np.array_equal(np.isnan(whole), np.isnan(two_step))
    met = ~np.isnan(whole)
    assert np.array_equal(whole[met].view(np.uint32), two_step[met].view(np.uint32))
    assert np.array_equal(reachable.astype(bool), met)       # the first step alone decides whether there is a distance
    assert 0.1 < met[:n // 3].mean() < 0.95                   # the aimed rays: both outcomes
    assert 0.1 < met[n // 3:2 * n // 3].mean() < 0.9          # the grazing rays: both outcomes
    assert met[2 * n // 3:n].mean() < 0.2                     # the rays aimed at nothing mostly pass by
