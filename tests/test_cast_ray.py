"""vrth_world_cast_ray — common::math::cast_ray (common/src/math.rs:153-226) over a ClientWorld, in strict binary32 — held to a
numpy float32 restatement of math.rs (tests/cast_ray_cases.py), on the issue's known answers and on fuzzed rays.  CPU only."""
import math

import numpy as np
import pytest

from voxelraytracing_amd import ClientWorld, _ffi, scenes
from voxelraytracing_amd.world import ray_queries

import cast_ray_cases as cc

START = (0.5, 2.5, 0.5)


@pytest.fixture(scope="module")
def floor():
    return cc.floor_world()


def _bits(x):
    return np.array([x], np.float32).view(np.uint32)[0]


def _check(world, start, dir, max_dist, status, pos=(0, 0, 0), face=(0, 0, 0), dist=0.0):
    dense = cc.DenseWorld(world)
    want = cc.cast_ray(start, dir, max_dist, dense.collides)
    got = world.cast_ray_record(start, dir, max_dist)
    assert want[0] == status and want[1] == pos and want[2] == face and _bits(want[3]) == _bits(dist), want
    assert (got.status, tuple(got.pos), tuple(got.face), _bits(got.dist)) == (status, pos, face, _bits(dist))


def test_known_answers_over_a_floor(floor):
    nan, inf = float("nan"), float("inf")
    # the player at pitch 0 / yaw 0: unit_step_size.x and .y are NaN, the first step takes the y branch with dist NaN
    _check(floor, START, (-0.0, -0.0, -1.0), 10.0, 0)
    # x and z tie: the y branch, dist = +inf
    _check(floor, START, (1.0, 0.0, 1.0), 10.0, 0)
    _check(floor, START, (0.0, -1.0, 0.0), 10.0, 1, (0, -1, 0), (0, 1, 0), 2.5)
    _check(floor, START, (0.3, -1.0, 0.2), 10.0, 1, (1, -1, 0), (0, 1, 0), 2.657536506652832)
    _check(floor, START, (1.0, -1.0, 1.0), 10.0, 1, (0, -1, 0), (0, 1, 0), 4.330126762390137)
    _check(floor, START, (0.0, 0.0, 0.0), 10.0, 0)
    # a NaN or negative max_dist takes no step
    _check(floor, START, (0.0, -1.0, 0.0), nan, 0)
    _check(floor, START, (0.0, -1.0, 0.0), -1.0, 0)
    # rejected: the reference would loop forever or leave i32
    for s, md in ((START, inf), (START, 1048577.0), ((nan, 2.5, 0.5), 10.0), ((0.5, inf, 0.5), 10.0),
                  ((0.5, 2.5, 16777216.0), 10.0), ((-16777216.0, 2.5, 0.5), 10.0)):
        _check(floor, s, (0.0, -1.0, 0.0), md, 2)
    # max_dist 2^20 is run; the ray leaves the world through the floor-less sky and misses
    _check(floor, START, (0.0, 1.0, 0.0), 1048576.0, 0)


def test_known_answers_with_the_voxel_above_solid():
    w = cc.floor_world()
    w.create_chunk((0, 0, 0), np.array([0], np.uint16))   # an air chunk above the floor, then one voxel in it
    w.set_voxel((0, 3, 0), 5)
    nan, inf = float("nan"), float("inf")
    for d, dist in (((-0.0, -0.0, -1.0), nan), ((1.0, 0.0, 1.0), inf), ((0.0, 0.0, 0.0), nan)):
        _check(w, START, d, 10.0, 1, (0, 3, 0), (0, -1, 0), dist)
    assert w.cast_ray(START, (1.0, 0.0, 1.0), 10.0) == ((0, 3, 0), (0, -1, 0))
    assert w.cast_ray(START, (0.0, -1.0, 0.0), 10.0) == ((0, -1, 0), (0, 1, 0))
    with pytest.raises(ValueError):
        w.cast_ray(START, (0.0, 1.0, 0.0), math.inf)


def test_scalar_and_lockstep_restatements_agree(floor):
    """The array form of the restatement against its scalar text (max_dist <= 300: the scalar loop has no early exit)."""
    for world in (floor, scenes.c1_flat().world):
        q = cc.fuzz_queries(world, 400, seed=5)
        q = q[~(q["max_dist"] > 300.0)]
        dense = cc.DenseWorld(world)
        arr = cc.cast_rays(q, dense)
        for i in range(q.size):
            s, p, f, dist = cc.cast_ray(q["start"][i], q["dir"][i], q["max_dist"][i], dense.collides)
            r = arr[i]
            assert (s, p, f, _bits(dist)) == (r["status"], tuple(r["pos"]), tuple(r["face"]), _bits(r["dist"])), (i, q[i])


def test_dense_world_is_get_voxel():
    w = scenes.procedural(4, (8, 8)).world
    dense = cc.DenseWorld(w)
    rng = np.random.default_rng(3)
    for p in rng.integers(-4, 4 * 32 + 4, (500, 3)):
        try:
            v = w.get_voxel(tuple(int(c) for c in p))
        except Exception:
            v = 0
        assert dense.collides(p) == (v != 0), p


@pytest.mark.parametrize("which", ["floor", "c1", "procedural"])
def test_host_cast_ray_is_the_restatement_on_fuzzed_rays(which, floor):
    world = {"floor": lambda: floor, "c1": lambda: scenes.c1_flat().world, "procedural": lambda: scenes.procedural(4, (8, 8)).world}[which]()
    q = cc.fuzz_queries(world, 7000, seed=11)
    want = cc.cast_rays(q, cc.DenseWorld(world))
    got = world.cast_rays(q["start"], q["dir"], q["max_dist"], threads=4)
    bad = cc.records_equal(want, got)
    assert bad.size == 0, (bad.size, q[bad[:5]], want[bad[:5]], got[bad[:5]])
    # the fuzz reaches every kind of result, and the single-ray entry point is the batch one
    assert {0, 1, 2} <= set(np.unique(got["status"]).tolist())
    for i in range(0, q.size, 97):
        one = world.cast_ray_record(q["start"][i], q["dir"][i], q["max_dist"][i])
        assert cc.records_equal(np.frombuffer(bytes(one), _ffi.RAY_HIT_DTYPE), got[i:i + 1]).size == 0


def test_misses_and_rejections_leave_every_other_field_zero(floor):
    q = ray_queries([(0.5, 2.5, 0.5), (0.5, 2.5, 0.5), (np.nan, 0, 0)], [(0, 1, 0), (0.2, 1, 0.1), (0, -1, 0)], [300.0, 10.0, 10.0])
    got = floor.cast_rays(q["start"], q["dir"], q["max_dist"])
    assert got["status"].tolist() == [0, 0, 2]
    assert not got["pos"].any() and not got["face"].any() and not got["dist"].view(np.uint32).any()


def test_world_edits_are_seen(floor):
    w = cc.floor_world()
    assert w.cast_ray(START, (0.0, -1.0, 0.0), 10.0) == ((0, -1, 0), (0, 1, 0))
    w.set_voxel((0, -1, 0), 0)
    assert w.cast_ray(START, (0.0, -1.0, 0.0), 10.0) == ((0, -2, 0), (0, 1, 0))
