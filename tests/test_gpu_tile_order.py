"""The orders a one-frame-at-a-time context launches its tiles in, entry for entry against tests/tile_order_ref.py: the five
tile_order_* kernels of csrc/vrt_kernels.hip on synthetic costs (vrt_selftest_tile_order: the product's launchers and constants),
and the orders real frames make (vrt_read_tile_order against the sort of vrt_read_tile_cost).  A frame comparison sees neither a
wrong set (a tile left out keeps the texels of the frame before) nor a wrong order of the right set (the same frame, slower)."""
import ctypes as C
import math

import numpy as np
import pytest

import tile_order_cases as cases
import tile_order_ref as ref
from util import gpu_for_scene
from voxelraytracing_amd import MODE_PRIMARY, MODE_PRIMARY_SHADOW, _ffi, scenes
from voxelraytracing_amd import graphics as g

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_OUT_OF_RANGE, ERR_STATE = -1, -2, -5
LIMESTONE = 4


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ---- synthetic costs ----

@pytest.mark.parametrize("pattern", cases.PATTERNS)
@pytest.mark.parametrize("n", cases.EXACT_SIZES)
def test_exact_sort_of_synthetic_costs(n, pattern):
    cost = cases.costs(pattern, n, 1)
    order = g.selftest_tile_order(cost, n, 1, -1)
    assert ref.check_exact_order(cost, order) == []


@pytest.mark.parametrize("shape,radius", cases.BLOCK_CASES, ids=_id)
def test_block_order_of_synthetic_costs(shape, radius):
    """Every pattern of the shape: the checker finds nothing, and what the kernel's LDS atomic does not decide is the canonical
    order's — where the keys (class', chunk of 64 blocks) change, and which tiles stand under each key."""
    tx, ty = shape
    for pattern in cases.pattern_names(tx, ty):
        cost = cases.costs(pattern, tx, ty)
        order = g.selftest_tile_order(cost, tx, ty, radius)
        assert ref.check_block_order(cost, tx, ty, radius, order) == [], pattern
        want = ref.canonical_block_order(cost, tx, ty, radius)
        keys = ref.position_keys(cost, tx, ty, radius, order)
        assert np.array_equal(keys, ref.position_keys(cost, tx, ty, radius, want)), pattern
        assert np.array_equal(ref.sorted_within_keys(order, keys), ref.sorted_within_keys(want, keys)), pattern


@pytest.mark.parametrize("shape,radius", cases.REFUSED, ids=_id)
def test_block_order_refusals_write_nothing(shape, radius):
    tx, ty = shape
    cost = cases.costs("random field", tx, ty)
    order = np.full(tx * ty, 0xABABABAB, dtype=np.uint32)
    rc = _ffi.vrt().vrt_selftest_tile_order(0, cost.ctypes.data_as(C.c_void_p), tx, ty, radius, order.ctypes.data_as(C.c_void_p))
    assert rc == ERR_OUT_OF_RANGE and (order == 0xABABABAB).all()
    with pytest.raises(g.VrtError) as e:
        g.selftest_tile_order(cost, tx, ty, radius)
    assert e.value.code == ERR_OUT_OF_RANGE


def test_selftest_arguments():
    lib = _ffi.vrt()
    cost = np.zeros(16, dtype=np.uint32)
    order = np.full(16, 0xABABABAB, dtype=np.uint32)
    pc, po = cost.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.c_void_p)
    for args in ((None, 4, 4, 1, po), (pc, 4, 4, 1, None), (pc, 0, 4, 1, po), (pc, 4, 0, -1, po), (pc, 4, 4, 0, po)):
        assert lib.vrt_selftest_tile_order(0, *args) == ERR_INVALID_ARG, args
    assert (order == 0xABABABAB).all()
    assert lib.vrt_selftest_tile_order(0, pc, 4, 4, -1, po) == 0 and order.tolist() == list(range(16))


# ---- the orders real frames make ----

_BASE = []


def _c2(size):
    """scenes.c2 at `size` over one world for the whole file (no test here edits it)."""
    if not _BASE:
        _BASE.append(scenes.c2((128, 64)))
    b = _BASE[0]
    return scenes._scene(f"C2 {size[0]}x{size[1]}", b.world, size, b.eye, b.rot, MODE_PRIMARY_SHADOW)


def _tiles(size):
    return (size[0] // 8) * (size[1] // 8)


def _state_error(gpu, tiles):
    with pytest.raises(g.VrtError) as e:
        gpu.read_tile_order(tiles)
    return e.value.code


@pytest.mark.parametrize("size,mode", [((128, 64), MODE_PRIMARY_SHADOW), ((200, 104), MODE_PRIMARY_SHADOW), ((640, 360), MODE_PRIMARY_SHADOW),
                                       ((640, 360), MODE_PRIMARY), ((1920, 1080), MODE_PRIMARY_SHADOW)], ids=_id)
def test_a_view_at_rest_gets_the_exact_order_of_its_trips(size, mode):
    """Three frames of one view: the third is launched in an order, the exact one, the stable sort of the trips read back — which have at
    least 8 classes and are not in screen order (tests/test_tile_order_ref.py says so of the oracle's step counts beforehand)."""
    gpu = gpu_for_scene(_c2(size))
    try:
        gpu.set_frames_in_flight(1)
        n = _tiles(size)
        assert _state_error(gpu, n) == ERR_STATE          # before any order
        for _ in range(2):
            gpu.render(mode)
        before = gpu.accel_info().ordered_frames
        gpu.render(mode)
        assert gpu.accel_info().ordered_frames == before + 1
        order, dilated = gpu.read_tile_order(n)
        cost = gpu.read_tile_cost(n)
        assert not dilated
        assert ref.check_exact_order(cost, order) == []
        assert len(set(ref.cost_class(cost).tolist())) >= 8
        assert not np.array_equal(order, np.arange(n))
    finally:
        gpu.close()


def test_two_shards_sort_their_own_tiles():
    sc = _c2((320, 184))
    seen = 0
    for rank in range(2):
        gpu = gpu_for_scene(sc, shard_rank=rank, shard_count=2)
        try:
            gpu.set_frames_in_flight(1)
            local, _, total = gpu.shard_info()
            assert total == 920 and 128 <= local < total
            for _ in range(3):
                gpu.render(MODE_PRIMARY_SHADOW)
            order, dilated = gpu.read_tile_order(local)
            cost = gpu.read_tile_cost(local)
            assert not dilated and ref.check_exact_order(cost, order) == []
            assert len(set(ref.cost_class(cost).tolist())) >= 2 and not np.array_equal(order, np.arange(local))
            seen += local
        finally:
            gpu.close()
    assert seen == 920


def _orbit(sc, k, size):
    """The camera step of test_gpu_parity.py::test_tiles_ordered_under_a_moving_camera_are_the_same_frames."""
    return g.cam_data_create((sc.rot[0] + 0.3 * k, sc.rot[1] + 0.9 * k, 0.0), (sc.eye[0] + 0.5 * k, sc.eye[1] + 0.1 * (k % 3), sc.eye[2] - 0.4 * k), 70.0,
                             (float(size[0]), float(size[1])))


@pytest.mark.parametrize("radius", [5, 1, 6])
@pytest.mark.parametrize("size", [(200, 104), (640, 360), (1920, 1080)], ids=_id)
def test_a_moving_view_gets_a_block_order_and_keeps_it(monkeypatch, size, radius):
    """A first frame, then one orbit step: the frame behind the step is launched in the block order of the first frame's trips, dilated
    over VRT_TILE_ORDER_RADIUS blocks.  At the default radius a second step: the very same order; and two more frames where the camera
    stands: the exact order.  (A radius of 1 covers less than two of these steps at 1080p.)"""
    if radius != 5:
        monkeypatch.setenv("VRT_TILE_ORDER_RADIUS", str(radius))
    sc = _c2(size)
    gpu = gpu_for_scene(sc)
    try:
        gpu.set_frames_in_flight(1)
        n, tx, ty = _tiles(size), size[0] // 8, size[1] // 8
        gpu.write_cam_data(_orbit(sc, 0, size))
        gpu.render(MODE_PRIMARY_SHADOW)
        gpu.write_cam_data(_orbit(sc, 1, size))
        gpu.render(MODE_PRIMARY_SHADOW)
        assert gpu.accel_info().ordered_frames == 1
        order, dilated = gpu.read_tile_order(n)
        cost = gpu.read_tile_cost(n)
        assert dilated
        assert ref.check_block_order(cost, tx, ty, radius, order) == []
        want = ref.canonical_block_order(cost, tx, ty, radius)
        keys = ref.position_keys(cost, tx, ty, radius, order)
        assert np.array_equal(keys, ref.position_keys(cost, tx, ty, radius, want))
        assert np.array_equal(ref.sorted_within_keys(order, keys), ref.sorted_within_keys(want, keys))
        bw, bh = ref.block_grid(tx, ty)
        if bw > 2 * radius + 1 or bh > 2 * radius + 1:   # (a frame no wider than the dilation may well be one class: 200 x 104 at radius 5 is)
            assert len(set((keys >> 32).tolist())) >= 2 and not np.array_equal(order, np.arange(n))
        if radius != 5:
            return
        gpu.write_cam_data(_orbit(sc, 2, size))
        gpu.render(MODE_PRIMARY_SHADOW)
        assert gpu.accel_info().ordered_frames == 2
        kept, dilated = gpu.read_tile_order(n)
        assert dilated and kept.tobytes() == order.tobytes()
        for _ in range(2):
            gpu.render(MODE_PRIMARY_SHADOW)
        order, dilated = gpu.read_tile_order(n)
        assert not dilated and ref.check_exact_order(gpu.read_tile_cost(n), order) == []
    finally:
        gpu.close()


def test_an_edit_under_a_resting_view_keeps_the_order_for_one_frame():
    """A voxel set six voxels in front of the eye: the edit's own frame is launched in the order from before it, the frame behind it notes
    its trips again, and the order is then the sort of those."""
    size = (200, 104)
    sc = scenes.c2(size)     # (a world of its own: it is edited)
    gpu = gpu_for_scene(sc)
    try:
        gpu.set_frames_in_flight(1)
        n = _tiles(size)
        for _ in range(3):
            gpu.render(MODE_PRIMARY_SHADOW)
        order, _ = gpu.read_tile_order(n)
        cost = gpu.read_tile_cost(n)
        assert ref.check_exact_order(cost, order) == []
        d = g.axis_rot_to_ray([math.radians(a) for a in sc.rot])
        at = tuple(int(math.floor(sc.eye[k] + 6.0 * d[k])) for k in range(3))
        assert sc.world.get_voxel(at) == 0
        start, count = sc.world.set_voxel(at, LIMESTONE)
        gpu.write_nodes(sc.world.nodes_ptr(), start, start + count)
        ordered = gpu.accel_info().ordered_frames
        gpu.render(MODE_PRIMARY_SHADOW)                      # the edit's frame
        kept, dilated = gpu.read_tile_order(n)
        assert not dilated and kept.tobytes() == order.tobytes() and gpu.read_tile_cost(n).tobytes() == cost.tobytes()
        gpu.render(MODE_PRIMARY_SHADOW)                      # the frame behind it: still the old order, its trips noted and sorted
        assert gpu.accel_info().ordered_frames == ordered + 2
        new_order, dilated = gpu.read_tile_order(n)
        new_cost = gpu.read_tile_cost(n)
        assert not dilated and ref.check_exact_order(new_cost, new_order) == []
        assert not np.array_equal(new_cost, cost), "the voxel in front of the eye changed no tile's trips"
        assert not np.array_equal(new_order, order)
    finally:
        gpu.close()


def test_no_order_to_read(monkeypatch):
    """VRT_ERR_STATE: two frames in flight, after a resize of the output, under VRT_TILE_ORDER=0 (before any order: the resting
    view's test)."""
    size = (128, 64)
    sc = _c2(size)
    n = _tiles(size)
    gpu = gpu_for_scene(sc)
    try:
        gpu.set_frames_in_flight(2)
        for _ in range(4):
            gpu.render(MODE_PRIMARY_SHADOW)
        assert _state_error(gpu, n) == ERR_STATE
        gpu.set_frames_in_flight(1)
        for _ in range(3):
            gpu.render(MODE_PRIMARY_SHADOW)
        order, _ = gpu.read_tile_order(n)
        assert ref.check_exact_order(gpu.read_tile_cost(n), order) == []
        gpu.resize_result_texture((136, 64))
        assert _state_error(gpu, 17 * 8) == ERR_STATE
        lib = _ffi.vrt()
        assert lib.vrt_read_tile_order(gpu._h, None, None) == ERR_INVALID_ARG
        assert lib.vrt_read_tile_order(None, order.ctypes.data_as(C.c_void_p), None) == ERR_INVALID_ARG
    finally:
        gpu.close()
    monkeypatch.setenv("VRT_TILE_ORDER", "0")
    gpu = gpu_for_scene(sc)
    try:
        gpu.set_frames_in_flight(1)
        for _ in range(3):
            gpu.render(MODE_PRIMARY_SHADOW)
        assert gpu.accel_info().ordered_frames == 0 and _state_error(gpu, n) == ERR_STATE
    finally:
        gpu.close()
