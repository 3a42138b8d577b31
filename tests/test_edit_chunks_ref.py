"""The host mirror of vrt_edit_chunks (include/vrt_host.h vrth_apply_shapes, vrth_edit_chunks) against tests/shapes_ref.py's
restatement of the reference's shapes, against the builders it is defined by, and against Svo::set_node one voxel at a time."""
import ctypes as C

import numpy as np
import pytest

from voxelraytracing_amd import _ffi
from voxelraytracing_amd import world as W
from voxelraytracing_amd.world import shape_disc, shape_line, shape_point, shape_sphere

import shapes_ref as R

SEED = 1
WOOD, LEAVES, WATER, STONE = 53, 62, 3, 5
INVALID, RANGE, OOM = _ffi.VRT_ERR_INVALID_ARG, _ffi.VRT_ERR_OUT_OF_RANGE, _ffi.VRT_ERR_OOM


def _pattern(pos):
    """A block that is neither empty nor uniform, so that carving and overwriting both show."""
    i = np.arange(32768)
    x, y, z = i & 31, (i >> 5) & 31, i >> 10
    return (((x + 2 * y + 3 * z + sum(pos)) % 5 == 0) * 7 + (y < 9) * 4).astype(np.uint16)


def _check_against_restatement(shapes, extra_chunks=()):
    """vrth_apply_shapes == the restatement, voxel for voxel, on every chunk the restatement touches and on `extra_chunks`.
    Returns the number of voxels the shapes changed."""
    chunks = sorted(set(R.touched_chunks(shapes)) | set(extra_chunks))
    moved = 0
    for pos in chunks:
        before = _pattern(pos)
        want = R.apply(before, pos, shapes)
        got = W.apply_shapes(before, pos, shapes)
        assert np.array_equal(got, want), f"chunk {pos}: {int((got != want).sum())} voxels differ"
        moved += int((want != before).sum())
    return moved


LINE_CASES = {
    "a == b": ((5, 6, 7), (5, 6, 7)),
    "x major +": ((1, 2, 3), (40, 9, 20)),
    "x major -": ((40, 9, 20), (1, 2, 3)),
    "y major +": ((1, 2, 3), (9, 50, 20)),
    "y major -": ((9, 50, 20), (1, 2, 3)),
    "z major +": ((1, 2, 3), (9, 20, 61)),
    "z major -": ((9, 20, 61), (1, 2, 3)),
    "equal x": ((4, 2, 3), (4, 30, 11)),
    "equal y": ((4, 2, 3), (33, 2, -11)),
    "equal z": ((4, 2, 3), (-20, 17, 3)),
    "equal x and z (a trunk)": ((4, 2, 3), (4, 40, 3)),
    "tie dist.x == dist.y": ((0, 0, 0), (20, -20, 7)),
    "tie dist.y == dist.z": ((0, 0, 0), (3, 25, -25)),
    "tie of all three": ((-3, -3, -3), (14, 14, -20)),
    "tie dist.x == dist.z, y smaller": ((0, 0, 0), (-18, 5, 18)),
}


@pytest.mark.parametrize("name", sorted(LINE_CASES))
def test_lines_walk_like_the_reference(name):
    a, b = LINE_CASES[name]
    pts = list(R.walk_line(a, b))
    dist = [abs(b[i] - a[i]) for i in range(3)]
    major = dist.index(max(dist))
    assert pts[0] == a and pts[-1][major] == b[major]
    assert len(pts) == max(abs(b[i] - a[i]) for i in range(3)) + 1
    assert _check_against_restatement([shape_line(a, b, WOOD)]) > 0


def test_a_line_of_dist_4096_and_one_longer():
    a, b = (-2048, 3, 5), (2048, 900, -700)
    assert len(R.touched_chunks([shape_line(a, b, WOOD)])) >= 129
    assert _check_against_restatement([shape_line(a, b, WOOD)]) >= 4096
    with pytest.raises(W.ShapeError) as e:
        W.apply_shapes(_pattern((0, 0, 0)), (0, 0, 0), [shape_line(a, (2049, 900, -700), WOOD)])
    assert e.value.code == INVALID


@pytest.mark.parametrize("r,count", [(0.0, 0), (0.4, 1), (1.0, 1), (3.0, None), (5.0, None), (4.9, None), (9.9, None)])
def test_spheres(r, count):
    s = [shape_sphere((16, 16, 16), r, LEAVES)]
    n = len(R.voxels(s[0]))
    if count is not None:
        assert n == count     # r = 0 places nothing; 0.4 and 1 the centre only (a neighbour is at distance 1, not below it)
    else:
        assert n > 50
    _check_against_restatement(s, extra_chunks=[(0, 0, 0)])
    # ... and across chunk faces, at negative coordinates
    _check_against_restatement([shape_sphere((-1, 31, -33), r, LEAVES)], extra_chunks=[(-1, 0, -2)])


@pytest.mark.parametrize("height", [0, 1, 3])
@pytest.mark.parametrize("w", range(0, 7))
def test_discs(w, height):
    """The spike's and the canopy's radii, r = w * 0.5 - 0.1 (gen.rs:467).  w = 0 gives r = -0.1, which the reference's loop turns
    into the centre voxel (r * r = 0.01) and this interface refuses (include/vrt.h: r negative): that is asserted instead."""
    r = float(np.float32(w) * np.float32(0.5) - np.float32(0.1))
    s = [shape_disc((30, 30, 1), r, height, STONE)]
    if w == 0:
        with pytest.raises(W.ShapeError) as e:
            W.apply_shapes(_pattern((0, 0, 0)), (0, 0, 0), s)
        assert e.value.code == INVALID
        return
    n = len(R.voxels(s[0]))
    assert (n == 0) == (height == 0)
    if height == 3 and w >= 5:      # the distance is three-dimensional: the layers above the centre's are smaller
        layer = [sum(1 for p in R.voxels(s[0]) if p[1] == 30 + k) for k in range(3)]
        assert layer[0] > layer[1] > layer[2] > 0
    _check_against_restatement(s, extra_chunks=[(0, 0, 0), (1, 0, 0), (0, 1, 0)])


def test_points_and_negative_coordinates():
    shapes = [shape_point((-1, -1, -1), STONE), shape_point((0, 0, 0), WOOD), shape_point((-32, -33, 31), WATER), shape_point((5, 5, 5), 0)]
    assert R.touched_chunks(shapes) == [(-1, -2, 0), (-1, -1, -1), (0, 0, 0)]     # the chunk of voxel -1 is chunk -1
    assert _check_against_restatement(shapes) >= 3
    got = W.apply_shapes(np.zeros(32768, np.uint16), (-1, -1, -1), shapes)
    assert got[31 + 32 * (31 + 32 * 31)] == STONE and int((got != 0).sum()) == 1


def test_a_shape_on_the_common_corner_of_eight_chunks():
    for corner in ((0, 0, 0), (64, -32, 96)):
        s = [shape_sphere(corner, 4.9, LEAVES), shape_disc(corner, 5.9, 2, STONE), shape_line((corner[0] - 7, corner[1] - 5, corner[2] - 3),
                                                                                              (corner[0] + 7, corner[1] + 5, corner[2] + 3), WOOD)]
        assert len(R.touched_chunks(s)) == 8
        assert _check_against_restatement(s) > 500


def test_a_later_shape_overwrites_an_earlier_one_the_lakes_order():
    surface = (33, 40, -2)
    shapes = R.lake(surface, 8, 4, WATER)
    assert [s[1] for s in shapes] == [WATER] * 4 + [0] * 5
    _check_against_restatement(shapes)
    # water first, then EMPTY over it: a disc of water put where the carving comes later ends up carved
    both = [shape_disc(surface, 3.9, 1, WATER), shape_disc(surface, 3.9, 1, 0)]
    pos = R.chunk_of(surface)
    full = np.full(32768, STONE, np.uint16)
    out = W.apply_shapes(full, pos, both)
    assert np.array_equal(out, R.apply(full, pos, both)) and (out == WATER).sum() == 0 and (out == 0).sum() > 10
    assert (W.apply_shapes(full, pos, both[::-1]) == WATER).sum() == (out == 0).sum()


def test_every_kind_in_one_list_a_tree_and_a_lake():
    surface = (31, 95, 32)
    shapes = R.tree(surface, 12, LEAVES, WOOD, WOOD, 7, (27, 106, 36)) + R.lake(surface, 8, 4, WATER) + [shape_point((31, 96, 32), STONE)]
    assert {s[0] for s in shapes} == {R.POINT, R.LINE, R.SPHERE, R.DISC}
    assert len(R.touched_chunks(shapes)) >= 6
    assert _check_against_restatement(shapes) > 500


# ---- vrth_edit_chunks ----

def _block(corner_chunk):
    """The 2 x 2 x 2 generated chunks whose common corner is the first voxel of corner_chunk: positions, nodes, offsets, blocks."""
    cx, cy, cz = corner_chunk
    pos = [(cx + dx, cy + dy, cz + dz) for dz in (-1, 0) for dy in (-1, 0) for dx in (-1, 0)]
    dense = [W.gen_dense(SEED, p) for p in pos]
    parts = [W.svo_build_bottom_up(d) for d in dense]
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    return pos, np.concatenate(parts), offs, dense


CORNER_CHUNK = (2, 3, 3)     # the corner voxel (64, 96, 96): seed 1's ground and sea there lie in the chunks below, air above


def _feature(corner_chunk):
    c = tuple(32 * v for v in corner_chunk)
    return R.tree((c[0] + 6, c[1], c[2]), 12, LEAVES, WOOD, WOOD, 7, (c[0] + 9, c[1] + 10, c[2] - 5)) + R.lake(c, 8, 4, WATER)


def test_edit_chunks_is_to_dense_shapes_bottom_up():
    pos, nodes, offs, dense = _block(CORNER_CHUNK)
    shapes = _feature(CORNER_CHUNK)
    out, ooffs, changed = W.edit_chunks(pos, nodes, offs, shapes, threads=4)
    assert ooffs[0] == 0 and ooffs[-1] == out.size
    n_changed = 0
    for i, p in enumerate(pos):
        want = R.apply(dense[i], p, shapes)
        tree = out[int(ooffs[i]):int(ooffs[i + 1])]
        assert np.array_equal(tree, W.svo_build_bottom_up(want)), p
        assert np.array_equal(W.svo_to_dense(tree), want), p
        assert changed[i] == int(not np.array_equal(want, dense[i])), p
        n_changed += int(changed[i])
    assert 4 <= n_changed < 8
    # one thread gives the same words
    out1, ooffs1, changed1 = W.edit_chunks(pos, nodes, offs, shapes, threads=1)
    assert np.array_equal(out1, out) and np.array_equal(ooffs1, ooffs) and np.array_equal(changed1, changed)


def test_edit_chunks_agrees_with_set_node_voxel_by_voxel():
    """World::place_features (server/src/world/mod.rs:28-55): every placement through Svo::set_node.  The same chunks in a
    world, every placement of the restatement through vrth_world_set_voxel in order; get_voxel then reads the edited blocks."""
    pos, nodes, offs, _ = _block(CORNER_CHUNK)
    shapes = _feature(CORNER_CHUNK)
    out, ooffs, _ = W.edit_chunks(pos, nodes, offs, shapes)
    world = W.ClientWorld(CORNER_CHUNK, 8 * 40000, 2)
    for i, p in enumerate(pos):
        world.create_chunk(p, nodes[int(offs[i]):int(offs[i + 1])])
    lib = _ffi.host()
    for p, v in R.placements(shapes):
        if R.chunk_of(p) in pos:
            assert lib.vrth_world_set_voxel(world._h, W._i3(p), v, None, None) in (0, 4), p     # 4: NoChange
    v = C.c_uint16()
    for i, p in enumerate(pos):
        block = W.svo_to_dense(out[int(ooffs[i]):int(ooffs[i + 1])])
        got = np.empty(32768, np.uint16)
        k = 0
        for z in range(32):
            for y in range(32):
                for x in range(32):
                    assert lib.vrth_world_get_voxel(world._h, (C.c_int32 * 3)(32 * p[0] + x, 32 * p[1] + y, 32 * p[2] + z), C.byref(v)) == 0
                    got[k] = v.value
                    k += 1
        assert np.array_equal(got, block), p


def test_a_set_node_built_tree_comes_back_canonical():
    dense = W.gen_dense(SEED, (1, 2, 1))
    loose = W.svo_build_by_set_node(dense)
    tight = W.svo_build_bottom_up(dense)
    assert not np.array_equal(loose, tight), "the case needs an input that is not canonical"
    out, ooffs, changed = W.edit_chunks([(1, 2, 1)], loose, [0, loose.size], [])
    assert np.array_equal(out, tight) and list(ooffs) == [0, tight.size] and list(changed) == [0]


def test_shapes_that_miss_and_the_empty_calls():
    pos, nodes, offs, dense = _block(CORNER_CHUNK)
    far = [shape_sphere((5000, 5000, 5000), 9.9, STONE), shape_line((-900, 0, 0), (-800, 40, 3), WOOD), shape_disc((40, 90, 40), 5.9, 0, STONE)]
    out, ooffs, changed = W.edit_chunks(pos, nodes, offs, far)
    assert np.array_equal(out, nodes) and np.array_equal(ooffs, offs) and not changed.any()
    out, ooffs, changed = W.edit_chunks(np.zeros((0, 3), np.int32), np.zeros(0, np.uint16), [0], far)
    assert out.size == 0 and list(ooffs) == [0] and changed.size == 0
    # a shape undone by a later one does not count
    assert pos[7] == (2, 3, 3)
    undo = [shape_point((72, 100, 104), STONE), shape_point((72, 100, 104), int(dense[7][8 + 32 * (4 + 32 * 8)]))]
    assert W.edit_chunks(pos, nodes, offs, undo[:1])[2].tolist() == [0] * 7 + [1]
    assert not W.edit_chunks(pos, nodes, offs, undo)[2].any()


def test_a_refused_tree_and_a_short_buffer():
    """vrt_build_chunks's outcomes: 4096 mixed cells -> an empty range and OUT_OF_RANGE, the others produced; cap_nodes one word
    short -> OOM, every offset written, nodes_out untouched."""
    pts = [shape_point((2 * i, 2 * j, 2 * k), STONE) for k in range(16) for j in range(16) for i in range(16)]
    second = W.svo_build_bottom_up(W.gen_dense(SEED, (1, 2, 1)))
    nodes = np.concatenate([[0], second]).astype(np.uint16)
    offs = np.array([0, 1, 1 + second.size], np.uint64)
    pos = [(0, 0, 0), (1, 2, 1)]
    with pytest.raises(W.ShapeError) as e:
        W.edit_chunks(pos, nodes, offs, pts)
    assert e.value.code == RANGE
    out, ooffs, changed = W.edit_chunks(pos, nodes, offs, pts, strict=False)
    assert list(ooffs) == [0, 0, second.size] and np.array_equal(out, second) and list(changed) == [1, 0]
    with pytest.raises(W.SetVoxelErr):
        W.svo_build_bottom_up(R.apply(np.zeros(32768, np.uint16), (0, 0, 0), pts))     # 4096 mixed cells

    lib = _ffi.host()
    sh = W.shape_records(pts[:1])
    p = np.array(pos[1:] + pos[1:], np.int32)
    nin = np.concatenate([second, second])
    oin = np.array([0, second.size, 2 * second.size], np.uint64)
    buf = np.full(2 * second.size, 0xABCD, np.uint16)
    oout = np.full(3, 99, np.uint64)
    ch = np.full(2, 9, np.uint8)
    rc = lib.vrth_edit_chunks(p.ctypes.data, 2, nin.ctypes.data, oin.ctypes.data, sh.ctypes.data, 1, buf.ctypes.data, buf.size - 1,
                              oout.ctypes.data, ch.ctypes.data, 1)
    assert rc == OOM and list(oout) == [0, second.size, 2 * second.size] and (buf == 0xABCD).all()


def rejections():
    """(name, status, keyword changes) of every call vrt_edit_chunks refuses before it does anything; shared with the GPU test."""
    ok = shape_point((1, 1, 1), STONE)
    bad_child = np.array([0x8001, 0, 0, 0, 0, 0, 0, 0], np.uint16)                  # a child block 1..9 in 8 words
    deep = np.zeros(1 + 8 * 6, np.uint16)                                           # a split at every depth 0..5
    for d in range(6):
        deep[0 if d == 0 else 1 + 8 * (d - 1)] = 0x8000 | (1 + 8 * d)
    nan = float("nan")
    cases = [
        ("unknown kind", INVALID, dict(shapes=[(4, STONE, (0, 0, 0), (0, 0, 0), 1.0, 1)])),
        ("voxel > 0x7FFF", INVALID, dict(shapes=[shape_point((0, 0, 0), 0x8000)])),
        ("r negative", INVALID, dict(shapes=[ok, shape_sphere((0, 0, 0), -0.1, STONE)])),
        ("r NaN", INVALID, dict(shapes=[shape_disc((0, 0, 0), nan, 1, STONE)])),
        ("r >= 32768", INVALID, dict(shapes=[shape_sphere((0, 0, 0), 32768.0, STONE)])),
        ("height > 32768", INVALID, dict(shapes=[shape_disc((0, 0, 0), 1.0, 32769, STONE)])),
        ("a outside (-2^22, 2^22)", INVALID, dict(shapes=[shape_point((0, 1 << 22, 0), STONE)])),
        ("a outside, negative", INVALID, dict(shapes=[shape_sphere((-(1 << 22), 0, 0), 1.0, STONE)])),
        ("b outside", INVALID, dict(shapes=[shape_line(((1 << 22) - 5, 0, 0), (1 << 22, 0, 0), STONE)])),
        ("line longer than 4096", INVALID, dict(shapes=[shape_line((0, 0, 0), (5, -4097, 0), STONE)])),
        ("chunk_pos outside", INVALID, dict(pos=[(0, 1 << 17, 0)])),
        ("offsets decreasing", INVALID, dict(pos=[(0, 0, 0), (1, 0, 0)], nodes=np.zeros(4, np.uint16), offsets=[2, 3, 1])),
        ("an empty range", INVALID, dict(pos=[(0, 0, 0), (1, 0, 0)], nodes=np.zeros(4, np.uint16), offsets=[0, 0, 1])),
        ("a range longer than 32761", INVALID, dict(nodes=np.zeros(32762, np.uint16), offsets=[0, 32762])),
        ("a child block that leaves the range", INVALID, dict(nodes=bad_child, offsets=[0, 8])),
        ("a split at depth 5", INVALID, dict(nodes=deep, offsets=[0, deep.size])),
        ("m > 65535", RANGE, dict(shapes=[ok] * 65536)),
        ("null shapes", INVALID, dict(null="shapes")),
        ("null chunk_pos", INVALID, dict(null="pos")),
        ("null nodes_in", INVALID, dict(null="nodes")),
        ("null offsets_in", INVALID, dict(null="offsets")),
        ("null nodes_out", INVALID, dict(null="out")),
        ("null offsets_out", INVALID, dict(null="offsets_out")),
        ("null changed", INVALID, dict(null="changed")),
    ]
    return cases


def too_many_pairs():
    """1025 chunks in a row and 1024 discs whose boxes each cover all of them: 2^20 + 2^10 (chunk, shape) pairs."""
    n, m = 1025, 1024
    return dict(pos=[(i, 0, 0) for i in range(n)], nodes=np.zeros(n, np.uint16), offsets=list(range(n + 1)),
                shapes=[shape_disc((16 * n, 3, 3), 32000.0, 1, STONE)] * m)


def call_raw(fn, kw, threads=None):
    """One refused call through the C ABI with sentinels in every output: (status, outputs untouched)."""
    pos = np.ascontiguousarray(np.array(kw.get("pos", [(0, 0, 0)]), np.int32).reshape(-1, 3))
    nodes = np.ascontiguousarray(kw.get("nodes", np.zeros(1, np.uint16)), np.uint16)
    offs = np.array(kw.get("offsets", [0, 1]), np.uint64)
    sh = W.shape_records(kw.get("shapes", [shape_point((1, 1, 1), STONE)]))
    n = pos.shape[0]
    out = np.full(4096, 0xABCD, np.uint16)
    oout = np.full(n + 1, 0x5555, np.uint64)
    ch = np.full(n, 0x77, np.uint8)
    null = kw.get("null")
    args = [None if null == "pos" else pos.ctypes.data, n, None if null == "nodes" else nodes.ctypes.data,
            None if null == "offsets" else offs.ctypes.data, None if null == "shapes" else sh.ctypes.data, sh.size,
            None if null == "out" else out.ctypes.data, out.size, None if null == "offsets_out" else oout.ctypes.data,
            None if null == "changed" else ch.ctypes.data]
    if threads is not None:
        args.append(threads)
    rc = fn(*args)
    return rc, bool((out == 0xABCD).all() and (oout == 0x5555).all() and (ch == 0x77).all())


@pytest.mark.parametrize("case", rejections(), ids=lambda c: c[0])
def test_rejections_leave_the_outputs_untouched(case):
    _, status, kw = case
    rc, untouched = call_raw(_ffi.host().vrth_edit_chunks, kw, threads=1)
    assert rc == status and untouched


def test_more_than_2_20_pairs_is_out_of_range():
    rc, untouched = call_raw(_ffi.host().vrth_edit_chunks, too_many_pairs(), threads=1)
    assert rc == RANGE and untouched
