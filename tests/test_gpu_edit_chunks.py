"""vrt_edit_chunks on the MI355X: nodes, offsets and changed held word for word to the host mirror's vrth_edit_chunks (which
tests/test_edit_chunks_ref.py holds to the reference's shapes).  Each case first asserts on the mirror alone that it exercises
what it claims."""
import numpy as np
import pytest

from voxelraytracing_amd import Gpu, MODE_PRIMARY, MODE_PRIMARY_SHADOW, VrtError, _ffi, scenes
from voxelraytracing_amd import world as W
from voxelraytracing_amd.world import shape_disc, shape_line, shape_point, shape_sphere

import shapes_ref as R
from test_edit_chunks_ref import (CORNER_CHUNK, LEAVES, SEED, STONE, WATER, WOOD, _block, _feature, call_raw, rejections, too_many_pairs)
from util import assert_frame_parity, gpu_for_scene

pytestmark = pytest.mark.gpu

BATCH = 2048
INVALID, RANGE, OOM = _ffi.VRT_ERR_INVALID_ARG, _ffi.VRT_ERR_OUT_OF_RANGE, _ffi.VRT_ERR_OOM


@pytest.fixture(scope="module")
def gpu():
    g = Gpu(1 << 16, 2, (64, 64), device=0)
    yield g
    g.close()


@pytest.fixture(scope="module")
def block():
    return _block(CORNER_CHUNK)


def _same(gpu, pos, nodes, offs, shapes):
    """Both sides, lenient about refused trees; returns the mirror's answer after asserting the GPU's is the same."""
    want = W.edit_chunks(pos, nodes, offs, shapes, strict=False, threads=4)
    got = gpu.edit_chunks(pos, nodes, offs, shapes, strict=False)
    for name, a, b in zip(("nodes", "offsets", "changed"), got, want):
        assert a.shape == b.shape, f"{name}: {a.shape} on the GPU, {b.shape} on the host"
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, f"{name}: {bad.size} entries differ, first at {bad[0]}: {a[bad[0]]:#x} host {b[bad[0]]:#x}"
    return want


def test_one_point_in_an_air_chunk(gpu):
    out, offs, changed = _same(gpu, [(0, 0, 0)], np.zeros(1, np.uint16), [0, 1], [shape_point((5, 6, 7), STONE)])
    assert out.size == 41 and list(offs) == [0, 41] and list(changed) == [1]
    _same(gpu, [(-1, -1, -1)], np.zeros(1, np.uint16), [0, 1], [shape_point((-1, -1, -1), STONE), shape_point((0, 0, 0), WOOD)])


def test_a_tree_and_a_lake_at_the_corner_of_eight_generated_chunks(gpu, block):
    pos, nodes, offs, dense = block
    shapes = _feature(CORNER_CHUNK)
    kinds = [s[0] for s in shapes]
    assert kinds[:4] == [R.SPHERE, R.SPHERE, R.LINE, R.LINE] and shapes[0][4] == 5.0 and shapes[1][4] == 3.0
    assert [s[1] for s in shapes[4:]] == [WATER] * 4 + [0] * 5 and set(kinds[4:]) == {R.DISC}
    _, _, changed = _same(gpu, pos, nodes, offs, shapes)
    assert changed.sum() >= 4 and (changed == 0).any()
    # the same with every shape on the corner itself: all eight chunks
    c = tuple(32 * v for v in CORNER_CHUNK)
    at_corner = [shape_sphere(c, 4.9, LEAVES), shape_disc(c, 5.9, 2, STONE),
                 shape_line((c[0] - 7, c[1] - 5, c[2] - 3), (c[0] + 7, c[1] + 5, c[2] + 3), WOOD)]
    _, _, changed = _same(gpu, pos, nodes, offs, at_corner)
    assert changed.all()
    with pytest.raises(VrtError) as e:     # (strict is the default; nothing is refused here, a bad shape is)
        gpu.edit_chunks(pos, nodes, offs, [shape_sphere(c, -1.0, STONE)])
    assert e.value.code == INVALID


def test_shapes_that_miss_every_chunk_and_no_shapes_at_all(gpu, block):
    pos, nodes, offs, _ = block
    far = [shape_sphere((5000, 5000, 5000), 9.9, STONE), shape_line((-900, 0, 0), (-800, 40, 3), WOOD), shape_disc((70, 90, 100), 5.9, 0, STONE)]
    for shapes in (far, []):
        out, ooffs, changed = _same(gpu, pos, nodes, offs, shapes)
        assert np.array_equal(out, nodes) and np.array_equal(ooffs, offs) and not changed.any()     # (the input is canonical)


def test_no_chunks(gpu):
    out, offs, changed = gpu.edit_chunks(np.zeros((0, 3), np.int32), np.zeros(0, np.uint16), [0], [shape_point((0, 0, 0), STONE)])
    assert out.size == 0 and list(offs) == [0] and changed.size == 0
    o = np.full(1, 7, np.uint64)
    assert _ffi.vrt().vrt_edit_chunks(gpu._h, None, 0, None, None, None, 0, None, 0, o.ctypes.data, None) == 0 and o[0] == 0


def test_a_set_node_built_tree(gpu):
    dense = W.gen_dense(SEED, (1, 2, 1))
    loose = W.svo_build_by_set_node(dense)
    assert not np.array_equal(loose, W.svo_build_bottom_up(dense))
    out, _, changed = _same(gpu, [(1, 2, 1)], loose, [0, loose.size], [])
    assert np.array_equal(out, W.svo_build_bottom_up(dense)) and list(changed) == [0]
    _, _, changed = _same(gpu, [(1, 2, 1)], loose, [0, loose.size], [shape_sphere((48, 80, 48), 9.9, STONE)])
    assert list(changed) == [1]


def test_a_refused_tree_beside_an_ordinary_chunk(gpu):
    pts = [shape_point((2 * i, 2 * j, 2 * k), STONE) for k in range(16) for j in range(16) for i in range(16)]
    second = W.svo_build_bottom_up(W.gen_dense(SEED, (1, 2, 1)))
    nodes = np.concatenate([[0], second]).astype(np.uint16)
    offs = np.array([0, 1, 1 + second.size], np.uint64)
    pos = [(0, 0, 0), (1, 2, 1)]
    block0 = R.apply(np.zeros(32768, np.uint16), (0, 0, 0), pts).reshape(16, 2, 16, 2, 16, 2)
    assert ((block0.max(axis=(1, 3, 5)) != block0.min(axis=(1, 3, 5))).sum()) >= 4096      # mixed level-4 cells
    out, ooffs, changed = _same(gpu, pos, nodes, offs, pts)
    assert list(ooffs) == [0, 0, second.size] and np.array_equal(out, second) and list(changed) == [1, 0]
    with pytest.raises(VrtError) as e:
        gpu.edit_chunks(pos, nodes, offs, pts)
    assert e.value.code == RANGE


def test_cap_nodes_one_word_short(gpu, block):
    pos, nodes, offs, _ = block
    sh = W.shape_records(_feature(CORNER_CHUNK))
    want, woffs, wchanged = W.edit_chunks(pos, nodes, offs, sh)
    p = np.array(pos, np.int32)
    buf = np.full(want.size + 16, 0xABCD, np.uint16)
    oout = np.full(len(pos) + 1, 99, np.uint64)
    ch = np.full(len(pos), 9, np.uint8)
    lib = _ffi.vrt()
    args = lambda cap: (gpu._h, p.ctypes.data, len(pos), nodes.ctypes.data, offs.ctypes.data, sh.ctypes.data, sh.size, buf.ctypes.data, cap,  # noqa: E731
                        oout.ctypes.data, ch.ctypes.data)
    assert lib.vrt_edit_chunks(*args(want.size - 1)) == OOM
    assert np.array_equal(oout, woffs) and (buf == 0xABCD).all()
    assert lib.vrt_edit_chunks(*args(want.size)) == 0
    assert np.array_equal(buf[:want.size], want) and (buf[want.size:] == 0xABCD).all() and np.array_equal(ch, wchanged)


def test_the_batch_boundary(gpu):
    """A call of one chunk more than a batch answers, and its last chunk is edited.  This is not the test of the per-batch
    offsets: the trees are one word each and the call has one (chunk, shape) pair, so the second batch's bin_off is 0.  That is
    tests/test_gpu_edit_matrix.py's batch cases (hand-made trees of many lengths, shapes on both sides of the boundary)."""
    n = BATCH + 1
    pos = [(i % 64, 0, i // 64) for i in range(n)]
    nodes = np.full(n, 4, np.uint16)
    nodes[::3] = 0
    last = pos[-1]
    out, offs, changed = _same(gpu, pos, nodes, np.arange(n + 1), [shape_point((32 * last[0] + 31, 31, 32 * last[2]), STONE)])
    assert changed.sum() == 1 and changed[-1] == 1 and out.size == BATCH + 41


@pytest.mark.parametrize("case", rejections() + [("more than 2^20 pairs", RANGE, too_many_pairs())], ids=lambda c: c[0])
def test_rejections_leave_the_outputs_untouched(gpu, case):
    """Status and outputs only: the call is refused on the host before anything is enqueued, and no kernel meets these inputs."""
    _, status, kw = case
    lib = _ffi.vrt()
    rc, untouched = call_raw(lambda *a: lib.vrt_edit_chunks(gpu._h, *a), kw)
    assert rc == status and untouched
    assert lib.vrt_last_error(gpu._h)


def test_the_call_touches_nothing_else(block):
    sc = scenes.c1_flat((64, 64))
    g = gpu_for_scene(sc)
    g.render(MODE_PRIMARY)
    rgb0, ids0, _ = g.read_output()
    info0 = bytes(g.accel_info())
    pos, nodes, offs, _ = block
    _, _, changed = g.edit_chunks(pos, nodes, offs, _feature(CORNER_CHUNK))
    assert changed.any()
    assert bytes(g.accel_info()) == info0
    rgb1, ids1, _ = g.read_output()
    assert rgb1.tobytes() == rgb0.tobytes() and ids1.tobytes() == ids0.tobytes()
    g.render(MODE_PRIMARY)
    rgb2, ids2, _ = g.read_output()
    assert rgb2.tobytes() == rgb0.tobytes() and ids2.tobytes() == ids0.tobytes()
    assert bytes(g.accel_info()) == info0
    g.close()


def brush_scene():
    """C1's superflat 2^3 world with a sphere of wood on the common corner of its eight chunks, in view: the scene, the shapes,
    and a second world edited voxel by voxel (the oracle's)."""
    sc = scenes.c1_flat((64, 64))
    shapes = [shape_sphere((32, 32, 32), 6.9, WOOD)]
    by_voxel = scenes.c1_flat((64, 64)).world
    for p in by_voxel.grid_positions():      # (an all-air cell holds no chunk: Svo::set_node needs one)
        if by_voxel.chunk_state(p) is None:
            by_voxel.create_chunk(p, np.zeros(1, np.uint16))
    for p, v in R.placements(shapes):
        try:
            by_voxel.set_voxel(p, v)
        except W.SetVoxelErr as e:
            assert e.kind == "NoChange"
    return sc, shapes, by_voxel


def test_a_brush_end_to_end_renders_the_voxel_by_voxel_worlds_frame(orc):
    sc, shapes, by_voxel = brush_scene()
    want_rgb, want_ids, _, _ = orc.OracleScene(by_voxel.nodes(), by_voxel.chunk_roots(), sc.materials, sc.cam, sc.settings,
                                               by_voxel.world_data()).render(orc.MODE_PRIMARY_SHADOW, 64, 64)
    hit = ((want_ids & _ffi.ID_HIT) != 0) & ((want_ids & _ffi.ID_VOXEL_MASK) == WOOD)
    assert hit.sum() >= 50, f"only {int(hit.sum())} pixels see the sphere"

    g = gpu_for_scene(sc)
    world = sc.world
    pos = [tuple(int(v) for v in p) for p in world.grid_positions()]
    assert len(pos) == 8
    trees = []
    for p in pos:      # the chunks as the world holds them: pool ranges, or the one word 0 for a cell without a chunk
        st = world.chunk_state(p)
        trees.append(np.zeros(1, np.uint16) if st is None else world.nodes()[st.range_start:st.range_start + st.last_used_addr + 1].copy())
    offs = np.concatenate([[0], np.cumsum([t.size for t in trees])]).astype(np.uint64)
    out, ooffs, changed = g.edit_chunks(pos, np.concatenate(trees), offs, shapes)
    assert changed.all()
    for i, p in enumerate(pos):      # the client's flow: create_chunk, then the range to the device
        tree = out[int(ooffs[i]):int(ooffs[i + 1])]
        root = world.create_chunk(p, tree)
        g.write_nodes(world.nodes_ptr(), root, root + tree.size)
    g.write_chunk_roots(world.chunk_roots())
    g.render(MODE_PRIMARY_SHADOW)
    rgb, ids, _ = g.read_output()
    assert_frame_parity(rgb, ids, want_rgb, want_ids, "a sphere placed through vrt_edit_chunks")
    g.close()


def test_a_multi_device_context_answers_like_one_device(gpu, block):
    pos, nodes, offs, _ = block
    grp = Gpu(1 << 16, 2, (64, 64), devices=[0, 0])
    a = grp.edit_chunks(pos, nodes, offs, _feature(CORNER_CHUNK))
    b = gpu.edit_chunks(pos, nodes, offs, _feature(CORNER_CHUNK))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[2].sum() >= 4
    grp.close()
