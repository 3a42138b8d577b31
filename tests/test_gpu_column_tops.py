"""vrt_get_voxels, vrt_column_tops and vrt_read_top_map on the MI355X — whole records held equal to the host twins
(vrth_world_column_tops, vrth_world_top_map) and to the numpy restatement of tests/column_cases.py, which tests/test_column_ref.py
holds to each other without a GPU."""
import numpy as np
import pytest

from voxelraytracing_amd import Gpu, MODE_PRIMARY_SHADOW, VrtError, _ffi, scenes
from voxelraytracing_amd.world import column_queries

import cast_ray_cases as rc
import column_cases as cc
from util import gpu_for_scene

pytestmark = pytest.mark.gpu


def _gpu(world, mats) -> Gpu:
    gpu = Gpu(world.max_nodes(), world.size_in_chunks(), (8, 8), device=0)
    gpu.upload_world(world, mats)
    return gpu


def _same(got, *wants, what=""):
    for k, want in enumerate(wants):
        bad = cc.records_differ(want, got)
        assert bad.size == 0, f"{what}: {bad.size} of {got.size} records differ from reference {k}, first at {bad[:3]}: " \
                              f"want {want.reshape(-1)[bad[:3]]} gpu {got.reshape(-1)[bad[:3]]}"
    return got


def _check_case(gpu, c):
    """Every query, every position and both maps of a case against the reference and the host twins."""
    got = _same(gpu.column_tops(c.q), c.want, c.world.column_tops(c.q, c.mats), what=f"{c.name} column tops")
    gotv = _same(gpu.get_voxels(c.pos), c.want_voxels, c.world.get_voxels(c.pos), what=f"{c.name} voxels")
    print(f"{c.name}: {got.size} column queries, by status {np.bincount(got['status'], minlength=3).tolist()}; "
          f"{gotv.size} positions, by status {np.bincount(gotv['status'], minlength=4).tolist()}")
    for solid in (False, True):
        m = _same(gpu.top_map(solid), c.want_maps[solid], c.world.top_map(solid, c.mats, threads=4), what=f"{c.name} map, solid={solid}")
        single = gpu.column_tops(cc.map_queries(c.dw, solid))                 # the map is (32 S)^2 single queries
        assert (single["status"] != _ffi.COLUMN_OUTSIDE).all()
        assert np.array_equal(single["y"], m["y"].ravel()) and np.array_equal(single["voxel"], m["voxel"].ravel())


@pytest.fixture(scope="module")
def c2():
    return scenes.c2((128, 72))


@pytest.mark.parametrize("name", ["leaf", "strata", "strata255", "mixed"])
def test_the_cases_through_the_tables(name):
    """Leaf jumps over leaves of every size, missing chunks, SOLID, FROM_Y and the bounds (column_cases.check_presence says
    which cases, and that they are there), asked of the derived tables."""
    c = cc.case(name)
    cc.check_presence(c)
    gpu = _gpu(c.world, c.mats)
    _check_case(gpu, c)
    assert gpu.accel_info().available == 1
    gpu.close()


@pytest.mark.parametrize("name", ["leaf", "mixed"])
def test_the_cases_through_the_octree_walk(name, monkeypatch):
    """A world beyond the tables' limit (VRT_ACCEL_MAX_S) is asked through chunk_roots and the node pool: the same answers,
    with the leaf sizes find_node's depth gives."""
    monkeypatch.setenv("VRT_ACCEL_MAX_S", "1")
    c = cc.case(name)
    cc.check_presence(c)
    gpu = _gpu(c.world, c.mats)
    _check_case(gpu, c)
    a = gpu.accel_info()
    assert (a.available, a.builds) == (0, 0)   # no tables were there to ask
    gpu.close()


def test_a_chunk_root_of_zero_is_no_chunk_even_when_node_0_is_solid():
    """The cell grid walks a root of 0 from node 0; get_voxel says NoChunk.  A pool whose node 0 is a solid leaf: the missing
    chunks above the floor hold nothing."""
    w = rc.floor_world()
    gpu = _gpu(w, cc.materials())
    pool = np.array(w.nodes())
    pool[0] = 7
    gpu.write_nodes(pool, 0, 2)
    dw = cc.Dense(w)
    pos = cc.voxel_cases(dw)
    got = _same(gpu.get_voxels(pos), cc.ref_get_voxels(dw, pos), what="root 0 voxels")
    assert (got["status"] == _ffi.VOXEL_NO_CHUNK).sum() > 0 and (got["voxel"][got["status"] != 0] == 0).all()
    assert set(np.unique(got["voxel"]).tolist()) == {0, 1}
    for solid in (False, True):
        m = _same(gpu.top_map(solid), cc.ref_top_map(dw, solid, cc.materials()), w.top_map(solid, cc.materials()), what="root 0 map")
        assert (m["y"] == -1).all() and (m["voxel"] == 1).all()                # only the floor
    gpu.close()


def test_a_material_table_written_after_the_world_is_seen_without_a_frame():
    c = cc.case("strata")
    gpu = _gpu(c.world, c.mats)
    sel = (c.q["flags"] & cc.SOLID) != 0
    q = c.q[sel]
    _same(gpu.column_tops(q), c.want[sel], what="first table")
    first_map = gpu.top_map(True)
    for mats in (cc.materials(liquid_sand=True), cc.materials(liquid_255=True, air_solid=True), c.mats):
        gpu.write_materials(mats)
        want = cc.ref_column_tops(c.dw, q, mats)
        got = _same(gpu.column_tops(q), want, c.world.column_tops(q, mats), what="rewritten table")
        m = _same(gpu.top_map(True), cc.ref_top_map(c.dw, True, mats), what="rewritten table, map")
        changed = cc.records_differ(c.want[sel], got).size
        assert (changed > 0) == (mats is not c.mats) and (cc.records_differ(first_map, m).size > 0) == (mats is not c.mats)
    # one entry alone: water turned solid
    solid_water = cc.materials()
    solid_water[cc.WATER].is_liquid = 0
    gpu.write_materials((_ffi.Material * 1)(solid_water[cc.WATER]), first=cc.WATER)
    got = _same(gpu.column_tops(q), cc.ref_column_tops(c.dw, q, solid_water), what="one entry")
    assert (got["voxel"] == cc.WATER).sum() > 0
    gpu.close()


def test_edits_are_seen_by_the_next_query_without_a_frame():
    w = cc.leaf_world()   # (a world of its own: the shared cases stay as they are)
    gpu = _gpu(w, cc.materials())
    x, y, z = (c - 32 for c in cc.LEAF_TOPS[8])
    q = column_queries([x, x, 20], [z, z, -20], solid=[False, True, False])

    def ask(what):
        dw = cc.Dense(w)
        got = _same(gpu.column_tops(q), cc.ref_column_tops(dw, q, cc.materials()), w.column_tops(q, cc.materials()), what=what)
        _same(gpu.top_map(False), cc.ref_top_map(dw, False), what=what + ", map")
        p = [(x, yy, z) for yy in range(y - 2, y + 12)]
        _same(gpu.get_voxels(p), cc.ref_get_voxels(dw, p), what=what + ", voxels")
        return got["y"].tolist(), got["status"].tolist()

    def edit(p, v):
        start, n = w.set_voxel(p, v)
        gpu.write_nodes(w.nodes_ptr(), start, start + n)

    assert ask("before") == ([y, y, -33], [1, 1, 0])
    edit((x, y + 9, z), cc.SAND)                       # raises the column: into what was an air leaf of side 16
    assert ask("raised") == ([y + 9, y + 9, -33], [1, 1, 0])
    edit((x, y + 10, z), cc.WATER)
    assert ask("water on top") == ([y + 10, y + 9, -33], [1, 1, 0])
    edit((x, y + 10, z), 0)
    edit((x, y + 9, z), 0)
    edit((x, y, z), 0)                                 # digs it down: nothing is left
    edit((20, 3, -20), cc.STONE)                       # ... and the all-air column gets a top
    assert ask("dug") == ([-33, -33, 3], [0, 0, 1])
    gpu.close()


def test_a_query_leaves_the_last_frame_alone(c2):
    gpu = gpu_for_scene(c2)
    gpu.set_frames_in_flight(2)
    lo, W = np.array(c2.world.min_voxel()), c2.world.size_in_voxels()
    rng = np.random.default_rng(8)
    pos = rng.integers(-8, W + 8, (4096, 3)) + lo
    q = column_queries(pos[:, 0], pos[:, 2], from_y=pos[:, 1], solid=rng.random(4096) < 0.5)
    gpu.encode_pass(MODE_PRIMARY_SHADOW)
    results = []
    for ask in (False, True, False, True):
        gpu.stats()
        gpu.encode_pass(MODE_PRIMARY_SHADOW)
        gpu.encode_pass(MODE_PRIMARY_SHADOW)
        if ask:
            gpu.get_voxels(pos)
            gpu.column_tops(q)
            gpu.top_map(True)
        rgb, ids, q8 = gpu.read_output(rgba8=True)
        scr = gpu.present((128, 72))
        s = gpu.stats()
        results.append((rgb, ids, q8, scr, (s.primary_rays, s.secondary_rays, s.hits)))
    for r in results[1:]:
        for a, b in zip(results[0][:4], r[:4]):
            assert np.array_equal(a, b)
        assert r[4] == results[0][4]
    gpu.close()


def test_the_map_of_c2(c2):
    """65 536 columns of the procedural world, both kinds, against the host twin on 16 threads; fuzzed queries with it."""
    gpu = gpu_for_scene(c2)
    W = c2.world.size_in_voxels()
    for solid in (False, True):
        m = _same(gpu.top_map(solid), c2.world.top_map(solid, c2.materials, threads=16), what=f"C2 map, solid={solid}")
        print(f"C2 map, solid={solid}: {int((m['voxel'] != 0).sum())} of {m.size} columns have a top, y from {int(m['y'].min())} to "
              f"{int(m['y'].max())}, {np.unique(m['voxel']).size} voxel ids; table builds {gpu.accel_info().builds}")
        assert m.shape == (W, W) and (m["voxel"] != 0).any()
    lo = np.array(c2.world.min_voxel())
    rng = np.random.default_rng(9)
    pos = rng.integers(-8, W + 8, (20000, 3)) + lo
    q = column_queries(pos[:, 0], pos[:, 2], from_y=pos[:, 1], solid=rng.random(20000) < 0.5)
    q["flags"][::2] &= ~np.uint32(cc.FROM_Y)
    got = _same(gpu.column_tops(q), c2.world.column_tops(q, c2.materials, threads=16), what="C2 fuzz")
    assert {0, 1, 2} <= set(np.unique(got["status"]).tolist())
    gpu.close()


def test_a_multi_device_rehearsal_answers_on_its_first_device():
    c = cc.case("mixed")
    grp = Gpu(c.world.max_nodes(), c.world.size_in_chunks(), (64, 64), devices=[0, 0])
    grp.upload_world(c.world, c.mats)
    _check_case(grp, c)
    grp.close()


BATCHES = (0, 1, 63, 64, 65, 256, 257)


def _batch_inputs(c):
    sel = np.random.default_rng(11).permutation(c.q.size)[:257]
    psel = np.random.default_rng(12).permutation(c.pos.shape[0])[:257]
    return c.q[sel], c.want[sel], np.ascontiguousarray(c.pos[psel]), c.want_voxels[psel]


def test_batch_sizes_from_host_memory():
    c = cc.case("mixed")
    gpu = _gpu(c.world, c.mats)
    q_all, want_all, p_all, wantp_all = _batch_inputs(c)
    for n in BATCHES:
        got = gpu.column_tops(q_all[:n])
        assert got.size == n and cc.records_differ(want_all[:n], got).size == 0, n
        gotp = gpu.get_voxels(p_all[:n])
        assert gotp.size == n and cc.records_differ(wantp_all[:n], gotp).size == 0, n
    gpu.close()


def test_batch_sizes_and_device_pointers():
    torch = pytest.importorskip("torch")
    c = cc.case("mixed")
    gpu = _gpu(c.world, c.mats)
    q_all, want_all, p_all, wantp_all = _batch_inputs(c)

    def on_device(fn, inp: np.ndarray, n, out_dtype):
        din = torch.from_numpy(inp.view(np.uint8).reshape(-1).copy()).to("cuda") if n else None
        dout = torch.full((max(n, 1) * out_dtype.itemsize,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        fn(din.data_ptr() if n else 0, n, dout.data_ptr() if n else 0)
        gpu.synchronize()
        out = dout.cpu().numpy()
        if n == 0:
            assert (out == 0xAB).all()   # n = 0 launches nothing
        return out.view(out_dtype)

    for n in BATCHES:
        d = on_device(gpu.column_tops_device, q_all[:n], n, _ffi.COLUMN_TOP_DTYPE)
        dp = on_device(gpu.get_voxels_device, p_all[:n], n, _ffi.VOXEL_AT_DTYPE)
        if n:
            assert cc.records_differ(want_all[:n], d).size == 0 and cc.records_differ(wantp_all[:n], dp).size == 0, n
    W = c.dw.W
    for flags, solid in ((0, False), (cc.SOLID, True)):
        dmap = torch.full((W * W * 8 + 8,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        gpu.top_map_device(dmap.data_ptr(), flags)
        gpu.synchronize()
        out = dmap.cpu().numpy()
        assert cc.records_differ(c.want_maps[solid], out[:W * W * 8].view(_ffi.TOP_ENTRY_DTYPE)).size == 0
        assert (out[W * W * 8:] == 0xAB).all()
    # what is refused: null and misaligned pointers, map flags other than 0 or SOLID
    buf = torch.zeros(W * W * 8 + 64, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    for call in (lambda: gpu.column_tops_device(0, 4, p), lambda: gpu.column_tops_device(p, 4, 0), lambda: gpu.get_voxels_device(0, 4, p),
                 lambda: gpu.get_voxels_device(p, 4, 0), lambda: gpu.column_tops_device(p + 2, 4, p), lambda: gpu.get_voxels_device(p, 4, p + 1),
                 lambda: gpu.top_map_device(0), lambda: gpu.top_map_device(p + 4), lambda: gpu.top_map_device(p, cc.FROM_Y),
                 lambda: gpu.top_map_device(p, 4), lambda: gpu._ck(gpu._lib.vrt_read_top_map(gpu._h, 0, None)),
                 lambda: gpu._ck(gpu._lib.vrt_read_top_map(gpu._h, 3, p)), lambda: gpu._ck(gpu._lib.vrt_column_tops(gpu._h, None, 1, p)),
                 lambda: gpu._ck(gpu._lib.vrt_get_voxels(gpu._h, p, 1, None))):
        with pytest.raises(VrtError) as e:
            call()
        assert e.value.code == -1
    gpu.synchronize()
    assert not buf.cpu().numpy().any()
    _same(gpu.column_tops(q_all), want_all, what="after the refusals")
    gpu.close()


def test_no_world_no_answer():
    """Where vrt_cast_rays fails for want of a world (validate_frame), so do these."""
    gpu = Gpu(1 << 12, 2, (8, 8), device=0)
    one = column_queries([0], [0])
    codes = []
    for call in (lambda: gpu.cast_rays([(0.5, 0.5, 0.5)], [(0.0, -1.0, 0.0)], 4.0), lambda: gpu.column_tops(one),
                 lambda: gpu.get_voxels([(0, 0, 0)]), lambda: gpu.top_map()):
        with pytest.raises(VrtError) as e:
            call()
        codes.append(e.value.code)
    assert len(set(codes)) == 1 and codes[0] != 0
    gpu.close()
