"""vrt_clip_moves on the MI355X — held bit for bit, whole 32-byte records, to the host mirror vrth_world_clip_moves, which
tests/test_clip_move.py holds to a numpy restatement of clip_aabb_movement and to answers derived by hand."""
import numpy as np
import pytest

from voxelraytracing_amd import Gpu, MODE_PATH, MODE_PRIMARY_SHADOW, VrtError, _ffi, scenes, std_materials
from voxelraytracing_amd.world import box_queries

import clip_cases as cl
from util import gpu_for_scene

pytestmark = pytest.mark.gpu


def _same(world, mats, gpu, q, what=""):
    want = world.clip_moves(q, mats)
    got = gpu.clip_moves(q)
    bad = cl.records_differ(want, got)
    assert bad.size == 0, f"{what}: {bad.size} of {q.size} boxes differ, first {q[bad[:3]]}: host {want[bad[:3]]} gpu {got[bad[:3]]}"
    return got


def _gpu_for_world(w, mats, **kw):
    gpu = Gpu(w.max_nodes(), w.size_in_chunks(), (8, 8), **({"device": 0} if "devices" not in kw else {}), **kw)
    gpu.upload_world(w, mats)
    return gpu


@pytest.fixture(scope="module")
def c2():
    return scenes.c2((64, 64))


@pytest.mark.parametrize("which", ["floor", "c1", "p4", "c2", "s16"])
def test_fuzzed_boxes_are_the_host_mirror(which, c2):
    if which == "floor":
        w, mats = cl.floor_world(), cl.floor_materials()
    else:
        sc = {"c1": lambda: scenes.c1_flat((64, 64)), "p4": lambda: scenes.procedural(4, (64, 64)), "c2": lambda: c2,
              "s16": lambda: scenes.procedural(16, (64, 64))}[which]()
        w, mats = sc.world, sc.materials
    gpu = _gpu_for_world(w, mats)
    q = cl.fuzz_queries(w, 20000, seed=31)
    got = _same(w, mats, gpu, q, which)
    facts = cl.population_facts(q, got)
    print(which, facts)
    cl.assert_population(facts, which)
    gpu.close()


def test_a_million_player_boxes_on_c2(c2):
    gpu = gpu_for_scene(c2)
    q = cl.player_queries(c2.world, 1 << 20, seed=41)
    got = _same(c2.world, c2.materials, gpu, q, "a million players")
    print("players:", cl.population_facts(q, got))
    assert ((got["flags"] & _ffi.BOX_CLIPPED_Y) != 0).mean() > 0.5 and ((got["flags"] & _ffi.BOX_STEPPED_UP) != 0).any()
    gpu.close()


def test_the_known_answers():
    """tests/test_clip_move.py's hand-derived records, on the GPU."""
    w, mats = cl.known_world(), std_materials()
    gpu = _gpu_for_world(w, mats)
    q = np.concatenate([box_queries([(0.25, 0.0, 0.25)], [(0.75, 2.0, 0.75)], [(0.0, -0.05, 0.0)]),
                        box_queries([(4.0, 0.0, -0.25)], [(4.5, 2.0, 0.25)], [(1.0, 0.0, 0.0)]),
                        box_queries([(1.0, 0.0, 10.25)], [(1.5, 2.0, 10.75)], [(1.0, -0.05, 0.0)]),
                        box_queries([(1.0, 0.0, 10.25)], [(1.5, 2.0, 10.75)], [(1.0, -0.05, 0.0)], False),
                        box_queries([(4.0, 0.0, 19.75)], [(4.5, 2.0, 20.25)], [(1.0, 0.0, 0.0)]),
                        box_queries([(1.0, 0.0, 10.0)], [(2.0, 2.0, 11.0)], [(0.25, 0.0, 0.0)], False),
                        box_queries([(0.25, 0.0, 0.25)], [(0.75, 2.0, 0.75)], [(-0.0, 0.0, -0.0)]),
                        box_queries([(0.0, 40.0, 0.0)], [(4096.0, 41.0, 1.0)], [(0.0, 0.0, 0.0)]),
                        box_queries([(0.0, 40.0, 0.0)], [(4097.0, 41.0, 1.0)], [(0.0, 0.0, 0.0)]),
                        box_queries([(0.25, np.nan, 0.25)], [(0.75, 2.0, 0.75)], [(0.0, -0.05, 0.0)])])
    got = _same(w, mats, gpu, q, "known answers")
    eps, half, one = 0x3727C5AC, 0x3EFFFEB0, 0x3F800054
    assert got["mv"].view(np.uint32).tolist() == [[0, eps, 0], [half, 0, 0], [0x3F800000, one, 0], [half, eps, 0], [0x3F800000, 0, 0],
                                                  [0xB727C5AC, 0, 0], [0x80000000, 0, 0x80000000], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert got["flags"].tolist() == [2, 1, 11, 3, 0, 1, 0, 0, 0, 0]
    assert got["boxes"].tolist() == [[1, 0], [4, 2], [3, 0], [3, 0], [0, 0], [1, 0], [0, 0], [0, 0], [0, 0], [0, 0]]
    assert got["status"].tolist() == [0] * 8 + [2, 2]
    gpu.close()


def test_the_octree_walk_without_tables(monkeypatch):
    """A world beyond the tables' limit (VRT_ACCEL_MAX_S) is asked through chunk_roots and the node pool."""
    monkeypatch.setenv("VRT_ACCEL_MAX_S", "1")
    sc = scenes.procedural(4, (64, 64))
    gpu = gpu_for_scene(sc)
    _same(sc.world, sc.materials, gpu, cl.fuzz_queries(sc.world, 20000, seed=32), "walk")
    gpu.close()


def test_a_world_whose_min_has_mixed_signs():
    from voxelraytracing_amd import ClientWorld
    w = ClientWorld((4, 2, -2), 1 << 22, 4)
    w.generate(0, 5)
    assert tuple(w.min_voxel()) == (64, 0, -128)
    mats = std_materials()
    gpu = _gpu_for_world(w, mats)
    q = cl.fuzz_queries(w, 20000, seed=34)
    got = _same(w, mats, gpu, q, "mixed-sign min")
    assert ((got["flags"] & 7) != 0).mean() > 0.1
    gpu.close()


def test_a_chunk_root_of_zero_is_no_chunk_even_when_node_0_is_solid():
    """The cell grid walks a root of 0 from node 0; the reference's get_voxel says NoChunk: the missing chunks above the
    floor gather nothing even when the pool's node 0 is a solid leaf."""
    w, mats = cl.floor_world(), cl.floor_materials()
    gpu = _gpu_for_world(w, mats)
    pool = np.array(w.nodes())
    pool[0] = 7
    gpu.write_nodes(pool, 0, 2)
    q = cl.fuzz_queries(w, 4096, seed=35)
    got = _same(w, mats, gpu, q, "root 0")
    assert ((got["flags"] & 7) != 0).any()
    up = box_queries([(-3.0, 5.0, -3.0)], [(3.0, 9.0, 3.0)], [(0.5, -0.5, 0.5)])
    assert _same(w, mats, gpu, up, "above the floor")["boxes"][0].tolist() == [0, 0]
    gpu.close()


def test_an_edit_and_a_material_write_are_seen_without_a_frame(c2):
    sc = scenes.c2((64, 64))
    gpu = gpu_for_scene(sc)
    gpu.encode_pass(MODE_PRIMARY_SHADOW)   # the tables exist and a frame is in flight
    w, mats = sc.world, sc.materials
    c = w.size_in_chunks() * 16
    y = w.highest_vox_at(c, c) + 1
    v = w.get_voxel((c, y - 1, c))
    assert cl.solid_table(mats)[v]
    q = box_queries([(c + 0.05, y, c + 0.05)], [(c + 0.95, y + 4.0, c + 0.95)], [(0.0, -0.05, 0.0)])
    first = _same(w, mats, gpu, q, "before the edit")
    assert first["flags"][0] == _ffi.BOX_CLIPPED_Y
    start, n = w.set_voxel((c, y - 1, c), 0)
    gpu.write_nodes(w.nodes_ptr(), start, start + n)
    second = _same(w, mats, gpu, q, "after the edit")
    assert second["flags"][0] == 0 and second["boxes"][0, 0] == 0
    start, n = w.set_voxel((c, y - 1, c), v)
    gpu.write_nodes(w.nodes_ptr(), start, start + n)
    assert _same(w, mats, gpu, q, "after the placement")["flags"][0] == _ffi.BOX_CLIPPED_Y
    # the same voxel's material turns liquid: nothing under the box any more
    mats[v].is_liquid = 1
    gpu.write_materials(mats)
    third = _same(w, mats, gpu, q, "after the material write")
    assert third["flags"][0] == 0 and third["boxes"][0, 0] == 0
    _same(w, mats, gpu, cl.fuzz_queries(w, 4000, seed=36), "the liquid world")
    gpu.close()


def test_a_clip_leaves_the_last_frame_alone(c2):
    sc = scenes.c2((128, 72))
    gpu = gpu_for_scene(sc)
    gpu.set_frames_in_flight(2)
    q = cl.player_queries(sc.world, 4096, seed=37)
    gpu.encode_pass(MODE_PRIMARY_SHADOW)
    results = []
    for clip in (False, True, False, True):
        gpu.stats()
        gpu.encode_pass(MODE_PRIMARY_SHADOW)
        gpu.encode_pass(MODE_PRIMARY_SHADOW)
        if clip:
            gpu.clip_moves(q)
        rgb, ids, q8 = gpu.read_output(rgba8=True)
        scr = gpu.present((128, 72))
        s = gpu.stats()
        results.append((rgb, ids, q8, scr, (s.primary_rays, s.secondary_rays, s.hits)))
    for r in results[1:]:
        for a, b in zip(results[0][:4], r[:4]):
            assert np.array_equal(a, b)
        assert r[4] == results[0][4]
    gpu.close()


def test_a_clip_does_not_restart_the_accumulation():
    sc = scenes.c4((64, 36))
    q = cl.player_queries(sc.world, 1024, seed=38)
    frames = []
    for clip in (False, True):
        gpu = gpu_for_scene(sc)
        for k in range(4):
            gpu.encode_pass(MODE_PATH, spp=1, seed=7, accumulate=True)
            if clip:
                gpu.clip_moves(q)
        rgb, ids, _ = gpu.read_output()
        assert gpu.accumulation()[0] == 4
        frames.append((rgb, ids))
        gpu.close()
    assert np.array_equal(frames[0][0], frames[1][0]) and np.array_equal(frames[0][1], frames[1][1])


def test_a_multi_device_rehearsal_answers_on_its_first_device(c2):
    grp = gpu_for_scene(c2, devices=[0, 0])
    _same(c2.world, c2.materials, grp, cl.fuzz_queries(c2.world, 4000, seed=39), "rehearsal")
    grp.close()


def test_batch_sizes_and_device_pointers(c2):
    torch = pytest.importorskip("torch")
    gpu = gpu_for_scene(c2)
    q_all = cl.fuzz_queries(c2.world, 257, seed=40)
    want_all = c2.world.clip_moves(q_all, c2.materials)
    for n in (0, 1, 63, 64, 65, 257):
        q = q_all[:n]
        got = gpu.clip_moves(q)
        assert got.size == n and cl.records_differ(want_all[:n], got).size == 0, n
        dq = torch.from_numpy(q.view(np.uint8).copy()).to("cuda")
        dout = torch.full((max(n, 1) * 32,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        gpu.clip_moves_device(dq.data_ptr() if n else 0, n, dout.data_ptr() if n else 0)
        gpu.synchronize()
        out = dout.cpu().numpy()
        if n:
            assert cl.records_differ(want_all[:n], out.view(_ffi.BOX_MOVE_DTYPE)).size == 0, n
        else:
            assert (out == 0xAB).all()   # n = 0 launches nothing
    dq = torch.zeros(4 * 48 + 8, dtype=torch.uint8, device="cuda")
    dout = torch.zeros(4 * 32 + 8, dtype=torch.uint8, device="cuda")
    for qp, op in ((0, 0), (dq.data_ptr() + 2, dout.data_ptr()), (dq.data_ptr(), dout.data_ptr() + 1)):   # null, misaligned
        with pytest.raises(VrtError) as e:
            gpu.clip_moves_device(qp, 4, op)
        assert e.value.code == -1
    gpu.close()


def test_one_wave_whose_lanes_all_gather_a_different_number_of_boxes():
    """64 boxes inside the floor world's solid half (x, z in [-32, 32), y in [-32, 0)): lane k's range is solid throughout and
    holds a number of voxels of its own, from none (lane 0, in the air) to the cap's 4096 (lane 63)."""
    w, mats = cl.floor_world(), cl.floor_materials()
    gpu = _gpu_for_world(w, mats)
    dims = [(0, 0, 0)] + [(k, 1 + k // 4, 1) for k in range(1, 63)] + [(16, 16, 16)]   # k (1 + k // 4) grows with k, to 992
    frm, to = [], []
    for nx, ny, nz in dims:
        if nx == 0:
            frm.append((0.0, 5.0, 0.0)), to.append((1.0, 6.0, 1.0))
        else:
            frm.append((-31.0, -20.0, -16.0)), to.append((-31.0 + nx, -20.0 + ny, -16.0 + nz))
    q = box_queries(frm, to, [(0.0, 0.0, 0.0)] * len(frm), True)
    assert q.size == 64
    got = _same(w, mats, gpu, q, "one wave")
    n = got["boxes"][:, 0].tolist()
    assert len(set(n)) == 64 and min(n) == 0 and max(n) == 4096, sorted(n)
    # ... and the same wave moving: every lane clips against its own number of boxes
    q["mv"] = (0.25, -0.25, 0.5)
    q["to"][63] = (-0.5, -4.5, -0.5)
    q["from"][63] = (-15.5, -19.5, -15.5)   # (expanded by mv it still spans 16 voxels on every axis)
    got = _same(w, mats, gpu, q, "one wave, moving")
    assert got["status"].tolist() == [0] * 64 and got["boxes"][63, 0] == 4096
    gpu.close()
