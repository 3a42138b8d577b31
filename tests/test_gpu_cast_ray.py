"""vrt_cast_rays on the MI355X — held bit for bit (pos, face, the bits of dist, status) to the host mirror vrth_world_cast_ray,
which tests/test_cast_ray.py holds to a numpy restatement of common::math::cast_ray."""
import numpy as np
import pytest

from voxelraytracing_amd import Gpu, MODE_PRIMARY_SHADOW, VrtError, _ffi, scenes
from voxelraytracing_amd.world import ray_queries

import cast_ray_cases as cc
from util import gpu_for_scene

pytestmark = pytest.mark.gpu

START = (0.5, 2.5, 0.5)


def _same(world, gpu, q, what=""):
    want = world.cast_rays(q["start"], q["dir"], q["max_dist"])
    got = gpu.cast_rays(q["start"], q["dir"], q["max_dist"])
    bad = cc.records_equal(want, got)
    assert bad.size == 0, f"{what}: {bad.size} of {q.size} rays differ, first {q[bad[:3]]}: host {want[bad[:3]]} gpu {got[bad[:3]]}"
    return got


def _camera_rays(sc, n_side=1024):
    """n_side^2 view rays around the scene camera's rotation (axis_rot_to_ray, math.rs:131-146, over a 70-degree square)."""
    pitch0, yaw0 = np.radians(np.float32(sc.rot[0])), np.radians(np.float32(sc.rot[1]))
    a = np.radians(np.linspace(-35.0, 35.0, n_side, dtype=np.float32))
    p, y = np.meshgrid(pitch0 + a, yaw0 + a, indexing="ij")
    p, y = p.ravel().astype(np.float32), y.ravel().astype(np.float32)
    r = np.cos(p)
    dirs = np.stack([r * -np.sin(y), -np.sin(p), r * -np.cos(y)], axis=1).astype(np.float32)
    return np.broadcast_to(np.asarray(sc.eye, np.float32), dirs.shape), dirs


@pytest.fixture(scope="module")
def c2():
    return scenes.c2((64, 64))


@pytest.mark.parametrize("which", ["c1", "c2", "s16"])
def test_fuzzed_rays_are_the_host_mirror(which, c2):
    sc = {"c1": lambda: scenes.c1_flat((64, 64)), "c2": lambda: c2, "s16": lambda: scenes.procedural(16, (64, 64))}[which]()
    gpu = gpu_for_scene(sc)
    q = cc.fuzz_queries(sc.world, 20000, seed=21)
    got = _same(sc.world, gpu, q, which)
    assert {0, 1, 2} <= set(np.unique(got["status"]).tolist())
    gpu.close()


def test_the_octree_walk_without_tables(monkeypatch):
    """A world beyond the tables' limit (VRT_ACCEL_MAX_S) is cast through chunk_roots and the node pool."""
    monkeypatch.setenv("VRT_ACCEL_MAX_S", "1")
    sc = scenes.c1_flat((64, 64))
    gpu = gpu_for_scene(sc)
    _same(sc.world, gpu, cc.fuzz_queries(sc.world, 20000, seed=22), "walk")
    gpu.close()


@pytest.mark.parametrize("max_dist", [10.0, 300.0])
def test_a_million_camera_rays_of_c2(max_dist, c2):
    gpu = gpu_for_scene(c2)
    starts, dirs = _camera_rays(c2)
    # half of them from the scene's eye, half from a player's eye 2.5 voxels above the terrain (the client's pick)
    c = c2.world.size_in_chunks() * 16
    starts = np.array(starts)
    starts[starts.shape[0] // 2:] = (c + 0.5, c2.world.highest_vox_at(c, c) + 2.5, c + 0.5)
    q = ray_queries(starts, dirs, max_dist)
    got = _same(c2.world, gpu, q, f"camera rays, max_dist {max_dist}")
    print(f"max_dist {max_dist}: {int((got['status'] == 1).sum())} of {q.size} hit")
    gpu.close()


def test_the_known_answers():
    w = cc.floor_world()
    gpu = Gpu(w.max_nodes(), w.size_in_chunks(), (8, 8), device=0)
    gpu.upload_world(w)
    dirs = [(-0.0, -0.0, -1.0), (1.0, 0.0, 1.0), (0.0, -1.0, 0.0), (0.3, -1.0, 0.2), (1.0, -1.0, 1.0), (0.0, 0.0, 0.0)]
    got = gpu.cast_rays([START] * len(dirs), dirs, 10.0)
    assert got["status"].tolist() == [0, 0, 1, 1, 1, 0]
    assert got["pos"][2:5].tolist() == [[0, -1, 0], [1, -1, 0], [0, -1, 0]]
    assert got["dist"][2:5].tolist() == [2.5, 2.657536506652832, 4.330126762390137]
    gpu.close()


def test_a_chunk_root_of_zero_is_no_chunk_even_when_node_0_is_solid():
    """The cell grid walks a root of 0 from node 0; the reference's get_voxel says NoChunk.  A pool whose node 0 is a solid
    leaf: the missing chunks above the floor must stay empty."""
    w = cc.floor_world()
    gpu = Gpu(w.max_nodes(), w.size_in_chunks(), (8, 8), device=0)
    gpu.upload_world(w)
    pool = np.array(w.nodes())
    pool[0] = 7
    gpu.write_nodes(pool, 0, 2)
    rng = np.random.default_rng(4)
    starts = rng.uniform([-31.0, 0.5, -31.0], [31.0, 31.0, 31.0], (4096, 3)).astype(np.float32)
    dirs = rng.normal(size=(4096, 3)).astype(np.float32)
    got = _same(w, gpu, ray_queries(starts, dirs, 300.0), "root 0")
    hit = got["status"] == 1
    assert hit.any() and (got["pos"][hit][:, 1] < 0).all()   # only the floor
    gpu.close()


def test_an_edit_is_seen_by_the_next_cast_without_a_frame(c2):
    sc = scenes.c2((64, 64))
    gpu = gpu_for_scene(sc)
    gpu.encode_pass(MODE_PRIMARY_SHADOW)   # the tables exist and a frame is in flight
    eye = np.asarray(sc.eye, np.float32)
    q = ray_queries([eye] * 3, [(0.0, -1.0, 0.0), (0.1, -1.0, 0.05), (-0.2, -1.0, 0.1)], 300.0)
    first = _same(sc.world, gpu, q, "before the edit")
    assert (first["status"] == 1).all()
    for p in {tuple(int(c) for c in p) for p in first["pos"]}:
        start, n = sc.world.set_voxel(p, 0)
        gpu.write_nodes(sc.world.nodes_ptr(), start, start + n)
    second = _same(sc.world, gpu, q, "after the edit")
    assert not np.array_equal(first["pos"], second["pos"])
    # ... and a voxel placed in front of the ray (the client's right click: hit.pos + hit.face)
    p = second["pos"][0] + second["face"][0]
    start, n = sc.world.set_voxel(tuple(int(c) for c in p), 4)
    gpu.write_nodes(sc.world.nodes_ptr(), start, start + n)
    third = _same(sc.world, gpu, q, "after the placement")
    assert third["pos"][0].tolist() == p.tolist()
    gpu.close()


def test_a_cast_leaves_the_last_frame_alone(c2):
    sc = scenes.c2((128, 72))
    gpu = gpu_for_scene(sc)
    gpu.set_frames_in_flight(2)
    starts, dirs = _camera_rays(sc, 64)
    gpu.encode_pass(MODE_PRIMARY_SHADOW)
    results = []
    for cast in (False, True, False, True):
        gpu.stats()
        gpu.encode_pass(MODE_PRIMARY_SHADOW)
        gpu.encode_pass(MODE_PRIMARY_SHADOW)
        if cast:
            gpu.cast_rays(starts, dirs, 300.0)
        rgb, ids, q = gpu.read_output(rgba8=True)
        scr = gpu.present((128, 72))
        s = gpu.stats()
        results.append((rgb, ids, q, scr, (s.primary_rays, s.secondary_rays, s.hits)))
    for r in results[1:]:
        for a, b in zip(results[0][:4], r[:4]):
            assert np.array_equal(a, b)
        assert r[4] == results[0][4]
    gpu.close()


def test_a_multi_device_rehearsal_casts_on_its_first_device(c2):
    grp = gpu_for_scene(c2, devices=[0, 0])
    _same(c2.world, grp, cc.fuzz_queries(c2.world, 4000, seed=23), "rehearsal")
    grp.close()


def test_batch_sizes_and_device_pointers(c2):
    torch = pytest.importorskip("torch")
    gpu = gpu_for_scene(c2)
    q_all = cc.fuzz_queries(c2.world, 65, seed=24)
    want_all = c2.world.cast_rays(q_all["start"], q_all["dir"], q_all["max_dist"])
    for n in (0, 1, 63, 65):
        q = q_all[:n]
        got = gpu.cast_rays(q["start"], q["dir"], q["max_dist"])
        assert got.size == n and cc.records_equal(want_all[:n], got).size == 0, n
        dq = torch.from_numpy(q.view(np.uint8).copy()).to("cuda")
        dout = torch.full((max(n, 1) * 32,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        gpu.cast_rays_device(dq.data_ptr() if n else 0, n, dout.data_ptr() if n else 0)
        gpu.synchronize()
        out = dout.cpu().numpy()
        if n:
            assert cc.records_equal(want_all[:n], out.view(_ffi.RAY_HIT_DTYPE)).size == 0, n
        else:
            assert (out == 0xAB).all()   # n = 0 launches nothing
    with pytest.raises(VrtError) as e:
        gpu.cast_rays_device(0, 4, 0)
    assert e.value.code == -1
    gpu.close()


def test_one_wave_of_ties_and_zero_components():
    sc = scenes.c1_flat((64, 64))
    gpu = gpu_for_scene(sc)
    dirs = [(1, 0, 1), (1, 1, 0), (0, 1, 1), (1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, -1, 1), (0, -1, 0), (-0.0, -1, -0.0),
            (-0.0, -0.0, -1), (0, 0, 0), (-0.0, -0.0, -0.0), (2, -2, 0), (0.5, -0.5, -0.5), (1, -1, -0.0), (-0.0, -1, 1)]
    starts = [(32.0, 20.0, 32.0), (32.5, 20.5, 32.5), (10.0, 16.5, 50.5), (0.5, 40.0, 0.0)]
    s = np.repeat(np.asarray(starts, np.float32), len(dirs), axis=0)
    d = np.tile(np.asarray(dirs, np.float32), (len(starts), 1))
    q = ray_queries(s, d, np.float32(60.0))
    assert q.size == 64
    _same(sc.world, gpu, q, "one wave")
    gpu.close()
