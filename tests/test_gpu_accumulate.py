"""Progressive accumulation of path-traced frames (VRT_RENDER_ACCUMULATE, include/vrt.h).

The identity: an accumulating frame with n samples in the sum traces samples n .. n + spp - 1 and adds them in sample order,
so K accumulated frames of s spp are, bit for bit, one plain frame of K * s spp with the same seed — whatever the frames in
flight, the chain boundaries (8 samples a launch chain), the one-sample and the plane paths in between."""
import numpy as np
import pytest

from voxelraytracing_amd import MODE_PATH, MODE_PRIMARY, MODE_PRIMARY_SHADOW, VrtError, _ffi, scenes
from voxelraytracing_amd import graphics as g

from util import assert_frame_parity, gpu_for_scene

pytestmark = pytest.mark.gpu

SEED = 11


def _plain(gpu, spp, seed=SEED, **kw):
    """The plain (non-accumulating) frame of `spp` samples, read back."""
    gpu.render(MODE_PATH, spp=spp, seed=seed, **kw)
    rgb, ids, _ = gpu.read_output()
    return rgb, ids


def _acc(gpu, spp, seed=SEED, **kw):
    gpu.render(MODE_PATH, spp=spp, seed=seed, accumulate=True, **kw)
    rgb, ids, _ = gpu.read_output()
    return rgb, ids


def _same(a, b, what):
    assert np.array_equal(a[1], b[1]), f"{what}: id words differ"
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f"{what}: radiance differs (max {np.abs(a[0] - b[0]).max()})"


@pytest.mark.parametrize("size", [(480, 272), (100, 60)])
@pytest.mark.parametrize("in_flight", [1, 2, 4])
def test_accumulated_frames_are_one_frame_of_all_their_samples(size, in_flight):
    sc = scenes.c4(size)
    gpu = gpu_for_scene(sc)
    gpu.set_frames_in_flight(in_flight)
    want = {n: _plain(gpu, n) for n in (1, 4, 6, 8)}
    # four 1-spp frames back to back, in flight together, read once
    for _ in range(4):
        gpu.render(MODE_PATH, spp=1, seed=SEED, accumulate=True)
    rgb, ids, _ = gpu.read_output()
    _same((rgb, ids), want[4], f"{size} in flight {in_flight}: 4 x 1 spp")
    assert gpu.accumulation() == (4, SEED)
    # 1, 3, 2, 2: the one-sample path, then the plane path across the 8-sample chain boundary; every frame's output is the
    # plain frame of the samples so far
    gpu.reset_accumulation()
    n = 0
    for spp in (1, 3, 2, 2):
        n += spp
        _same(_acc(gpu, spp), want[n], f"{size} in flight {in_flight}: after {n} samples")
        assert gpu.accumulation() == (n, SEED)
    # the same sequence without a read in between (the sum's steps ordered across the frame sets' streams)
    gpu.reset_accumulation()
    for spp in (1, 3, 2, 2):
        gpu.render(MODE_PATH, spp=spp, seed=SEED, accumulate=True)
    rgb, ids, _ = gpu.read_output()
    _same((rgb, ids), want[8], f"{size} in flight {in_flight}: 1 + 3 + 2 + 2 unread")
    gpu.close()


def test_accumulation_matches_the_oracle(orc):
    sc = scenes.c4((128, 72))
    gpu = gpu_for_scene(sc)
    for spp in (1, 2, 1, 4):
        gpu.render(MODE_PATH, spp=spp, seed=SEED, accumulate=True)
    rgb, ids, _ = gpu.read_output()
    assert gpu.accumulation() == (8, SEED)
    r_rgb, r_ids, _, _ = orc.from_package_scene(sc).render(orc.MODE_PATH, 128, 72, spp=8, seed=SEED)
    assert_frame_parity(rgb, ids, r_rgb, r_ids, "8 accumulated samples")
    gpu.close()


def _restart_case(gpu, sc, what, change):
    """Accumulate a few samples, apply `change`, and check that the next frame starts again."""
    gpu.reset_accumulation()
    for _ in range(3):
        gpu.render(MODE_PATH, spp=1, seed=SEED, accumulate=True)
    seed = change() or SEED
    got = _acc(gpu, 1, seed=seed)
    assert gpu.accumulation() == (1, seed), what
    _same(got, _plain(gpu, 1, seed=seed), f"restart on {what}")


def test_what_restarts_the_accumulation():
    sc = scenes.c4((128, 72))
    gpu = gpu_for_scene(sc)
    w, h = sc.size
    world = sc.world

    def camera():
        gpu.write_cam_data(g.cam_data_create((sc.rot[0] + 3.0, sc.rot[1] + 5.0, sc.rot[2]), sc.eye, 70.0, (float(w), float(h))))

    def settings():
        sc.settings.sun_pos[0] += 40.0
        gpu.write_settings(sc.settings)

    def world_bytes():
        wd = world.world_data()
        wd.min[0] -= 1
        gpu.write_world_data(wd)

    def world_back():
        gpu.write_world_data(world.world_data())

    def materials():
        sc.materials[3].color[0] *= 0.5
        gpu.write_materials(sc.materials)

    def nodes():   # any non-empty write, even of the same bytes
        gpu.write_nodes(world.nodes_ptr(), 0, 2)

    roots = np.array(world.chunk_roots(), dtype=np.uint32)

    def chunk_roots():
        r = roots.copy()
        r[len(r) // 2] = 0
        gpu.write_chunk_roots(r)

    def roots_back():
        gpu.write_chunk_roots(roots)

    def resize_world():
        gpu.resize_chunk_buffer(world.size_in_chunks())
        gpu.write_chunk_roots(roots)

    def resize_output():
        gpu.resize_result_texture((w + 8, h))

    def seed():
        return SEED + 1

    for what, change in [("camera", camera), ("settings", settings), ("world data", world_bytes), ("world data back", world_back),
                         ("materials", materials), ("nodes", nodes), ("chunk roots", chunk_roots), ("chunk roots back", roots_back),
                         ("resize_world", resize_world), ("resize_output", resize_output), ("seed", seed)]:
        _restart_case(gpu, sc, what, change)
    gpu.close()


def test_what_does_not_restart_the_accumulation():
    sc = scenes.c4((128, 72))
    gpu = gpu_for_scene(sc)
    world = sc.world
    roots = np.array(world.chunk_roots(), dtype=np.uint32)
    want = {n: _plain(gpu, n) for n in range(1, 10)}
    steps = [
        ("identical camera", lambda: gpu.write_cam_data(sc.cam)),
        ("identical settings", lambda: gpu.write_settings(sc.settings)),
        ("identical world data", lambda: gpu.write_world_data(world.world_data())),
        ("identical chunk roots", lambda: gpu.write_chunk_roots(roots)),
        ("tagged chunk roots", lambda: (gpu.write_chunk_roots(roots, tag=77), gpu.write_chunk_roots(roots, tag=77))),
        ("a primary frame", lambda: gpu.render(MODE_PRIMARY)),
        ("a primary + shadow frame", lambda: gpu.render(MODE_PRIMARY_SHADOW)),
        ("a plain path frame of another seed", lambda: gpu.render(MODE_PATH, spp=3, seed=SEED + 5)),
    ]
    _acc(gpu, 1)
    for n, (what, step) in enumerate(steps, start=2):
        step()
        got = _acc(gpu, 1)
        assert gpu.accumulation() == (n, SEED), what
        _same(got, want[n], f"after {what}")
    gpu.close()


def test_present_and_rgba8_of_an_accumulated_frame():
    sc = scenes.c4((128, 72))
    gpu = gpu_for_scene(sc)
    gpu.render(MODE_PATH, spp=6, seed=SEED)
    _, _, q_want = gpu.read_output(rgb=False, ids=False, rgba8=True)
    p_want = gpu.present()
    p2_want = gpu.present((200, 100))
    for spp in (2, 1, 3):
        gpu.render(MODE_PATH, spp=spp, seed=SEED, accumulate=True)
    _, _, q = gpu.read_output(rgb=False, ids=False, rgba8=True)
    assert np.array_equal(q, q_want)
    assert np.array_equal(gpu.present(), p_want)
    assert np.array_equal(gpu.present((200, 100)), p2_want)
    gpu.close()


def test_stats_frames_accumulate():
    sc = scenes.c4((128, 72))
    gpu = gpu_for_scene(sc)
    want = _plain(gpu, 5)
    gpu.render(MODE_PATH, spp=2, seed=SEED, accumulate=True, stats=True)
    gpu.render(MODE_PATH, spp=1, seed=SEED, accumulate=True)
    got = _acc(gpu, 2, stats=True)
    _same(got, want, "stats frames")
    assert gpu.stats().primary_rays > 0
    gpu.close()


def test_shards_and_devices_accumulate_their_own_tiles():
    sc = scenes.c4((160, 96))
    whole = gpu_for_scene(sc)
    want = _plain(whole, 3)
    whole.close()
    acc_rgb, acc_ids = np.zeros_like(want[0]), np.zeros_like(want[1])
    for r in range(4):
        sh = gpu_for_scene(sc, shard_rank=r, shard_count=4)
        sh.render(MODE_PATH, spp=1, seed=SEED, accumulate=True)
        rgb, ids = _acc(sh, 2)
        assert sh.accumulation() == (3, SEED)
        acc_rgb += rgb
        acc_ids |= ids
        sh.close()
    _same((acc_rgb, acc_ids), want, "the union of four shards")
    grp = gpu_for_scene(sc, devices=[0, 0], texel_messages=True)
    grp.render(MODE_PATH, spp=2, seed=SEED, accumulate=True)
    grp.render(MODE_PATH, spp=1, seed=SEED, accumulate=True)
    rgb, ids, _ = grp.read_output()
    assert grp.accumulation() == (3, SEED)
    _same((rgb, ids), want, "two devices with texel messages")
    grp.reset_accumulation()
    _same(_acc(grp, 3), want, "two devices after a reset")
    grp.close()


def test_a_bound_output_receives_the_mean():
    import torch
    from voxelraytracing_amd.shard import texels_to_frame
    sc = scenes.c4((128, 72))
    gpu = gpu_for_scene(sc)
    want = _plain(gpu, 3)
    buf = torch.zeros((72, 128, 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gpu.bind_output(buf.data_ptr())
    gpu.render(MODE_PATH, spp=1, seed=SEED, accumulate=True)
    gpu.render(MODE_PATH, spp=2, seed=SEED, accumulate=True)
    gpu.synchronize()
    _same(texels_to_frame(buf.cpu().numpy().view(np.uint32)), want, "bound output")
    gpu.bind_output(0)
    gpu.close()


def test_refused_frames_enqueue_nothing():
    sc = scenes.c4((128, 72))
    gpu = gpu_for_scene(sc)
    first = _acc(gpu, 2)
    for mode in (MODE_PRIMARY, MODE_PRIMARY_SHADOW):
        with pytest.raises(VrtError) as e:
            gpu.render(mode, accumulate=True)
        assert e.value.code == _ffi.VRT_ERR_INVALID_ARG
    with pytest.raises(VrtError) as e:
        gpu.render(MODE_PATH, spp=(1 << 24) - 1, seed=SEED, accumulate=True)   # 2 + 2^24 - 1 > 2^24
    assert e.value.code == _ffi.VRT_ERR_OUT_OF_RANGE
    assert gpu.accumulation() == (2, SEED)
    rgb, ids, _ = gpu.read_output()
    _same((rgb, ids), first, "the output after the refused frames")
    _same(_acc(gpu, 1), _plain(gpu, 3), "the accumulation after the refused frames")
    gpu.close()
