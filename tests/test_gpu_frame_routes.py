"""The routes a frame can take through vrt_render (csrc/vrt_frame_plan.h: one launch or two, the fallback to the octree walk, frames
in flight, stats frames, the path trace's chains and every schedule of its launches) on the small C1 world: at 128 x 64 — 128 tiles, the smallest frame at which the
tile order engages — and at 44 x 20, which is not whole tiles, so every buffer that is read as a whole frame must start out zero.
The route is observable through vrt_get_stats: a timed frame planned as one launch has no second kernel time.  Every frame is
held to the oracle's.  A vrt_render that refuses its arguments leaves the frame before it readable."""
import ctypes as C

import numpy as np
import pytest

from voxelraytracing_amd import MODE_PATH, MODE_PRIMARY, MODE_PRIMARY_SHADOW, VrtError, _ffi, graphics as g, scenes

from util import assert_frame_parity, gpu_for_scene

pytestmark = pytest.mark.gpu

SIZES = [(128, 64), (44, 20)]
ROUTES = [(mode, variant) for mode in (MODE_PRIMARY, MODE_PRIMARY_SHADOW) for variant in range(4)]   # + (MODE_PATH, 0)
SEED = 11


def _path_settings(bounces=2):
    return g.make_settings(sun_pos=scenes.SUN_POS, max_ray_bounces=bounces)


@pytest.fixture(scope="module")
def refs(orc):
    """The oracle's frames, once: [size][mode] = (rgb, ids, steps, stats); the path trace's [size]["path", spp] = (rgb, ids)."""
    out = {}
    for size in SIZES:
        sc = scenes.c1_flat(size)
        o = orc.from_package_scene(sc)
        out[size] = {MODE_PRIMARY: o.render(orc.MODE_PRIMARY, *size, want_steps=True),
                     MODE_PRIMARY_SHADOW: o.render(orc.MODE_PRIMARY_SHADOW, *size, want_steps=True)}
        o.set_settings(_path_settings())
        for spp in (2, 4):
            out[size]["path", spp] = o.render(orc.MODE_PATH, *size, spp=spp, seed=SEED)[:2]
        for v in out[size].values():
            for a in v[:3]:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return out


def _one_launch(mode, variant, tables, compact):
    """What vrt_render plans, said again without its code: primary rays alone are one launch; primary + shadow is one launch for
    the default march over the derived tables and, on 8-byte records, for the octree walk (variant 2, or 0 without the tables)."""
    if mode == MODE_PRIMARY:
        return True
    if variant in (0, 3) and not tables:
        variant = 2
    return variant == 0 or (variant == 2 and compact)


@pytest.mark.parametrize("tables, compact", [(True, False), (False, False), (True, True), (False, True)])
def test_the_route_shows_in_the_stats(refs, monkeypatch, tables, compact):
    size = SIZES[0]
    if not tables:
        monkeypatch.setenv("VRT_ACCEL_MAX_S", "0")   # (read when the context is made: variants 0 and 3 fall back to the octree walk)
    sc = scenes.c1_flat(size)
    gpu = gpu_for_scene(sc, tile_major=compact, compact=compact)
    shadow_rays = refs[size][MODE_PRIMARY_SHADOW][3].secondary_rays
    assert shadow_rays > 0
    for mode, variant in ROUTES:
        if compact and variant not in (0, 2):
            with pytest.raises(VrtError) as e:
                gpu.render(mode, variant=variant)
            assert e.value.code == _ffi.VRT_ERR_STATE
            continue
        for in_flight in (1, 2):
            gpu.set_frames_in_flight(in_flight)
            gpu.render(mode, variant=variant, timed=True)
            st = gpu.stats()
            what = f"mode {mode} variant {variant} tables {tables} compact {compact} in flight {in_flight}"
            print(what, "ms_primary", st.ms_primary, "ms_secondary", st.ms_secondary, "secondary_rays", st.secondary_rays)
            assert st.ms_primary > 0.0, what
            if _one_launch(mode, variant, tables, compact):
                assert st.ms_secondary == 0.0, what
            else:
                assert st.ms_secondary > 0.0, what
            assert st.primary_rays == size[0] * size[1], what
            assert st.secondary_rays == (shadow_rays if mode == MODE_PRIMARY_SHADOW else 0), what
    assert bool(gpu.accel_info().available) == tables
    gpu.close()


@pytest.mark.parametrize("tables", [True, False])
@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("size", SIZES)
def test_every_route_renders_the_oracles_frame(refs, monkeypatch, size, in_flight, tables):
    if not tables:
        monkeypatch.setenv("VRT_ACCEL_MAX_S", "0")
    w, h = size
    cw, ch = w & ~7, h & ~7
    sc = scenes.c1_flat(size)
    gpu = gpu_for_scene(sc)
    gpu.set_frames_in_flight(in_flight)
    for mode, variant in ROUTES:
        r_rgb, r_ids, r_steps, r_st = refs[size][mode]
        what = f"{w}x{h} mode {mode} variant {variant} tables {tables} in flight {in_flight}"

        def plain(n):
            for _ in range(n):
                gpu.render(mode, variant=variant)
            rgb, ids, _ = gpu.read_output()
            assert_frame_parity(rgb, ids, r_rgb, r_ids, what)
            assert not rgb[:, cw:].any() and not rgb[ch:, :].any() and not ids[:, cw:].any() and not ids[ch:, :].any(), what

        plain(1)
        gpu.render(mode, variant=variant, stats=True)   # a stats frame between plain ones: alone, on the context's stream
        steps = gpu.read_steps()
        assert np.array_equal(steps, r_steps), what
        assert not steps[:, cw:].any() and not steps[ch:, :].any(), what
        st = gpu.stats()
        assert (st.primary_rays, st.secondary_rays, st.hits, st.steps, st.node_visits) == \
               (r_st.primary_rays, r_st.secondary_rays, r_st.hits, r_st.steps, r_st.node_visits), what
        rgb, ids, _ = gpu.read_output()
        assert_frame_parity(rgb, ids, r_rgb, r_ids, what + " (the stats frame)")
        plain(1)
        plain(in_flight)   # (every frame set, and at 128 tiles the frames that note and use a tile order)
    gpu.close()


@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("size", SIZES)
def test_path_frames_plain_and_accumulating(refs, size, in_flight):
    w, h = size
    cw, ch = w & ~7, h & ~7
    sc = scenes.c1_flat(size)
    gpu = gpu_for_scene(sc)
    gpu.write_settings(_path_settings())
    gpu.set_frames_in_flight(in_flight)

    def check(spp, what):
        rgb, ids, _ = gpu.read_output()
        r_rgb, r_ids = refs[size]["path", spp]
        assert_frame_parity(rgb, ids, r_rgb, r_ids, f"{w}x{h} in flight {in_flight}: {what}")
        assert not rgb[:, cw:].any() and not rgb[ch:, :].any() and not ids[:, cw:].any() and not ids[ch:, :].any(), what

    for _ in range(in_flight):
        gpu.render(MODE_PATH, spp=2, seed=SEED)
    check(2, "2 spp")
    gpu.render(MODE_PATH, spp=2, seed=SEED, accumulate=True)
    check(2, "2 spp accumulating, the first frame")
    gpu.render(MODE_PATH, spp=2, seed=SEED, accumulate=True)
    check(4, "2 + 2 spp accumulated")
    assert gpu.accumulation() == (4, SEED)
    assert gpu.stats().primary_rays == cw * ch * 2
    gpu.close()


PATH_BOUNCES = (0, 1, 2, 3, 5)   # the memset alone; no bounce launch; a cells launch of one segment; the three cursor sets past one turn
PATH_SPP = (1, 3, 5)
# what selects another schedule of a path-traced frame's launches (vrt_frame_plan.h: plan_path): the context's switches (read when
# the context is made), a stats frame, the same samples accumulated over two frames
PATH_ROUTES = {"default": {}, "pool off": {"VRT_PATH_POOL": "0"}, "cells off": {"VRT_PATH_CELLS": "0"},
               "1 sample per chain": {"VRT_PATH_SAMPLES_PER_CHAIN": "1"}, "2 samples per chain": {"VRT_PATH_SAMPLES_PER_CHAIN": "2"},
               "stats": {}, "accumulated": {}}
ACCUMULATED_IN = {1: (1,), 3: (1, 2), 5: (2, 3)}   # the frames whose samples make up the oracle's frame of 1, 3 and 5


@pytest.fixture(scope="module")
def path_refs(orc):
    """The oracle's path-traced frames, once: [size, bounces, spp] = (rgb, ids)."""
    out = {}
    for size in SIZES:
        sc = scenes.c1_flat(size)   # (the oracle reads the scene's own node pool: it stays alive while the oracle renders)
        o = orc.from_package_scene(sc)
        for bounces in PATH_BOUNCES:
            o.set_settings(_path_settings(bounces))
            for spp in PATH_SPP:
                out[size, bounces, spp] = o.render(orc.MODE_PATH, *size, spp=spp, seed=SEED)[:2]
                for a in out[size, bounces, spp]:
                    a.setflags(write=False)
    return out


@pytest.mark.parametrize("bounces", PATH_BOUNCES)
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("route", list(PATH_ROUTES))
def test_every_schedule_of_a_path_frame_renders_the_oracles_frame(path_refs, monkeypatch, route, size, bounces):
    """The launches of a path-traced frame — which cursor set and which path buffer each takes, how many segments a bounce launch
    traces, which pass finishes a chain of samples and with what first / last / count — on every route plan_path can choose, with one
    and two frames in flight and enough frames to visit both frame sets: every frame is the oracle's."""
    for k, v in PATH_ROUTES[route].items():
        monkeypatch.setenv(k, v)
    w, h = size
    cw, ch = w & ~7, h & ~7
    sc = scenes.c1_flat(size)
    gpu = gpu_for_scene(sc)
    gpu.write_settings(_path_settings(bounces))

    def check(spp, what):
        rgb, ids, _ = gpu.read_output()
        r_rgb, r_ids = path_refs[size, bounces, spp]
        what = f"{w}x{h} {bounces} bounces {spp} spp, {route}, {what}"
        assert_frame_parity(rgb, ids, r_rgb, r_ids, what)
        assert not rgb[:, cw:].any() and not rgb[ch:, :].any() and not ids[:, cw:].any() and not ids[ch:, :].any(), what

    for in_flight in (1, 2):
        gpu.set_frames_in_flight(in_flight)
        for spp in PATH_SPP:
            for frame in range(in_flight + 1):   # (every frame set, and the first one again)
                if route == "accumulated":
                    gpu.reset_accumulation()
                    for n in ACCUMULATED_IN[spp]:
                        gpu.render(MODE_PATH, spp=n, seed=SEED, accumulate=True)
                    assert gpu.accumulation() == (spp, SEED)
                else:
                    gpu.render(MODE_PATH, spp=spp, seed=SEED, stats=route == "stats")
                check(spp, f"{in_flight} in flight, frame {frame}")
    gpu.close()


def test_a_refused_render_leaves_the_last_frame_readable(refs):
    size = SIZES[0]
    sc = scenes.c1_flat(size)
    r_rgb, r_ids, _, r_st = refs[size][MODE_PRIMARY_SHADOW]
    # a world.size that does not match size_in_chunks * 32
    gpu = gpu_for_scene(sc)
    gpu.render(MODE_PRIMARY_SHADOW)
    a_rgb, a_ids, _ = gpu.read_output()
    a_img = gpu.present()
    assert_frame_parity(a_rgb, a_ids, r_rgb, r_ids, "frame A")
    good = sc.world.world_data()
    bad = sc.world.world_data()
    bad.size = good.size + 1
    gpu.write_world_data(bad)
    for mode in (MODE_PRIMARY, MODE_PRIMARY_SHADOW, MODE_PATH):
        with pytest.raises(VrtError) as e:
            gpu.render(mode)
        assert e.value.code == _ffi.VRT_ERR_STATE
    gpu.write_world_data(good)
    rgb, ids, _ = gpu.read_output()
    assert np.array_equal(ids, a_ids) and np.array_equal(rgb.view(np.uint32), a_rgb.view(np.uint32))
    assert np.array_equal(gpu.present(), a_img)
    st = gpu.stats()
    assert (st.primary_rays, st.secondary_rays) == (size[0] * size[1], r_st.secondary_rays)
    gpu.close()
    # a path frame on a VRT_FLAG_COMPACT context (its 8-byte records are read where they lie)
    sh = gpu_for_scene(sc, tile_major=True, compact=True)
    hip_memcpy = _ffi.vrt().hipMemcpy
    hip_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def records():
        sh.synchronize()
        ptr, nbytes = sh.device_output()
        assert nbytes == size[0] * size[1] * 8
        host = np.empty(nbytes, dtype=np.uint8)
        assert hip_memcpy(host.ctypes.data, ptr, nbytes, 2) == 0    # hipMemcpyDeviceToHost
        return ptr, host

    sh.render(MODE_PRIMARY_SHADOW)
    a_ptr, a_rec = records()
    assert a_rec.any()
    for kw in (dict(mode=MODE_PATH), dict(mode=MODE_PRIMARY_SHADOW, variant=1), dict(mode=MODE_PRIMARY, variant=3)):
        with pytest.raises(VrtError) as e:
            sh.render(**kw)
        assert e.value.code == _ffi.VRT_ERR_STATE
    ptr, rec = records()
    assert ptr == a_ptr and np.array_equal(rec, a_rec)
    st = sh.stats()
    assert (st.primary_rays, st.secondary_rays) == (size[0] * size[1], r_st.secondary_rays)
    sh.close()
