"""tests/water_ref.c, the reference of vrt_set_water_optics, without a GPU: with the setting off it is tests/path_ref.c's loop bit for
bit; known answers on the hand-built pool (tests/water_cases.py); and the scenes the GPU tests use exercise every branch of the
contract — counted on the reference alone, before any kernel is asked."""
import numpy as np
import pytest

import path_ref
import water_cases as K
import water_ref
from voxelraytracing_amd import _ffi

F32 = np.float32


@pytest.fixture(scope="module")
def wref(tmp_path_factory):
    return water_ref.load(tmp_path_factory.mktemp("water_ref"))


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return path_ref.load(tmp_path_factory.mktemp("path_ref"))


def _tables():
    emission = np.zeros(256, F32)
    emission[K.SLATE] = 1.5
    polish = path_ref.polish_table({K.SLATE: (0.5, 0.0, (1.0, 0.9, 0.8))})
    tr = path_ref.translucency_table({K.SLATE: (0.25, (0.9, 0.6, 0.3))})
    return emission, polish, tr


def test_with_the_setting_off_it_is_path_refs_loop(wref, pref, orc):
    e, p, t = _tables()
    for sc, size in ((K.pool("grazing", (40, 24)), (40, 24)), (K.c4_lake("water", (40, 24)), (40, 24)), (K.c4_lake("underwater", (24, 16)), (24, 16))):
        s = orc.from_package_scene(sc)
        for kw in ({}, {"sun": 1.0}, {"emission": e, "polish": p, "translucency": t}, {"sun": 0.5, "emission": e, "polish": p, "translucency": t}):
            a_rgb, a_ids, a = wref.render(s, *size, water=None, spp=3, seed=K.SEED, **kw)
            b_rgb, b_ids, b = pref.render(s, *size, spp=3, seed=K.SEED, **kw)
            assert np.array_equal(a_rgb.view(np.uint32), b_rgb.view(np.uint32)) and np.array_equal(a_ids, b_ids), (sc.name, kw)
            assert (a.steps, a.bounce_segments, a.sun_rays, a.sun_unoccluded, a.passes, a.polished_bounces) == \
                   (b.steps, b.bounce_segments, b.sun_rays, b.sun_unoccluded, b.passes, b.polished_bounces)
            assert a.surface == a.wet_w == a.wet_bounces == 0


def test_straight_down_the_bed_is_reached_with_the_transmittance_of_three_voxels(wref, orc):
    """reflectance 0, the centre pixel of the camera that looks straight down: the surface event lets the path through (c = 1, F =
    0), the wet segment behind it runs the pool's three voxels to the bed, and thr there is vexp_neg(absorb * w).  w is that
    segment's water_dist: it starts at the hit position, which the march left at most 0.001 along the ray behind the face, and
    its own start nudge and last step add at most 0.001 each — so w lies in [3 - 0.004, 3]."""
    size = (16, 8)
    absorb = np.array(K.OPTICS[0], F32)
    s = orc.from_package_scene(K.pool("down", size, bounces=4))
    light, idw, n, thr = wref.trace_pixel(s, *size, 8, 4, water=(absorb, 0.0), seed=K.SEED)
    assert n.surface >= 1 and n.transmitted >= 1 and n.wet_hit >= 1
    assert (idw & 0x7FFF) == K.WATER and not (idw & (1 << 20)), hex(idw)   # the water voxel's face, VRT_ID_WATER clear
    lo, hi = _ffi.water_transmittance(absorb, F32(3.0)), _ffi.water_transmittance(absorb, F32(3.0 - 0.004))
    print("thr at the bed", thr, "bounds", lo, hi)
    assert np.all(thr >= lo) and np.all(thr <= hi)
    # red is absorbed most
    assert thr[0] < thr[1] < thr[2] < 1.0


def test_a_perfect_mirror_never_lets_a_path_into_the_water(wref, orc):
    size = (100, 60)
    s = orc.from_package_scene(K.pool("down", size))
    _, ids, n = wref.render(s, *size, water=(K.OPTICS[0], 1.0), spp=3, seed=K.SEED)
    assert n.surface >= 1000 and n.reflected >= 1 and n.transmitted == 0 and n.wet_w == 0 and n.wet_bounces == 0 and n.wet_hit == 0


def test_clear_water_without_a_mirror_costs_segments_and_draws_only(wref, orc):
    """absorb 0, reflectance 0: a surface event almost always lets the path through (F = m^5), multiplies thr by exactly 1 and
    changes nothing but the path's segment count and its RNG stream.  Seen where neither matters: slate gives off light, a frame
    of two segments with the setting on against a frame of one with it off — through water both end on the same bed voxel with
    thr 1.  Only the pixels whose event reflected may differ."""
    size = (100, 60)
    emission = np.zeros(256, F32)
    emission[K.SLATE] = 1.5
    on = K.pool("down", size, bounces=2)
    off = K.pool("down", size, bounces=1)
    a_rgb, a_ids, a = wref.render(orc.from_package_scene(on), *size, water=(0.0, 0.0), seed=K.SEED, emission=emission)
    b_rgb, b_ids, b = wref.render(orc.from_package_scene(off), *size, water=None, seed=K.SEED, emission=emission)
    wet = (a_ids & 0x7FFF) == K.WATER
    # (surface events on a path's last allowed segment are counted and draw nothing: the primary ones are the wet pixels)
    assert wet.sum() >= 1000 and a.surface >= wet.sum() and a.transmitted + a.reflected == wet.sum()
    differ = np.any(a_rgb.view(np.uint32) != b_rgb.view(np.uint32), axis=2)
    # (the other pixels have a second segment in one frame and not in the other)
    assert (differ & wet).sum() <= a.reflected, ((differ & wet).sum(), a.reflected)
    assert np.all(b_rgb[wet & ~differ] > 0)
    assert b.bounce_segments == 0 and a.wet_bounces == a.transmitted and a.wet_hit == a.transmitted


@pytest.mark.parametrize("size", [(100, 60), (128, 72)])
def test_the_grazing_view_takes_every_branch(wref, orc, size):
    s = orc.from_package_scene(K.pool("grazing", size))
    _, _, n = wref.render(s, *size, water=K.OPTICS, spp=1, seed=K.SEED)
    print(size, n)
    assert n.reflected >= 1 and n.transmitted >= 1 and n.wet_hit >= 1
    assert n.wet_bounces > n.transmitted, "a bounce off the bed that starts wet"


@pytest.mark.parametrize("scene", ["pool under_bed", "pool under_up", "c4 underwater"])
def test_the_underwater_views_start_wet(wref, orc, scene):
    size = (128, 72)
    sc = K.c4_lake("underwater", size) if scene.startswith("c4") else K.pool(scene.split()[1], size)
    _, ids, n = wref.render(orc.from_package_scene(sc), *size, water=K.OPTICS, spp=1, seed=K.SEED)
    print(scene, n)
    assert n.wet_primary_w == size[0] * size[1]
    assert ((ids & (1 << 20)) != 0).all()   # VRT_ID_WATER: the primary's own march passed water


def test_c4s_lake_from_above_has_surface_events_of_both_kinds(wref, orc):
    size = (128, 72)
    _, ids, n = wref.render(orc.from_package_scene(K.c4_lake("water", size)), *size, water=K.OPTICS, spp=1, seed=K.SEED)
    print(n)
    assert n.reflected >= 1 and n.transmitted >= 1 and n.wet_hit >= 1 and n.wet_bounces > n.transmitted
    assert ((ids & 0x7FFF) == K.WATER).sum() >= 1000
