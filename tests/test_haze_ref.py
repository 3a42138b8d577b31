"""tests/haze_ref.c, the reference of vrt_set_haze, without a GPU: with the setting off it is tests/path_ref.c's loop bit for bit; the
host library's vrth_haze_distance / vrth_haze_exit (csrc/both/haze_math.h, the text the kernels compile) equal the reference's own
statements value for value; the free paths it draws are exponential; and with albedo 0 nothing behind an event is seen."""
import math

import numpy as np
import pytest

import haze_cases as K
import haze_ref
import path_ref
from voxelraytracing_amd import _ffi

F32 = np.float32


@pytest.fixture(scope="module")
def href(tmp_path_factory):
    return haze_ref.load(tmp_path_factory.mktemp("haze_ref"))


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return path_ref.load(tmp_path_factory.mktemp("path_ref"))


def _bits(a):
    return np.asarray(a, F32).view(np.uint32)


def test_with_the_setting_off_it_is_path_refs_loop(href, pref, orc):
    e, p, t = K.tables()
    for name, size in (("terrain", (40, 24)), ("roof", (40, 24)), ("roof", (24, 16))):
        s = orc.from_package_scene(K.scene(name, size))
        for kw in ({}, {"sun": 1.0}, {"emission": e, "polish": p, "translucency": t}, {"sun": 0.5, "emission": e, "polish": p, "translucency": t}):
            a_rgb, a_ids, a = href.render(s, *size, haze=None, spp=3, seed=K.SEED, **kw)
            b_rgb, b_ids, b = pref.render(s, *size, spp=3, seed=K.SEED, **kw)
            assert np.array_equal(_bits(a_rgb), _bits(b_rgb)) and np.array_equal(a_ids, b_ids), (name, kw)
            assert (a.steps, a.bounce_segments, a.sun_rays, a.sun_unoccluded, a.passes, a.polished_bounces) == \
                   (b.steps, b.bounce_segments, b.sun_rays, b.sun_unoccluded, b.passes, b.polished_bounces)
            assert a.ev_primary == a.ev_later == a.no_event == 0
    # a density of -0 is off as well
    s = orc.from_package_scene(K.scene("roof", (24, 16)))
    a = href.render(s, 24, 16, haze=(-0.0, K.ALBEDO), spp=2, seed=K.SEED, sun=1.0)
    b = pref.render(s, 24, 16, spp=2, seed=K.SEED, sun=1.0)
    assert np.array_equal(_bits(a[0]), _bits(b[0]))


def test_the_logarithm_is_the_oracles(href, orc):
    """haze_ref.c's statement of vlog against the oracle's own orc_log, over draws as rng_next makes them and the clamp's value."""
    x = np.concatenate([np.array([1.0e-10, 1.0, np.nextafter(F32(1), F32(0)), 0.5, 0.70710677, 0.70710683, 1.4142135, 1.4142137], F32),
                        (np.random.default_rng(5).integers(1, 2**32 - 1, 4096, dtype=np.uint64).astype(np.float64) / 4294967295.0).astype(F32)])
    assert np.array_equal(_bits(href.log(x)), _bits(orc.log_n(x)))


def test_the_librarys_distance_is_the_references(href):
    nan = F32(np.nan)
    below_one = np.nextafter(F32(1), F32(0))
    u = np.concatenate([np.array([0.0, -0.0, 1.0e-10, np.nextafter(F32(1.0e-10), F32(0)), np.nextafter(F32(1.0e-10), F32(1)), 1.0, below_one, 0.5, 0.25,
                                  1.0e-20, 1.0e-38, 1.0e-45, 0.70710677, 0.70710683, nan, -1.0, 2.0, np.inf], F32),
                        (np.random.default_rng(7).integers(0, 2**32, 8192, dtype=np.uint64).astype(np.float64) / 4294967295.0).astype(F32)])
    for density in (2.0 ** -20, 0.02, 0.05, 1.0, 3.0, 64.0):
        inv = F32(1.0) / F32(density)
        got, want = _ffi.haze_distance(u, inv), href.distance(u, inv)
        assert np.array_equal(_bits(got), _bits(want)), density
    inv = F32(1.0) / F32(0.05)
    t = _ffi.haze_distance(np.array([0.0, 1.0e-10, 1.0, below_one], F32), inv)
    assert t[0] == t[1] and abs(float(t[1]) - 23.02585 * 20.0) < 1e-3      # the clamp
    assert _bits(t[2]) == 0x80000000 and 0.0 < float(t[3]) < 2e-6           # u = 1: -0; just below: a tiny distance


def test_the_librarys_exit_is_the_references(href):
    W = 64.0
    nan, inf = float("nan"), float("inf")
    origins = [(16.5, 20.25, 40.0), (0.001, 63.999, 32.0)]
    # on and beyond each face, and a NaN in each place
    for k in range(3):
        for v in (0.0, -0.0, W, -1.0, W + 1.0, np.nextafter(F32(W), F32(0)), np.nextafter(F32(0), F32(1)), nan, inf, -inf):
            o = [10.0, 20.0, 30.0]
            o[k] = v
            origins.append(tuple(o))
    dirs = [(0.6, 0.0, 0.8), (0.6, -0.0, -0.8), (0.0, 0.0, 1.0), (-0.0, -1.0, 0.0), (0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (0.267, -0.534, 0.802), (-0.577, 0.577, -0.577),
            (nan, 0.6, 0.8), (0.6, nan, nan), (nan, nan, nan), (1e-30, 1e-30, -1e-30), (1e-45, 0.0, 0.0), (inf, 1.0, 0.0), (-inf, -inf, inf)]
    n = 0
    for o in origins:
        for d in dirs:
            got, want = _ffi.haze_exit(o, d, W), href.exit(o, d, W)
            assert _bits(got) == _bits(want), (o, d, got, want)
            n += 1
    assert n >= 400
    # known answers
    assert _ffi.haze_exit((16.0, 16.0, 16.0), (0.0, 0.0, 1.0), 64.0) == 48.0
    assert _ffi.haze_exit((16.0, 16.0, 16.0), (0.0, -0.0, -1.0), 64.0) == 16.0
    assert _ffi.haze_exit((16.0, 16.0, 16.0), (0.0, 0.0, 0.0), 64.0) == np.inf
    assert _bits(_ffi.haze_exit((0.0, 16.0, 16.0), (1.0, 0.0, 0.0), 64.0)) == 0 and _bits(_ffi.haze_exit((16.0, 64.0, 16.0), (1.0, 0.0, 0.0), 64.0)) == 0
    assert _bits(_ffi.haze_exit((16.0, nan, 16.0), (1.0, 0.0, 0.0), 64.0)) == 0


def test_free_paths_are_exponential(href, orc):
    """One all-air chunk, the camera at its centre, one pixel's ray: the primary segment never hits, its length in the haze is the
    exit from the box, L, and an event happens with probability 1 - exp(-density * L).  65 536 samples at p = 0.5: the share's
    standard deviation is 0.00195, the bound 0.01 is five of them."""
    size = (8, 8)
    s = orc.from_package_scene(K.air(size))
    o, d = href.primary_ray(s, 3, 4)
    L = float(href.exit(o, d, 32.0))
    assert 15.0 < L < 28.0 and L == float(_ffi.haze_exit(o, d, 32.0))
    density = float(F32(math.log(2.0) / L))
    n = href.count_pixel(s, *size, 3, 4, 65536, haze=(density, K.ALBEDO), seed=K.SEED)
    p = 1.0 - math.exp(-density * L)
    share = n.ev_primary / 65536
    print(f"L {L:.4f}, density {density:.5f}: p {p:.5f}, share {share:.5f}")
    assert abs(p - 0.5) < 1e-3
    assert n.ev_primary + n.no_event == 65536 and n.ev_hit == 0 and n.ev_miss == n.ev_primary
    assert abs(share - p) <= 0.01


@pytest.mark.parametrize("name", K.SCENES)
def test_with_albedo_0_and_the_sun_off_nothing_behind_an_event_is_seen(href, orc, name):
    """thr is 0 behind the event: a sample with an event on its first segment has no light at all, and every sample's light is the
    light of its segments in front of its first event — the same sample traced with max_ray_bounces cut there."""
    size = (40, 24)
    e, p, t = K.tables()
    sc = K.scene(name, size, 4)
    s = orc.from_package_scene(sc)
    seen = checked = 0
    for sample in range(3):
        ev = np.zeros((1, 4, size[1], size[0]), np.uint8)
        rgb, _, n = href.render(s, *size, haze=(K.DENSITY[name], 0.0), seed=K.SEED, sample_base=sample, emission=e, polish=p, translucency=t, events=ev)
        first = np.where(ev[0].any(axis=0), ev[0].argmax(axis=0), 4)   # the first segment with an event; 4: none
        assert not rgb[first == 0].any()
        seen += int((first == 0).sum())
        for b in (1, 2, 3):
            cut = K.scene(name, size, b)
            cut_rgb, _, _ = href.render(orc.from_package_scene(cut), *size, haze=(K.DENSITY[name], 0.0), seed=K.SEED, sample_base=sample, emission=e, polish=p,
                                        translucency=t)
            m = first == b
            # (the cut frame's segment b - 1 is its last allowed one and draws what it draws in the long frame: the light is the same)
            assert np.array_equal(_bits(rgb[m]), _bits(cut_rgb[m])), (sample, b)
            checked += int(m.sum())
    print(name, "events on the first segment", seen, "later first events", checked)
    assert seen >= 500 and checked >= 300
