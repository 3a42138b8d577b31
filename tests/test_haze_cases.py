"""The scenes of tests/test_gpu_haze.py (tests/haze_cases.py), from the reference alone: at the chosen densities every route of
vrt_set_haze's contract is taken at least once on each scene, so that no GPU test passes on frames in which nothing scatters; the
frames are exact to compare (no texel depends on the sky's pow); and the large frame takes a bounce launch past one workgroup per
segment."""
import numpy as np
import pytest

import haze_cases as K
import haze_ref
import segment_cases as S

F32 = np.float32
ID_HIT = 1 << 16


@pytest.fixture(scope="module")
def href(tmp_path_factory):
    return haze_ref.load(tmp_path_factory.mktemp("haze_ref"))


def _render(href, orc, name, size, bounces=4, sun=K.SUN, tables=None, spp=3, **kw):
    sc = K.scene(name, size, bounces)
    e, p, t = tables if tables is not None else (None, None, None)
    return href.render(orc.from_package_scene(sc), *size, haze=(K.DENSITY[name], K.ALBEDO), spp=spp, seed=K.SEED, sun=sun, emission=e, polish=p,
                       translucency=t, **kw)


@pytest.mark.parametrize("size", [(40, 24), (8, 8)])
@pytest.mark.parametrize("name", K.SCENES)
def test_every_route_is_taken(href, orc, name, size):
    rgb, ids, n = _render(href, orc, name, size)
    print(name, size, n)
    assert (ids & ID_HIT).all(), "a primary ray that misses would put the sky's green into its texel"
    assert n.ev_primary >= 1 and n.ev_later >= 1 and n.ev_last >= 1 and n.ev_hit >= 1 and n.ev_miss >= 1 and n.no_event >= 1
    assert n.ev_sun_rays >= 1 and n.ev_sun_unoccluded >= 1 and n.ev_sun_rays - n.ev_sun_unoccluded >= 1, "an event's sun ray of either fate"
    assert n.sun_rays > n.ev_sun_rays and n.sun_unoccluded > n.ev_sun_unoccluded, "a hit's sun ray of either fate"
    assert n.ev_primary + n.ev_later + n.no_event == size[0] * size[1] * 3 + n.bounce_segments
    # one allowed segment: every event is on the last one, and its sun ray is still sent
    _, _, one = _render(href, orc, name, size, bounces=1)
    assert one.ev_primary == one.ev_last >= 1 and one.ev_later == 0 and one.ev_sun_rays == one.ev_primary and one.bounce_segments == 0
    # the sun off: the same events (the sun term draws nothing), no sun ray
    _, _, dark = _render(href, orc, name, size, sun=0.0)
    assert (dark.ev_primary, dark.ev_later, dark.ev_hit, dark.ev_miss, dark.no_event) == (n.ev_primary, n.ev_later, n.ev_hit, n.ev_miss, n.no_event)
    assert dark.sun_rays == 0


@pytest.mark.parametrize("name", K.SCENES)
def test_the_tables_take_part(href, orc, name):
    plain = _render(href, orc, name, (40, 24))
    for which in range(3):
        tables = [None, None, None]
        tables[which] = K.tables()[which]
        rgb, _, n = _render(href, orc, name, (40, 24), tables=tables)
        assert not np.array_equal(rgb, plain[0]), which
        assert (n.polished_bounces >= 1) == (which == 1) and (n.passes >= 1) == (which == 2)
    rgb, _, n = _render(href, orc, name, (40, 24), tables=K.tables())
    assert n.polished_bounces >= 1 and n.passes >= 1 and n.ev_later >= 1 and n.ev_sun_unoccluded >= 1


@pytest.mark.parametrize("name", K.SCENES)
def test_the_setting_is_not_a_no_op_and_the_frames_are_exact_to_compare(href, orc, name):
    size = (40, 24)
    sc = K.scene(name, size)
    on = _render(href, orc, name, size)
    off = href.render(orc.from_package_scene(sc), *size, haze=None, spp=3, seed=K.SEED, sun=K.SUN)
    assert not np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    # green reaches no texel (haze_cases.py), red and blue do, and they differ
    for rgb in (on[0], off[0], _render(href, orc, name, size, tables=K.tables())[0]):
        assert not rgb[..., 1].any() and not np.signbit(rgb[..., 1]).any()
        assert (rgb[..., 0] > 0).sum() >= 100 and (rgb[..., 2] > 0).sum() >= 100 and not np.array_equal(rgb[..., 0], rgb[..., 2])


def test_the_skys_red_does_not_depend_on_the_pow():
    """ray_sky's gradient with sky_color[0] == 1: 1 * (1 - t) + 1 * t in binary32 is 1 for every t in [0, 1] — whatever the last
    bits of t = pow(s, 0.35) are.  And its blue, 0 * (1 - t) + 0 * t, is 0."""
    t = np.concatenate([np.linspace(0, 1, 1 << 20, dtype=np.float64).astype(F32), np.random.default_rng(3).random(1 << 20, dtype=F32),
                        np.array([0.0, 1.0, 0.5, np.nextafter(F32(0.5), F32(0)), np.nextafter(F32(1), F32(0)), 1e-30, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25], F32)])
    one, zero = F32(1.0), F32(0.0)
    assert np.all(one * (one - t) + one * t == one)
    assert not np.any(zero * (one - t) + zero * t)


def test_the_large_frame_takes_a_bounce_launch_past_one_workgroup_per_segment(href, orc):
    """tests/segment_cases.py's "one_over" size: 1025 tiles, 257 primary workgroups, hit_seg_cap 512.  A haze frame's primary lanes
    all go on — the march hits for every pixel, and an event goes on as well — so segment 0 hands the second launch the 320 paths of
    its two producers: workgroup part 1 of segment 0 has records to read."""
    size = S.CASES["one_over"].size
    assert S.workgroups("one_over") == 257 and S.capacity("one_over") == 512
    ev = np.zeros((1, 4, size[1], size[0]), np.uint8)
    _, ids, n = _render(href, orc, "terrain", size, spp=1, events=ev)
    alive = ((ids & ID_HIT) != 0) | (ev[0, 0] != 0)
    loads = S.segment_loads(alive, *size)
    print("the second launch reads", loads[0], "paths of segment 0, at most", loads[1:].max(), "of any other;", n)
    assert loads[0] > 256 and loads[1:].max() <= 256
    assert n.ev_primary >= 1000 and n.ev_later >= 1000 and n.ev_sun_unoccluded >= 1000
