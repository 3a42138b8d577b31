"""tests/polish_ref.py, the tests' reference for the polish table (vrt_write_polish: tests/path_ref.c with every later term off),
without a GPU: with a table of zeros it is the emission reference — its frames as tests/golden/path_ref_pins.json recorded them —
and the oracle's path trace bit for bit, one bounce sees no table, the coat's draw is taken on every hit of a polished frame, and
on a case small enough to check by hand it does what the contract says."""
import numpy as np
import pytest

import emission_ref
import polish_ref
from emission_cases import common
from golden.make_path_ref_pins import is_frame, load_pins, sha
from voxelraytracing_amd import scenes

SEED = 11
W, H = 64, 40
F = np.float32
PINS = load_pins()


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return polish_ref.load(tmp_path_factory.mktemp("polish_ref"))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _some_table():
    return polish_ref.table({i: (0.5 + (i % 3), 0.25 * (i % 4), (0.25, 0.5, 0.75)) for i in range(0, 256, 2)})


def test_it_compiles_with_the_oracles_flags(pref):
    flags = emission_ref.oracle_cflags()
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags
    assert not any("fast-math" in f and not f.startswith("-fno-") for f in flags)


@pytest.mark.parametrize("spp", [1, 3, 8])
def test_a_table_of_zeros_is_the_emission_reference_and_the_oracle(pref, orc, spp):
    sc = scenes.c4((W, H))   # (kept alive: the oracle's scene points into it)
    o = orc.from_package_scene(sc)
    plain_rgb, plain_ids, _, _ = o.render(orc.MODE_PATH, W, H, spp=spp, seed=SEED)
    e = np.zeros(256, np.float32)
    e[common(plain_ids, 1)[0]], e[255] = 1.75, 3.0   # (the one material this small frame's primary rays hit, and an entry nothing uses)
    zeros = polish_ref.table()
    zeros["color"], zeros["scatter"] = (0.25, 0.5, 0.75), 0.5   # (a chance of 0, whatever the other fields hold)
    zeros["chance"][1::2] = -0.0
    want = PINS[f"emission/E2/spp{spp}"]   # (the emission reference's frame under this table, from before the two were one loop)
    assert is_frame(pref.render(o, e, zeros, W, H, spp=spp, seed=SEED), want)
    assert pref.polished_bounces == 0
    assert want["rgb"] != sha(plain_rgb)   # (the emission table is not a no-op here)
    rgb, ids = pref.render(o, None, zeros, W, H, spp=spp, seed=SEED)
    assert np.array_equal(ids, plain_ids) and np.array_equal(_bits(rgb), _bits(plain_rgb))


def test_one_bounce_sees_no_table(pref, orc):
    sc = scenes.c4((W, H), bounces=1)   # (kept alive: the oracle's scene points into it)
    o = orc.from_package_scene(sc)
    e = np.zeros(256, np.float32)
    e[4] = 1.5
    want = pref.render(o, e, None, W, H, spp=3, seed=SEED)
    got = pref.render(o, e, _some_table(), W, H, spp=3, seed=SEED)
    assert np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[0]), _bits(want[0]))
    assert pref.polished_bounces == 0


def test_the_draw_is_unconditional(pref, orc):
    """Only entry 255 has a chance, and no ray meets it: nothing bounces off a coat, and still every path's RNG stream has
    moved by one draw per hit."""
    sc = scenes.c4((W, H), bounces=2)   # (kept alive: the oracle's scene points into it)
    o = orc.from_package_scene(sc)
    zero = pref.render(o, None, None, W, H, spp=3, seed=SEED)
    got = pref.render(o, None, polish_ref.table({255: (0.5, 0.0, (1.0, 1.0, 1.0))}), W, H, spp=3, seed=SEED)
    assert pref.polished_bounces == 0
    assert np.array_equal(got[1], zero[1])
    differ = int((np.abs(got[0] - zero[0]).max(axis=2) > 1e-3).sum())
    print(f"pixels that differ by more than 1e-3: {differ} of {W * H}")
    assert differ > 500


def _normalize(v):
    """orc_normalize in f32: v / sqrt(dot(v, v)), the dot summed left to right."""
    d = F(F(F(v[0] * v[0]) + F(v[1] * v[1])) + F(v[2] * v[2]))
    return v / np.sqrt(d)


def _dot(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def test_a_mirror_coat_by_hand(pref, orc):
    """Two segments, one sample, every entry chance 2 (always), scatter 0, colour (0.25, 0.5, 0.75): every hit bounces off the
    coat as off a mirror, so a pixel whose primary ray hits is 0 when the mirrored ray hits again (its second segment is its
    last) and sky * colour otherwise — the throughput is the coat's colour, not the face-shaded mc."""
    sc = scenes.c4((W, H), bounces=2)   # (kept alive: the oracle's scene points into it)
    o = orc.from_package_scene(sc)
    color = np.array([0.25, 0.5, 0.75], F)
    t = polish_ref.table({i: (2.0, 0.0, tuple(color)) for i in range(256)})
    rgb, ids = pref.render(o, None, t, W, H, spp=1, seed=SEED)
    hit = (ids & orc.ID_HIT) != 0
    assert pref.polished_bounces == int(hit.sum())
    n_sky = 0
    for py, px in np.argwhere(hit):
        _, _, d, out = o.trace_pixel(orc.MODE_PRIMARY, int(px), int(py))
        d, pos, norm = np.array(d, F), np.array(out[0:3], F), np.array(out[3:6], F)
        dn = _dot(norm, d)
        spec = d - F(2.0) * norm * dn        # (mix(spec, sc, 0) = spec * 1 + sc * 0 = spec)
        nd = _normalize(spec)
        origin = pos + norm * F(0.002)
        idw, _, _ = o.ray_world(origin, nd)
        if idw & orc.ID_HIT:
            want = np.zeros(3, F)
        else:
            want = np.array(o.ray_sky(origin, nd), F) * color
            n_sky += 1
        assert np.array_equal(_bits(rgb[py, px]), _bits(want)), (px, py, rgb[py, px], want)
    print(f"{int(hit.sum())} pixels hit, {n_sky} of them carry sky")
    assert n_sky >= 50


def test_sample_base_continues_the_samples(pref, orc):
    sc = scenes.c4((W, H))   # (kept alive: the oracle's scene points into it)
    o = orc.from_package_scene(sc)
    e = np.zeros(256, np.float32)
    e[40] = 1.5
    t = _some_table()
    whole, ids = pref.render(o, e, t, W, H, spp=4, seed=SEED)
    a, ids_a = pref.render(o, e, t, W, H, spp=1, seed=SEED)
    b, _ = pref.render(o, e, t, W, H, spp=3, seed=SEED, sample_base=1)
    assert np.array_equal(ids_a, ids)
    assert np.allclose(whole, (a + 3 * b) / 4, atol=1e-5)
