"""tests/refract_ref.c, the reference of vrt_set_water_refraction, without a GPU: with ior = 0 it is tests/water_ref.c's frame bit for
bit; known answers for the two bends (A and C of the contract); and the host mirror — vrth_water_refract, vrth_world_water_span,
which compile csrc/both/refract_math.h, the kernels' text — equals the reference's own statement of them bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import path_ref
import refract_cases as RC
import refract_ref
import water_cases as K
import water_ref
from voxelraytracing_amd import _ffi

F32 = np.float32
IOR = RC.IOR


@pytest.fixture(scope="module")
def rref(tmp_path_factory):
    return refract_ref.load(tmp_path_factory.mktemp("refract_ref"))


@pytest.fixture(scope="module")
def wref(tmp_path_factory):
    return water_ref.load(tmp_path_factory.mktemp("water_ref"))


def _tables():
    emission = np.zeros(256, F32)
    emission[K.SLATE] = 1.5
    polish = path_ref.polish_table({K.SLATE: (0.5, 0.0, (1.0, 0.9, 0.8))})
    tr = path_ref.translucency_table({K.SLATE: (0.25, (0.9, 0.6, 0.3))})
    return emission, polish, tr


SCENES = [f"pool {cam}" for cam in K.CAMERAS] + ["c4 water", "c4 underwater", "c4 water down"]


def _scene(name, size, bounces=4):
    kind, cam = name.split(" ", 1)
    return K.pool(cam, size, bounces) if kind == "pool" else K.c4_lake(cam, size, bounces)


@pytest.mark.parametrize("name", SCENES)
def test_with_ior_0_it_is_water_refs_frame(rref, wref, orc, name):
    e, p, t = _tables()
    size = (40, 24)
    sc = _scene(name, size)   # (kept: the oracle's scene reads the world's own arrays)
    s = orc.from_package_scene(sc)
    for water in (K.OPTICS, None):
        for refract in (None, (0.0, 7)):
            for kw in ({}, {"sun": 1.0}, {"sun": 0.5, "emission": e, "polish": p, "translucency": t}):
                a_rgb, a_ids, a = rref.render(s, *size, water=water, refract=refract, spp=3, seed=K.SEED, **kw)
                b_rgb, b_ids, b = wref.render(s, *size, water=water, spp=3, seed=K.SEED, **kw)
                assert np.array_equal(a_rgb.view(np.uint32), b_rgb.view(np.uint32)) and np.array_equal(a_ids, b_ids), (name, water, refract, kw)
                assert tuple(a)[:len(b)] == tuple(b), (name, water, refract, kw)
                assert not any(tuple(a)[len(b):]), a


def test_with_water_optics_off_an_ior_changes_nothing(rref, wref, orc):
    size = (40, 24)
    sc = _scene("c4 underwater", size)
    s = orc.from_package_scene(sc)
    a = rref.render(s, *size, water=None, refract=IOR, spp=3, seed=K.SEED)
    b = wref.render(s, *size, water=None, spp=3, seed=K.SEED)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and not any(tuple(a[2])[len(b[2]):])


def _unit(theta_deg, phi_deg=0.0, down=True):
    """A unit vector at theta from the y axis, heading down (-y) or up."""
    t, p = math.radians(theta_deg), math.radians(phi_deg)
    return np.array([math.sin(t) * math.cos(p), (-1.0 if down else 1.0) * math.cos(t), math.sin(t) * math.sin(p)], F32)


UP, DOWN = np.array([0, 1, 0], F32), np.array([0, -1, 0], F32)


def test_normal_incidence_keeps_the_direction(rref):
    for ior in (1.0, IOR, 2.5, 4.0):
        d, branch = rref.bend(ior, 0.04, DOWN, UP)                      # entering through the +y face
        assert branch == 0 and np.array_equal(d, DOWN), (ior, d)
        d, branch = rref.bend(ior, 0.04, UP, DOWN, u=0.5, leaving=True)   # leaving through it: F = reflectance = 0.04 < u
        assert branch == 3 and np.array_equal(d, UP), (ior, d)
        d, branch = rref.bend(ior, 0.04, UP, DOWN, u=0.01, leaving=True)  # ... and reflected by the draw: the mirror image
        assert branch == 2 and np.array_equal(d, DOWN), (ior, d)


def test_ior_1_gives_normalize_d_to_the_last_bits(rref):
    """eta = 1: s2 = 1 - c * c, ct = sqrt(1 - s2) is c up to rounding, g is a rounding error, and d' = normalize(d + g * nn).  Not d
    itself bit for bit — so a frame with ior = 1 may differ from the frame with the setting off in last bits above the water."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(500):
        d = _unit(rng.uniform(0, 89), rng.uniform(0, 360))
        got, _ = rref.bend(1.0, 0.04, d, UP)
        d64 = d.astype(np.float64)
        worst = max(worst, float(np.abs(got - d64 / np.linalg.norm(d64)).max()))
    print("ior 1: max |d' - normalize(d)|", worst)
    # 1 - c * c is rounded to 2^-25 (a value in [1/2, 1)), so the radicand 1 - s2 is c * c to within 2^-25 and ct is c to within
    # 2^-25 / (2 c): with c >= cos(89 degrees) that is |g| <= 2^-26 / cos(89 degrees) = 8.5e-7, times a component of nn at most 1;
    # the remaining roundings (eta * d, the add, the normalisation's sqrt and divide) are half an ulp of a value below 1 each
    assert worst <= 2.0 ** -26 / math.cos(math.radians(89.0)) + 4 * 2.0 ** -25


def test_the_critical_angle_of_water_on_either_side(rref):
    crit = math.degrees(math.asin(1.0 / IOR))   # 48.75 degrees
    n = DOWN                                    # the face's normal, back into the water below it
    for phi in (0.0, 37.0, 200.0):
        d, branch = rref.bend(IOR, 0.0, _unit(crit + 0.5, phi, down=False), n, u=0.999, leaving=True)
        assert branch == 1 and d[1] < 0, "past the critical angle: total, whatever the draw; mirrored back down"
        inside = _unit(crit - 0.5, phi, down=False)
        d, branch = rref.bend(IOR, 0.0, inside, n, u=0.999, leaving=True)
        assert branch == 3 and d[1] > 0
        # Snell: sin(out) = ior * sin(in), in float64
        want = math.degrees(math.asin(IOR * math.sin(math.radians(crit - 0.5))))
        got = math.degrees(math.acos(float(d[1]) / float(np.linalg.norm(d.astype(np.float64)))))
        assert abs(got - want) < 0.05, (got, want)   # (near grazing a degree is a few 1e-4 of the cosine)
        assert abs(float(np.linalg.norm(d.astype(np.float64))) - 1.0) < 1e-6
        # at 30 degrees inside: 41.68 degrees outside, and F is Schlick's of the outside cosine
        d, branch = rref.bend(IOR, 0.0, _unit(30.0, phi, down=False), n, u=0.999, leaving=True)
        assert branch == 3 and abs(math.degrees(math.acos(float(d[1]))) - math.degrees(math.asin(IOR * 0.5))) < 1e-3
        # entering at a grazing angle ends just inside the critical angle; entering and leaving are inverse
        d, branch = rref.bend(IOR, 0.0, _unit(89.9, phi), UP)
        got = math.degrees(math.acos(-float(d[1])))
        assert branch == 0 and crit - 0.01 < got < crit, (got, crit)
        d_in, _ = rref.bend(IOR, 0.0, _unit(40.0, phi), UP)
        assert abs(math.degrees(math.acos(-float(d_in[1]))) - math.degrees(math.asin(math.sin(math.radians(40.0)) / IOR))) < 1e-3
        d_out, branch = rref.bend(IOR, 0.0, -d_in, n, u=0.999, leaving=True)
        assert branch == 3 and np.allclose(d_out, -_unit(40.0, phi), atol=2e-6)
    # reflectance 1: every event inside the critical angle is reflected by the draw
    assert rref.bend(IOR, 1.0, _unit(10.0, 0.0, down=False), n, u=0.999, leaving=True)[1] == 2


def test_a_zero_normal_gives_normalize_eta_d(rref):
    zero = np.zeros(3, F32)
    rng = np.random.default_rng(6)
    for ior in (1.0, IOR, 4.0):
        eta = F32(1.0) / F32(ior)
        for _ in range(100):
            d = _unit(rng.uniform(0, 180), rng.uniform(0, 360))
            v = eta * d
            length = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2], dtype=F32)
            got, branch = rref.bend(ior, 0.04, d, zero)
            assert branch == 0 and np.array_equal(got, v / length), (ior, d, got)


FACES = [np.array(f, F32) for f in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, 0, 0))]


def test_the_host_mirrors_bends_are_the_references_bit_for_bit(rref):
    """vrth_water_refract compiles csrc/both/refract_math.h, the kernels' text; tests/refract_ref.c states A and C again."""
    rng = np.random.default_rng(7)
    taken = set()
    n_cases = 0
    for ior in (1.0, IOR, 1.5, 2.5, 4.0):
        for _ in range(700):
            d = rng.normal(size=3).astype(F32)
            if rng.random() < 0.7:
                d = (d / np.linalg.norm(d)).astype(F32)
            normal = FACES[rng.integers(len(FACES))] if rng.random() < 0.8 else rng.normal(size=3).astype(F32)
            u, refl = float(F32(rng.random())), float(F32(rng.choice([0.0, 0.04, 0.5, 1.0])))
            for leaving in (False, True):
                want, want_branch = rref.bend(ior, refl, d, normal, u, leaving)
                got, got_branch = _ffi.water_refract(ior, refl, d, normal, u, leaving)
                assert got_branch == want_branch and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (ior, refl, d, normal, u, leaving, got, want)
                taken.add(got_branch)
                n_cases += 1
    assert taken == {_ffi.REFRACT_ENTERED, _ffi.REFRACT_TOTAL, _ffi.REFRACT_MIRRORED, _ffi.REFRACT_LEFT} and n_cases == 7000
    with pytest.raises(ValueError):
        _ffi.water_refract(0.5, 0.0, DOWN, UP)
    with pytest.raises(ValueError):
        _ffi.water_refract(float("nan"), 0.0, DOWN, UP)


def _walk_queries(rng, n):
    """Origins inside the basin's water and directions: random ones, axis-parallel ones (a zero component: the DDA's divisions
    by zero), ones with two zero components, and near-grazing ones."""
    o = np.stack([rng.uniform(K.X0, K.X1, n), rng.uniform(K.FLOOR_TOP, K.SURFACE, n), rng.uniform(K.X0, K.X1, n)], axis=1).astype(F32)
    d = rng.normal(size=(n, 3)).astype(F32)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    kind = rng.integers(0, 6, n)
    for i in range(n):
        if kind[i] == 0:
            d[i, rng.integers(3)] = 0.0
        elif kind[i] == 1:
            axis = rng.integers(3)
            d[i] = 0.0
            d[i, axis] = rng.choice([-1.0, 1.0])
        elif kind[i] == 2:
            d[i, 1] *= F32(1e-3)
        elif kind[i] == 3:
            d[i, rng.integers(3)] = -0.0
            o[i] = np.floor(o[i]) + F32(0.5)
    return o, d


@pytest.mark.parametrize("world", ["pool", "two liquid", "two solid", "column"])
def test_the_host_mirrors_span_walk_is_the_references(rref, orc, world):
    """vrth_world_water_span over the host world against the reference's walk over the oracle's scene: dist bit for bit (a NaN is a
    NaN), prev, m, v, the steps taken and the event.  An axis-parallel direction leaves lens of inf and NaN: where the last step's dist is
    one of them there is no event."""
    sc = {"pool": lambda: K.pool("down", (8, 8)), "two liquid": lambda: K.two_liquids("down", (8, 8)),
          "two solid": lambda: K.two_liquids("down", (8, 8), liquid=False), "column": lambda: RC.column("column_up", (8, 8))}[world]()
    s = orc.from_package_scene(sc)
    rng = np.random.default_rng(8)
    o, d = _walk_queries(rng, 3000)
    seen = {"event": 0, "solid": 0, "cap": 0, "not finite": 0, "crossed": 0, "no chunk": 0}
    for i in range(len(o)):
        for span in (64, 2, 1024) if i % 10 == 0 else (64,):
            want = rref.span(s, o[i], d[i], span)
            got = _ffi.world_water_span(sc.world._h, sc.materials, o[i], d[i], span)
            got_bits = int(np.array([got.dist], F32).view(np.uint32)[0])
            both_nan = math.isnan(got.dist) and math.isnan(float(np.array([want.dist], np.uint32).view(F32)[0]))
            assert got_bits == want.dist or both_nan, (o[i], d[i], span, got.dist, want)
            assert (tuple(got.prev), tuple(got.m), got.v, got.steps, bool(got.event)) == (want.prev, want.m, want.v, want.steps, want.event), (o[i], d[i], span, want)
            finite = math.isfinite(got.dist)
            assert not (got.event and not (finite and got.dist >= 0.0))
            seen["event"] += want.event
            seen["solid"] += want.ended and want.v != 0
            seen["cap"] += not want.ended
            seen["not finite"] += want.ended and want.v == 0 and not finite
            seen["crossed"] += want.crossed
            seen["no chunk"] += want.event and want.m[1] >= 32
    print(world, seen)
    assert seen["event"] >= 100 and seen["solid"] >= 100 and seen["cap"] >= 10
    if world == "two liquid":
        assert seen["crossed"] >= 50
    if world == "column":
        assert seen["no chunk"] >= 5
    # max_span 0 is 64; more than 1024 is refused
    want = rref.span(s, o[0], d[0], 64)
    got = _ffi.world_water_span(sc.world._h, sc.materials, o[0], d[0], 0)
    assert (got.steps, bool(got.event)) == (want.steps, want.event)
    with pytest.raises(ValueError):
        _ffi.world_water_span(sc.world._h, sc.materials, o[0], d[0], 1025)


def test_a_not_finite_dist_yields_no_event(rref, orc):
    """Straight up the middle of a voxel column: x and z never move (their lens are NaN: inf * 0), every step is y's and its dist is
    finite — an event at the surface.  Straight along x at the height of the pool: y's len is NaN, so neither `lx < ly` nor `lz < lx
    && lz < ly` ever holds and the DDA steps y — its dist NaN — out through the surface: no event, whatever the voxel."""
    sc = K.pool("down", (8, 8))
    s = orc.from_package_scene(sc)
    up = rref.span(s, (37.5, 10.5, 37.5), (0.0, 1.0, 0.0))
    assert up.event and up.m == (37, K.SURFACE, 37) and up.prev == (37, K.SURFACE - 1, 37) and up.steps == 2
    assert float(np.array([up.dist], np.uint32).view(F32)[0]) == 1.5
    along = rref.span(s, (37.5, 10.5, 37.5), (1.0, 0.0, 0.0))
    print(along)
    dist = float(np.array([along.dist], np.uint32).view(F32)[0])
    assert along.ended and along.v == 0 and not math.isfinite(dist) and not along.event
    got = _ffi.world_water_span(sc.world._h, sc.materials, (37.5, 10.5, 37.5), (1.0, 0.0, 0.0), 64)
    assert not got.event and tuple(got.m) == along.m and got.steps == along.steps
