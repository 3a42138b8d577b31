"""Refraction for water (vrt_set_water_refraction, include/vrt.h) on the GPU: the kernels of vrt_path_refract.h.

Against tests/refract_ref.py (A to C of the contract around the oracle's march) on the hand-built pool from its six cameras, on the
two-liquids worlds, on the column world (tests/refract_cases.py) and on C4's scene from its three lake cameras — on every route
through the kernels: the default (the grid march), the march cells behind a chunk directory, the literal march, the counting
kernels of a stats frame and a world without derived tables — at one wave, two waves, a frame that is not whole tiles and a frame of
several workgroups; 1, 2 and 4 bounces; 1 and 3 samples; one and two frames in flight; ior 1.33 and 1; water alone, with sunlight,
with the three tables, and with both.  The routes and their helpers are tests/test_gpu_water_edges.py's and tests/test_gpu_water.py's.
tests/test_refract_cases.py shows from the reference alone that the cases here take every branch of the contract.  Frames against the
reference: util.assert_frame_parity (id words equal, radiance within RADIANCE_TOL).  GPU against GPU, bit for bit: off after on,
the primary modes, accumulation, shards and devices, the denoiser.  Every test here calls vrt_set_water_refraction."""
import ctypes as C

import numpy as np
import pytest

import emission_cases as E
import refract_cases as RC
import refract_ref
import segment_cases as SC
import water_cases as K
from test_gpu_water import SEED, SUN, _all_modes, _frame, _write
from test_gpu_water import _gpu as _gpu_of_water
from test_gpu_water_edges import NO_TABLES, _none
from test_gpu_water_edges import _gpu as _gpu_of_edges
from test_gpu_water_edges import _scene as _water_scene
from test_gpu_water_edges import _tables
from voxelraytracing_amd import MODE_PATH, MODE_PRIMARY, MODE_PRIMARY_SHADOW, _ffi
from voxelraytracing_amd.graphics import VrtError

from util import assert_frame_parity

pytestmark = pytest.mark.gpu

IOR = RC.IOR
ID_HIT = 1 << 16
# (environment, stats, literal, without the derived tables)
ROUTES = {"default": ({}, False, False, False), "directory": ({"VRT_MARCH_DIRECT_MAX_S": "0"}, False, False, False),
          "literal": ({}, False, True, False), "stats": ({}, True, False, False), "no tables": ({}, False, False, True)}
KINDS = {"alone": (False, 0.0), "sun": (False, SUN), "tables": (True, 0.0), "tables + sun": (True, SUN)}
SCENES = [f"pool {cam}" for cam in K.CAMERAS] + ["c4 water", "c4 underwater", "c4 water down"]
EDGE_SCENES = ["two across", "solid across", "two under_bed", "column column_up"]


@pytest.fixture(scope="module")
def rref(tmp_path_factory):
    return refract_ref.load(tmp_path_factory.mktemp("refract_ref"))


def _scene(name, size, bounces=4, literal=False):
    """tests/test_gpu_water_edges.py's scenes, and "column <camera>" (tests/refract_cases.py)."""
    if name.startswith("column"):
        sc = RC.column(name.split(" ", 1)[1], size, bounces)
        if literal:
            sc.materials[0].is_liquid = 1
        return sc
    return _water_scene(name, size, bounces, literal)


def _gpu(monkeypatch, sc, route="default", **kw):
    """A context on a route: without the derived tables tests/test_gpu_water_edges.py's, else tests/test_gpu_water.py's with the
    route's environment."""
    env, _, _, no_tables = ROUTES[route]
    if no_tables:
        return _gpu_of_edges(monkeypatch, sc, True, **kw)
    monkeypatch.delenv(NO_TABLES, raising=False)
    return _gpu_of_water(monkeypatch, sc, env, **kw)


def _set_raw(gpu, ior=IOR, max_span=0, flags=0, reserved=0):
    o = _ffi.WaterRefraction(ior, max_span, flags, reserved)
    return gpu._lib.vrt_set_water_refraction(gpu._h, C.byref(o))


_refs = {}


def _ref(rref, orc, key, sc, tables, spp, sun=0.0, refract=IOR, sample_base=0, prim=False):
    """(rgb, ids, counts[, prim]) of the reference frame, computed once and never changed; `key` names the scene (world, materials,
    camera, bounces, size)."""
    tables = tables if tables is not None else (None, None, None)
    k = (key, tuple(None if t is None else t.tobytes() for t in tables), spp, sun, refract, sample_base, prim)
    if k not in _refs:
        plane = np.zeros((sc.size[1], sc.size[0]), np.uint8) if prim else None
        r = rref.render(orc.from_package_scene(sc), *sc.size, water=K.OPTICS, refract=refract, spp=spp, seed=SEED, sun=sun, sample_base=sample_base,
                        emission=tables[0], polish=tables[1], translucency=tables[2], prim=plane)
        _refs[k] = r + (plane,) if prim else r
    return _refs[k]


def _check(got, ref, what):
    err = np.abs(got[0] - ref[0])
    print(f"{what}: max radiance {float(ref[0].max()):.4g}, max error {float(err[np.isfinite(err)].max()):.3g}; {ref[2]}")
    assert_frame_parity(got[0], got[1], ref[0], ref[1], what)


def _check_stats(gpu, ref, what):
    """A stats frame's counts are the frame's own marches': the walk is counted nowhere."""
    st = gpu.stats()
    counts = ref[2]
    assert st.secondary_rays == counts.bounce_segments + counts.sun_rays, what
    assert st.steps == counts.steps, what
    assert st.hits == int(((ref[1] & ID_HIT) != 0).sum()), what


def _frames_of_a_scene(rref, orc, monkeypatch, name, route, size, iors=(IOR,), bounces_of=K.BOUNCES, kinds=tuple(KINDS)):
    """Every kind at 1 and 3 spp with one and two frames in flight, every bounce count and every ior, on one route, one context."""
    _, stats, literal, no_tables = ROUTES[route]
    sc = _scene(name, size, 4, literal)
    gpu = _gpu(monkeypatch, sc, route)
    all_tables = _tables(gpu, "pool" if name.startswith("column") else name)
    gpu.set_water_optics(*K.OPTICS)
    for bounces in bounces_of:
        sc.settings.max_ray_bounces = bounces
        gpu.write_settings(sc.settings)
        key = f"{name} {size} b{bounces} literal {literal}"
        for kind in kinds:
            with_tables, sun = KINDS[kind]
            tables = all_tables if with_tables else None
            _write(gpu, tables if tables is not None else _none())
            gpu.set_sun_light(sun)
            for ior in iors:
                gpu.set_water_refraction(*ior) if isinstance(ior, tuple) else gpu.set_water_refraction(ior)
                for n, spp in ((1, 1), (2, 3)) if kind != "alone" else ((1, 1), (1, 3), (2, 1), (2, 3)):
                    gpu.set_frames_in_flight(n)
                    what = f"{name} {size} b{bounces} {route} {kind} ior {ior}, {n} in flight, spp {spp}"
                    ref = _ref(rref, orc, key, sc, tables, spp, sun, ior)
                    _check(_frame(gpu, spp, stats=stats), ref, what)
                    if stats:
                        _check_stats(gpu, ref, what)
    if no_tables:
        assert gpu.accel_info().available == 0
    sc.settings.max_ray_bounces = 4
    gpu.close()


# ---- 1. frames against the reference, route by route ----

@pytest.mark.parametrize("size", K.SIZES)
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", SCENES)
def test_refracting_frames_match_the_reference(rref, orc, monkeypatch, name, route, size):
    _frames_of_a_scene(rref, orc, monkeypatch, name, route, size, iors=(IOR, 1.0))


@pytest.mark.parametrize("size", [(128, 72), (16, 8)])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", EDGE_SCENES)
def test_two_liquids_the_cap_and_the_exit_into_no_chunk(rref, orc, monkeypatch, name, route, size):
    """The liquid boundary crossed and ended on (id 300 liquid and solid), max_span = 2 on the same view, and the column whose
    top face leads into a chunk that chunk_roots holds 0 for."""
    iors = (IOR, (IOR, 2)) if name.endswith("across") else (IOR,)
    _frames_of_a_scene(rref, orc, monkeypatch, name, route, size, iors=iors, bounces_of=(4,), kinds=("alone", "tables + sun"))


def test_the_setting_is_not_a_no_op_on_these_scenes(rref, orc):
    """The frames above would also match a reference that ignored the setting, if the setting changed nothing: it does."""
    for name in SCENES + EDGE_SCENES:
        sc = _scene(name, K.SIZES[3])
        on = _ref(rref, orc, f"{name} {K.SIZES[3]} b4 literal False", sc, None, 3)
        off = _ref(rref, orc, f"{name} {K.SIZES[3]} b4 literal False", sc, None, 3, refract=None)
        assert not np.array_equal(on[0], off[0]), name
        assert on[2].under + on[2].bent >= 1, name


# ---- 2. past 256 primary workgroups ----

@pytest.mark.parametrize("route", ["default", "stats"])
def test_a_refracting_frame_past_256_workgroups(rref, orc, monkeypatch, route):
    """water_cases.SEGMENT_CASES["one_over"]: part > 0 in the bounce kernel, and every second segment follows a bent entry."""
    case = "one_over"
    size = SC.CASES[case].size
    name = f"c4 {K.SEGMENT_CASES[case]}"
    sc = _scene(name, size, 4)
    gpu = _gpu(monkeypatch, sc, route)
    tables = _tables(gpu, name)
    _write(gpu, tables)
    gpu.set_sun_light(SUN)
    gpu.set_water_optics(*K.OPTICS)
    gpu.set_water_refraction(IOR)
    ref = _ref(rref, orc, f"{name} {size} b4 literal False", sc, tables, 1, SUN)
    assert ref[2].bent >= 50000 and ref[2].under >= 10000, ref[2]
    assert float(ref[0].max()) < 512.0   # (1e-4 is above an ulp)
    _check(_frame(gpu, 1, stats=ROUTES[route][1]), ref, f"{case} {name} {route}")
    if ROUTES[route][1]:
        _check_stats(gpu, ref, f"{case} {name} {route}")
    gpu.close()


# ---- 3. GPU against GPU, bit for bit ----

@pytest.mark.parametrize("name", ["pool under_up", "c4 water"])
def test_off_is_the_plain_water_frame_and_the_primary_modes_ignore_it(monkeypatch, name):
    sc = _scene(name, K.SIZES[3])
    gpu = _gpu(monkeypatch, sc)
    _write(gpu, _tables(gpu, name))
    plain = _all_modes(gpu)   # water optics off: the plain frames
    gpu.set_water_refraction(IOR)
    got = _all_modes(gpu)
    for k in plain:
        E.assert_bit_identical(got[k], plain[k], f"the setting with water optics off: {k}")
    gpu.set_water_refraction(0.0)
    gpu.set_water_optics(*K.OPTICS)
    want = _all_modes(gpu)    # the plain water frames of a context whose refraction is off
    fresh = _gpu(monkeypatch, sc)
    _write(fresh, _tables(fresh, name))
    fresh.set_water_optics(*K.OPTICS)
    never = _all_modes(fresh)   # ... and of one that never called it
    fresh.close()
    for k in want:
        E.assert_bit_identical(want[k], never[k], f"a context that never called it: {k}")
    gpu.set_water_refraction(IOR)
    on = _all_modes(gpu)
    assert not np.array_equal(on[("path", 3)][0], want[("path", 3)][0])
    # the id words are the primary segment's own march's, and the primary modes are what they were
    for k in want:
        assert np.array_equal(on[k][1], want[k][1]), k
    for k in (("primary", 1), ("primary+shadow", 1)):
        E.assert_bit_identical(on[k], want[k], f"{k} with the setting on")
    for off_name, off in (("None", lambda: gpu._lib.vrt_set_water_refraction(gpu._h, None)), ("ior 0", lambda: _set_raw(gpu, 0.0)),
                          ("ior -0", lambda: _set_raw(gpu, -0.0)), ("ior 0, max_span 7", lambda: _set_raw(gpu, 0.0, 7)),
                          ("ior 0, max_span 1024", lambda: _set_raw(gpu, 0.0, 1024))):
        gpu.set_water_refraction(IOR)
        assert off() == 0, off_name
        for n in (1, 2):
            gpu.set_frames_in_flight(n)
            got = _all_modes(gpu)
            for k in want:
                E.assert_bit_identical(got[k], want[k], f"{off_name}, {n} in flight: {k}")
    gpu.close()


def test_steps_and_guide_are_the_plain_water_frames(monkeypatch):
    sc = _scene("c4 underwater", K.SIZES[2])
    gpu = _gpu(monkeypatch, sc)
    gpu.set_water_optics(*K.OPTICS)
    gpu.set_denoise(3, 0.0)
    out = {}
    for ior in (0.0, IOR):
        gpu.set_water_refraction(ior)
        rgb, ids = _frame(gpu, 1, stats=True)
        out[ior] = (rgb, ids, gpu.read_steps() & 0xFFFF, gpu.read_guide())   # (the low half: the primary segment's steps)
    assert np.array_equal(out[IOR][1], out[0.0][1]) and np.array_equal(out[IOR][2], out[0.0][2]) and np.array_equal(out[IOR][3], out[0.0][3])
    assert not np.array_equal(out[IOR][0], out[0.0][0])
    # one segment per path: the whole word, and every count of the stats frame — the walk is counted nowhere
    sc.settings.max_ray_bounces = 1
    gpu.write_settings(sc.settings)
    one = {}
    for ior in (0.0, IOR):
        gpu.set_water_refraction(ior)
        _, ids = _frame(gpu, 1, stats=True)
        st = gpu.stats()
        one[ior] = (ids, gpu.read_steps(), (st.primary_rays, st.secondary_rays, st.hits, st.steps, st.node_visits))
    gpu.close()
    assert np.array_equal(one[IOR][0], one[0.0][0]) and np.array_equal(one[IOR][1], one[0.0][1]) and one[IOR][2] == one[0.0][2]


@pytest.mark.parametrize("in_flight", [1, 2])
def test_accumulated_refracting_frames_are_one_frame_of_all_their_samples(monkeypatch, in_flight):
    sc = _scene("pool under_up", K.SIZES[2])
    gpu = _gpu(monkeypatch, sc)
    _write(gpu, _tables(gpu, "pool"))
    gpu.set_sun_light(SUN)
    gpu.set_water_optics(*K.OPTICS)
    gpu.set_water_refraction(IOR)
    gpu.set_frames_in_flight(in_flight)
    want = {n: _frame(gpu, n) for n in (3, 6, 12)}
    for _ in range(4):
        gpu.render(MODE_PATH, spp=3, seed=SEED, accumulate=True)
    rgb, ids, _ = gpu.read_output()
    E.assert_bit_identical((rgb, ids), want[12], f"{in_flight} in flight: 4 x 3 spp")
    assert gpu.accumulation() == (12, SEED)
    # an identical call does not restart the sum (max_span 0 and 64 are one setting), nor does a refused one
    gpu.set_water_refraction(IOR)
    gpu.set_water_refraction(IOR, 64)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(ior=nan), dict(ior=-1.33), dict(ior=inf), dict(ior=-inf), dict(ior=0.5), dict(ior=0.999), dict(ior=4.5), dict(ior=1e-30),
                dict(max_span=1025), dict(max_span=0xFFFFFFFF), dict(flags=1), dict(reserved=1), dict(ior=0.0, flags=2), dict(ior=0.0, max_span=1025),
                dict(ior=0.0, reserved=3)):
        assert _set_raw(gpu, **bad) == _ffi.VRT_ERR_INVALID_ARG, bad
    assert gpu._lib.vrt_set_water_refraction(None, None) == _ffi.VRT_ERR_INVALID_ARG
    assert gpu.accumulation() == (12, SEED)
    gpu.reset_accumulation()
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), want[3], "a refused call changed nothing")
    gpu.set_water_refraction(IOR, 64)
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), want[6], "after an identical call: the sum goes on")
    assert gpu.accumulation() == (6, SEED)
    gpu.set_water_refraction(1.5)
    gpu.set_water_refraction(IOR)
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), want[3], "after ior changed: the sum starts again")
    gpu.set_water_refraction(IOR, 32)
    gpu.set_water_refraction(IOR)
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), want[3], "after max_span changed: the sum starts again")
    # off on a context that is off already does not restart the sum
    gpu.set_water_refraction(0.0)
    off = {n: _frame(gpu, n) for n in (3, 6)}
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), off[3], "off: the sum started again")
    gpu.set_water_refraction(0.0, 9)
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), off[6], "off again: the sum goes on")
    gpu.close()


def test_shards_and_devices_assemble_the_whole_frame(monkeypatch):
    sc = _scene("c4 underwater", (160, 96))
    whole = _gpu(monkeypatch, sc)
    tables = _tables(whole, "c4")

    def settings(g):
        _write(g, tables)
        g.set_sun_light(SUN)
        g.set_water_optics(*K.OPTICS)
        g.set_water_refraction(IOR)

    settings(whole)
    want = _frame(whole, 3)
    whole.set_water_refraction(0.0)
    assert not np.array_equal(_frame(whole, 3)[0], want[0])
    whole.close()
    sum_rgb, all_ids = np.zeros_like(want[0]), np.zeros_like(want[1])
    for r in range(2):
        sh = _gpu(monkeypatch, sc, shard_rank=r, shard_count=2)
        settings(sh)   # (a shard's context keeps its own setting)
        rgb, ids = _frame(sh, 3)
        sum_rgb += rgb
        all_ids |= ids
        sh.close()
    E.assert_bit_identical((sum_rgb, all_ids), want, "the union of two shards")
    grp = _gpu(monkeypatch, sc, devices=[0, 0], texel_messages=True)
    settings(grp)      # (replicated to every device)
    E.assert_bit_identical(_frame(grp, 3), want, "two devices with texel messages")
    grp.close()


@pytest.mark.parametrize("name", ["pool under_up", "c4 water"])
def test_a_denoised_refracting_frame_is_the_host_filter_over_its_own_frame(monkeypatch, name):
    sc = _scene(name, K.SIZES[2])
    gpu = _gpu(monkeypatch, sc)
    gpu.set_water_optics(*K.OPTICS)
    gpu.set_water_refraction(IOR)
    for spp in (1, 3):
        raw = _frame(gpu, spp)
        gpu.set_denoise(3, 0.0)
        got = _frame(gpu, spp)
        guide = gpu.read_guide()
        gpu.set_denoise(0)
        assert np.array_equal(got[1], raw[1])
        E.assert_bit_identical((got[0], got[1]), (_ffi.denoise(raw[0], raw[1], guide, 3, 0.0), raw[1]), f"{name} spp {spp}: the filter over the raw frame")
    gpu.close()


# ---- 4. refusals ----

def test_the_refused_pairs_are_refused_with_refraction_on(monkeypatch):
    sc = _scene("pool grazing", K.SIZES[2])
    gpu = _gpu(monkeypatch, sc)
    emission = np.zeros(256, np.float32)
    emission[K.SLATE] = 1.0
    gpu.write_emission(emission)
    gpu.set_water_optics(*K.OPTICS)
    gpu.set_water_refraction(IOR)
    last = _frame(gpu, 1)
    for name, on, off, word in (("lamp light", lambda: gpu.set_lamp_light(1.0), lambda: gpu.set_lamp_light(0.0), "vrt_set_lamp_light"),
                                ("camera sampling", lambda: gpu.set_camera_sampling(1.0), lambda: gpu.set_camera_sampling(0.0), "vrt_set_camera_sampling")):
        on()
        with pytest.raises(VrtError) as e:
            gpu.render(MODE_PATH, spp=1, seed=SEED)
        assert e.value.code == _ffi.VRT_ERR_STATE and "vrt_set_water_optics" in str(e.value) and word in str(e.value), str(e.value)
        rgb, ids, _ = gpu.read_output()
        E.assert_bit_identical((rgb, ids), last, f"{name}: the last frame is still readable")
        gpu.render(MODE_PRIMARY)   # (the primary modes are not refused)
        gpu.render(MODE_PRIMARY_SHADOW)
        off()
        E.assert_bit_identical(_frame(gpu, 1), last, f"{name} off again")
    gpu.close()


def test_every_invalid_argument_leaves_the_setting_as_it_was(monkeypatch):
    sc = _scene("pool under_up", K.SIZES[1])
    gpu = _gpu(monkeypatch, sc)
    gpu.set_water_optics(*K.OPTICS)
    nan, inf = float("nan"), float("inf")
    bads = (dict(ior=nan), dict(ior=-1.0), dict(ior=-1e-3), dict(ior=inf), dict(ior=0.99999994), dict(ior=4.0000005), dict(max_span=1025),
            dict(flags=1), dict(flags=0x80000000), dict(reserved=1), dict(ior=0.0, flags=1), dict(ior=0.0, reserved=1), dict(ior=0.0, max_span=2000))
    for ior, span in ((0.0, 0), (IOR, 0), (4.0, 1024), (1.0, 1)):
        assert _set_raw(gpu, ior, span) == 0
        want = _frame(gpu, 3)
        for bad in bads:
            assert _set_raw(gpu, **bad) == _ffi.VRT_ERR_INVALID_ARG, bad
            assert "vrt_set_water_refraction" in gpu._lib.vrt_last_error(gpu._h).decode()
        E.assert_bit_identical(_frame(gpu, 3), want, f"after the refused calls, ior {ior} max_span {span}")
    gpu.close()


# ---- 5. one visible check that is not parity ----

def test_total_reflection_is_darker_than_the_window(rref, orc, monkeypatch):
    """From inside the pool looking up: the pixels whose primary underside event is totally reflected see the pool's dark inside
    mirrored, those transmitted see the sky through Snell's window.  The sets are the reference's at 1 spp — the branch of the first
    sample's primary event: total reflection is geometry, the same for all 12 samples of the frame; a pixel of the transmitted set is
    one whose first sample left the water, and others of its samples may have been mirrored by their own draws."""
    size = (128, 72)
    sc = _scene("pool under_up", size, 4)
    ref = _ref(rref, orc, f"pool under_up {size} b4 literal False", sc, None, 1, prim=True)
    total, out = ref[3] == refract_ref.PRIM_TOTAL, ref[3] == refract_ref.PRIM_OUT
    assert total.sum() >= 1000 and out.sum() >= 1000
    gpu = _gpu(monkeypatch, sc)
    gpu.set_water_optics(*K.OPTICS)
    plain = _frame(gpu, 12)
    gpu.set_water_refraction(IOR)
    got = _frame(gpu, 12)
    gpu.close()
    mean_total, mean_out = float(got[0][total].mean()), float(got[0][out].mean())
    print(f"mean radiance: totally reflected {mean_total:.4g} ({int(total.sum())} pixels), transmitted {mean_out:.4g} ({int(out.sum())} pixels)")
    assert mean_total < mean_out
    assert not np.array_equal(got[0][total], plain[0][total]) and not np.array_equal(got[0][out], plain[0][out])
