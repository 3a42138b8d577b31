"""The water kernels (vrt_path_water.h, vrt_water.h, vrt_denoise.hip's water guide) where tests/test_gpu_water.py does not take them,
against tests/water_ref.py:

1. a world without derived tables (VRT_ACCEL_MAX_S below the world's size): the MARCH = 2 builds of both trace kernels and of
   the guide kernel, and water_voxel_at's walk from the chunk's root;
2. a camera in a chunk that does not exist ("pool above"), and the two-liquids worlds (tests/water_cases.py): a liquid set that
   is no id range and holds entry 255, a liquid-to-liquid boundary, a solid with an id above 255 behind water;
3. frames past 256 primary workgroups (tests/segment_cases.py's sizes from the lake cameras): part > 0 and record indices past
   256 in path_water_bounce_kernel, with wet and dry lanes in one wave, and sun records appended past 256;
4. the guide words of a denoised water frame, the whole frame bit for bit against water_ref's guide(), and the denoised frame
   against tests/denoise_ref.py's filter over the raw frame and that guide;
5. edits of the world between water frames, through the context's own update path, with one and two frames in flight.

tests/test_water_cases.py shows from the reference alone that each case reaches what it is here for.  Frames against the
reference: util.assert_frame_parity (id words equal, radiance within RADIANCE_TOL)."""
import numpy as np
import pytest

import denoise_ref
import emission_cases as E
import path_ref
import segment_cases as SC
import water_cases as K
import water_ref
from test_gpu_water import ENV, SCENES, SEED, SUN, _frame, _write
from test_gpu_water import _tables as _tables_of_a_world
from voxelraytracing_amd import MODE_PATH

from util import assert_frame_parity, gpu_for_scene

pytestmark = pytest.mark.gpu

NO_TABLES = "VRT_ACCEL_MAX_S"
# (stats, literal, without the derived tables)
ROUTES = {"default": (False, False, False), "literal": (False, True, False), "stats": (True, False, False), "no tables": (False, False, True)}
KINDS = ("alone", "sun", "tables + sun")
SPPS = (1, 3)


@pytest.fixture(scope="module")
def wref(tmp_path_factory):
    return water_ref.load(tmp_path_factory.mktemp("water_ref"))


@pytest.fixture(scope="module")
def dref(tmp_path_factory):
    return denoise_ref.load(tmp_path_factory.mktemp("denoise_ref"))


def _scene(name, size, bounces=4, literal=False):
    """"pool <camera>", "two <camera>" (two liquids, entry 255 liquid), "solid <camera>" (entry 255 solid), "c4 <lake camera>"."""
    kind, cam = name.split(" ", 1)
    sc = {"pool": K.pool, "c4": K.c4_lake, "two": K.two_liquids, "solid": lambda *a: K.two_liquids(*a, liquid=False)}[kind](cam, size, bounces)
    if literal:
        sc.materials[0].is_liquid = 1
    return sc


def _gpu(monkeypatch, sc, no_tables=False, **kw):
    """A context for the scene; no_tables: created under VRT_ACCEL_MAX_S below the world's size in chunks (read when the context
    is created), so that it keeps no derived tables and every march is the octree walk."""
    for k in ENV + [NO_TABLES]:
        monkeypatch.delenv(k, raising=False)
    if no_tables:
        s = sc.world.size_in_chunks()
        monkeypatch.setenv(NO_TABLES, {2: "1", 8: "4"}[s])
    gpu = gpu_for_scene(sc, **kw)
    monkeypatch.delenv(NO_TABLES, raising=False)
    return gpu


def _tables(gpu, name):
    """tests/test_gpu_water.py's tables: the pool's for every pool world (entry 255, the two-liquids worlds' second id, passes half
    of the time with a black tint where it is solid), C4's from the context's own frame."""
    return _tables_of_a_world(gpu, name if name.startswith("c4") else "pool")


_refs = {}


def _ref(wref, orc, key, sc, tables, spp, sun, sample_base=0):
    """(rgb, ids, counts) of the reference frame, computed once; `key` names the scene (world, materials, camera, bounces, size)."""
    tables = tables if tables is not None else (None, None, None)
    k = (key, tuple(None if t is None else t.tobytes() for t in tables), spp, sun, sample_base)
    if k not in _refs:
        _refs[k] = wref.render(orc.from_package_scene(sc), *sc.size, water=K.OPTICS, spp=spp, seed=SEED, sun=sun, sample_base=sample_base,
                               emission=tables[0], polish=tables[1], translucency=tables[2])
    return _refs[k]


def _none():
    return np.zeros(256, np.float32), path_ref.polish_table(), path_ref.translucency_table()


def _set_kind(gpu, kind, all_tables):
    """The tables and the sun of a kind; what the reference is given."""
    tables, sun = {"alone": (None, 0.0), "sun": (None, SUN), "tables + sun": (all_tables, SUN)}[kind]
    _write(gpu, tables if tables is not None else _none())
    gpu.set_sun_light(sun)
    return tables, sun


def _check(got, ref, what):
    err = np.abs(got[0] - ref[0])
    print(f"{what}: max radiance {float(ref[0].max()):.4g}, max error {float(err[np.isfinite(err)].max()):.3g}; {ref[2]}")
    assert_frame_parity(got[0], got[1], ref[0], ref[1], what)


def _check_stats(gpu, counts, what):
    st = gpu.stats()
    assert st.secondary_rays == counts.bounce_segments + counts.sun_rays, what
    assert st.steps == counts.steps, what


def _frames_of_a_scene(wref, orc, monkeypatch, name, route, size, bounces, stats_frame=False):
    """Every kind at 1 and 3 spp on one route, one context; stats_frame: then the last frame again as a stats frame."""
    stats, literal, no_tables = ROUTES[route]
    sc = _scene(name, size, bounces, literal)
    gpu = _gpu(monkeypatch, sc, no_tables)
    key = f"{name} {size} b{bounces} literal {literal}"
    all_tables = _tables(gpu, name)
    gpu.set_water_optics(*K.OPTICS)
    for kind in KINDS:
        tables, sun = _set_kind(gpu, kind, all_tables)
        for spp in SPPS:
            what = f"{name} {size} b{bounces} {route} {kind} spp {spp}"
            ref = _ref(wref, orc, key, sc, tables, spp, sun)
            _check(_frame(gpu, spp, stats=stats), ref, what)
            if stats:
                _check_stats(gpu, ref[2], what)
    if stats_frame:
        _check(_frame(gpu, spp, stats=True), ref, what + ", stats")
        _check_stats(gpu, ref[2], what + ", stats")
    if no_tables:
        assert gpu.accel_info().available == 0
    gpu.close()
    return sc


# ---- 1. without the derived tables ----

@pytest.mark.parametrize("bounces", [1, 4])
@pytest.mark.parametrize("size", [(8, 8), (100, 60), (128, 72)])
@pytest.mark.parametrize("name", SCENES + ["pool above"])
def test_a_world_without_tables_walks_the_octree(wref, orc, monkeypatch, name, size, bounces):
    _frames_of_a_scene(wref, orc, monkeypatch, name, "no tables", size, bounces, stats_frame=True)


# ---- 2. a camera in a chunk that does not exist; a liquid set that is no range, ids above 255 ----

EDGE_SCENES = ["pool above"] + [f"{world} {cam}" for world in ("two", "solid") for cam in ("down", "across", "under_bed", "grazing")]


@pytest.mark.parametrize("size", [(128, 72), (16, 8)])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", EDGE_SCENES)
def test_the_camera_above_and_the_two_liquids_worlds(wref, orc, monkeypatch, name, route, size):
    sc = _frames_of_a_scene(wref, orc, monkeypatch, name, route, size, 4)
    if name.startswith("two") and route != "literal":
        assert not K.is_one_range_below_255(K.liquid_ids(sc.materials))


# ---- 3. past 256 workgroups ----

def _lake(case):
    return f"c4 {K.SEGMENT_CASES[case]}"


SEGMENT_FRAMES = [("three_parts", r, 4) for r in ("default", "stats", "no tables")] + \
                 [(c, r, 4) for c in ("one_over", "one_over_ragged") for r in ("default", "stats")] + \
                 [("four_parts", r, b) for r in ("default", "stats") for b in (1, 2, 4)]


@pytest.mark.parametrize("case,route,bounces", SEGMENT_FRAMES)
def test_water_frames_past_256_workgroups(wref, orc, monkeypatch, case, route, bounces):
    size = SC.CASES[case].size
    stats, literal, no_tables = ROUTES[route]
    name = _lake(case)
    sc = _scene(name, size, bounces)
    gpu = _gpu(monkeypatch, sc, no_tables)
    key = f"{name} {size} b{bounces} literal False"
    all_tables = _tables(gpu, name)
    gpu.set_water_optics(*K.OPTICS)
    for kind in KINDS:
        tables, sun = _set_kind(gpu, kind, all_tables)
        for spp in SPPS:
            what = f"{case} {name} b{bounces} {route} {kind} spp {spp}"
            ref = _ref(wref, orc, key, sc, tables, spp, sun)
            assert float(ref[0].max()) < 512.0, what   # (1e-4 is above an ulp)
            rgb, ids = _frame(gpu, spp, stats=stats)
            _check((rgb, ids), ref, what)
            if stats:
                _check_stats(gpu, ref[2], what)
            if case == "one_over_ragged":
                w, h = SC.CASES["one_over"].size
                assert not rgb[h:].any() and not rgb[:, w:].any() and not ids[h:].any() and not ids[:, w:].any(), what
    if no_tables:
        assert gpu.accel_info().available == 0
    gpu.close()


def _four_parts(wref, orc, monkeypatch, **kw):
    """A sun-lit context with every table for four_parts, and what its reference is given."""
    case = "four_parts"
    name, size = _lake(case), SC.CASES[case].size
    sc = _scene(name, size)
    gpu = _gpu(monkeypatch, sc, **kw)
    tables = _tables(gpu, name)
    _write(gpu, tables)
    gpu.set_sun_light(SUN)
    gpu.set_water_optics(*K.OPTICS)
    return gpu, sc, tables, f"{name} {size} b4 literal False"


def test_the_union_of_two_shards_of_four_parts_is_the_reference_frame(wref, orc, monkeypatch):
    whole, sc, tables, key = _four_parts(wref, orc, monkeypatch)
    whole.close()
    ref = _ref(wref, orc, key, sc, tables, 3, SUN)
    sum_rgb, all_ids = np.zeros_like(ref[0]), np.zeros_like(ref[1])
    for r in range(2):
        sh = _gpu(monkeypatch, sc, shard_rank=r, shard_count=2)
        _write(sh, tables)
        sh.set_sun_light(SUN)
        sh.set_water_optics(*K.OPTICS)
        rgb, ids = _frame(sh, 3)
        assert not (all_ids != 0)[ids != 0].any()   # (the shards' tiles are disjoint)
        sum_rgb += rgb
        all_ids |= ids
        sh.close()
    _check((sum_rgb, all_ids), ref, "four_parts: the union of two shards")


@pytest.mark.parametrize("in_flight", [1, 2])
def test_four_parts_three_water_frames_back_to_back(wref, orc, monkeypatch, in_flight):
    gpu, sc, tables, key = _four_parts(wref, orc, monkeypatch)
    gpu.set_frames_in_flight(in_flight)
    for _ in range(3):
        gpu.render(MODE_PATH, spp=3, seed=SEED)
    rgb, ids, _ = gpu.read_output()
    _check((rgb, ids), _ref(wref, orc, key, sc, tables, 3, SUN), f"four_parts, the third of three frames, {in_flight} in flight")
    gpu.close()


@pytest.mark.parametrize("in_flight", [1, 2])
def test_four_accumulated_water_frames_are_the_references_four_samples(wref, orc, monkeypatch, in_flight):
    gpu, sc, tables, key = _four_parts(wref, orc, monkeypatch)
    gpu.set_frames_in_flight(in_flight)
    for _ in range(4):
        gpu.render(MODE_PATH, spp=1, seed=SEED, accumulate=True)
    rgb, ids, _ = gpu.read_output()
    assert gpu.accumulation() == (4, SEED)
    _check((rgb, ids), _ref(wref, orc, key, sc, tables, 4, SUN), f"four_parts: 4 x 1 spp accumulated, {in_flight} in flight")
    gpu.close()


# ---- 4. the guide, the whole frame ----

@pytest.mark.parametrize("route", ["default", "literal", "no tables"])
@pytest.mark.parametrize("name", SCENES + ["pool above", "two down", "two across"])
def test_the_water_guide_is_the_references_and_the_denoised_frame_its_filter(wref, dref, orc, monkeypatch, name, route):
    _, literal, no_tables = ROUTES[route]
    for size in ((100, 60), (128, 72)):
        sc = _scene(name, size, 4, literal)
        gpu = _gpu(monkeypatch, sc, no_tables)
        gpu.set_water_optics(*K.OPTICS)
        o = orc.from_package_scene(sc)
        want_guide, want_ids = wref.guide(dref, o, *size, water=K.OPTICS)
        for spp in SPPS:
            what = f"{name} {size} {route} spp {spp}"
            raw = _frame(gpu, spp)
            gpu.set_denoise(3, 0.0)
            got = _frame(gpu, spp)
            guide = gpu.read_guide()
            gpu.set_denoise(0)
            assert np.array_equal(raw[1], want_ids) and np.array_equal(got[1], want_ids), what
            bad = np.argwhere(guide != want_guide)
            assert bad.size == 0, f"{what}: {len(bad)} guide words differ from the reference's, first at (y, x) = {tuple(bad[0])}: " \
                                  f"{guide[tuple(bad[0])]} against {want_guide[tuple(bad[0])]}"
            want = dref.denoise(raw[0], raw[1], want_guide, 3, 0.0)
            assert np.array_equal(denoise_ref.bits(got[0]), denoise_ref.bits(want)), f"{what}: the filter over the raw frame and the reference's guide"
        assert want_guide.any() or name == "pool under_up", what   # (that camera looks out of the water at the sky: no face, guide 0)
        gpu.close()


# ---- 5. edits between water frames ----

@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("route", ["default", "no tables"])
def test_edits_between_water_frames(wref, orc, monkeypatch, route, in_flight):
    """A water frame's kernels read chunk_roots and the node pool themselves (water_voxel_at), so an upload waits for them: the
    dry "grazing" eye gets a water voxel around it and turns wet, loses it again, then a column of the basin is drained."""
    size = (128, 72)
    sc = K.pool("grazing", size, world=K.fresh_pool_world())
    gpu = _gpu(monkeypatch, sc, ROUTES[route][2])
    gpu.set_sun_light(SUN)
    gpu.set_water_optics(*K.OPTICS)
    gpu.set_frames_in_flight(in_flight)
    eye = tuple(int(c) for c in K.CAMERAS["grazing"][0])

    def edit(pos, v):
        start, n = sc.world.set_voxel(pos, v)
        gpu.write_nodes(sc.world.nodes_ptr(), start, start + n)
        gpu.write_chunk_roots(sc.world.chunk_roots())

    def frame(what, wet):
        got = _frame(gpu, 3)
        o = orc.from_package_scene(sc)   # the world as it is now
        assert wref.eye_is_wet(o) == wet, what
        ref = wref.render(o, *size, water=K.OPTICS, spp=3, seed=SEED, sun=SUN)
        _check(got, ref, f"{what}, {route}, {in_flight} in flight")
        return got, ref

    first, ref_first = frame("the pool", False)
    edit(eye, K.WATER)
    wet, ref_wet = frame("a water voxel around the eye", True)
    assert ref_wet[2].wet_primary_w > 0 and not np.array_equal(ref_wet[0], ref_first[0])
    edit(eye, 0)
    third, _ = frame("the voxel removed", False)
    E.assert_bit_identical(third, first, "the third frame is the first")
    for y in range(K.FLOOR_TOP, K.SURFACE):
        edit((K.X0, y, 32), 0)   # the column nearest to the eye on its line of sight
    _, ref_drained = frame("a column of the basin drained", False)
    assert not np.array_equal(ref_drained[1], ref_first[1])   # (the camera sees it)
    if ROUTES[route][2]:
        assert gpu.accel_info().available == 0
    gpu.close()
