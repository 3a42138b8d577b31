"""The lamp list of vrt_set_lamp_light (vrt_lamp.hip: a count per workgroup, a one-workgroup scan, an ordered write under a cap) held
to tests/lamp_ref.py's list where test_gpu_lamp.py does not reach, and the frames that index it to its frames (tests/path_ref.c).

A. Worlds of 9^3 and 11^3 chunks (lamp_cases.scan_world): 1458 and 2662 workgroups, so a scan thread owns 2 or 3 sums, one thread
   a clipped range and the ones behind it nothing; faces in workgroup 0, in the last one, in workgroups of one thread and in
   neighbours of different threads.  A cap on the base of the last workgroup with faces.  A frame of each.
B. The hand-made world under every cap at a workgroup's edge: each base, one below, one above; 1; the face count and either side
   of it.  VRT_LAMP_CAP's own bounds.
C. Random worlds of 3^3 chunks (a workgroup straddles rows and planes of the 24^3 cells): checkerboard cells, lamps next to
   lamps, voxel id 300 from a leaf entry and from a brick; the list after a change of the liquid set.  A frame.
D. The hand-made world's frames from two cameras from which lamp rays arrive at every kind of its lamps, on every route.

What no read-back shows: a scan thread that runs past the n sums (hi = lo + per) reads and writes words behind the two buffers and
changes the total only by what it finds there, and a write kernel that lets the entry at the cap through writes list[cap], one
past the allocation, and nothing below it differently.  Neither is observable through vrt_read_lamps, vrt_get_lamp_info or a frame.

What the worlds and cameras must provide is asserted from the reference alone in tests/test_lamp_ref.py.  Lists are compared
exactly, frames with util.assert_frame_parity."""
import numpy as np
import pytest

import lamp_cases as LC
import lamp_ref
from test_gpu_lamp import ENV, LAMP, ROUTES, SEED, _frame, _gpu, _same_list
from util import assert_frame_parity

pytestmark = pytest.mark.gpu

LIST_ROUTES = (("direct", {}), ("directory", {"VRT_MARCH_DIRECT_MAX_S": "0"}))
assert "VRT_LAMP_CAP" in ENV and "VRT_MARCH_DIRECT_MAX_S" in ENV   # (_gpu clears them)


@pytest.fixture(scope="module")
def lref(tmp_path_factory):
    return lamp_ref.load(tmp_path_factory.mktemp("lamp_ref"))


def _lit(monkeypatch, sc, e, env=None, lamp=LAMP):
    gpu = _gpu(monkeypatch, sc, env)
    gpu.write_emission(e)
    gpu.set_lamp_light(*lamp)
    return gpu


def _held(lref, o, sc, gpu, lamps, e, spp, what, stats=False):
    """One frame of the context against the reference's over `lamps`; the reference's counts."""
    rgb, ids = _frame(gpu, spp, stats=stats)
    ref_rgb, ref_ids = lref.render(o, LAMP, lamps, *sc.size, spp=spp, seed=SEED, emission=e)
    counts = lref.counts
    assert float(ref_rgb.max()) < 512.0, what   # (where 1e-4 is above an ulp)
    err = np.abs(rgb - ref_rgb)
    print(f"{what}: max radiance {float(ref_rgb.max()):.4g}, max error {float(err[np.isfinite(err)].max()):.3g}; {counts}")
    assert_frame_parity(rgb, ids, ref_rgb, ref_ids, what)
    return counts


# ---- A. worlds past one scan pass ----

@pytest.mark.parametrize("S", [9, 11])
def test_the_list_of_a_world_whose_scan_threads_own_several_workgroups(lref, orc, monkeypatch, S):
    world = LC.scan_world(S)
    sc = LC.scan_scene(world, S)
    e = LC.emission(lamp=2.0, ore=1.0)
    o = orc.from_package_scene(sc)
    want = lref.lamps(o, e)
    b, base, _ = LC.workgroups(want, S)
    assert b[0] == 0 and b[-1] == (8 * S) ** 3 // 256 - 1 and 0 < base[-1] < len(want)   # (tests/test_lamp_ref.py has the rest)
    # the reference's frame first: lamp rays are marched and some arrive
    ref_rgb, ref_ids = lref.render(o, LAMP, want, *sc.size, spp=3, seed=SEED, emission=e)
    counts = lref.counts
    assert counts.lamp_rays >= 1 and counts.unoccluded >= 1, counts
    assert float(ref_rgb.max()) < 512.0
    for route, env in LIST_ROUTES:
        gpu = _lit(monkeypatch, sc, e, env)
        rgb, ids = _frame(gpu, 3)
        assert gpu.read_march_cells()[1] == (route == "direct")
        _same_list(gpu.read_lamps(), want, f"S = {S}, {route}")
        info = gpu.lamp_info()
        print(f"S = {S}, {route}: {info}; {counts}; max error {float(np.abs(rgb - ref_rgb).max()):.3g}")
        assert info["listed"] == info["faces"] == len(want) and info["cap"] == 1 << 20
        assert_frame_parity(rgb, ids, ref_rgb, ref_ids, f"S = {S}, {route}")
        gpu.close()
    if S == 11:   # a cap on the base of the last workgroup that has faces: that workgroup writes nothing, every one before it everything
        cap = int(base[-1])
        gpu = _lit(monkeypatch, sc, e, {"VRT_LAMP_CAP": str(cap)})
        _frame(gpu, 1)
        _same_list(gpu.read_lamps(), want[:cap], f"S = {S}, VRT_LAMP_CAP={cap}")
        info = gpu.lamp_info()
        assert info["listed"] == cap and info["cap"] == cap and info["faces"] == len(want)
        gpu.close()


# ---- B. the cap at every workgroup edge ----

def _edge_caps(want):
    b, base, _ = LC.workgroups(want, LC.S)
    F = len(want)
    caps = {1, F - 1, F, F + 1}
    for x in base.tolist():
        caps |= {x - 1, x + 1} | ({x} if x > 0 else set())
    return sorted(c for c in caps if 1 <= c <= 1 << 24), [int(x) for x in base]


def test_a_cap_at_every_workgroup_edge(lref, orc, monkeypatch):
    world = LC.hand_made_world()
    eye, rot = LC.EDGE_CAMERAS[0]
    sc = LC.hand_made_scene(world, eye=eye, rot=rot)
    e = LC.emission(lamp=2.0, ore=1.0)
    o = orc.from_package_scene(sc)
    want = lref.lamps(o, e)
    F = len(want)
    assert F == 442 + 5
    caps, bases = _edge_caps(want)
    inner = [x for x in bases if x > 0]
    assert len(inner) >= 4 and bases[0] == 0 and all(x - 1 in caps and x in caps and x + 1 in caps for x in inner)
    print(f"{F} faces; the bases of the workgroups with faces: {bases}; caps: {caps}")
    framed = (inner[len(inner) // 2], inner[len(inner) // 2] + 1, 1)   # a base, a base + 1, and 1
    assert all(c in caps for c in framed)
    for cap in caps:
        gpu = _lit(monkeypatch, sc, e, {"VRT_LAMP_CAP": str(cap)})
        n = min(cap, F)
        if cap in framed:
            _held(lref, o, sc, gpu, want[:cap], e, 1, f"VRT_LAMP_CAP={cap}")
        else:
            _frame(gpu, 1)
        _same_list(gpu.read_lamps(), want[:n], f"VRT_LAMP_CAP={cap}")
        info = gpu.lamp_info()
        assert info["listed"] == n and info["cap"] == cap and info["faces"] == F, (cap, info)
        gpu.close()


@pytest.mark.parametrize("value, cap", [("0", 1 << 20), ("-3", 1 << 20), ("16777217", 1 << 20), ("x", 1 << 20), ("16777216", 1 << 24)])
def test_the_bounds_of_the_cap_itself(lref, orc, monkeypatch, value, cap):
    world = LC.hand_made_world()
    sc = LC.hand_made_scene(world)
    e = LC.emission(lamp=2.0, ore=1.0)
    want = lref.lamps(orc.from_package_scene(sc), e)
    gpu = _lit(monkeypatch, sc, e, {"VRT_LAMP_CAP": value})
    _frame(gpu, 1)
    info = gpu.lamp_info()
    assert info["cap"] == cap and info["listed"] == info["faces"] == len(want), (value, info)
    _same_list(gpu.read_lamps(), want, f"VRT_LAMP_CAP={value}")
    gpu.close()


# ---- C. random worlds and voxel ids above 255 ----

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_list_of_a_random_world(lref, orc, monkeypatch, seed):
    world = LC.random_world(seed)
    sc = LC.random_scene(world)
    e = LC.emission_big(lamp=2.0, ore=1.0)
    o = orc.from_package_scene(sc)
    want = lref.lamps(o, e)
    assert 0 < len(want) < 1 << 20 and (want["voxel"] == LC.BIG).any()
    if seed == 0:
        ref_rgb, _ = lref.render(o, LAMP, want, *sc.size, spp=3, seed=SEED, emission=e)
        assert lref.counts.unoccluded >= 1, lref.counts
    for route, env in LIST_ROUTES:
        gpu = _lit(monkeypatch, sc, e, env)
        if seed == 0:
            _held(lref, o, sc, gpu, want, e, 3, f"seed {seed}, {route}")
        else:
            _frame(gpu, 1)
        assert gpu.read_march_cells()[1] == (route == "direct")
        _same_list(gpu.read_lamps(), want, f"seed {seed}, {route}")
        info = gpu.lamp_info()
        assert info["listed"] == info["faces"] == len(want) and info["builds"] == 1
        gpu.close()


def test_the_list_of_a_random_world_follows_the_liquid_set(lref, orc, monkeypatch):
    world = LC.random_world(1)
    sc = LC.random_scene(world)
    e = LC.emission_big(lamp=2.0, ore=1.0)
    gpu = _lit(monkeypatch, sc, e)
    gpu.set_frames_in_flight(1)   # (one frame set, so one list: vrt_lamp_info.builds counts the rebuilds of the list it reports)
    lengths, builds = [], 0
    for what, voxel, liquid in (("as uploaded", None, None), ("water solid", LC.WATER, 0), ("lamps liquid", LC.LAMP, 1)):
        if voxel is not None:
            sc.materials[voxel].is_liquid = liquid
            gpu.write_materials(sc.materials)
        o = orc.from_package_scene(sc)
        want = lref.lamps(o, e)
        _held(lref, o, sc, gpu, want, e, 1, what)
        _same_list(gpu.read_lamps(), want, what)
        info = gpu.lamp_info()
        assert info["builds"] > builds and info["listed"] == info["faces"] == len(want), (what, info)
        builds = info["builds"]
        lengths.append(len(want))
    # water solid: the lamp faces that looked at water are gone; the lamp material liquid: what is left is the ore's and id 300's
    assert lengths[0] > lengths[1] > lengths[2] > 0 and set(np.unique(want["voxel"]).tolist()) == {LC.ORE, LC.BIG}
    gpu.close()


# ---- D. frames of the hand-made world on every route ----

_refs = {}


def _edge_ref(lref, orc, world, camera, size, literal, spp, e):
    """(scene, rgb, ids, counts, the list) of the reference, computed once"""
    k = (camera, size, literal, spp)
    if k not in _refs:
        eye, rot = LC.EDGE_CAMERAS[camera]
        sc = LC.hand_made_scene(world, size=size, eye=eye, rot=rot)
        if literal:
            sc.materials[0].is_liquid = 1
        o = orc.from_package_scene(sc)
        lamps = lref.lamps(o, e)   # (under the scene's own liquid set)
        rgb, ids = lref.render(o, LAMP, lamps, *size, spp=spp, seed=SEED, emission=e)
        _refs[k] = (rgb, ids, lref.counts, lamps)
    return _refs[k]


@pytest.fixture(scope="module")
def edge_world():
    return LC.hand_made_world()


@pytest.mark.parametrize("size", LC.EDGE_SIZES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_frames_of_the_hand_made_world_match_the_reference(lref, orc, monkeypatch, edge_world, route, size):
    env, stats, literal = ROUTES[route]
    e = LC.emission(lamp=2.0, ore=1.0)
    for camera, (eye, rot) in enumerate(LC.EDGE_CAMERAS):
        sc = LC.hand_made_scene(edge_world, size=size, bounces=2, eye=eye, rot=rot)
        if literal:
            sc.materials[0].is_liquid = 1
        gpu = _lit(monkeypatch, sc, e, env)
        for spp in LC.EDGE_SPPS:
            what = f"camera {camera} {size} {route}, spp {spp}"
            ref_rgb, ref_ids, counts, lamps = _edge_ref(lref, orc, edge_world, camera, size, literal, spp, e)
            assert counts.lamp_rays >= 1 and counts.unoccluded >= 1, what
            assert float(ref_rgb.max()) < 512.0, what
            rgb, ids = _frame(gpu, spp, stats=stats)
            err = np.abs(rgb - ref_rgb)
            print(f"{what}: max radiance {float(ref_rgb.max()):.4g}, max error {float(err[np.isfinite(err)].max()):.3g}; {counts}")
            assert_frame_parity(rgb, ids, ref_rgb, ref_ids, what)
            if stats:
                st = gpu.stats()
                assert st.secondary_rays == counts.bounce_segments + counts.sun_rays + counts.lamp_rays, what
                assert st.steps == counts.steps, what
        if route == "directory":
            assert gpu.read_march_cells()[1] == False, "the context's march cells are in the direct layout"   # noqa: E712
        _same_list(gpu.read_lamps(), lamps, f"camera {camera} {size} {route}")
        gpu.close()
