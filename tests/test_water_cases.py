"""tests/water_cases.py's newer cases without a GPU: from the reference alone (tests/water_ref.py), that each of them reaches the code
tests/test_gpu_water_edges.py is there for — a camera in a chunk that does not exist, a liquid set that is no id range and holds
entry 255, a liquid-to-liquid boundary, a solid with an id above 255 behind water, and water frames whose path and sun segments
hold more than 256 and 512 records with wet and dry lanes in one wave.  The load planes and the guide helper are held to what they
are said to be as well.  A case that stops reaching the code fails here, not there."""
import numpy as np
import pytest

import denoise_ref
import segment_cases as SC
import water_cases as K
import water_ref
from water_ref import LOAD_PATH, LOAD_SUN, LOAD_WET

SIZE = (128, 72)
ID_WATER = 1 << 20
VOXEL = 0x7FFF


@pytest.fixture(scope="module")
def wref(tmp_path_factory):
    return water_ref.load(tmp_path_factory.mktemp("water_ref"))


@pytest.fixture(scope="module")
def dref(tmp_path_factory):
    return denoise_ref.load(tmp_path_factory.mktemp("denoise_ref"))


# ---- the load planes ----

def test_the_load_planes_change_nothing_and_sum_to_the_counts(wref, orc):
    sc = K.pool("grazing", (100, 60))
    o = orc.from_package_scene(sc)
    plain = wref.render(o, 100, 60, water=K.OPTICS, spp=3, seed=K.SEED, sun=1.0)
    load = np.zeros((3, 4, 60, 100), np.uint8)
    got = wref.render(o, 100, 60, water=K.OPTICS, spp=3, seed=K.SEED, sun=1.0, load=load)
    assert np.array_equal(plain[0].view(np.uint32), got[0].view(np.uint32)) and np.array_equal(plain[1], got[1]) and plain[2] == got[2]
    n = got[2]
    assert not load[:, :, 56:].any() and not load[:, :, :, 96:].any() and not (load & ~np.uint8(7)).any()
    assert int(((load & LOAD_SUN) != 0).sum()) == n.sun_rays
    assert int(((load[:, 1:] & LOAD_WET) != 0).sum()) == n.wet_bounces
    # a path alive into segment b + 1 is a bounce segment — except behind the last allowed segment, which nothing enters
    assert not (load[:, 3] & LOAD_PATH).any()
    assert int(((load[:, :3] & LOAD_PATH) != 0).sum()) == n.bounce_segments
    # a segment that nobody entered has no bits
    entered = np.concatenate([np.ones_like(load[:, :1], bool), (load[:, :3] & LOAD_PATH) != 0], axis=1)
    entered[:, :, 56:] = False
    entered[:, :, :, 96:] = False
    assert not load[~entered].any()
    # with the setting off no segment starts wet
    off = np.zeros((1, 4, 60, 100), np.uint8)
    wref.render(o, 100, 60, water=None, spp=1, seed=K.SEED, load=off)
    assert not (off & LOAD_WET).any() and (off & LOAD_PATH).any()


# ---- "above": a camera inside the world box in a chunk that does not exist ----

def test_the_camera_above_sits_in_a_chunk_without_a_root(wref, orc):
    sc = K.pool("above", SIZE)
    o = orc.from_package_scene(sc)
    eye = K.CAMERAS["above"][0]
    w = sc.world.size_in_chunks()
    ch = (int(eye[0]) >> 5) + w * ((int(eye[1]) >> 5) + w * (int(eye[2]) >> 5))
    assert all(0.0 <= c < 32.0 * w for c in eye)
    assert int(sc.world.chunk_roots()[ch]) == 0
    assert wref.voxel_at_floor(o, eye) == 0 and not wref.eye_is_wet(o)
    # (the chunk below it exists, and the reference's look-up finds the pool's voxels there)
    assert wref.voxel_at_floor(o, (37.5, 10.5, 37.5)) == K.WATER and wref.voxel_at_floor(o, (37.5, 8.5, 37.5)) == K.SLATE
    assert wref.voxel_at_floor(o, (-0.5, 10.5, 37.5)) == 0 and wref.voxel_at_floor(o, (37.5, 64.0, 37.5)) == 0
    _, ids, n = wref.render(o, *SIZE, water=K.OPTICS, spp=1, seed=K.SEED)
    water = int(((ids & VOXEL) == K.WATER).sum())
    print(f"pool above {SIZE}: {water} water pixels, {n}")
    assert water >= 1000 and n.surface >= water
    assert (water, n.surface) == (1819, 1842)   # water_cases.py's comment


def test_a_camera_outside_the_world_box_traces_nothing(wref, orc):
    """Why there is no such frame case: the march gives up before its first step."""
    sc = K.pool("above", SIZE)
    sc.cam = K.g.cam_data_create((90.0, 0.0, 0.0), (37.5, 70.5, 37.5), 70.0, (float(SIZE[0]), float(SIZE[1])))
    _, ids, n = wref.render(orc.from_package_scene(sc), *SIZE, water=K.OPTICS, spp=1, seed=K.SEED)
    assert n.steps == 0 and not ids.any()


# ---- two liquids ----

def test_the_two_liquids_tables_are_no_range(orc):
    own = K.liquid_ids(K.pool("down", SIZE).materials)   # the pack's: ids 2 and 3, one range (only 3 is in these worlds)
    assert K.WATER in own and K.is_one_range_below_255(own)
    sc = K.two_liquids("down", SIZE, liquid=True)
    ids = K.liquid_ids(sc.materials)
    assert ids == own + [255] and not K.is_one_range_below_255(ids)   # not contiguous, and entry 255 among them
    assert K.liquid_ids(K.two_liquids("down", SIZE, liquid=False).materials) == own
    w = sc.world
    assert w.get_voxel((31, 10, 37)) == K.WATER and w.get_voxel((32, 10, 37)) == K.OTHER and w.get_voxel((43, 11, 43)) == K.OTHER
    assert w is not K.pool_world() and K.pool_world().get_voxel((32, 10, 37)) == K.WATER


def test_two_liquids_with_entry_255_liquid(wref, orc):
    down = K.two_liquids("down", SIZE, liquid=True)
    _, ids, n = wref.render(orc.from_package_scene(down), *SIZE, water=K.OPTICS, spp=3, seed=K.SEED)
    a, b = int(((ids & VOXEL) == K.WATER).sum()), int(((ids & VOXEL) == K.OTHER).sum())
    print(f"two liquids, down: {a} pixels of id {K.WATER}, {b} of id {K.OTHER}; {n}")
    assert a > 0 and b > 0 and n.surface >= a + b
    assert (a, b, n.surface) == (2189, 5256, 22543)
    across = K.two_liquids("across", SIZE, liquid=True)
    o = orc.from_package_scene(across)
    assert wref.eye_is_wet(o) and wref.voxel_at_floor(o, K.CAMERAS["across"][0]) == K.WATER
    load = np.zeros((3, 4, SIZE[1], SIZE[0]), np.uint8)
    _, ids, n = wref.render(o, *SIZE, water=K.OPTICS, spp=3, seed=K.SEED, load=load)
    wet = int(((load[:, 0] & LOAD_WET) != 0).sum())
    print(f"two liquids, across: {wet} wet primaries; {n}")
    assert wet >= 1000 and wet == 3 * SIZE[0] * SIZE[1] == 27648
    # an eye inside id 300 is wet through entry 255
    for cam in ("under_bed", "under_up"):
        o = orc.from_package_scene(K.two_liquids(cam, SIZE, liquid=True))
        assert wref.voxel_at_floor(o, K.CAMERAS[cam][0]) == K.OTHER and wref.eye_is_wet(o)


def test_two_liquids_with_entry_255_solid(wref, orc):
    across = K.two_liquids("across", SIZE, liquid=False)
    _, ids, n = wref.render(orc.from_package_scene(across), *SIZE, water=K.OPTICS, spp=3, seed=K.SEED)
    seen = int((((ids & VOXEL) == K.OTHER) & ((ids & ID_WATER) != 0)).sum())
    print(f"two liquids (entry 255 solid), across: {seen} pixels of id {K.OTHER} through water; {n}")
    assert seen >= 1000 and seen == 1688
    for cam in ("under_bed", "under_up"):   # the eye inside the solid block: dry
        o = orc.from_package_scene(K.two_liquids(cam, SIZE, liquid=False))
        load = np.zeros((3, 4, SIZE[1], SIZE[0]), np.uint8)
        _, _, n = wref.render(o, *SIZE, water=K.OPTICS, spp=3, seed=K.SEED, load=load)
        print(f"two liquids (entry 255 solid), {cam}: {n}")
        assert not wref.eye_is_wet(o) and not (load & LOAD_WET).any() and n.wet_w == 0 and n.wet_bounces == 0


# ---- the guide helper ----

def test_the_guide_is_the_dry_scenes_for_a_dry_camera_and_the_scenes_own_for_a_wet_one(wref, dref, orc):
    for sc, wet in ((K.pool("down", SIZE), False), (K.pool("above", SIZE), False), (K.pool("under_bed", SIZE), True),
                    (K.two_liquids("across", SIZE), True), (K.two_liquids("under_bed", SIZE, liquid=False), False)):
        o = orc.from_package_scene(sc)
        assert wref.eye_is_wet(o) == wet, sc.name
        guide, ids = wref.guide(dref, o, *SIZE, water=K.OPTICS)
        _, ref_ids, _ = wref.render(o, *SIZE, water=K.OPTICS, spp=1, seed=K.SEED)
        assert np.array_equal(ids, ref_ids), sc.name   # the primary segments the frame marches
        plain, plain_ids = dref.guide(o, *SIZE)
        off, off_ids = wref.guide(dref, o, *SIZE, water=None)
        assert np.array_equal(off, plain) and np.array_equal(off_ids, plain_ids)
        if wet:
            assert np.array_equal(guide, plain) and np.array_equal(ids, plain_ids), sc.name
        assert [m.is_liquid for m in o.mats][K.WATER] == 1   # (the scene is left as it was)
    # from above the water the two differ: the face of the water, y = 12, against the bed's, y = 9
    o = orc.from_package_scene(K.pool("down", SIZE))
    guide, ids = wref.guide(dref, o, *SIZE, water=K.OPTICS)
    plain, _ = dref.guide(o, *SIZE)
    water = (ids & VOXEL) == K.WATER
    # (through the water a few pixels see the side of a wall or of the pillar instead of the bed)
    assert water.sum() >= 1000 and (guide[water] == K.SURFACE).all() and (plain[water] == K.FLOOR_TOP).sum() >= 1000


# ---- past 256 workgroups ----

_frames = {}


def _lake(wref, orc, case, spp=1):
    """The lake camera's reference frame at a segment case's size, 4 bounces, the sun on, with its load planes."""
    if (case, spp) not in _frames:
        size = SC.CASES[case].size
        sc = K.c4_lake(K.SEGMENT_CASES[case], size)
        load = np.zeros((spp, 4, size[1], size[0]), np.uint8)
        rgb, ids, n = wref.render(orc.from_package_scene(sc), *size, water=K.OPTICS, spp=spp, seed=K.SEED, sun=1.0, load=load)
        _frames[case, spp] = (rgb, ids, n, load)
    return _frames[case, spp]


# (bounce segments, surface events, sun rays, wet bounce segments) at 4 bounces, 1 spp, sun 1.0: water_cases.py's table
WATER_LOADS = {
    "one_over": (145343, 66016, 58522, 139825),
    "one_over_ragged": (145414, 66053, 58975, 139857),
    "three_parts": (319558, 104288, 124149, 222593),
    "four_parts": (456677, 179876, 140675, 300357),
}


def test_why_one_over_looks_down(wref, orc):
    """From the lake camera itself a 328 x 200 frame's segment 0 never holds more than 256 sun records."""
    size = SC.CASES["one_over"].size
    load = np.zeros((1, 4, size[1], size[0]), np.uint8)
    sc = K.c4_lake("water", size)   # (kept alive: the oracle's scene points into its world)
    _, _, n = wref.render(orc.from_package_scene(sc), *size, water=K.OPTICS, spp=1, seed=K.SEED, sun=1.0, load=load)
    assert (n.bounce_segments, n.surface, n.sun_rays, n.wet_bounces) == (143743, 50262, 51678, 100362)
    fullest = max(int(SC.segment_loads((load[0, b] & LOAD_SUN) != 0, *size).max()) for b in range(4))
    print(f"one_over from the lake camera: the fullest sun segment of any launch holds {fullest} records")
    assert fullest <= 256


@pytest.mark.parametrize("case", K.SEGMENT_CASES)
def test_the_lake_fills_path_and_sun_segments_past_256_with_wet_and_dry_lanes(wref, orc, case):
    size = SC.CASES[case].size
    rgb, ids, n, load = _lake(wref, orc, case)
    print(f"{case} {size}: {n.bounce_segments} bounce segments, {n.surface} surface events, {n.sun_rays} sun rays, {n.wet_bounces} wet bounce segments")
    assert (n.bounce_segments, n.surface, n.sun_rays, n.wet_bounces) == WATER_LOADS[case]
    assert np.isfinite(rgb).all() and float(rgb.max()) < 512.0   # (1e-4 is above an ulp)
    # what bounce launch b reads is what launch b - 1 appended; its sun records are its own segment's
    path = [SC.segment_loads((load[0, b] & LOAD_PATH) != 0, *size) for b in range(3)]
    sun = [SC.segment_loads((load[0, b] & LOAD_SUN) != 0, *size) for b in range(4)]
    print(f"    the primary launch appends at most {sun[0].max()} sun rays to a segment ({int((sun[0] > 256).sum())} segments over 256)")
    for b in range(3):
        print(f"    bounce launch {b + 1} reads at most {path[b].max()} paths of a segment ({int((path[b] > 256).sum())} segments over 256, "
              f"{int((path[b] > 512).sum())} over 512); launch {b + 1} appends at most {sun[b + 1].max()} sun rays ({int((sun[b + 1] > 256).sum())} over 256, "
              f"{int((sun[b + 1] > 512).sum())} over 512)")
    assert max(p.max() for p in path) > 256
    assert max(s.max() for s in sun) > 256
    if case == "three_parts":
        assert max(p.max() for p in path) > 512
    if case == "one_over_ragged":
        w, h = SC.CASES["one_over"].size
        assert not load[:, :, h:].any() and not load[:, :, :, w:].any() and not rgb[h:].any() and not rgb[:, w:].any()
    # tiles whose 64 pixels hold both a wet-start and a dry-start live second segment: the primary launch appends a tile's
    # paths next to each other, so the bounce launch's waves carry both kinds of lane
    live = (load[0, 0] & LOAD_PATH) != 0
    wet = live & ((load[0, 1] & LOAD_WET) != 0)
    dry = live & ((load[0, 1] & LOAD_WET) == 0)
    tx, ty = size[0] // 8, size[1] // 8
    per_tile = lambda p: p[:ty * 8, :tx * 8].reshape(ty, 8, tx, 8).any(axis=(1, 3))   # noqa: E731
    mixed = int((per_tile(wet) & per_tile(dry)).sum())
    print(f"    {int(wet.sum())} wet-start and {int(dry.sum())} dry-start second segments; {mixed} tiles hold both")
    assert mixed >= 100
