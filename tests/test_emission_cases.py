"""The cases of tests/emission_cases.py hold what they claim: counted on the reference alone (tests/emission_ref.py and the plain
oracle), without a GPU.  Each claim has a floor of 50 pixels, as tests/test_emission_ref.py uses, and prints its count.

Also here: what the reference says about tables that should change nothing (liquids, air, -0.0)."""
import numpy as np
import pytest

import emission_cases as E
import emission_ref
import step_limit_scenes as L
from voxelraytracing_amd import MODE_PATH

FLOOR = 50
SIZE = (128, 72)
SEED = E.SEED


@pytest.fixture(scope="module")
def eref(tmp_path_factory):
    return emission_ref.load(tmp_path_factory.mktemp("emission_ref"))


@pytest.fixture(scope="module")
def step_world():
    return L.build_world()


def _plain(orc, sc, spp=1, seed=SEED):
    rgb, ids, _, _ = orc.from_package_scene(sc).render(orc.MODE_PATH, *sc.size, spp=spp, seed=seed)
    return rgb, ids


def _ref(eref, orc, sc, table, spp=1, seed=SEED):
    return eref.render(orc.from_package_scene(sc), table, *sc.size, spp=spp, seed=seed)


def _differs(a, b):
    """Pixels where two frames differ in any channel, bit for bit."""
    return (a.view(np.uint32) != b.view(np.uint32)).any(axis=2)


def _entry_of_primary(ids, table):
    """The table entry of each pixel's primary hit (0 where the primary ray missed)."""
    hit = (ids & E.ID_HIT) != 0
    return np.where(hit, table[np.minimum(ids & E.ID_VOXEL_MASK, 255)], np.float32(0.0))


def _later_segment_light(ref_rgb, plain_rgb, ids, table):
    """Pixels whose light changes through a later segment: the emissive reference differs from the plain oracle and the
    primary hit's entry is 0."""
    return int((_differs(ref_rgb, plain_rgb) & (_entry_of_primary(ids, table) == 0)).sum())


def _last_segment_light(eref, orc, make, table, bounces, spp=1):
    """Pixels whose light changes through the last segment.  A path of b - 1 bounces is a path of b cut short (the same
    random numbers), and a segment either hits (an emission term) or misses (the sky's): where the plain frames of b and
    b - 1 bounces are equal no sample's last segment saw the sky, so a difference between the emissive references is the last
    segment's emission."""
    sc_b, sc_a = make(bounces), make(bounces - 1)
    ref_b, _ = _ref(eref, orc, sc_b, table, spp)
    ref_a, _ = _ref(eref, orc, sc_a, table, spp)
    plain_b, _ = _plain(orc, sc_b, spp)
    plain_a, _ = _plain(orc, sc_a, spp)
    return int((_differs(ref_b, ref_a) & ~_differs(plain_b, plain_a)).sum())


def _report(what, n, floor=FLOOR):
    print(f"{what}: {n} (floor {floor})")
    assert n >= floor, f"{what}: {n} is below the floor of {floor}"


@pytest.mark.parametrize("bounces", [2, 3, 4])
@pytest.mark.parametrize("spp", [1, 3])
def test_c4_has_later_and_last_segment_light(eref, orc, bounces, spp):
    sc = E.c4(SIZE, bounces)
    plain, ids = _plain(orc, sc, spp)
    table = E.two_common(ids)
    ref, r_ids = _ref(eref, orc, sc, table, spp)
    assert np.array_equal(r_ids, ids)
    _report(f"C4 {SIZE} b{bounces} spp {spp}: later-segment light", _later_segment_light(ref, plain, ids, table))
    _report(f"C4 {SIZE} b{bounces} spp {spp}: last-segment light",
            _last_segment_light(eref, orc, lambda b: E.c4(SIZE, b), table, bounces, spp))


def test_c4_at_one_and_no_bounces(eref, orc):
    """1 bounce: emissive primary hits, other hits (black), sky.  0 bounces: nothing is traced, the frame is zero."""
    sc = E.c4(SIZE, 1)
    plain, ids = _plain(orc, sc)
    table = E.two_common(ids)
    ref, _ = _ref(eref, orc, sc, table)
    entry = _entry_of_primary(ids, table)
    hit = (ids & E.ID_HIT) != 0
    _report("C4 b1: emissive primary hits", int((entry != 0).sum()))
    _report("C4 b1: other hits", int((hit & (entry == 0)).sum()))
    _report("C4 b1: sky pixels", int((~hit).sum()))
    assert (ref[entry != 0] > 0).any(axis=1).all() and not ref[hit & (entry == 0)].any()
    sc0 = E.c4(SIZE, 0)
    ref0, ids0 = _ref(eref, orc, sc0, table, spp=3)
    assert not ref0.any() and not ids0.any()


@pytest.mark.parametrize("kind", E.MATERIAL_KINDS)
@pytest.mark.parametrize("bounces", [2, 4])
def test_material_scenes_have_later_and_last_segment_light(eref, orc, kind, bounces):
    _, ids = _plain(orc, E.c4(SIZE, 1))
    table, emitter = E.mirror_emitter(ids)
    make = lambda b: E.material_scene(kind, SIZE, emitter, b)   # noqa: E731
    sc = make(bounces)
    plain, ids = _plain(orc, sc, 3)
    ref, _ = _ref(eref, orc, sc, table, 3)
    _report(f"{kind} b{bounces}: later-segment light", _later_segment_light(ref, plain, ids, table))
    _report(f"{kind} b{bounces}: last-segment light", _last_segment_light(eref, orc, make, table, bounces, 3))
    if kind != "all mirrors":   # (the scene is not the diffuse C4 under another name, nor the all-mirror one)
        assert _differs(plain, _plain(orc, E.c4(SIZE, bounces), 3)[0]).sum() >= FLOOR
        assert _differs(plain, _plain(orc, E.c4_all_mirrors(SIZE, bounces), 3)[0]).sum() >= FLOOR


def test_high_id_world_shows_ids_above_255(eref, orc):
    sc = E.c4_high_ids(SIZE, 4)
    plain, ids = _plain(orc, sc, 3)
    hit = (ids & E.ID_HIT) != 0
    vox = ids & E.ID_VOXEL_MASK
    for v in E.HIGH_IDS:
        _report(f"high ids: pixels whose primary hit is voxel {v:#x}", int((hit & (vox == v)).sum()))
    table = E.entry_255_only()
    ref, r_ids = _ref(eref, orc, sc, table, 3)
    assert np.array_equal(r_ids, ids)
    high = hit & (vox > 255)
    assert _differs(ref, plain)[high].all(), "a pixel that sees an id above 255 does not get entry 255's light"
    _report("high ids: later-segment light from entry 255", _later_segment_light(ref, plain, ids, table))
    _report("high ids: last-segment light from entry 255", _last_segment_light(eref, orc, lambda b: E.c4_high_ids(SIZE, b), table, 4, 3))
    # entry 255 alone lights nothing in the world without such voxels
    c4 = E.c4(SIZE, 4)
    E.assert_bit_identical(_ref(eref, orc, c4, table, 3), _plain(orc, c4, 3), "entry 255 on plain C4")


def test_c5_small_has_later_and_last_segment_light(eref, orc):
    sc = E.c5_small()
    assert sc.world.size_in_chunks() == 32
    plain, ids = _plain(orc, sc, 3)
    table = E.two_common(ids)
    ref, _ = _ref(eref, orc, sc, table, 3)
    _report("C5 32^3 b4: later-segment light", _later_segment_light(ref, plain, ids, table))
    for b in (2, 4):
        _report(f"C5 32^3 b{b}: last-segment light", _last_segment_light(eref, orc, lambda n: E.c5_small(bounces=n), table, b, 3))


def _exhaustion_counts(orc, sc, emissive):
    """Pixels of a 1-spp step-limit frame (seed 3, as tests/test_gpu_step_limit.py) with a segment that ran out of lookups
    (500 of them, no solid voxel) and a hit on an `emissive` voxel: -> (that hit follows the segment, it precedes it, it IS the
    segment: the ray ran out on an emissive voxel)."""
    w, h = sc.size
    o = orc.from_package_scene(sc)
    after = before = on = 0
    for py in range(h - h % 8):
        for px in range(w - w % 8):
            segs = o.trace_segments(MODE_PATH, px, py, w, h, 0, 3)
            out = [k for k, s in enumerate(segs) if s["steps"] == 500 and not s["solid"]]
            if not out:
                continue
            lit = [k for k, s in enumerate(segs) if s["hit"] and s["voxel"] in emissive]
            after += any(k > out[0] for k in lit)
            before += any(k < out[-1] and k not in out for k in lit)
            on += any(k in out for k in lit)
    return after, before, on


@pytest.mark.parametrize("bounces", [2, 3, 4])
def test_step_limit_frames_mix_exhausted_segments_and_emissive_hits(eref, orc, step_world, bounces):
    """With limestone emissive: an emissive hit before a segment that runs out (the camera's rays land on the limestone, then
    climb through the water lattice).  A ray that runs out in the water ends on a water voxel, which ray_world reports as a hit:
    the reference adds water's entry there — a liquid's entry is not always dead (see
    test_liquid_and_air_entries_change_nothing_above_water) — and the path goes on from it with water's colour in its
    throughput.  The issue asks for an emissive hit that follows OR precedes; in these frames the segment after one that ran out
    leaves the world, so none follows (the count is printed, without a floor)."""
    after = before = on_water = 0
    for sc in E.step_limit_scenes(step_world, bounces):
        if sc.size == L.BIG:
            _, b, _ = _exhaustion_counts(orc, sc, (E.LIMESTONE,))
            a, _, w = _exhaustion_counts(orc, sc, (E.LIMESTONE, E.WATER))
            after, before, on_water = after + a, before + b, on_water + w
            plain, ids = _plain(orc, sc, 1, 3)
            for table in (E.step_limit_table(), E.step_limit_table_with_water()):
                ref, _ = _ref(eref, orc, sc, table, 1, 3)
                assert _differs(ref, plain).sum() >= FLOOR
    _report(f"step limit b{bounces}: pixels with an emissive hit before a segment that ran out", before)
    _report(f"step limit b{bounces}: pixels that ran out on a water voxel", on_water)
    print(f"step limit b{bounces}: pixels with an emissive hit (limestone or water) after a segment that ran out: {after} (no floor)")


def test_liquid_entries_light_rays_that_run_out_in_water(eref, orc, step_world):
    n = 0
    for sc in E.step_limit_scenes(step_world, 3):
        if sc.size == L.BIG:
            n += int(_differs(_ref(eref, orc, sc, E.liquid_only(), 1, 3)[0], _plain(orc, sc, 1, 3)[0]).sum())
    _report("step limit b3: pixels that liquid_only changes", n)


def test_huge_frames_overflow_in_places(eref, orc):
    """FLT_MAX on a common material (grass: its largest colour channel is 0.45, so a sample's own terms stay finite): +inf
    texels, where a pixel's samples add up beyond FLT_MAX, next to finite emissive ones, and no NaN or -inf anywhere (no
    inf - inf, no 0 * inf in the reference).  A 1-spp frame holds no +inf at all, and must hold none on the GPU."""
    for bounces, spp in ((2, 3), (4, 1), (4, 3), (4, 6), (2, 8)):
        sc = E.c4(SIZE, bounces)
        plain, ids = _plain(orc, sc, spp)
        table, emitter = E.huge(ids)
        ref, _ = _ref(eref, orc, sc, table, spp)
        inf = np.isposinf(ref).any(axis=2)
        finite_emissive = np.isfinite(ref).all(axis=2) & (ref > 1e30).any(axis=2)
        _report(f"huge b{bounces} spp {spp}: +inf texels", int(inf.sum()), FLOOR if spp > 1 else 0)
        _report(f"huge b{bounces} spp {spp}: finite emissive texels", int(finite_emissive.sum()))
        assert not np.isnan(ref).any() and not np.isneginf(ref).any()


def test_denormal_entry_is_not_zero(eref, orc):
    """1 bounce, 1e-40 on a common material: its pixels are exactly mc * e, denormal and not zero."""
    sc = E.c4(SIZE, 1)
    _, ids = _plain(orc, sc)
    table, emitter = E.denormal(ids)
    ref, _ = _ref(eref, orc, sc, table)
    on = ((ids & E.ID_HIT) != 0) & ((ids & E.ID_VOXEL_MASK) == emitter)
    _report("denormal: emissive primary hits", int(on.sum()))
    px = ref[on]
    assert (px > 0).any(axis=1).all() and (px < np.finfo(np.float32).tiny).all()
    shades = np.array([1.0, 0.5, 0.7, 0.2], np.float32)   # a face's shading (ray_tracer.wgsl:296-314): none, x, z, the underside
    c = np.array(sc.materials[emitter].color[:3], np.float32)
    want = {(c * s * table[emitter]).astype(np.float32).tobytes() for s in shades}
    assert {p.tobytes() for p in px} <= want


@pytest.mark.parametrize("spp", [1, 3])
def test_liquid_and_air_entries_change_nothing_above_water(eref, orc, spp):
    """C4's camera looks over water (pixels with the water flag): a ray passes through a liquid and through air, it never hits
    them, so their entries are dead and the frame is the plain oracle's bit for bit.  (Not so for a ray that runs out of
    lookups inside water: test_liquid_entries_light_rays_that_run_out_in_water.)"""
    for make in (E.c4, E.c4_all_mirrors):
        sc = make(SIZE, 4)
        plain = _plain(orc, sc, spp)
        assert ((plain[1] & (1 << 20)) != 0).sum() >= FLOOR, "no water in view"   # (VRT_ID_WATER)
        for name, table in (("liquid_only", E.liquid_only()), ("air_only", E.air_only()), ("minus_zero_only", E.minus_zero_only())):
            E.assert_bit_identical(_ref(eref, orc, sc, table, spp), plain, f"{name} spp {spp}")


def test_air_entry_adds_nothing_where_rays_run_out_in_air(eref, orc, step_world):
    """A ray that runs out in air reports a hit on voxel 0, whose colour is black: (0 * e) * thr = +0 joins the light, which
    is the plain frame's value bit for bit."""
    for sc in E.step_limit_scenes(step_world, 3):
        if sc.size != L.BIG:
            E.assert_bit_identical(_ref(eref, orc, sc, E.air_only(), 1, 3), _plain(orc, sc, 1, 3), sc.name)


def test_minus_zero_is_zero_on_every_case_world(eref, orc, step_world):
    for sc in [E.c4_high_ids(SIZE, 4), E.c5_small((64, 40))] + [s for s in E.step_limit_scenes(step_world, 3) if s.size != L.BIG]:
        seed = 3 if sc.name.startswith("step limit") else SEED
        E.assert_bit_identical(_ref(eref, orc, sc, E.minus_zero_only(), 1, seed), _plain(orc, sc, 1, seed), sc.name)


def test_lone_wave_scenes_are_lit(eref, orc):
    """The small frames (64 to 512 pixels) cannot hold 50 pixels of each kind apiece; over all cameras and sizes they do."""
    worlds = E.lone_wave_worlds()
    changed = later = 0
    for size in E.LONE_SIZES:
        for cam in E.LONE_CAMERAS:
            sc = E.lone_wave_scene(worlds, cam, size, 4)
            plain, ids = _plain(orc, sc, 1, 3)
            if not ((ids & E.ID_HIT) != 0).any():
                continue
            table = E.every_solid()
            ref, _ = _ref(eref, orc, sc, table, 1, 3)
            changed += int(_differs(ref, plain).sum())
            later += _later_segment_light(ref, plain, ids, table)
    _report("lone waves: pixels the table changes", changed)
    print(f"lone waves: pixels lit through a later segment alone: {later} (every hit emits: only a primary miss could count)")


def test_the_comparison_notices_what_it_should():
    """assert_emissive_parity on made-up frames: moved or extra non-finite values, an error beyond the scaled bound."""
    ids = np.zeros((8, 8), np.uint32)
    ref = np.ones((8, 8, 3), np.float32)
    ref[0, 0, 0], ref[1, 1, 1], ref[2, 2, 2] = np.inf, 1e30, 100.0
    E.assert_emissive_parity(ref.copy(), ids, ref, ids)
    ok = ref.copy()
    ok[1, 1, 1], ok[2, 2, 2], ok[3, 3, 0] = np.float32(1e30) * np.float32(1 + 5e-5), 100.009, 1.00009
    E.assert_emissive_parity(ok, ids, ref, ids)
    for y, x, c, v in ((0, 0, 0, 1.0), (0, 0, 0, -np.inf), (0, 0, 0, np.nan), (4, 4, 0, np.inf), (4, 4, 0, np.nan), (4, 4, 0, -np.inf),
                       (3, 3, 0, 1.00011), (2, 2, 2, 100.011), (1, 1, 1, 1.0002e30)):
        bad = ref.copy()
        bad[y, x, c] = v
        with pytest.raises(AssertionError):
            E.assert_emissive_parity(bad, ids, ref, ids)
    with pytest.raises(AssertionError):
        E.assert_emissive_parity(ref.copy(), ids + 1, ref, ids)
