"""Lamp light in the path trace (vrt_set_lamp_light, include/vrt.h) on the GPU.

The list: vrt_read_lamps against tests/lamp_ref.py's list from a dense copy of the world — a hand-made world with a lamp in a
split cell, in a size-2 leaf, an 8^3 block, lamps across a chunk border, on the world's border, under a missing chunk and under
water; a world that gives off nothing; a cut-off list; and after a node edit, an emission write and a change of the liquid
set, with one and two frames in flight.

Frames against tests/lamp_ref.py on every route through the kernels — the default, the march cells behind a chunk directory, the
literal march (air flagged liquid) and the counting kernels of a stats frame — at one wave, two waves and a frame that is not
whole tiles; 1, 2 and 4 bounces; 1 and 3 samples; the lamps alone and together with the sun, a second emissive material, a coat,
two pass-through materials and camera sampling: util.assert_frame_parity.  A stats frame's secondary rays and steps are the
reference's counts.  GPU against GPU, bit for bit: strength 0 after strength 1, accumulation, the primary modes, the denoiser's
guide, two shards.  Every test here calls vrt_set_lamp_light."""
import ctypes as C

import numpy as np
import pytest

import emission_cases as E
import lamp_cases as LC
import lamp_ref
import polish_ref
import translucent_ref
from voxelraytracing_amd import MODE_PATH, MODE_PRIMARY, MODE_PRIMARY_SHADOW, VrtError, _ffi, scenes

from util import assert_frame_parity, gpu_for_scene

pytestmark = pytest.mark.gpu

SEED = 11
SUN = 1.0
LAMP = (1.0, 0.01)        # (strength, max_geometry): some geometry factors are clamped, some are not
LENS = (1.0, 0.05, 20.0)
SIZES = [(8, 8), (16, 8), (100, 60)]
BOUNCES = (1, 2, 4)
SPPS = (1, 3)
ENV = ["VRT_MARCH_DIRECT_MAX_S", "VRT_PATH_POOL", "VRT_PATH_CELLS", "VRT_PATH_POOL_K", "VRT_PATH_POOL_REFILL", "VRT_PATH_SAMPLES_PER_CHAIN",
       "VRT_LAMP_CAP"]
HALF = (0.5, (0.9, 0.6, 0.3))             # (chance, colour): passes half of the time, with a tint
ALWAYS = (2.0, (0.25, 0.5, 0.75))         # always passes
COAT_A = (0.5, 0.0, (1.0, 0.9, 0.8))      # (chance, scatter, colour): a mirror half of the time
# (environment, stats, literal)
ROUTES = {"default": ({}, False, False), "directory": ({"VRT_MARCH_DIRECT_MAX_S": "0"}, False, False), "literal": ({}, False, True),
          "stats": ({}, True, False)}


@pytest.fixture(scope="module")
def lref(tmp_path_factory):
    return lamp_ref.load(tmp_path_factory.mktemp("lamp_ref"))


def _gpu(monkeypatch, sc, env=None, **kw):
    """A context for the scene under exactly `env` of the backend's switches (read when the context is created)."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return gpu_for_scene(sc, **kw)


def _frame(gpu, spp, seed=SEED, **kw):
    gpu.render(MODE_PATH, spp=spp, seed=seed, **kw)
    rgb, ids, _ = gpu.read_output()
    return rgb, ids


def _same_list(got, want, what):
    assert got.dtype == _ffi.LAMP_DTYPE
    assert len(got) == len(want), f"{what}: {len(got)} entries, the reference has {len(want)}"
    for name in ("pos", "voxel", "face", "_reserved"):
        assert np.array_equal(got[name], want[name]), f"{what}: {name} differs, first at entry {int(np.argwhere((got[name] != want[name]).reshape(len(got), -1).any(1))[0, 0])}"


# ---- 1. the list ----

def test_the_list_of_the_hand_made_world(lref, orc, monkeypatch):
    world = LC.hand_made_world()
    sc = LC.hand_made_scene(world)
    e = LC.emission(lamp=2.0, ore=1.0)
    want = lref.lamps(orc.from_package_scene(sc), e)
    assert len(want) == 442 + 5
    for route, env in (("direct", {}), ("directory", {"VRT_MARCH_DIRECT_MAX_S": "0"})):
        gpu = _gpu(monkeypatch, sc, env)
        gpu.write_emission(e)
        with pytest.raises(VrtError):
            gpu.lamp_info()   # VRT_ERR_STATE before the first lamp-lit frame
        _frame(gpu, 1)
        with pytest.raises(VrtError):
            gpu.read_lamps()  # (a frame with the setting off builds nothing)
        gpu.set_lamp_light(1.0)
        _frame(gpu, 1)
        _same_list(gpu.read_lamps(), want, route)
        info = gpu.lamp_info()
        print(f"{route}: {info}")
        assert info["listed"] == len(want) and info["faces"] == len(want) and info["cap"] == 1 << 20 and info["builds"] == 1
        assert info["last_build_ms"] > 0.0
        _frame(gpu, 3)   # nothing changed: no rebuild (one frame in flight here: the same frame set)
        gpu.close()


def test_a_world_that_gives_off_nothing_has_an_empty_list_and_the_off_frame(lref, orc, monkeypatch):
    world = LC.hand_made_world()
    sc = LC.hand_made_scene(world, size=(16, 8))
    gpu = _gpu(monkeypatch, sc)
    want = {spp: _frame(gpu, spp) for spp in SPPS}
    gpu.set_lamp_light(1.0)
    for spp in SPPS:
        rgb, ids = _frame(gpu, spp)
        assert len(gpu.read_lamps()) == 0 and gpu.lamp_info()["faces"] == 0
        # (N = 0: no lamp term; the three draws are still taken, so the paths differ from the off frame's behind their first hit)
        ref_rgb, ref_ids = lref.render(orc.from_package_scene(sc), (1.0, 0.0), np.zeros(0, _ffi.LAMP_DTYPE), *sc.size, spp=spp, seed=SEED)
        assert_frame_parity(rgb, ids, ref_rgb, ref_ids, f"N = 0, spp {spp}")
        assert np.array_equal(ids, want[spp][1])
    gpu.close()


def test_a_cut_off_list_is_the_first_entries_and_counts_them_all(lref, orc, monkeypatch):
    world = LC.hand_made_world()
    sc = LC.hand_made_scene(world, size=(16, 8))
    e = LC.emission(lamp=2.0)
    o = orc.from_package_scene(sc)
    want = lref.lamps(o, e)
    gpu = _gpu(monkeypatch, sc, {"VRT_LAMP_CAP": "5"})
    gpu.write_emission(e)
    gpu.set_lamp_light(*LAMP)
    rgb, ids = _frame(gpu, 3)
    _same_list(gpu.read_lamps(), want[:5], "VRT_LAMP_CAP=5")
    info = gpu.lamp_info()
    assert info["listed"] == 5 and info["cap"] == 5 and info["faces"] == len(want) == 442
    ref_rgb, ref_ids = lref.render(o, LAMP, want[:5], *sc.size, spp=3, seed=SEED, emission=e)
    assert_frame_parity(rgb, ids, ref_rgb, ref_ids, "VRT_LAMP_CAP=5")
    gpu.close()


@pytest.mark.parametrize("in_flight", [1, 2])
def test_the_list_follows_edits_emission_writes_and_the_liquid_set(lref, orc, monkeypatch, in_flight):
    world = LC.hand_made_world()
    sc = LC.hand_made_scene(world, size=(16, 8))
    e = LC.emission(lamp=2.0)
    gpu = _gpu(monkeypatch, sc)
    gpu.write_emission(e)
    gpu.set_frames_in_flight(in_flight)
    gpu.set_lamp_light(*LAMP)

    def check(what, frames=2):
        o = orc.from_package_scene(sc)
        want = lref.lamps(o, e)
        for i in range(frames):   # (two frames in flight: one frame on each frame set, each with a list of its own)
            rgb, ids = _frame(gpu, 1)
            _same_list(gpu.read_lamps(), want, f"{what}, frame {i}")
            ref_rgb, ref_ids = lref.render(o, LAMP, want, *sc.size, spp=1, seed=SEED, emission=e)
            assert_frame_parity(rgb, ids, ref_rgb, ref_ids, f"{what}, frame {i}")
        return len(want), gpu.lamp_info()["builds"]

    n0, b0 = check("as uploaded")
    assert n0 == 442
    _, b1 = check("nothing changed")
    assert b1 == b0   # (no rebuild)
    # a node edit: a new lamp voxel in the air, then the lone lamp taken away
    for pos, voxel in (((20, 20, 6), LC.LAMP), ((5, 6, 5), 0)):
        start, n = world.set_voxel(pos, voxel)
        gpu.write_nodes(world.nodes_ptr(), start, start + n)
        gpu.write_chunk_roots(world.chunk_roots())
        n1, b2 = check(f"set_voxel {pos} {voxel}")
        assert b2 > b1
        b1 = b2
    assert n1 == 442
    # an emission write: the ore gives off light too, then the lamps do no longer
    e = LC.emission(lamp=2.0, ore=1.0)
    gpu.write_emission(e)
    n2, b3 = check("the ore lit")
    assert n2 == n1 + 5 and b3 > b1
    e = LC.emission(ore=1.0)
    gpu.write_emission(e)
    n3, b4 = check("the lamps dark")
    assert n3 == 5 and b4 > b3
    # the liquid set: water solid — the lamp under it has no face left; the lamp material liquid — no lamp at all
    e = LC.emission(lamp=2.0)
    gpu.write_emission(e)
    sc.materials[LC.WATER].is_liquid = 0
    gpu.write_materials(sc.materials)
    n4, b5 = check("water solid")
    assert n4 == 442 - 6 and b5 > b4
    sc.materials[LC.LAMP].is_liquid = 1
    gpu.write_materials(sc.materials)
    n5, _ = check("lamps liquid")
    assert n5 == 0
    gpu.close()


# ---- 2. frames against the reference, route by route ----

def _tables(gpu):
    """From the context's own 1-spp frame (the setting off): the material its primary rays hit most is the lamp; in "all" the
    second passes half of the time with a tint and gives off light too (a lamp seen through a pane still shines), the third
    always passes, the fourth has coat A (as many of them as the frame hits)."""
    gpu.render(MODE_PATH, spp=1, seed=SEED)
    _, ids, _ = gpu.read_output(rgb=False)
    counts = E.hit_counts(ids)
    top = [int(t) for t in np.argsort(counts)[::-1][:4] if counts[t] > 0]
    assert len(top) >= 1
    alone = np.zeros(256, np.float32)
    alone[top[0]] = 1.5
    emission = alone.copy()
    tr = translucent_ref.table()
    polish = polish_ref.table()
    if len(top) > 1:
        tr = translucent_ref.table({top[1]: HALF})
        emission[top[1]] = 0.75
    if len(top) > 2:
        tr = translucent_ref.table({top[1]: HALF, top[2]: ALWAYS})
    if len(top) > 3:
        polish[top[3]]["chance"], polish[top[3]]["scatter"], polish[top[3]]["color"] = COAT_A
    return (alone, None, None), (emission, polish, tr)


def _write(gpu, tables):
    gpu.write_emission(tables[0])
    gpu.write_polish(tables[1] if tables[1] is not None else polish_ref.table())
    gpu.write_translucency(tables[2] if tables[2] is not None else translucent_ref.table())


_refs, _lists = {}, {}


def _list(lref, orc, sc, literal, emission):
    k = (literal, emission.tobytes())
    if k not in _lists:
        _lists[k] = lref.lamps(orc.from_package_scene(sc), emission)
    return _lists[k]


def _ref(lref, orc, key, sc, literal, tables, spp, sun, setting, lamp=LAMP, seed=SEED):
    """(rgb, ids, counts) of the reference frame, computed once; `key` names the scene (its world, materials, camera, bounces, size)."""
    k = (key, tuple(None if t is None else t.tobytes() for t in tables), spp, sun, setting, lamp, seed)
    if k not in _refs:
        lamps = _list(lref, orc, sc, literal, tables[0])
        rgb, ids = lref.render(orc.from_package_scene(sc), lamp, lamps, *sc.size, spp=spp, seed=seed, sun=sun, setting=setting, emission=tables[0],
                               polish=tables[1], translucency=tables[2])
        _refs[k] = (rgb, ids, lref.counts)
    return _refs[k]


def _scene(size, bounces=4, literal=False):
    sc = scenes.c4(size, bounces=bounces)
    if literal:
        sc.materials[0].is_liquid = 1
    return sc


@pytest.mark.parametrize("bounces", BOUNCES)
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_lamp_lit_frames_match_the_reference(lref, orc, monkeypatch, route, size, bounces):
    env, stats, literal = ROUTES[route]
    sc = _scene(size, bounces, literal)
    gpu = _gpu(monkeypatch, sc, env)
    if route == "directory":
        gpu.render(MODE_PATH, spp=1, seed=SEED)
        assert gpu.read_march_cells()[1] == False, "the context's march cells are in the direct layout"   # noqa: E712
    key = f"c4 {size} b{bounces} literal {literal}"
    alone, everything = _tables(gpu)
    gpu.set_lamp_light(*LAMP)
    worst = 0.0
    for kind, tables, sun, setting in (("alone", alone, 0.0, lamp_ref.OFF), ("all", everything, SUN, LENS)):
        _write(gpu, tables)
        gpu.set_sun_light(sun)
        gpu.set_camera_sampling(*setting)
        for spp in SPPS:
            what = f"{size} b{bounces} {route} {kind}, spp {spp}"
            rgb, ids = _frame(gpu, spp, stats=stats)
            ref_rgb, ref_ids, counts = _ref(lref, orc, key, sc, literal, tables, spp, sun, setting)
            # (where 1e-4 is above an ulp: the reference's radiance stays below 512)
            worst = max(worst, float(ref_rgb.max()))
            assert float(ref_rgb.max()) < 512.0, what
            err = np.abs(rgb - ref_rgb)
            print(f"{what}: max radiance {float(ref_rgb.max()):.4g}, max error {float(err[np.isfinite(err)].max()):.3g}; {counts}")
            assert_frame_parity(rgb, ids, ref_rgb, ref_ids, what)
            if stats:
                st = gpu.stats()
                print(f"    secondary_rays {st.secondary_rays} steps {st.steps}")
                assert st.secondary_rays == counts.bounce_segments + counts.sun_rays + counts.lamp_rays, what
                assert st.steps == counts.steps, what
    # (the setting is not a no-op here: lamp rays are marched, and on the frame of several workgroups some arrive and some do not)
    _, _, counts = _ref(lref, orc, key, sc, literal, alone, 3, 0.0, lamp_ref.OFF)
    if size[0] >= 100:
        assert 1 <= counts.unoccluded < counts.lamp_rays
        if bounces > 1:
            assert counts.emission_dropped >= 1
    gpu.close()


# ---- 3. GPU against GPU, bit for bit ----

def _all_modes(gpu):
    out = {("path", spp): _frame(gpu, spp) for spp in (1, 3)}
    out[("path stats", 3)] = _frame(gpu, 3, stats=True)
    for name, mode in (("primary", MODE_PRIMARY), ("primary+shadow", MODE_PRIMARY_SHADOW)):
        gpu.render(mode)
        out[(name, 1)] = gpu.read_output()[:2]
    return out


def test_strength_0_after_strength_1_gives_the_frame_from_before(monkeypatch):
    sc = _scene(SIZES[2])
    gpu = _gpu(monkeypatch, sc)
    _write(gpu, _tables(gpu)[1])
    gpu.set_sun_light(SUN)
    want = _all_modes(gpu)
    gpu.set_lamp_light(*LAMP)
    assert not np.array_equal(_frame(gpu, 3)[0], want[("path", 3)][0])
    for name, off in (("strength 0", lambda: gpu.set_lamp_light(0.0, 0.5)), ("strength -0", lambda: gpu.set_lamp_light(-0.0)),
                      ("NULL", lambda: gpu._ck(gpu._lib.vrt_set_lamp_light(gpu._h, None)))):
        gpu.set_lamp_light(*LAMP)
        off()
        for n in (1, 2):
            gpu.set_frames_in_flight(n)
            got = _all_modes(gpu)
            for k in want:
                E.assert_bit_identical(got[k], want[k], f"{name}, {n} in flight: {k}")
    gpu.close()


def test_the_primary_modes_ignore_the_setting(monkeypatch):
    sc = _scene(SIZES[2])
    gpu = _gpu(monkeypatch, sc)
    gpu.write_emission(_tables(gpu)[0][0])
    want = {}
    for mode in (MODE_PRIMARY, MODE_PRIMARY_SHADOW):
        gpu.render(mode)
        want[mode] = gpu.read_output()[:2]
    gpu.set_lamp_light(*LAMP)
    for n in (1, 2):
        gpu.set_frames_in_flight(n)
        for mode in (MODE_PRIMARY, MODE_PRIMARY_SHADOW):
            gpu.render(mode)
            E.assert_bit_identical(gpu.read_output()[:2], want[mode], f"mode {mode}, {n} in flight")
    gpu.close()


def _set_raw(gpu, strength, max_geometry=0.0, flags=0, reserved=0):
    o = _ffi.LampLight(strength, max_geometry, flags, reserved)
    return gpu._lib.vrt_set_lamp_light(gpu._h, C.byref(o))


BAD = ((-0.5, 0.0, 0, 0), (float("nan"), 0.0, 0, 0), (float("inf"), 0.0, 0, 0), (2.0, -1.0, 0, 0), (2.0, float("nan"), 0, 0),
       (2.0, float("inf"), 0, 0), (2.0, 0.0, 1, 0), (2.0, 0.0, 0, 1))


@pytest.mark.parametrize("in_flight", [1, 2])
def test_accumulated_lamp_lit_frames_are_one_frame_of_all_their_samples(monkeypatch, in_flight):
    sc = _scene(SIZES[2])
    gpu = _gpu(monkeypatch, sc)
    _write(gpu, _tables(gpu)[1])
    gpu.set_lamp_light(*LAMP)
    gpu.set_frames_in_flight(in_flight)
    want = {n: _frame(gpu, n) for n in (3, 6, 12)}
    for _ in range(4):
        gpu.render(MODE_PATH, spp=3, seed=SEED, accumulate=True)
    rgb, ids, _ = gpu.read_output()
    E.assert_bit_identical((rgb, ids), want[12], f"{in_flight} in flight: 4 x 3 spp")
    assert gpu.accumulation() == (12, SEED)
    # an identical call does not restart the sum, nor does a refused one; a call that changes the setting does
    gpu.set_lamp_light(*LAMP)
    for bad in BAD:
        assert _set_raw(gpu, *bad) == _ffi.VRT_ERR_INVALID_ARG, bad
    assert gpu.accumulation() == (12, SEED)
    gpu.reset_accumulation()
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), want[3], "a refused call changed nothing")
    gpu.set_lamp_light(*LAMP)
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), want[6], "after an identical call: the sum goes on")
    assert gpu.accumulation() == (6, SEED)
    gpu.set_lamp_light(LAMP[0], 0.5)
    gpu.set_lamp_light(*LAMP)
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), want[3], "after the setting changed: the sum starts again")
    assert gpu.accumulation() == (3, SEED)
    # off on a context that is off already — strength 0, -0 or NULL — does not restart the sum; turning it off does
    gpu.set_lamp_light(0.0)
    off = {n: _frame(gpu, n) for n in (3, 6)}
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), off[3], "off: the sum started again")
    gpu.set_lamp_light(0.0, 0.25)
    gpu.set_lamp_light(-0.0)
    gpu._ck(gpu._lib.vrt_set_lamp_light(gpu._h, None))
    assert gpu.accumulation() == (3, SEED)
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), off[6], "off again, three ways: the sum goes on")
    gpu.close()


def test_the_denoisers_guide_is_unchanged(monkeypatch):
    sc = _scene(SIZES[2])
    gpu = _gpu(monkeypatch, sc)
    gpu.write_emission(_tables(gpu)[0][0])
    gpu.set_denoise(3, 0.0)
    before = _frame(gpu, 1)
    guide_before = gpu.read_guide()
    gpu.set_denoise(0)
    gpu.set_lamp_light(*LAMP)
    for spp in (1, 3):
        raw = _frame(gpu, spp)
        gpu.set_denoise(3, 0.0)
        got = _frame(gpu, spp)
        guide = gpu.read_guide()
        gpu.set_denoise(0)
        assert np.array_equal(guide, guide_before) and np.array_equal(got[1], raw[1]) and np.array_equal(got[1], before[1])
        E.assert_bit_identical((got[0], got[1]), (_ffi.denoise(raw[0], raw[1], guide, 3, 0.0), raw[1]), f"spp {spp}: the filter over the raw frame")
        assert not np.array_equal(got[0], raw[0])
    gpu.close()


def test_the_union_of_two_shards_is_the_whole_frame(monkeypatch):
    sc = scenes.c4((160, 96))
    whole = _gpu(monkeypatch, sc)
    tables = _tables(whole)[1]
    _write(whole, tables)
    whole.set_lamp_light(*LAMP)
    want = _frame(whole, 3)
    want_list = whole.read_lamps()
    whole.close()
    sum_rgb, all_ids = np.zeros_like(want[0]), np.zeros_like(want[1])
    for r in range(2):
        sh = _gpu(monkeypatch, sc, shard_rank=r, shard_count=2)
        _write(sh, tables)
        sh.set_lamp_light(*LAMP)   # (a shard's context keeps its own setting, and builds its own list)
        rgb, ids = _frame(sh, 3)
        _same_list(sh.read_lamps(), want_list, f"shard {r}")
        sum_rgb += rgb
        all_ids |= ids
        sh.close()
    E.assert_bit_identical((sum_rgb, all_ids), want, "the union of two shards")
    grp = _gpu(monkeypatch, sc, devices=[0, 0], texel_messages=True)
    _write(grp, tables)
    grp.set_lamp_light(*LAMP)   # (replicated to every device)
    E.assert_bit_identical(_frame(grp, 3), want, "two devices with texel messages")
    _same_list(grp.read_lamps(), want_list, "the group's root")
    grp.close()


# ---- 4. refusals ----

def test_refusals(monkeypatch):
    sc = _scene(SIZES[1])
    gpu = _gpu(monkeypatch, sc)
    gpu.write_emission(_tables(gpu)[0][0])
    gpu.set_lamp_light(0.5, 0.25)
    half = _frame(gpu, 3)
    for bad in BAD:
        assert _set_raw(gpu, *bad) == _ffi.VRT_ERR_INVALID_ARG, bad
    E.assert_bit_identical(_frame(gpu, 3), half, "after refused calls: the setting is what it was")
    assert gpu._lib.vrt_set_lamp_light(None, None) == _ffi.VRT_ERR_INVALID_ARG
    gpu.close()
    # a world that keeps no derived tables: a lamp-lit path frame is refused; every other frame is what it was
    monkeypatch.setenv("VRT_ACCEL_MAX_S", "4")
    small = _gpu(monkeypatch, sc)
    monkeypatch.delenv("VRT_ACCEL_MAX_S")
    small.write_emission(_tables(small)[0][0])
    want = _frame(small, 1)
    small.set_lamp_light(*LAMP)
    assert small._lib.vrt_render(small._h, C.byref(_ffi.RenderOpts(mode=MODE_PATH, spp=1, seed=SEED))) == _ffi.VRT_ERR_STATE
    small.render(MODE_PRIMARY)
    small.set_lamp_light(0.0)
    E.assert_bit_identical(_frame(small, 1), want, "the setting off again")
    small.close()
