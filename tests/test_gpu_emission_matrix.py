"""The emissive path kernels beyond C4's defaults, against tests/emission_ref.py: both layouts of the march cells, every bounce
count, every route and switch of the bounce launch, mirrors and mixed scatter, rays that run out of lookups, lone waves and the
edges of the table.  The cases are tests/emission_cases.py's; tests/test_emission_cases.py counts on the CPU what each holds.

Which instantiation a test runs (the host's choice, vrt_path.hip launch_path_bounce_cells): path_bounce_cells_kernel<true, 4, EMIT>
with one frame in flight on a direct world, <true, 5> with two (or VRT_PATH_POOL_K=5), <false, 4> on a world with a chunk directory
(VRT_MARCH_DIRECT_MAX_S=0, C5's 32^3 chunks); path_bounce_kernel<EMIT> for VRT_PATH_POOL=0 / VRT_PATH_CELLS=0, stats frames and
the literal march; path_primary_kernel<EMIT> always.  Every context that has march cells asserts
their layout through read_march_cells (a literal-march context builds none)."""
import numpy as np
import pytest

import emission_cases as E
import emission_ref
import step_limit_scenes as L
from voxelraytracing_amd import MODE_PATH, MODE_PRIMARY, MODE_PRIMARY_SHADOW

from util import gpu_for_scene

pytestmark = pytest.mark.gpu

SEED = E.SEED
SIZE = (128, 72)
SPPS = (1, 3, 8)
ENV = ["VRT_MARCH_DIRECT_MAX_S", "VRT_PATH_POOL", "VRT_PATH_CELLS", "VRT_PATH_POOL_K", "VRT_PATH_POOL_REFILL", "VRT_PATH_SAMPLES_PER_CHAIN"]
DIRECT, DIRECTORY = {}, {"VRT_MARCH_DIRECT_MAX_S": "0"}
LAYOUTS = {"direct": DIRECT, "directory": DIRECTORY}
# route -> (environment, the frame is a stats frame, air is flagged liquid: the literal march)
ROUTES = {"cells": ({}, False, False), "lane": ({"VRT_PATH_POOL": "0"}, False, False), "no cells": ({"VRT_PATH_CELLS": "0"}, False, False),
          "literal": ({}, False, True), "stats": ({}, True, False)}


@pytest.fixture(scope="module")
def eref(tmp_path_factory):
    return emission_ref.load(tmp_path_factory.mktemp("emission_ref"))


@pytest.fixture(scope="module")
def step_world():
    return L.build_world()


@pytest.fixture(scope="module")
def c4_ids(orc):
    """The id words of C4's frame (they do not depend on the bounce count from 1 up): what the tables are chosen from."""
    sc = E.c4(SIZE, 1)
    return orc.from_package_scene(sc).render(orc.MODE_PATH, *SIZE, spp=1, seed=SEED)[1]


def _gpu(monkeypatch, sc, env, direct=None):
    """A context for the scene under exactly `env` of the backend's switches; asserts the layout of its march cells (direct:
    None = the world is small enough for the direct layout and the environment does not switch it off; "none" = the scene flags
    air as a liquid, so its frames take the literal march, which reads no march cells: there are none to have a layout)."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)   # (read when the context is created)
    gpu = gpu_for_scene(sc)
    gpu.render(MODE_PATH, spp=1, seed=SEED)
    if direct == "none":
        return gpu
    if direct is None:
        direct = env.get("VRT_MARCH_DIRECT_MAX_S", "16") != "0"
    assert gpu.read_march_cells()[1] == direct, f"the context's march cells are {'not ' if direct else ''}in the direct layout"
    return gpu


def _frame(gpu, spp, seed=SEED, **kw):
    gpu.render(MODE_PATH, spp=spp, seed=seed, **kw)
    rgb, ids, _ = gpu.read_output()
    return rgb, ids


_refs = {}


def _ref(eref, orc, key, sc, table, spp, seed=SEED):
    """The reference frame; `key` names the scene (its world, materials, camera, bounces and size)."""
    k = (key, table.tobytes(), spp, seed)
    if k not in _refs:
        _refs[k] = eref.render(orc.from_package_scene(sc), table, *sc.size, spp=spp, seed=seed)
    return _refs[k]


def _check(gpu, eref, orc, key, sc, table, what, spps=SPPS, in_flight=(1, 2), seed=SEED, exact_hits=False, **kw):
    """Frames of every sample count with one and two in flight (pool depth 4 and 5 on a direct world) against the reference;
    exact_hits: a 1-bounce scene, whose hit pixels are exactly mc * e at 1 spp (tests/test_emission_ref.py)."""
    for n in in_flight:
        gpu.set_frames_in_flight(n)
        for spp in spps:
            rgb, ids = _frame(gpu, spp, seed, **kw)
            r_rgb, r_ids = _ref(eref, orc, key, sc, table, spp, seed)
            w = f"{what}, {n} in flight, spp {spp}"
            E.assert_emissive_parity(rgb, ids, r_rgb, r_ids, w)
            if exact_hits and spp == 1:
                hit = (r_ids & E.ID_HIT) != 0
                assert np.array_equal(rgb[hit].view(np.uint32), r_rgb[hit].view(np.uint32)), f"{w}: a hit pixel is not exactly mc * e"


# ---- layouts ----

@pytest.mark.parametrize("max_s", [None, "16", "0"])
def test_layouts_of_c4(eref, orc, monkeypatch, c4_ids, max_s):
    sc = E.c4(SIZE, 4)
    table = E.two_common(c4_ids)
    gpu = _gpu(monkeypatch, sc, {} if max_s is None else {"VRT_MARCH_DIRECT_MAX_S": max_s})
    gpu.write_emission(table)
    _check(gpu, eref, orc, "c4 b4", sc, table, f"C4, VRT_MARCH_DIRECT_MAX_S {max_s}")
    gpu.close()


@pytest.mark.parametrize("bounces", [2, 4])
def test_c5_world_has_the_directory_without_a_switch(eref, orc, monkeypatch, bounces):
    sc = E.c5_small(bounces=bounces)
    ids = orc.from_package_scene(sc).render(orc.MODE_PATH, *sc.size, spp=1, seed=SEED)[1]
    table = E.two_common(ids)
    gpu = _gpu(monkeypatch, sc, {}, direct=False)
    gpu.write_emission(table)
    _check(gpu, eref, orc, f"c5 b{bounces}", sc, table, f"C5 32^3 b{bounces}")
    gpu.close()


# ---- bounces x routes ----

@pytest.mark.parametrize("bounces", E.BOUNCES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_every_bounce_count_on_every_route(eref, orc, monkeypatch, c4_ids, route, bounces):
    env, stats, literal = ROUTES[route]
    sc = E.c4(SIZE, bounces)
    if literal:
        sc.materials[0].is_liquid = 1
    table = E.two_common(c4_ids)
    gpu = _gpu(monkeypatch, sc, env, direct="none" if literal else None)
    gpu.write_emission(table)
    _check(gpu, eref, orc, f"c4 b{bounces} literal {literal}", sc, table, f"C4 b{bounces} {route}", stats=stats, exact_hits=bounces == 1)
    if bounces == 0:   # nothing is traced: all zero, and the frame of a context with no table
        with_table = _frame(gpu, 3, stats=stats)
        assert not with_table[0].any() and not with_table[1].any()
        never = _gpu(monkeypatch, sc, env, direct="none" if literal else None)
        E.assert_bit_identical(with_table, _frame(never, 3, stats=stats), f"0 bounces {route}")
        never.close()
    gpu.close()


# ---- switches ----

SWITCHES = [{"VRT_PATH_POOL_K": "4"}, {"VRT_PATH_POOL_K": "5"}, {"VRT_PATH_POOL_REFILL": "4"}, {"VRT_PATH_POOL_REFILL": "48"},   # (default: 16)
            {"VRT_PATH_SAMPLES_PER_CHAIN": "1"}, {"VRT_PATH_SAMPLES_PER_CHAIN": "2"}, {"VRT_PATH_SAMPLES_PER_CHAIN": "16"}]


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("bounces", [2, 4])
@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: "%s=%s" % next(iter(s.items())))
def test_backend_switches(eref, orc, monkeypatch, c4_ids, switch, bounces, layout):
    sc = E.c4(SIZE, bounces)
    table = E.two_common(c4_ids)
    gpu = _gpu(monkeypatch, sc, {**switch, **LAYOUTS[layout]})
    gpu.write_emission(table)
    _check(gpu, eref, orc, f"c4 b{bounces} literal False", sc, table, f"C4 b{bounces} {layout} {switch}")
    gpu.close()


# ---- materials ----

@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("bounces", [2, 4])
@pytest.mark.parametrize("kind", E.MATERIAL_KINDS)
def test_mirrors_and_mixed_scatter(eref, orc, monkeypatch, c4_ids, kind, bounces, layout):
    table, emitter = E.mirror_emitter(c4_ids)
    sc = E.material_scene(kind, SIZE, emitter, bounces)
    gpu = _gpu(monkeypatch, sc, LAYOUTS[layout])
    gpu.write_emission(table)
    _check(gpu, eref, orc, f"{kind} b{bounces}", sc, table, f"{kind} b{bounces} {layout}")
    gpu.close()


def test_mirrors_on_the_lane_route(eref, orc, monkeypatch, c4_ids):
    table, emitter = E.mirror_emitter(c4_ids)
    for kind in E.MATERIAL_KINDS:
        sc = E.material_scene(kind, SIZE, emitter, 4)
        gpu = _gpu(monkeypatch, sc, {"VRT_PATH_POOL": "0"})
        gpu.write_emission(table)
        _check(gpu, eref, orc, f"{kind} b4", sc, table, f"{kind} b4 lane", in_flight=(2,))
        _check(gpu, eref, orc, f"{kind} b4", sc, table, f"{kind} b4 stats", spps=(3,), in_flight=(2,), stats=True)
        gpu.close()


# ---- the step limit ----

@pytest.mark.parametrize("bounces", [2, 3, 4])
@pytest.mark.parametrize("route", ["default", "directory", "lane"])
def test_step_limit_with_a_table(eref, orc, monkeypatch, step_world, route, bounces):
    """Rays that run out of lookups inside the emissive copy of the hand-written loop, limestone emissive and then water too
    (a ray that runs out on a water voxel reports a hit there: the pool kernel reloads that voxel from the brick and reads its
    entry).  The stats frame's per-pixel step counts are the oracle's: the table changes no step count."""
    env = {"default": {}, "directory": DIRECTORY, "lane": {"VRT_PATH_POOL": "0"}}[route]
    for i, sc in enumerate(E.step_limit_scenes(step_world, bounces)):
        r_steps = orc.from_package_scene(sc).render(MODE_PATH, *sc.size, want_steps=True, spp=1, seed=3)[2]
        gpu = _gpu(monkeypatch, sc, env)
        for tname, table in (("limestone", E.step_limit_table()), ("limestone and water", E.step_limit_table_with_water())):
            gpu.write_emission(table)
            what = f"{sc.name} scene {i} b{bounces} {route}, {tname}"
            for n in (1, 2):
                gpu.set_frames_in_flight(n)
                gpu.render(MODE_PATH, spp=1, seed=3, timed=True)
                rgb, ids = _frame(gpu, 1, 3, timed=True)   # (two frames back to back: with two in flight the second overlaps the first)
                E.assert_emissive_parity(rgb, ids, *_ref(eref, orc, f"step {i} b{bounces}", sc, table, 1, 3), f"{what}, {n} in flight")
            rgb, ids = _frame(gpu, 1, 3, stats=True)
            E.assert_emissive_parity(rgb, ids, *_ref(eref, orc, f"step {i} b{bounces}", sc, table, 1, 3), f"{what}, stats")
            assert np.array_equal(gpu.read_steps(), r_steps), f"{what}: step counts"
        if sc.size == L.BIG:
            _check(gpu, eref, orc, f"step {i} b{bounces}", sc, table, what, spps=(3,), seed=3)
        gpu.close()


# ---- lone waves ----

@pytest.mark.parametrize("bounces", [1, 2, 3, 4])
@pytest.mark.parametrize("size", E.LONE_SIZES)
def test_lone_waves_with_a_table(eref, orc, monkeypatch, size, bounces):
    """One tile, eight tiles and a ragged frame on the cameras whose rays tie, every solid emissive: the emissive copy of the
    bounce march with nothing else resident to cover a wave's latency."""
    worlds = E.lone_wave_worlds()
    table = E.every_solid()
    for c, cam in enumerate(E.LONE_CAMERAS):
        sc = E.lone_wave_scene(worlds, cam, size, bounces)
        gpu = _gpu(monkeypatch, sc, {})
        gpu.write_emission(table)
        for n in (1, 2):
            gpu.set_frames_in_flight(n)
            gpu.render(MODE_PATH, spp=1, seed=3, timed=True)
            rgb, ids = _frame(gpu, 1, 3, timed=True)
            r_rgb, r_ids = _ref(eref, orc, f"lone {c} {size} b{bounces}", sc, table, 1, 3)
            E.assert_emissive_parity(rgb, ids, r_rgb, r_ids, f"{sc.name} {size} b{bounces}, {n} in flight")
            if bounces == 1:
                hit = (r_ids & E.ID_HIT) != 0
                assert np.array_equal(rgb[hit].view(np.uint32), r_rgb[hit].view(np.uint32)), f"{sc.name}: a hit pixel is not exactly mc * e"
        _check(gpu, eref, orc, f"lone {c} {size} b{bounces}", sc, table, f"{sc.name} {size} b{bounces}", spps=(3,), seed=3)
        gpu.close()


# ---- the table's edges ----

@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("bounces", [1, 2, 4])
def test_ids_above_255_read_entry_255(eref, orc, monkeypatch, layout, bounces):
    sc = E.c4_high_ids(SIZE, bounces)
    table = E.entry_255_only()
    gpu = _gpu(monkeypatch, sc, LAYOUTS[layout])
    gpu.write_emission(table)
    _check(gpu, eref, orc, f"high ids b{bounces}", sc, table, f"ids above 255, b{bounces} {layout}", exact_hits=bounces == 1)
    _check(gpu, eref, orc, f"high ids b{bounces}", sc, table, f"ids above 255, b{bounces} {layout} stats", spps=(3,), stats=True)
    gpu.close()


def _all_modes(gpu):
    out = {}
    for spp in (1, 3, 8):
        out[("path", spp)] = _frame(gpu, spp)
    out[("path stats", 3)] = _frame(gpu, 3, stats=True)
    for name, mode in (("primary", MODE_PRIMARY), ("primary+shadow", MODE_PRIMARY_SHADOW)):
        gpu.render(mode)
        rgb, ids, _ = gpu.read_output()
        out[(name, 1)] = (rgb, ids)
    return out


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("mirrors", [False, True])
def test_dead_entries_are_no_table(monkeypatch, layout, mirrors):
    """Above water (C4's camera) a liquid's, air's and a -0.0 entry change nothing: every mode's frame is bit for bit that of a
    context that never had a table.  (Where rays run out inside water a liquid's entry does give light:
    test_step_limit_with_a_table.)"""
    sc = (E.c4_all_mirrors if mirrors else E.c4)(SIZE, 4)
    never = _gpu(monkeypatch, sc, LAYOUTS[layout])
    want = _all_modes(never)
    never.close()
    for name, table in (("liquid_only", E.liquid_only()), ("air_only", E.air_only()), ("minus_zero_only", E.minus_zero_only())):
        gpu = _gpu(monkeypatch, sc, LAYOUTS[layout])
        gpu.write_emission(table)
        for n in (1, 2):
            gpu.set_frames_in_flight(n)
            got = _all_modes(gpu)
            for k in want:
                E.assert_bit_identical(got[k], want[k], f"{name} {layout}, {n} in flight: {k}")
        gpu.close()


def test_air_entry_where_rays_run_out_in_air(eref, orc, monkeypatch, step_world):
    """A ray that runs out in air reports a hit on voxel 0, black: its term is +0 and the frame is the plain one's."""
    for i, sc in enumerate(E.step_limit_scenes(step_world, 3)):
        gpu = _gpu(monkeypatch, sc, {})
        want = _frame(gpu, 1, 3)
        gpu.write_emission(E.air_only())
        E.assert_bit_identical(_frame(gpu, 1, 3), want, f"{sc.name} scene {i}")
        E.assert_emissive_parity(*_frame(gpu, 1, 3), *_ref(eref, orc, f"step {i} b3", sc, E.air_only(), 1, 3), f"{sc.name} scene {i}")
        gpu.close()


@pytest.mark.parametrize("route", ["cells", "lane", "stats"])
def test_a_denormal_entry_is_not_zero(eref, orc, monkeypatch, c4_ids, route):
    env, stats, _ = ROUTES[route]
    table, emitter = E.denormal(c4_ids)
    tiny = np.finfo(np.float32).tiny
    for bounces in (1, 4):
        sc = E.c4(SIZE, bounces)
        gpu = _gpu(monkeypatch, sc, env)
        gpu.write_emission(table)
        _check(gpu, eref, orc, f"c4 b{bounces} literal False", sc, table, f"denormal b{bounces} {route}", stats=stats, exact_hits=bounces == 1)
        if bounces == 1:
            rgb, ids = _frame(gpu, 1, stats=stats)
            on = ((ids & E.ID_HIT) != 0) & ((ids & E.ID_VOXEL_MASK) == emitter)
            assert on.sum() > 50 and (rgb[on] > 0).any(axis=1).all() and (rgb[on] < tiny).all(), "the denormal term was flushed"
        gpu.close()


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("bounces", [2, 4])
def test_a_huge_entry_overflows_where_the_reference_does(eref, orc, monkeypatch, c4_ids, bounces, layout):
    """FLT_MAX: identical +inf masks, no NaN (no inf - inf, no 0 * inf), finite pixels within the scaled tolerance — in plain
    frames, on the lane route's stats frame, and in an accumulating run of 1 + 3 + 2 samples against the 6-spp reference."""
    table, _ = E.huge(c4_ids)
    sc = E.c4(SIZE, bounces)
    key = f"c4 b{bounces} literal False"
    gpu = _gpu(monkeypatch, sc, LAYOUTS[layout])
    gpu.write_emission(table)
    _check(gpu, eref, orc, key, sc, table, f"huge b{bounces} {layout}", spps=(1, 3, 6, 8))
    _check(gpu, eref, orc, key, sc, table, f"huge b{bounces} {layout} stats", spps=(3,), stats=True)
    for n in (1, 2):
        gpu.set_frames_in_flight(n)
        gpu.reset_accumulation()
        total = 0
        for spp in (1, 3, 2):
            total += spp
            rgb, ids = _frame(gpu, spp, accumulate=True)
            if total in (1, 6):
                E.assert_emissive_parity(rgb, ids, *_ref(eref, orc, key, sc, table, total), f"huge b{bounces} {layout}: accumulated {total}, {n} in flight")
        assert gpu.accumulation() == (6, SEED)
        assert np.isposinf(rgb).sum() > 50 and not np.isnan(rgb).any()
    gpu.close()


def test_a_huge_entry_with_one_sample_per_chain(eref, orc, monkeypatch, c4_ids):
    table, _ = E.huge(c4_ids)
    sc = E.c4(SIZE, 4)
    gpu = _gpu(monkeypatch, sc, {"VRT_PATH_SAMPLES_PER_CHAIN": "1"})
    gpu.write_emission(table)
    _check(gpu, eref, orc, "c4 b4 literal False", sc, table, "huge, one sample per chain", spps=(3, 8))
    gpu.close()


# ---- accumulation ----

@pytest.mark.parametrize("case", ["directory b4", "directory b2", "direct b2", "direct b1", "c5 b4", "lane b2"])
def test_accumulated_frames_are_one_frame_of_all_their_samples(orc, monkeypatch, c4_ids, case):
    """The existing rule (tests/test_gpu_emission.py), on the kernels that never met it: 1 + 3 + 2 + 2 samples accumulated equal
    one frame of all of them bit for bit, after every step."""
    where, b = case.split(" b")
    if where == "c5":
        sc = E.c5_small(bounces=int(b))
        table = E.two_common(orc.from_package_scene(sc).render(orc.MODE_PATH, *sc.size, spp=1, seed=SEED)[1])
        gpu = _gpu(monkeypatch, sc, {}, direct=False)
    else:
        sc = E.c4((160, 96), int(b))
        table = E.two_common(c4_ids)
        gpu = _gpu(monkeypatch, sc, {"directory": DIRECTORY, "direct": DIRECT, "lane": {"VRT_PATH_POOL": "0"}}[where])
    gpu.write_emission(table)
    for in_flight in (1, 2):
        gpu.set_frames_in_flight(in_flight)
        want = {n: _frame(gpu, n) for n in (1, 4, 6, 8)}
        gpu.reset_accumulation()
        n = 0
        for spp in (1, 3, 2, 2):
            n += spp
            E.assert_bit_identical(_frame(gpu, spp, accumulate=True), want[n], f"{case}, {in_flight} in flight: 1 + 3 + 2 + 2, after {n} samples")
            assert gpu.accumulation() == (n, SEED)
    gpu.close()
