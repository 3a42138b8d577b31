"""Polished materials in the path trace (vrt_write_polish, include/vrt.h) on the GPU.

Against tests/polish_ref.py (the oracle's path loop with path_tracer.wgsl's emission term and its coat) on every route through
the kernels, both layouts of the march cells, every bounce count, one sample per chain, lone waves and the edges of the table;
a table without a chance renders exactly as no table; accumulated polished frames are one frame of all their samples, bit for
bit; what restarts the sum and what is refused; the primary modes; shards and devices.  Frames against the reference:
util.assert_frame_parity (id words equal, radiance within RADIANCE_TOL); GPU against GPU: bit for bit.

Which instantiation a test runs (the host's choice, vrt_path.hip): path_bounce_cells_kernel<true, 4, EMIT, POLISH> with one frame in flight
on a direct world, <true, 5> with two, <false, 4> on a world with a chunk directory (VRT_MARCH_DIRECT_MAX_S=0);
path_bounce_kernel<.., EMIT, POLISH> for VRT_PATH_POOL=0, stats frames and the literal march; path_primary_kernel<.., EMIT, POLISH> always (its
chained form where a frame of several samples has more than one per chain)."""
import numpy as np
import pytest

import emission_cases as E
import polish_ref
import step_limit_scenes as L
from voxelraytracing_amd import MODE_PATH, MODE_PRIMARY, MODE_PRIMARY_SHADOW, VrtError, _ffi, scenes

from util import assert_frame_parity, gpu_for_scene

pytestmark = pytest.mark.gpu

SEED = 11
SIZES = [(128, 72), (100, 60)]
SPPS = (1, 3, 12)
ENV = ["VRT_MARCH_DIRECT_MAX_S", "VRT_PATH_POOL", "VRT_PATH_CELLS", "VRT_PATH_POOL_K", "VRT_PATH_POOL_REFILL", "VRT_PATH_SAMPLES_PER_CHAIN"]
COAT_A = (0.5, 0.0, (1.0, 0.9, 0.8))      # (chance, scatter, colour): a mirror half of the time
COAT_B = (2.0, 0.25, (0.25, 0.5, 0.75))   # always, a little rough
DEAD = (0.5, 0.0, (0.0, 0.0, 0.0))        # entry 255: no voxel of C4 reads it


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return polish_ref.load(tmp_path_factory.mktemp("polish_ref"))


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


def _tables(gpu):
    """(emission, polish) from the context's own 1-spp frame: the material its primary rays hit most has coat A, the second
    coat B, the third gives off light; entry 255 has a chance and no voxel to use it."""
    gpu.render(MODE_PATH, spp=1, seed=SEED)
    _, ids, _ = gpu.read_output(rgb=False)
    top = E.common(ids, 3)
    emission = np.zeros(256, np.float32)
    emission[top[2]] = 1.5
    return emission, polish_ref.table({top[0]: COAT_A, top[1]: COAT_B, 255: DEAD})


def _write(gpu, tables):
    gpu.write_emission(tables[0])
    gpu.write_polish(tables[1])


_refs = {}


def _ref(pref, orc, key, sc, tables, spp, seed=SEED):
    """The reference frame, computed once; `key` names the scene (its world, materials, camera, bounces and size)."""
    emission, polish = tables if tables is not None else (None, None)
    k = (key, None if emission is None else emission.tobytes(), None if polish is None else polish.tobytes(), spp, seed)
    if k not in _refs:
        _refs[k] = pref.render(orc.from_package_scene(sc), emission, polish, *sc.size, spp=spp, seed=seed)
    return _refs[k]


def _check(gpu, pref, orc, key, sc, tables, what, spps=SPPS, in_flight=(1, 2), seed=SEED, **kw):
    for n in in_flight:
        gpu.set_frames_in_flight(n)
        for spp in spps:
            rgb, ids = _frame(gpu, spp, seed, **kw)
            assert_frame_parity(rgb, ids, *_ref(pref, orc, key, sc, tables, spp, seed), f"{what}, {n} in flight, spp {spp}")


def _differ(a, b, by=1e-3):
    """How many pixels of two frames differ by more than `by` in some channel."""
    return int((np.abs(a[0] - b[0]).max(axis=2) > by).sum())


# ---- 1. the routes ----

# the pool kernel over the march cells (plain frames), the lane = path bounce kernel, the literal march (air flagged liquid) and
# the counting kernels of a stats frame
ROUTES = {"cells": ({}, False, False), "lane": ({"VRT_PATH_POOL": "0"}, False, False), "literal": ({}, False, True), "stats": ({}, True, False)}


def _route_scene(size, route, bounces=4):
    sc = scenes.c4(size, bounces=bounces)
    if ROUTES[route][2]:
        sc.materials[0].is_liquid = 1
    return sc


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_polished_frames_match_the_reference(pref, orc, monkeypatch, size, route):
    env, stats, literal = ROUTES[route]
    sc = _route_scene(size, route)
    gpu = _gpu(monkeypatch, sc, env)
    tables = _tables(gpu)
    _write(gpu, tables)
    key = f"c4 {size} b4 literal {literal}"
    _check(gpu, pref, orc, key, sc, tables, f"{size} {route}", stats=stats)
    # (the table is not a no-op here: the reference with it is not the reference without it)
    assert _differ(_ref(pref, orc, key, sc, tables, 3), _ref(pref, orc, key, sc, None, 3)) > 100
    gpu.close()


# ---- 2. the march cells behind a chunk directory ----

@pytest.mark.parametrize("size", SIZES)
def test_the_directory_layout(pref, orc, monkeypatch, size):
    sc = scenes.c4(size)
    gpu = _gpu(monkeypatch, sc, {"VRT_MARCH_DIRECT_MAX_S": "0"})
    tables = _tables(gpu)
    assert gpu.read_march_cells()[1] == False, "the context's march cells are in the direct layout"   # noqa: E712
    _write(gpu, tables)
    _check(gpu, pref, orc, f"c4 {size} b4 literal False", sc, tables, f"{size} directory")
    gpu.close()


# ---- 3. one sample per chain ----

def test_one_sample_per_chain(pref, orc, monkeypatch):
    size = SIZES[0]
    sc = scenes.c4(size)
    gpu = _gpu(monkeypatch, sc, {"VRT_PATH_SAMPLES_PER_CHAIN": "1"})
    tables = _tables(gpu)
    _write(gpu, tables)
    _check(gpu, pref, orc, f"c4 {size} b4 literal False", sc, tables, "one sample per chain")
    gpu.close()


# ---- 4. the bounce counts ----

@pytest.mark.parametrize("bounces", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("route", ["cells", "lane"])
def test_every_bounce_count(pref, orc, monkeypatch, route, bounces):
    size = SIZES[0]
    sc = scenes.c4(size, bounces=bounces)
    gpu = _gpu(monkeypatch, sc, ROUTES[route][0])
    if bounces == 0:   # nothing is traced: no id words to choose a table from
        tables = (E._one(62, 1.5), polish_ref.table({40: COAT_A, 39: COAT_B, 255: DEAD}))
    else:
        tables = _tables(gpu)
    before = {spp: _frame(gpu, spp) for spp in (1, 3)}
    _write(gpu, tables)
    _check(gpu, pref, orc, f"c4 {size} b{bounces} literal False", sc, tables, f"b{bounces} {route}", spps=(1, 3))
    if bounces == 0:
        rgb, ids = _frame(gpu, 3)
        assert not rgb.any() and not ids.any()
    if bounces == 1:   # the path's only segment is its last: nothing drawn is observed, and the emission table is all there is
        gpu.write_emission(np.zeros(256, np.float32))
        for spp in (1, 3):
            E.assert_bit_identical(_frame(gpu, spp), before[spp], f"b1 {route}: spp {spp} with the polish table and without")
    gpu.close()


# ---- 5. a lone wave ----

@pytest.mark.parametrize("size", [(8, 8), (16, 8)])
def test_a_lone_wave(pref, orc, monkeypatch, size):
    """One tile and two: the pool kernel with its pool nearly empty, the smallest shape at which its compaction can go wrong."""
    for bounces in (2, 4):
        sc = scenes.c4(size, bounces=bounces)
        gpu = _gpu(monkeypatch, sc)
        tables = _tables(gpu)
        _write(gpu, tables)
        _check(gpu, pref, orc, f"c4 {size} b{bounces} literal False", sc, tables, f"{size} b{bounces}", in_flight=(1,))
        gpu.close()


# ---- 6. the table's edges ----

def test_ids_above_255_read_entry_255(pref, orc, monkeypatch):
    size = SIZES[0]
    sc = E.c4_high_ids(size)
    gpu = _gpu(monkeypatch, sc)
    emission, polish = _tables(gpu)
    polish[255]["chance"], polish[255]["scatter"], polish[255]["color"] = COAT_B
    _write(gpu, (emission, polish))
    key = f"high ids {size}"
    _check(gpu, pref, orc, key, sc, (emission, polish), "ids above 255")
    _check(gpu, pref, orc, key, sc, (emission, polish), "ids above 255, stats", spps=(3,), stats=True)
    # entry 255 is what those voxels read: without it the pixels that see them are others
    dead = polish.copy()
    dead[255] = 0
    with_, without = _ref(pref, orc, key, sc, (emission, polish), 3), _ref(pref, orc, key, sc, (emission, dead), 3)
    high = ((with_[1] & E.ID_HIT) != 0) & ((with_[1] & E.ID_VOXEL_MASK) > 255)
    assert high.sum() > 300 and (np.abs(with_[0] - without[0]).max(axis=2)[high] > 1e-3).sum() > 100
    gpu.close()


@pytest.fixture(scope="module")
def step_world():
    return L.build_world()


def test_rays_that_run_out_of_lookups(pref, orc, monkeypatch, step_world):
    """Rays that run out on water and in air report a hit there (ray_tracer.wgsl:220, :293): the one way the water's entry and
    entry 0 are read.  Both always bounce off their coat."""
    tables = (np.zeros(256, np.float32), polish_ref.table({L.WATER: COAT_B, 0: (2.0, 0.5, (1.0, 0.9, 0.8))}))
    for i, sc in enumerate(E.step_limit_scenes(step_world, 3)):
        gpu = _gpu(monkeypatch, sc)
        _write(gpu, tables)
        key = f"step {i}"
        _check(gpu, pref, orc, key, sc, tables, f"{sc.name} scene {i}", spps=(1, 3), seed=3)
        _check(gpu, pref, orc, key, sc, tables, f"{sc.name} scene {i}, stats", spps=(1,), in_flight=(1,), seed=3, stats=True)
        if sc.size == L.BIG and i % 2 == 0:   # (the mirror scene: its first bounce climbs through the water and runs out)
            assert _differ(_ref(pref, orc, key, sc, tables, 1, 3), _ref(pref, orc, key, sc, (tables[0], polish_ref.table({255: DEAD})), 1, 3)) > 100
        gpu.close()


def _all_modes(gpu):
    out = {}
    for spp in SPPS:
        out[("path", spp)] = _frame(gpu, spp)
    out[("path stats", 3)] = _frame(gpu, 3, stats=True)
    for name, mode in (("primary", MODE_PRIMARY), ("primary+shadow", MODE_PRIMARY_SHADOW)):
        gpu.render(mode)
        rgb, ids, _ = gpu.read_output()
        out[(name, 1)] = (rgb, ids)
    return out


def test_a_table_without_a_chance_is_no_table(monkeypatch):
    """All zero bytes, and chances of -0.0 under colours and scatters that are not zero, each written over a live context: every
    frame is byte for byte the frame from before — and with a chance written and taken back again."""
    sc = scenes.c4(SIZES[0])
    gpu = _gpu(monkeypatch, sc)
    emission, polish = _tables(gpu)
    gpu.write_emission(emission)
    want = _all_modes(gpu)
    minus_zero = polish_ref.table()
    minus_zero["chance"], minus_zero["scatter"], minus_zero["color"] = -0.0, 0.5, (0.25, 0.5, 0.75)
    for name, table in (("zeros", polish_ref.table()), ("-0.0 chances", minus_zero)):
        gpu.write_polish(table)
        for n in (1, 2):
            gpu.set_frames_in_flight(n)
            got = _all_modes(gpu)
            for k in want:
                E.assert_bit_identical(got[k], want[k], f"{name}, {n} in flight: {k}")
    gpu.write_polish(polish)
    assert not np.array_equal(_frame(gpu, 3)[0], want[("path", 3)][0])
    gpu.write_polish(minus_zero)
    got = _all_modes(gpu)
    for k in want:
        E.assert_bit_identical(got[k], want[k], f"a chance taken back: {k}")
    gpu.close()


# ---- 7. accumulation ----

@pytest.mark.parametrize("in_flight", [1, 2])
def test_accumulated_polished_frames_are_one_frame_of_all_their_samples(monkeypatch, in_flight):
    sc = scenes.c4(SIZES[1])
    gpu = _gpu(monkeypatch, sc)
    tables = _tables(gpu)
    _write(gpu, tables)
    gpu.set_frames_in_flight(in_flight)
    want = {n: _frame(gpu, n) for n in (3, 6, 12)}
    for _ in range(4):
        gpu.render(MODE_PATH, spp=3, seed=SEED, accumulate=True)
    rgb, ids, _ = gpu.read_output()
    E.assert_bit_identical((rgb, ids), want[12], f"{in_flight} in flight: 4 x 3 spp")
    assert gpu.accumulation() == (12, SEED)
    # a write that is not empty restarts the sum, an empty or a refused one does not
    gpu.write_polish(tables[1][:4])   # (the same values)
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), want[3], "after a write")
    assert gpu.accumulation() == (3, SEED)
    gpu.write_polish(polish_ref.table()[:0])
    bad = tables[1].copy()
    bad[9]["chance"] = np.nan
    with pytest.raises(VrtError):
        gpu.write_polish(bad)
    assert gpu.accumulation() == (3, SEED)
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), want[6], "after an empty write and a refused one")
    assert gpu.accumulation() == (6, SEED)
    gpu.close()


# ---- 8. refusals ----

def test_refusals_change_nothing(monkeypatch):
    sc = scenes.c4(SIZES[0])
    gpu = _gpu(monkeypatch, sc)
    tables = _tables(gpu)
    _write(gpu, tables)
    want = _frame(gpu, 3)
    cases = []
    for field in ("color0", "color1", "color2", "chance", "scatter"):
        for value in (-0.25, np.nan, np.inf, -np.inf):
            bad = polish_ref.table({i: COAT_A for i in range(256)})   # (a refused call writes nothing: none of these either)
            if field.startswith("color"):
                bad[200]["color"][int(field[-1])] = value
            else:
                bad[200][field] = value
            cases.append((f"{field} {value}", bad, 0, _ffi.VRT_ERR_INVALID_ARG))
    one = polish_ref.table({i: COAT_A for i in range(256)})
    cases += [("255 + 2", one[:2], 255, _ffi.VRT_ERR_OUT_OF_RANGE), ("256 + 1", one[:1], 256, _ffi.VRT_ERR_OUT_OF_RANGE),
              ("0 + 257", np.concatenate([one, one[:1]]), 0, _ffi.VRT_ERR_OUT_OF_RANGE),
              ("2^32 - 1 + 2", one[:2], 0xFFFFFFFF, _ffi.VRT_ERR_OUT_OF_RANGE)]
    for name, entries, first, code in cases:
        with pytest.raises(VrtError) as e:
            gpu.write_polish(entries, first=first)
        assert e.value.code == code, name
    assert gpu._lib.vrt_write_polish(gpu._h, 0, None, 4) == _ffi.VRT_ERR_INVALID_ARG   # NULL with n > 0
    assert gpu._lib.vrt_write_polish(None, 0, one.ctypes.data, 4) == _ffi.VRT_ERR_INVALID_ARG   # a null context
    E.assert_bit_identical(_frame(gpu, 3), want, "the frame after the refused writes")
    gpu.close()


# ---- 9. the primary modes ----

def test_the_primary_modes_ignore_the_table(monkeypatch):
    sc = scenes.c4(SIZES[0])
    gpu = _gpu(monkeypatch, sc)
    tables = _tables(gpu)
    want = {}
    for mode in (MODE_PRIMARY, MODE_PRIMARY_SHADOW):
        gpu.render(mode)
        want[mode] = gpu.read_output()[:2]
    _write(gpu, tables)
    for n in (1, 2):
        gpu.set_frames_in_flight(n)
        for mode in (MODE_PRIMARY, MODE_PRIMARY_SHADOW):
            gpu.render(mode)
            E.assert_bit_identical(gpu.read_output()[:2], want[mode], f"mode {mode}, {n} in flight")
    gpu.close()


# ---- 10. shards and devices ----

def test_shards_and_devices_give_the_one_device_frame(monkeypatch):
    sc = scenes.c4((160, 96))
    whole = _gpu(monkeypatch, sc)
    tables = _tables(whole)
    _write(whole, tables)
    want = _frame(whole, 3)
    whole.close()
    sum_rgb, all_ids = np.zeros_like(want[0]), np.zeros_like(want[1])
    for r in range(2):
        sh = _gpu(monkeypatch, sc, shard_rank=r, shard_count=2)
        _write(sh, tables)   # (a shard's context keeps its own table)
        rgb, ids = _frame(sh, 3)
        sum_rgb += rgb
        all_ids |= ids
        sh.close()
    E.assert_bit_identical((sum_rgb, all_ids), want, "the union of two shards")
    grp = _gpu(monkeypatch, sc, devices=[0, 0], texel_messages=True)
    _write(grp, tables)   # (replicated to every device)
    E.assert_bit_identical(_frame(grp, 3), want, "two devices with texel messages")
    grp.close()
