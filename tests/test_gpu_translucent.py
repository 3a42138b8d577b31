"""Translucent materials in the path trace (vrt_write_translucency, include/vrt.h) on the GPU.

Against tests/translucent_ref.py (the oracle's path loop with path_tracer.wgsl's emission term, its coat and the pass-through
lobe) on every route through the kernels, both layouts of the march cells, every bounce count, one sample per chain, lone waves
and the edges of the table; a table without a chance renders exactly as no table; accumulated translucent frames are one frame
of all their samples, bit for bit; what restarts the sum and what is refused; the primary modes; the denoiser; shards and
devices.  Frames against the reference: util.assert_frame_parity (id words equal, radiance within RADIANCE_TOL); GPU against
GPU: bit for bit.

Two sets of tables, both chosen from the context's own 1-spp frame: "alone" is the translucency table with nothing else (the
translucent kernels with the coat word 0: no coat's draw), "all" adds a coat and an emitter (the coat word 1).

Which instantiation a test runs (the host's choice, vrt_path.hip): path_bounce_cells_kernel<true, 4, EMIT, false, TRANSLUCENT> with one frame in
flight on a direct world, <true, 5> with two, <false, 4> on a world with a chunk directory (VRT_MARCH_DIRECT_MAX_S=0);
path_bounce_kernel<.., EMIT, false, TRANSLUCENT> for VRT_PATH_POOL=0, stats frames and the literal march; path_primary_kernel<.., EMIT, false, TRANSLUCENT> always
(its chained form where a frame of several samples has more than one per chain).

That a table without a chance runs the kernels that ran before is the plan's doing (PathFacts::translucent is false while no
chance is set; tests/test_frame_plan.py holds the plan to its launches); here it shows as frames that are bit for bit the
frames from before, under colours that are not 0 — the translucent kernels would have moved every path's RNG stream."""
import numpy as np
import pytest

import emission_cases as E
import polish_ref
import translucent_ref
from voxelraytracing_amd import MODE_PATH, MODE_PRIMARY, MODE_PRIMARY_SHADOW, VrtError, _ffi, scenes

from util import assert_frame_parity, gpu_for_scene

pytestmark = pytest.mark.gpu

SEED = 11
SIZES = [(128, 72), (100, 60)]
SPPS = (1, 3, 12)
ENV = ["VRT_MARCH_DIRECT_MAX_S", "VRT_PATH_POOL", "VRT_PATH_CELLS", "VRT_PATH_POOL_K", "VRT_PATH_POOL_REFILL", "VRT_PATH_SAMPLES_PER_CHAIN"]
HALF = (0.5, (0.9, 0.6, 0.3))             # (chance, colour): passes half of the time, with a tint
ALWAYS = (2.0, (0.25, 0.5, 0.75))         # always passes
DEAD = (0.5, (0.0, 0.0, 0.0))             # entry 255: no voxel of C4 reads it
COAT_A = (0.5, 0.0, (1.0, 0.9, 0.8))      # (chance, scatter, colour): a mirror half of the time
KINDS = ("alone", "all")


@pytest.fixture(scope="module")
def tref(tmp_path_factory):
    return translucent_ref.load(tmp_path_factory.mktemp("translucent_ref"))


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


def _tables(gpu, kind="all"):
    """(emission, polish, translucency) from the context's own 1-spp frame: the material its primary rays hit most passes half
    of the time with a tint, the second always passes, the third has coat A, the fourth gives off light (as many of them as the
    frame hits: a lone wave sees three); entry 255 has a chance and no voxel to use it.  kind "alone": the translucency table
    with the other two left as they are in a new context."""
    gpu.render(MODE_PATH, spp=1, seed=SEED)
    _, ids, _ = gpu.read_output(rgb=False)
    counts = E.hit_counts(ids)
    top = [int(t) for t in np.argsort(counts)[::-1][:4] if counts[t] > 0]
    assert len(top) >= 2
    tr = translucent_ref.table({top[0]: HALF, top[1]: ALWAYS, 255: DEAD})
    if kind == "alone":
        return None, None, tr
    emission = np.zeros(256, np.float32)
    polish = polish_ref.table()
    if len(top) > 2:
        polish[top[2]]["chance"], polish[top[2]]["scatter"], polish[top[2]]["color"] = COAT_A
    if len(top) > 3:
        emission[top[3]] = 1.5
    return emission, polish, tr


def _write(gpu, tables):
    if tables[0] is not None:
        gpu.write_emission(tables[0])
    if tables[1] is not None:
        gpu.write_polish(tables[1])
    gpu.write_translucency(tables[2])


_refs = {}


def _ref(tref, orc, key, sc, tables, spp, seed=SEED):
    """The reference frame, computed once; `key` names the scene (its world, materials, camera, bounces and size)."""
    tables = tables if tables is not None else (None, None, None)
    k = (key, tuple(None if t is None else t.tobytes() for t in tables), spp, seed)
    if k not in _refs:
        _refs[k] = tref.render(orc.from_package_scene(sc), *tables, *sc.size, spp=spp, seed=seed)
    return _refs[k]


def _check(gpu, tref, orc, key, sc, tables, what, spps=SPPS, in_flight=(1, 2), seed=SEED, **kw):
    for n in in_flight:
        gpu.set_frames_in_flight(n)
        for spp in spps:
            rgb, ids = _frame(gpu, spp, seed, **kw)
            assert_frame_parity(rgb, ids, *_ref(tref, orc, key, sc, tables, spp, seed), f"{what}, {n} in flight, spp {spp}")


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
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_translucent_frames_match_the_reference(tref, orc, monkeypatch, size, route, kind):
    env, stats, literal = ROUTES[route]
    sc = _route_scene(size, route)
    gpu = _gpu(monkeypatch, sc, env)
    tables = _tables(gpu, kind)
    _write(gpu, tables)
    key = f"c4 {size} b4 literal {literal}"
    _check(gpu, tref, orc, key, sc, tables, f"{size} {route} {kind}", stats=stats)
    # (the table is not a no-op here: the reference with it is not the reference without it)
    assert _differ(_ref(tref, orc, key, sc, tables, 3), _ref(tref, orc, key, sc, None, 3)) > 100
    gpu.close()


# ---- 2. the march cells behind a chunk directory ----

@pytest.mark.parametrize("size", SIZES)
def test_the_directory_layout(tref, orc, monkeypatch, size):
    sc = scenes.c4(size)
    gpu = _gpu(monkeypatch, sc, {"VRT_MARCH_DIRECT_MAX_S": "0"})
    tables = _tables(gpu)
    assert gpu.read_march_cells()[1] == False, "the context's march cells are in the direct layout"   # noqa: E712
    _write(gpu, tables)
    _check(gpu, tref, orc, f"c4 {size} b4 literal False", sc, tables, f"{size} directory")
    gpu.close()


# ---- 3. one sample per chain ----

def test_one_sample_per_chain(tref, orc, monkeypatch):
    size = SIZES[0]
    sc = scenes.c4(size)
    gpu = _gpu(monkeypatch, sc, {"VRT_PATH_SAMPLES_PER_CHAIN": "1"})
    tables = _tables(gpu)
    _write(gpu, tables)
    _check(gpu, tref, orc, f"c4 {size} b4 literal False", sc, tables, "one sample per chain")
    gpu.close()


# ---- 4. the bounce counts ----

@pytest.mark.parametrize("bounces", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("route", ["cells", "lane"])
def test_every_bounce_count(tref, orc, monkeypatch, route, bounces):
    size = SIZES[0]
    sc = scenes.c4(size, bounces=bounces)
    gpu = _gpu(monkeypatch, sc, ROUTES[route][0])
    if bounces == 0:   # nothing is traced: no id words to choose a table from
        tables = (None, None, translucent_ref.table({40: HALF, 62: ALWAYS, 255: DEAD}))
    else:
        tables = _tables(gpu, "alone")
    before = {spp: _frame(gpu, spp) for spp in (1, 3)}
    _write(gpu, tables)
    _check(gpu, tref, orc, f"c4 {size} b{bounces} literal False", sc, tables, f"b{bounces} {route}", spps=(1, 3))
    if bounces == 0:
        rgb, ids = _frame(gpu, 3)
        assert not rgb.any() and not ids.any()
    if bounces <= 1:   # the path's only segment is its last: nothing drawn is observed
        for n in (1, 2):
            gpu.set_frames_in_flight(n)
            for spp in (1, 3):
                E.assert_bit_identical(_frame(gpu, spp), before[spp], f"b{bounces} {route}: spp {spp} with the table and without")
    gpu.close()


# ---- 5. a lone wave ----

@pytest.mark.parametrize("size", [(8, 8), (16, 8)])
def test_a_lone_wave(tref, orc, monkeypatch, size):
    """One tile and two: the pool kernel with its pool nearly empty, the smallest shape at which its compaction can go wrong —
    and where a whole wave can pass at once, the one place the bounce's draws are branched around."""
    for bounces in (2, 4):
        sc = scenes.c4(size, bounces=bounces)
        gpu = _gpu(monkeypatch, sc)
        tables = _tables(gpu)
        _write(gpu, tables)
        _check(gpu, tref, orc, f"c4 {size} b{bounces} literal False", sc, tables, f"{size} b{bounces}", in_flight=(1,))
        gpu.close()


# ---- 6. the table's edges ----

def test_ids_above_255_read_entry_255(tref, orc, monkeypatch):
    size = SIZES[0]
    sc = E.c4_high_ids(size)
    gpu = _gpu(monkeypatch, sc)
    emission, polish, tr = _tables(gpu)
    tr[255]["chance"], tr[255]["color"] = ALWAYS
    tables = (emission, polish, tr)
    _write(gpu, tables)
    key = f"high ids {size}"
    _check(gpu, tref, orc, key, sc, tables, "ids above 255")
    _check(gpu, tref, orc, key, sc, tables, "ids above 255, stats", spps=(3,), stats=True)
    # entry 255 is what those voxels read: with another entry there the pixels that see them are others
    other = tr.copy()
    other[255]["chance"], other[255]["color"] = 0.0, (0.0, 0.0, 0.0)
    other[254]["chance"] = 0.5   # (still a translucent frame: the same draws, another decision)
    with_, without = _ref(tref, orc, key, sc, tables, 3), _ref(tref, orc, key, sc, (emission, polish, other), 3)
    high = ((with_[1] & E.ID_HIT) != 0) & ((with_[1] & E.ID_VOXEL_MASK) > 255)
    assert high.sum() > 300 and (np.abs(with_[0] - without[0]).max(axis=2)[high] > 1e-3).sum() > 100
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


@pytest.mark.parametrize("kind", KINDS)
def test_a_table_without_a_chance_is_no_table(monkeypatch, kind):
    """All zero bytes, and chances of -0.0 under colours that are not zero, each written over a live context (with and without
    the other two tables): every frame is byte for byte the frame from before — and with a chance written and taken back."""
    sc = scenes.c4(SIZES[0])
    gpu = _gpu(monkeypatch, sc)
    emission, polish, tr = _tables(gpu, kind)
    if kind == "all":
        gpu.write_emission(emission)
        gpu.write_polish(polish)
    want = _all_modes(gpu)
    minus_zero = translucent_ref.table()
    minus_zero["chance"], minus_zero["color"] = -0.0, (0.25, 0.5, 0.75)
    for name, table in (("zeros", translucent_ref.table()), ("-0.0 chances", minus_zero)):
        gpu.write_translucency(table)
        for n in (1, 2):
            gpu.set_frames_in_flight(n)
            got = _all_modes(gpu)
            for k in want:
                E.assert_bit_identical(got[k], want[k], f"{name}, {n} in flight: {k}")
    gpu.write_translucency(tr)
    assert not np.array_equal(_frame(gpu, 3)[0], want[("path", 3)][0])
    gpu.write_translucency(minus_zero)
    got = _all_modes(gpu)
    for k in want:
        E.assert_bit_identical(got[k], want[k], f"a chance taken back: {k}")
    gpu.close()


def test_a_coat_written_and_taken_back(tref, orc, monkeypatch):
    """The translucent kernels take the coat's draw under a word that vrt_write_polish keeps on the device: a translucent frame
    with a coat, then with the coat's chances taken back to 0, then with the coat again — each the reference's frame for its
    tables, on the pool kernel and on the lane = path kernels (a stats frame)."""
    size = SIZES[0]
    sc = scenes.c4(size)
    gpu = _gpu(monkeypatch, sc)
    emission, polish, tr = _tables(gpu)
    key = f"c4 {size} b4 literal False"
    _write(gpu, (emission, polish, tr))
    for name, table in (("a coat", polish), ("taken back", polish_ref.table()), ("again", polish)):
        gpu.write_polish(table)
        _check(gpu, tref, orc, key, sc, (emission, table, tr), f"coat {name}", spps=(1, 3))
        _check(gpu, tref, orc, key, sc, (emission, table, tr), f"coat {name}, stats", spps=(3,), in_flight=(1,), stats=True)
    assert _differ(_ref(tref, orc, key, sc, (emission, polish, tr), 3), _ref(tref, orc, key, sc, (emission, polish_ref.table(), tr), 3)) > 100
    gpu.close()


# ---- 7. accumulation ----

@pytest.mark.parametrize("in_flight", [1, 2])
def test_accumulated_translucent_frames_are_one_frame_of_all_their_samples(monkeypatch, in_flight):
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
    gpu.write_translucency(tables[2][:4])   # (the same values)
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), want[3], "after a write")
    assert gpu.accumulation() == (3, SEED)
    gpu.write_translucency(translucent_ref.table()[:0])
    bad = tables[2].copy()
    bad[9]["chance"] = np.nan
    with pytest.raises(VrtError):
        gpu.write_translucency(bad)
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
    for field in ("color0", "color1", "color2", "chance"):
        for value in (-0.25, np.nan, np.inf, -np.inf):
            bad = translucent_ref.table({i: ALWAYS for i in range(256)})   # (a refused call writes nothing: none of these either)
            if field.startswith("color"):
                bad[200]["color"][int(field[-1])] = value
            else:
                bad[200][field] = value
            cases.append((f"{field} {value}", bad, 0, _ffi.VRT_ERR_INVALID_ARG))
    one = translucent_ref.table({i: ALWAYS for i in range(256)})
    cases += [("255 + 2", one[:2], 255, _ffi.VRT_ERR_OUT_OF_RANGE), ("256 + 1", one[:1], 256, _ffi.VRT_ERR_OUT_OF_RANGE),
              ("0 + 257", np.concatenate([one, one[:1]]), 0, _ffi.VRT_ERR_OUT_OF_RANGE),
              ("2^32 - 1 + 2", one[:2], 0xFFFFFFFF, _ffi.VRT_ERR_OUT_OF_RANGE)]
    for name, entries, first, code in cases:
        with pytest.raises(VrtError) as e:
            gpu.write_translucency(entries, first=first)
        assert e.value.code == code, name
    assert gpu._lib.vrt_write_translucency(gpu._h, 0, None, 4) == _ffi.VRT_ERR_INVALID_ARG   # NULL with n > 0
    assert gpu._lib.vrt_write_translucency(None, 0, one.ctypes.data, 4) == _ffi.VRT_ERR_INVALID_ARG   # a null context
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


# ---- 10. the denoiser ----

def test_denoised_translucent_frames(tref, orc, monkeypatch):
    """The filter behind a translucent frame is the filter behind any path frame: the frame is vrth_denoise of its own raw
    frame bit for bit, and of the reference's frame within RADIANCE_TOL — sigma_color 0, so a tap's weight comes from the id
    and guide words alone, which are equal on both sides, and every output is a convex combination of inputs that are within
    the tolerance.  The guide is the guide of the context without the table: it comes from the primary segment."""
    size = SIZES[1]
    sc = scenes.c4(size)
    gpu = _gpu(monkeypatch, sc)
    gpu.set_denoise(3, 0.0)
    gpu.render(MODE_PATH, spp=1, seed=SEED)
    guide_before = gpu.read_guide()
    gpu.set_denoise(0)
    tables = _tables(gpu)
    _write(gpu, tables)
    for spp in (1, 3):
        raw = _frame(gpu, spp)
        gpu.set_denoise(3, 0.0)
        got = _frame(gpu, spp)
        guide = gpu.read_guide()
        gpu.set_denoise(0)
        assert np.array_equal(guide, guide_before) and np.array_equal(got[1], raw[1])
        E.assert_bit_identical((got[0], got[1]), (_ffi.denoise(raw[0], raw[1], guide, 3, 0.0), raw[1]), f"spp {spp}: the filter over the raw frame")
        ref_rgb, ref_ids = _ref(tref, orc, f"c4 {size} b4 literal False", sc, tables, spp)
        assert_frame_parity(got[0], got[1], _ffi.denoise(ref_rgb, ref_ids, guide, 3, 0.0), ref_ids, f"spp {spp}: the filter over the reference")
        assert not np.array_equal(got[0], raw[0])
    gpu.close()


# ---- 11. shards and devices ----

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
