"""Camera sampling in the path trace (vrt_set_camera_sampling, include/vrt.h) on the GPU.

Against tests/lens_ref.py (tests/sun_ref.py's loop with a primary ray of its own for every sample) on every route through the
kernels — the default (several samples per launch chain, the pool kernel behind bounce 0), the march cells behind a chunk
directory, the literal march (air flagged liquid) and the counting kernels of a stats frame — at one wave, two waves, a frame
whose size is not whole tiles and a frame of several workgroups; 1, 2 and 4 bounces; 1, 3 and 12 samples (12: more than one
chain of 8); one and two frames in flight; jitter alone, the lens alone and both — each alone at every size, and at 100 x 60 with
the emission, polish and translucency tables of tests/test_gpu_sun.py, with and without its sun.  Frames against the reference:
util.assert_frame_parity (id words equal, radiance within RADIANCE_TOL).  A stats frame's steps and secondary rays are the
reference's counts.  GPU against GPU, bit for bit: off after on, the id words / step counts / guide of an on frame, the denoiser,
accumulation, shards, refusals.  Every test here calls vrt_set_camera_sampling.

FOCUS is tests/test_lens_ref.py's: at 32 voxels most of C4's lens samples hit the face their pixel's pinhole ray hits (sharp)
and a few hundred another (blurred)."""
import ctypes as C

import numpy as np
import pytest

import emission_cases as E
import lens_ref
from test_gpu_sun import ROUTES, SEED, STRENGTH, _frame, _gpu, _scene, _tables, _write
from test_lens_ref import BOTH, FOCUS, JITTER, LENS
from voxelraytracing_amd import MODE_PATH, MODE_PRIMARY, MODE_PRIMARY_SHADOW, _ffi, scenes

from util import assert_frame_parity

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (16, 8), (100, 60), (128, 72)]
BOUNCES = (1, 2, 4)
SPPS = (1, 3, 12)
SETTINGS = {"jitter": JITTER, "lens": LENS, "both": BOTH}


@pytest.fixture(scope="module")
def lref(tmp_path_factory):
    return lens_ref.load(tmp_path_factory.mktemp("lens_ref"))


_refs = {}


def _ref(lref, orc, key, sc, setting, tables, spp, strength=0.0, seed=SEED):
    """(rgb, ids, counts) of the reference frame, computed once; `key` names the scene (its world, materials, camera, bounces, size)."""
    tables = tables if tables is not None else (None, None, None)
    k = (key, setting, tuple(None if t is None else t.tobytes() for t in tables), spp, strength, seed)
    if k not in _refs:
        rgb, ids = lref.render(orc.from_package_scene(sc), setting, *sc.size, spp=spp, seed=seed, strength=strength, emission=tables[0],
                               polish=tables[1], translucency=tables[2])
        _refs[k] = (rgb, ids, lref.counts)
    return _refs[k]


def _check(gpu, lref, orc, key, sc, setting, tables, strength, stats, what):
    for n in (1, 2):
        gpu.set_frames_in_flight(n)
        for spp in SPPS:
            w = f"{what}, {n} in flight, spp {spp}"
            rgb, ids = _frame(gpu, spp, stats=stats)
            ref_rgb, ref_ids, counts = _ref(lref, orc, key, sc, setting, tables, spp, strength)
            err = np.abs(rgb - ref_rgb)
            print(f"{w}: max radiance error {float(err[np.isfinite(err)].max()):.3g}; {counts}")
            assert_frame_parity(rgb, ids, ref_rgb, ref_ids, w)
            if stats:
                st = gpu.stats()
                print(f"    secondary_rays {st.secondary_rays} steps {st.steps} hits {st.hits}")
                assert st.secondary_rays == counts.bounce_segments + counts.sun_rays, w
                assert st.steps == counts.steps, w
                assert st.hits == int(((ref_ids & orc.ID_HIT) != 0).sum()), w


# ---- 1. frames against the reference, route by route ----

@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("bounces", BOUNCES)
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_frames_with_camera_sampling_match_the_reference(lref, orc, monkeypatch, route, size, bounces, setting):
    env, stats, literal = ROUTES[route]
    sc = _scene(size, bounces, literal)
    gpu = _gpu(monkeypatch, sc, env)
    if route == "directory":
        gpu.render(MODE_PATH, spp=1, seed=SEED)
        assert gpu.read_march_cells()[1] == False, "the context's march cells are in the direct layout"   # noqa: E712
    gpu.set_camera_sampling(*SETTINGS[setting])
    _check(gpu, lref, orc, f"c4 {size} b{bounces} literal {literal}", sc, SETTINGS[setting], None, 0.0, stats, f"{size} b{bounces} {route} {setting}")
    gpu.close()


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("bounces", BOUNCES)
@pytest.mark.parametrize("route", list(ROUTES))
def test_with_the_tables_and_the_sun(lref, orc, monkeypatch, route, bounces, setting):
    """The tables of tests/test_gpu_sun.py (a pass-through half of the time, one always, a coat, an emitter): first without the
    sun — on the default route that is the translucent form of the chains of several samples and of the pool kernel — then with
    it, where every sample's sun ray starts from its own hit."""
    env, stats, literal = ROUTES[route]
    size = SIZES[2]
    sc = _scene(size, bounces, literal)
    gpu = _gpu(monkeypatch, sc, env)
    tables = _tables(gpu)
    _write(gpu, tables)
    gpu.set_camera_sampling(*SETTINGS[setting])
    key = f"c4 {size} b{bounces} literal {literal}"
    for strength in (0.0, STRENGTH):
        gpu.set_sun_light(strength)
        _check(gpu, lref, orc, key, sc, SETTINGS[setting], tables, strength, stats, f"{size} b{bounces} {route} {setting} tables, sun {strength}")
    _, _, counts = _ref(lref, orc, key, sc, SETTINGS[setting], tables, 3, STRENGTH)
    assert counts.sun_rays >= 1 and counts.jitter_changed >= 1
    gpu.close()


# ---- 2. GPU against GPU, bit for bit ----

def _all_modes(gpu):
    out = {("path", spp): _frame(gpu, spp) for spp in (1, 3)}
    out[("path stats", 3)] = _frame(gpu, 3, stats=True)
    for name, mode in (("primary", MODE_PRIMARY), ("primary+shadow", MODE_PRIMARY_SHADOW)):
        gpu.render(mode)
        out[(name, 1)] = gpu.read_output()[:2]
    return out


def test_off_after_on_gives_the_frame_from_before(monkeypatch):
    sc = _scene(SIZES[3])
    gpu = _gpu(monkeypatch, sc)
    _write(gpu, _tables(gpu))
    want = _all_modes(gpu)
    gpu.set_camera_sampling(*BOTH)
    assert not np.array_equal(_frame(gpu, 3)[0], want[("path", 3)][0])
    for name, off in (("zeros", lambda: gpu.set_camera_sampling(0.0)), ("-0, and a focus distance nobody reads", lambda: gpu.set_camera_sampling(-0.0, -0.0, 7.0)),
                      ("NULL", lambda: gpu._ck(gpu._lib.vrt_set_camera_sampling(gpu._h, None)))):
        gpu.set_camera_sampling(*BOTH)
        off()
        for n in (1, 2):
            gpu.set_frames_in_flight(n)
            got = _all_modes(gpu)
            for k in want:
                E.assert_bit_identical(got[k], want[k], f"{name}, {n} in flight: {k}")
    gpu.close()


def test_the_primary_modes_ignore_the_setting(monkeypatch):
    sc = _scene(SIZES[3])
    gpu = _gpu(monkeypatch, sc)
    want = {}
    for mode in (MODE_PRIMARY, MODE_PRIMARY_SHADOW):
        gpu.render(mode)
        want[mode] = gpu.read_output()[:2]
    gpu.set_camera_sampling(*BOTH)
    for n in (1, 2):
        gpu.set_frames_in_flight(n)
        for mode in (MODE_PRIMARY, MODE_PRIMARY_SHADOW):
            gpu.render(mode)
            E.assert_bit_identical(gpu.read_output()[:2], want[mode], f"mode {mode}, {n} in flight")
    gpu.close()


@pytest.mark.parametrize("bounces", [1, 4])
def test_id_words_step_counts_and_guide_are_the_off_frames(monkeypatch, bounces):
    """They come from the pixel's own pinhole ray.  vrt_read_steps' word is primary | later segments << 16: the primary count is
    the off frame's at any number of bounces, and at one bounce — no later segment — so is the whole word."""
    sc = _scene(SIZES[2], bounces)
    gpu = _gpu(monkeypatch, sc)
    gpu.set_denoise(3, 0.0)
    _, ids_off = _frame(gpu, 3, stats=True)
    steps_off, guide_off, hits_off = gpu.read_steps(), gpu.read_guide(), gpu.stats().hits
    for name, setting in SETTINGS.items():
        gpu.set_camera_sampling(*setting)
        for spp in (1, 3):
            _, ids = _frame(gpu, spp, stats=True)
            steps = gpu.read_steps()
            assert np.array_equal(ids, ids_off), (name, spp)
            assert np.array_equal(steps & 0xFFFF, steps_off & 0xFFFF), (name, spp)
            if bounces == 1:
                assert np.array_equal(steps, steps_off), (name, spp)
            assert np.array_equal(gpu.read_guide(), guide_off), (name, spp)
            assert gpu.stats().hits == hits_off, (name, spp)
            _, ids = _frame(gpu, spp)
            assert np.array_equal(ids, ids_off) and np.array_equal(gpu.read_guide(), guide_off), (name, spp)
    gpu.close()


def test_the_denoised_frame_is_the_host_filter_over_the_raw_one(monkeypatch):
    sc = _scene(SIZES[2])
    gpu = _gpu(monkeypatch, sc)
    gpu.set_camera_sampling(*BOTH)
    for spp in (1, 3):
        raw = _frame(gpu, spp)
        gpu.set_denoise(3, 0.0)
        got = _frame(gpu, spp)
        guide = gpu.read_guide()
        gpu.set_denoise(0)
        assert np.array_equal(got[1], raw[1])
        E.assert_bit_identical((got[0], got[1]), (_ffi.denoise(raw[0], raw[1], guide, 3, 0.0), raw[1]), f"spp {spp}: the filter over the raw frame")
        assert not np.array_equal(got[0], raw[0])
    gpu.close()


def _set_raw(gpu, spread, aperture=0.0, focus=0.0, flags=0):
    o = _ffi.CameraSampling(spread, aperture, focus, flags)
    return gpu._lib.vrt_set_camera_sampling(gpu._h, C.byref(o))


NAN, INF = float("nan"), float("inf")
REFUSED = [(-0.5, 0.0, 0.0, 0), (NAN, 0.0, 0.0, 0), (INF, 0.0, 0.0, 0), (1.0, -0.25, 4.0, 0), (1.0, NAN, 4.0, 0), (1.0, INF, 4.0, 0),
           (1.0, 0.25, -4.0, 0), (1.0, 0.25, NAN, 0), (1.0, 0.25, INF, 0), (0.0, 0.0, -1.0, 0), (0.0, 0.0, NAN, 0), (8.5, 0.0, 0.0, 0),
           (1.0, 0.25, 0.0, 0), (0.0, 0.25, -0.0, 0), (1.0, 0.0, 0.0, 1), (0.0, 0.0, 0.0, 2)]


@pytest.mark.parametrize("in_flight", [1, 2])
def test_accumulated_frames_are_one_frame_of_all_their_samples(monkeypatch, in_flight):
    sc = _scene(SIZES[2])
    gpu = _gpu(monkeypatch, sc)
    _write(gpu, _tables(gpu))
    gpu.set_camera_sampling(*BOTH)
    gpu.set_frames_in_flight(in_flight)
    want = {n: _frame(gpu, n) for n in (3, 6, 12)}
    for _ in range(4):
        gpu.render(MODE_PATH, spp=3, seed=SEED, accumulate=True)
    rgb, ids, _ = gpu.read_output()
    E.assert_bit_identical((rgb, ids), want[12], f"{in_flight} in flight: 4 x 3 spp")
    assert gpu.accumulation() == (12, SEED)
    # an identical call does not restart the sum, nor does a refused one
    gpu.set_camera_sampling(*BOTH)
    for bad in REFUSED:
        assert _set_raw(gpu, *bad) == _ffi.VRT_ERR_INVALID_ARG, bad
    assert gpu.accumulation() == (12, SEED)
    gpu.reset_accumulation()
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), want[3], "a refused call changed nothing")
    gpu.set_camera_sampling(*BOTH)
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), want[6], "after an identical call: the sum goes on")
    assert gpu.accumulation() == (6, SEED)
    # a change of any field restarts it
    for changed in ((0.5, BOTH[1], BOTH[2]), (BOTH[0], 0.5, BOTH[2]), (BOTH[0], BOTH[1], 16.0)):
        gpu.set_camera_sampling(*changed)
        gpu.set_camera_sampling(*BOTH)
        E.assert_bit_identical(_frame(gpu, 3, accumulate=True), want[3], f"after {changed} and back: the sum starts again")
        assert gpu.accumulation() == (3, SEED)
        E.assert_bit_identical(_frame(gpu, 3, accumulate=True), want[6], "... and goes on")
    # without a lens the focus distance is not read, and not compared
    gpu.set_camera_sampling(1.0, 0.0, 5.0)
    jit = {n: _frame(gpu, n) for n in (3, 6)}
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), jit[3], "jitter alone: the sum started again")
    gpu.set_camera_sampling(1.0, 0.0, 9.0)
    gpu.set_camera_sampling(1.0, -0.0, 0.0)
    assert gpu.accumulation() == (3, SEED)
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), jit[6], "another focus distance without a lens: the sum goes on")
    # off on a context that is off already does not restart the sum; turning it off does
    gpu.set_camera_sampling(0.0)
    off = {n: _frame(gpu, n) for n in (3, 6)}
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), off[3], "off: the sum started again")
    gpu.set_camera_sampling(0.0)
    gpu.set_camera_sampling(-0.0, -0.0, 3.0)
    gpu._ck(gpu._lib.vrt_set_camera_sampling(gpu._h, None))
    assert gpu.accumulation() == (3, SEED)
    E.assert_bit_identical(_frame(gpu, 3, accumulate=True), off[6], "off again, three ways: the sum goes on")
    gpu.close()


def test_a_refused_call_leaves_the_next_frame_unchanged(monkeypatch):
    sc = _scene(SIZES[2])
    gpu = _gpu(monkeypatch, sc)
    off = _frame(gpu, 3)
    for bad in REFUSED:
        assert _set_raw(gpu, *bad) == _ffi.VRT_ERR_INVALID_ARG, bad
        E.assert_bit_identical(_frame(gpu, 3), off, f"off, after {bad}")
    gpu.set_camera_sampling(*BOTH)
    on = _frame(gpu, 3)
    assert not np.array_equal(on[0], off[0])
    for bad in REFUSED:
        assert _set_raw(gpu, *bad) == _ffi.VRT_ERR_INVALID_ARG, bad
        E.assert_bit_identical(_frame(gpu, 3), on, f"on, after {bad}")
    assert _set_raw(gpu, 8.0) == _ffi.VRT_OK   # (the widest filter allowed)
    gpu.close()


def test_the_union_of_two_shards_is_the_whole_frame(monkeypatch):
    sc = scenes.c4((160, 96))
    whole = _gpu(monkeypatch, sc)
    tables = _tables(whole)
    _write(whole, tables)
    whole.set_camera_sampling(*BOTH)
    want = _frame(whole, 3)
    whole.close()
    sum_rgb, all_ids = np.zeros_like(want[0]), np.zeros_like(want[1])
    for r in range(2):
        sh = _gpu(monkeypatch, sc, shard_rank=r, shard_count=2)
        _write(sh, tables)
        sh.set_camera_sampling(*BOTH)   # (a shard's context keeps its own setting)
        rgb, ids = _frame(sh, 3)
        sum_rgb += rgb
        all_ids |= ids
        sh.close()
    E.assert_bit_identical((sum_rgb, all_ids), want, "the union of two shards")
    grp = _gpu(monkeypatch, sc, devices=[0, 0], texel_messages=True)
    _write(grp, tables)
    grp.set_camera_sampling(*BOTH)   # (replicated to every device)
    E.assert_bit_identical(_frame(grp, 3), want, "two devices with texel messages")
    grp.close()
