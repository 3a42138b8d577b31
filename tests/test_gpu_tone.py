"""Exposure and tone mapping of presented path frames on the GPU (vrt_set_tone_map, include/vrt.h) against tests/tone_ref.py.

Metering: the histogram and every field of vrt_tone_info are the reference's over the very radiance vrt_read_output gives, bit
for bit.  Adaptation: the exposure follows the reference recurrence over the per-frame targets with one to three frames in
flight.  The presented image: vrt_present / vrt_present_device are the oracle's blit over the reference's map of the frame's
texels, byte for byte, on every blit kernel.  Off is off, and the setting touches nothing but the presented image."""
import ctypes as C

import numpy as np
import pytest

import tone_cases as tc
import tone_ref as tr
from voxelraytracing_amd import MODE_PATH, MODE_PRIMARY, MODE_PRIMARY_SHADOW, Gpu, VrtError, _ffi

from util import gpu_for_scene

pytestmark = pytest.mark.gpu

SEED = tc.SEED
F = np.float32


def tone_gpu(size=tc.MAIN, bounces=4, in_flight=None, **kw):
    sc = tc.scene(size, bounces)
    gpu = gpu_for_scene(sc, **kw)
    gpu.set_sun_light(tc.SUN)
    gpu.write_emission(tc.emission_table())
    if in_flight:
        gpu.set_frames_in_flight(in_flight)
    return sc, gpu


def same(a, b):
    return tr.bits(F(a)) == tr.bits(F(b))


def check_info(gpu, rgb, s, prev, frames, what):
    """The last frame's record and bins against the reference over the radiance it left; -> the reference record."""
    want, want_bins = tr.meter(rgb, s, prev, frames)
    info, bins = gpu.tone_info(), gpu.tone_histogram()
    print(f"{what}: E {info.exposure!r} target {info.target!r} L {info.luminance!r} bin {info.bin} counted {info.counted} skipped {info.skipped} "
          f"frames {info.frames}; reference {want}")
    assert np.array_equal(bins.astype(np.uint64), want_bins), f"{what}: {int((bins != want_bins).sum())} bins differ"
    assert (info.counted, info.skipped, info.bin, info.frames, info._reserved) == (want.counted, want.skipped, want.bin, frames, 0), what
    for name in ("exposure", "target", "luminance"):
        assert same(getattr(info, name), getattr(want, name)), f"{what}: {name} {getattr(info, name)!r}, reference {getattr(want, name)!r}"
    return want, want_bins


def not_vacuous(want, bins, size, what):
    assert int((bins > 0).sum()) >= 8, f"{what}: the histogram occupies {int((bins > 0).sum())} bins"
    assert want.counted >= (size[0] & ~7) * (size[1] & ~7) // 2, f"{what}: {want.counted} pixels counted"


AUTO = tr.Setting(curve=tr.FILMIC, flags=tr.AUTO, exposure=1.25, key=0.18, adapt=1.0, percentile=500)


# ---- metering ----
@pytest.mark.parametrize("size", [(8, 8), (64, 40), (250, 131)])
@pytest.mark.parametrize("percentile", [500, 0, 1000])
def test_metering_is_the_reference_over_the_frames_radiance(size, percentile):
    sc, gpu = tone_gpu(size)
    s = tr.Setting(curve=tr.FILMIC, flags=tr.AUTO, exposure=1.25, percentile=percentile, min_auto=0.01, max_auto=50.0)
    gpu.set_tone_map(opts=s.ffi())
    gpu.render(MODE_PATH, seed=SEED)
    rgb, _, _ = gpu.read_output()
    want, bins = check_info(gpu, rgb, s, None, 1, f"{size} p{percentile}")
    assert want.counted + want.skipped == (size[0] & ~7) * (size[1] & ~7)
    if size == (250, 131):
        assert not rgb[128:].any() and not rgb[:, 248:].any()   # (only the traced area counts, and it is all there is)
    if size != (8, 8):
        not_vacuous(want, bins, size, str(size))
    gpu.close()


def test_metering_a_frame_without_light():
    sc, gpu = tone_gpu(bounces=0)
    s = tr.Setting(curve=tr.REINHARD, flags=tr.AUTO, exposure=0.75, adapt=0.5)
    gpu.set_tone_map(opts=s.ffi())
    gpu.render(MODE_PATH, seed=SEED)
    rgb, _, _ = gpu.read_output()
    assert not rgb.any()
    want, bins = check_info(gpu, rgb, s, None, 1, "no bounces")
    assert want.counted == 0 and want.skipped == 64 * 40 and same(want.exposure, 0.75) and not bins.any()
    gpu.render(MODE_PATH, seed=SEED)   # ... and again: the target is the exposure before it
    check_info(gpu, gpu.read_output()[0], s, want.exposure, 2, "no bounces, second frame")
    gpu.close()


def test_metering_the_denoised_frame():
    sc, gpu = tone_gpu()
    gpu.set_tone_map(opts=AUTO.ffi())
    gpu.render(MODE_PATH, seed=SEED)
    raw, _, _ = gpu.read_output()
    raw_info, raw_bins = check_info(gpu, raw, AUTO, None, 1, "raw")
    gpu.set_denoise(3, 0.0)
    gpu.render(MODE_PATH, seed=SEED)
    rgb, _, _ = gpu.read_output()
    assert not np.array_equal(tr.bits(rgb), tr.bits(raw))
    want, bins = check_info(gpu, rgb, AUTO, raw_info.exposure, 2, "3 passes")   # (adapt 1: the previous exposure is not in it)
    not_vacuous(want, bins, tc.MAIN, "denoised")
    assert not np.array_equal(bins, raw_bins), "the filtered frame's histogram is the raw frame's"
    gpu.close()


@pytest.mark.parametrize("in_flight", [1, 2])
def test_metering_the_accumulated_mean(in_flight):
    sc, gpu = tone_gpu(in_flight=in_flight)
    s = tr.Setting(curve=tr.FILMIC, flags=tr.AUTO, adapt=0.5)
    gpu.set_tone_map(opts=s.ffi())
    prev, seen = None, []
    for k in range(3):
        gpu.render(MODE_PATH, seed=SEED, accumulate=True)
        rgb, _, _ = gpu.read_output()
        want, bins = check_info(gpu, rgb, s, prev, k + 1, f"accumulated frame {k}")
        prev = want.exposure
        seen.append(tr.bits(rgb).copy())
    assert gpu.accumulation() == (3, SEED)
    assert not np.array_equal(seen[0], seen[2])
    not_vacuous(want, bins, tc.MAIN, "the mean of 3")
    gpu.close()


# ---- adaptation ----
def reference_targets(gpu, sc, s):
    """Each view's target, from the radiance of a frame of its own (rendered alone: adapt 1 and a fresh adaptation)."""
    out = []
    for pitch in (tc.SKY_PITCH, tc.DOWN_PITCH):
        gpu.set_tone_map(curve=_ffi.TONE_OFF)
        gpu.write_cam_data(tc.view(sc, pitch, tc.MAIN))
        gpu.render(MODE_PATH, seed=SEED)
        info, _ = tr.meter(gpu.read_output()[0], s)
        out.append(info.target)
    return out


@pytest.mark.parametrize("in_flight", [1, 2, 3])
def test_adaptation_across_frames_in_flight(in_flight):
    sc, gpu = tone_gpu(in_flight=in_flight)
    s = tr.Setting(curve=tr.FILMIC, flags=tr.AUTO, adapt=0.25)
    targets = reference_targets(gpu, sc, s)
    assert max(targets) / min(targets) >= F(2), f"the two views meter {targets}"
    cams = [tc.view(sc, p, tc.MAIN) for p in (tc.SKY_PITCH, tc.DOWN_PITCH)]

    def burst(n, start_prev, first_frame):
        """n frames back to back, nothing read in between; the last one's record against the recurrence."""
        E = start_prev
        for k in range(n):
            gpu.write_cam_data(cams[k % 2])
            gpu.render(MODE_PATH, seed=SEED)
            E = tr.adapt(targets[k % 2], s, E)
        info = gpu.tone_info()
        print(f"in flight {in_flight}, {n} frames: E {info.exposure!r}, recurrence {E!r}, target {info.target!r}")
        assert same(info.target, targets[(n - 1) % 2]) and info.frames == first_frame + n - 1
        assert same(info.exposure, E), f"in flight {in_flight}: after {n} frames E {info.exposure!r}, the recurrence gives {E!r}"
        return E

    # after every frame of 8: each burst starts the adaptation again (a changed setting), so frame n is checked behind n - 1
    # frames that were in flight with it
    for n in range(1, 9):
        gpu.set_tone_map(opts=tr.Setting(curve=tr.LINEAR, flags=tr.AUTO, adapt=0.25).ffi())
        gpu.set_tone_map(opts=s.ffi())
        E = burst(n, None, 1)
    # rewriting the identical setting does not start it again: 2 more frames continue the 8
    gpu.set_tone_map(opts=s.ffi())
    E = burst(2, E, 9)
    assert not same(E, targets[1])
    # a resize does: the first frame behind it takes its target (the same size again: the same views)
    gpu.resize_result_texture((72, 48))
    gpu.resize_result_texture(tc.MAIN)
    with pytest.raises(VrtError) as e:
        gpu.tone_info()
    assert e.value.code == _ffi.VRT_ERR_STATE
    burst(1, None, 1)
    gpu.close()


# ---- the presented image ----
def crafted_grid(w, h, white):
    """Texel colours that walk through 0, denormals, 1e-6 .. 1e6, exactly 1, `white`, negatives and 3e38; zero beyond the traced area."""
    tiny = np.array([1, 0x007FFFFF], dtype=np.uint32).view(np.float32)
    vals = np.concatenate([[0.0, -0.0, 1.0, white, -0.5, -3.0, 3e38, 0.18, 0.5, 2.0], tiny, np.exp2(np.linspace(np.log2(1e-6), np.log2(1e6), 229))]).astype(np.float32)
    n = w * h
    idx = np.arange(n)
    rgb = np.stack([vals[idx % vals.size], vals[(idx * 7 + 3) % vals.size], vals[(idx * 13 + 5) % vals.size]], axis=-1).reshape(h, w, 3)
    rgb[h & ~7:] = 0
    rgb[:, w & ~7:] = 0
    return np.ascontiguousarray(rgb, dtype=np.float32)


def hip_memcpy():
    fn = _ffi.vrt().hipMemcpy   # the HIP runtime libvrt.so itself is linked against
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return fn


def overwrite_texels(gpu, rgb, ids):
    h, w = ids.shape
    tex = np.zeros((h, w), dtype=[("rgb", "<f4", 3), ("id", "<u4")])
    tex["rgb"], tex["id"] = rgb, ids
    ptr, nbytes = gpu.device_output()
    assert nbytes == tex.nbytes
    assert hip_memcpy()(ptr, tex.ctypes.data, nbytes, 1) == 0   # hipMemcpyHostToDevice


def read_device(ptr, nbytes, shape):
    host = np.empty(nbytes, dtype=np.uint8)
    assert hip_memcpy()(host.ctypes.data, ptr, nbytes, 2) == 0
    return host.reshape(shape)


# (texture size, window size, crosshair style): the plain kernel, its box pixels, the general kernel, a ragged frame
WINDOWS = [((64, 40), (64, 40), 0), ((64, 40), (64, 40), 2), ((64, 40), (96, 54), 2), ((250, 131), (250, 131), 1), ((250, 131), (120, 64), 0)]
MAPS = [tr.Setting(curve=c, white=wh, flags=f, exposure=e) for c, wh, e in ((tr.LINEAR, 0.0, 0.6), (tr.REINHARD, 0.0, 1.7), (tr.REINHARD, 4.0, 1.7), (tr.FILMIC, 0.0, 0.9))
        for f in (0, tr.GAMMA2)]


@pytest.mark.parametrize("size", [(64, 40), (250, 131)])
def test_the_map_in_the_blit(orc, size):
    sc, gpu = tone_gpu(size, in_flight=1)
    windows = [(win, style) for tex, win, style in WINDOWS if tex == size]
    shown = set()
    for s in MAPS:
        gpu.set_tone_map(opts=s.ffi())
        gpu.render(MODE_PATH, seed=SEED)
        _, ids, _ = gpu.read_output()
        info = gpu.tone_info()
        assert same(info.exposure, s.exposure) and (info.counted, info.skipped, info.target) == (0, 0, 0.0)
        rgb = crafted_grid(*size, white=4.0)
        overwrite_texels(gpu, rgb, ids)
        mapped = tr.tone(rgb, s, s.exposure)
        for win, style in windows:
            want = orc.present(mapped, win, style=style)
            got = gpu.present(win, style=style)
            bad = np.argwhere((got != want).any(axis=2))
            assert bad.size == 0, f"{s} window {win} style {style}: {len(bad)} pixels differ, first at (y, x) = {tuple(bad[0])}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"
            ptr, nbytes = gpu.present_device(win, style=style)
            gpu.synchronize()
            assert np.array_equal(read_device(ptr, nbytes, want.shape), want), f"{s} window {win}: vrt_present_device"
            shown.add(want.tobytes())
        assert not np.array_equal(gpu.present(size, style=0), orc.present(rgb, size, style=0)), "the mapped image is the unmapped one"
    assert len(shown) == len(MAPS) * len(windows), "two settings present alike"
    gpu.close()


@pytest.mark.parametrize("size", [(64, 40), (250, 131)])
def test_the_blit_reads_a_metered_exposure_from_the_device(orc, size):
    sc, gpu = tone_gpu(size, in_flight=2)
    for s in (tr.Setting(curve=tr.FILMIC, flags=tr.AUTO | tr.GAMMA2, adapt=0.5), tr.Setting(curve=tr.REINHARD, white=3.0, flags=tr.AUTO, exposure=2.0)):
        gpu.set_tone_map(opts=s.ffi())
        prev = None
        for k in range(3):   # (frame sets in turn: each blit reads its own set's word)
            gpu.render(MODE_PATH, seed=SEED + k)
            shown = {(win, style): gpu.present(win, style=style) for tex, win, style in WINDOWS if tex == size}
            rgb, _, _ = gpu.read_output()
            want, _ = check_info(gpu, rgb, s, prev, k + 1, f"{size} frame {k}")
            prev = want.exposure
            mapped = tr.tone(rgb, s, want.exposure)
            for (win, style), got in shown.items():
                assert np.array_equal(got, orc.present(mapped, win, style=style)), f"{s} frame {k} window {win} style {style}"
                assert not np.array_equal(got, orc.present(rgb, win, style=style)), f"{s} frame {k} window {win}: the unmapped image"
    gpu.close()


# ---- off is off, and scope ----
def outputs(gpu, mode, **kw):
    gpu.render(mode, seed=SEED, **kw)
    rgb, ids, q = gpu.read_output(rgba8=True)
    return tr.bits(rgb), ids, q, gpu.present(), gpu.present((96, 54), style=1)


def assert_same_outputs(a, b, what):
    for x, y, name in zip(a, b, ("rgb", "ids", "rgba8", "present", "present 96x54")):
        assert np.array_equal(x, y), f"{what}: {name}"


def test_off_is_off():
    lib = _ffi.vrt()
    setups = {"never": lambda gpu: None, "NULL": lambda gpu: gpu._ck(lib.vrt_set_tone_map(gpu._h, None)),
              "curve OFF": lambda gpu: gpu.set_tone_map(curve=_ffi.TONE_OFF, exposure=3.0, gamma2=True),
              "on, then off": lambda gpu: (gpu.set_tone_map(auto=True), gpu.set_tone_map(curve=_ffi.TONE_OFF))}
    got = {}
    for name, setup in setups.items():
        sc, gpu = tone_gpu()
        setup(gpu)
        got[name] = [outputs(gpu, mode) for mode in (MODE_PATH, MODE_PRIMARY, MODE_PRIMARY_SHADOW)]
        for fn in (gpu.tone_info, gpu.tone_histogram):
            with pytest.raises(VrtError) as e:
                fn()
            assert e.value.code == _ffi.VRT_ERR_STATE, name
        gpu.close()
    for name in list(setups)[1:]:
        for a, b in zip(got["never"], got[name]):
            assert_same_outputs(a, b, name)


def test_the_setting_touches_the_presented_path_frame_only():
    sc, plain = tone_gpu()
    sc, gpu = tone_gpu()
    gpu.set_tone_map(curve=_ffi.TONE_FILMIC, auto=True)
    # the primary modes are never mapped: texels, read-backs and presented bytes, the fused presentation included
    for mode in (MODE_PRIMARY, MODE_PRIMARY_SHADOW):
        assert_same_outputs(outputs(plain, mode), outputs(gpu, mode), f"mode {mode}")
        for g_ in (plain, gpu):
            g_.set_presentation()
        assert_same_outputs(outputs(plain, mode), outputs(gpu, mode), f"mode {mode}, fused presentation")
        for g_ in (plain, gpu):
            g_.set_presentation(off=True)
    with pytest.raises(VrtError) as e:
        gpu.tone_info()   # (nothing was mapped or metered yet)
    assert e.value.code == _ffi.VRT_ERR_STATE
    # a path frame: everything vrt_read_output gives is the unmapped frame's; only the presented image differs
    a, b = outputs(plain, MODE_PATH), outputs(gpu, MODE_PATH)
    assert_same_outputs(a[:3], b[:3], "path frame read-backs")
    assert not np.array_equal(a[3], b[3]) and not np.array_equal(a[4], b[4])
    assert gpu.tone_info().frames == 1
    # a primary frame behind it is unmapped again
    assert_same_outputs(outputs(plain, MODE_PRIMARY_SHADOW), outputs(gpu, MODE_PRIMARY_SHADOW), "primary + shadow behind a mapped frame")
    # K accumulated frames are one frame of K x spp, and changing the setting in between does not restart the sum
    plain.render(MODE_PATH, seed=SEED, spp=6)
    want = tr.bits(plain.read_output()[0])
    for k, spp in enumerate((2, 1, 3)):
        gpu.set_tone_map(curve=_ffi.TONE_REINHARD, auto=True, exposure=1.0 + k)
        gpu.render(MODE_PATH, seed=SEED, spp=spp, accumulate=True)
    assert gpu.accumulation() == (6, SEED)
    assert np.array_equal(tr.bits(gpu.read_output()[0]), want)
    plain.close()
    gpu.close()


def test_a_frame_presents_with_the_setting_it_was_rendered_under(orc):
    sc, gpu = tone_gpu(in_flight=1)
    a = tr.Setting(curve=tr.FILMIC, exposure=0.4)
    gpu.set_tone_map(opts=a.ffi())
    gpu.render(MODE_PATH, seed=SEED)
    rgb, _, _ = gpu.read_output()
    want = orc.present(tr.tone(rgb, a, a.exposure), tc.MAIN)
    for change in (lambda: gpu.set_tone_map(curve=_ffi.TONE_REINHARD, exposure=5.0, gamma2=True), lambda: gpu.set_tone_map(curve=_ffi.TONE_OFF),
                   lambda: gpu.set_tone_map(auto=True)):
        change()
        assert np.array_equal(gpu.present(), want)
    # ... and an unmapped frame stays unmapped when the setting comes on behind it
    gpu.set_tone_map(curve=_ffi.TONE_OFF)
    gpu.render(MODE_PATH, seed=SEED)
    gpu.set_tone_map(opts=a.ffi())
    assert np.array_equal(gpu.present(), orc.present(rgb, tc.MAIN))
    gpu.close()


def _set(gpu, s):
    return _ffi.vrt().vrt_set_tone_map(gpu._h, None if s is None else C.byref(s.ffi() if isinstance(s, tr.Setting) else s))


def test_refusals_change_nothing(orc):
    sc, gpu = tone_gpu(in_flight=1)
    kept = tr.Setting(curve=tr.REINHARD, white=2.0, exposure=0.8, flags=tr.GAMMA2)
    gpu.set_tone_map(opts=kept.ffi())
    nan, inf = float("nan"), float("inf")
    S = tr.Setting
    bad = [S(curve=4), S(flags=4), S(flags=8 | tr.AUTO), S(curve=tr.OFF, flags=tr.AUTO), S(percentile=1001),
           S(exposure=0.0), S(exposure=-1.0), S(exposure=nan), S(exposure=inf), S(white=-1.0), S(white=nan), S(white=inf),
           S(key=-0.1), S(key=nan), S(key=inf), S(flags=tr.AUTO, key=0.0), S(adapt=nan), S(adapt=-0.5), S(flags=tr.AUTO, adapt=0.0),
           S(flags=tr.AUTO, adapt=1.0001), S(flags=tr.AUTO, adapt=inf), S(min_auto=-1.0), S(min_auto=nan), S(max_auto=inf), S(max_auto=-2.0),
           S(min_auto=2.0, max_auto=1.0)]
    for s in bad:
        assert _set(gpu, s) == _ffi.VRT_ERR_INVALID_ARG, s
        assert _ffi.vrt().vrt_last_error(gpu._h)
    for k in range(3):
        o = S().ffi()
        o._reserved[k] = 1
        assert _set(gpu, o) == _ffi.VRT_ERR_INVALID_ARG
    assert _ffi.vrt().vrt_set_tone_map(None, C.byref(kept.ffi())) == _ffi.VRT_ERR_INVALID_ARG
    gpu.render(MODE_PATH, seed=SEED)   # the setting is still `kept`
    rgb, _, _ = gpu.read_output()
    assert np.array_equal(gpu.present(), orc.present(tr.tone(rgb, kept, kept.exposure), tc.MAIN))
    assert same(gpu.tone_info().exposure, kept.exposure)
    gpu.close()
    for kw in (dict(shard_rank=0, shard_count=2), dict(tile_major=True)):
        shard = gpu_for_scene(sc, **kw)
        assert _set(shard, S()) == _ffi.VRT_ERR_STATE and _set(shard, S(flags=tr.AUTO)) == _ffi.VRT_ERR_STATE
        assert _set(shard, S(curve=tr.OFF)) == _ffi.VRT_OK and _set(shard, None) == _ffi.VRT_OK
        assert _set(shard, S(curve=9)) == _ffi.VRT_ERR_INVALID_ARG
        shard.close()
    group = Gpu(sc.world.max_nodes(), sc.world.size_in_chunks(), sc.size, devices=[0, 0], texel_messages=True)
    assert _set(group, S()) == _ffi.VRT_ERR_STATE and _set(group, None) == _ffi.VRT_OK and _set(group, S(curve=tr.OFF)) == _ffi.VRT_OK
    for fn in (group.tone_info, group.tone_histogram):
        with pytest.raises(VrtError) as e:
            fn()
        assert e.value.code == _ffi.VRT_ERR_STATE
    group.close()
