"""The path trace's denoiser on the GPU (vrt_set_denoise, include/vrt.h) against tests/denoise_ref.c.

The guide words are the oracle's primary march's, bit for bit.  A denoised frame is the reference filter applied to the very
frame the same context renders with denoising off (same seed, spp, settings) and the oracle's guide: radiance bit for bit (a NaN
only where the reference has a NaN, channel by channel, its sign and payload aside: tests/test_denoise_ref.py says why), id
words untouched.  Off is off; accumulation keeps its identity."""
import functools
import os
import sys

import numpy as np
import pytest

import denoise_ref
from voxelraytracing_amd import MODE_PATH, MODE_PRIMARY, MODE_PRIMARY_SHADOW, Gpu, VrtError, _ffi, scenes
from voxelraytracing_amd import graphics as g

from util import gpu_for_scene

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_wgsl_fixtures as mk   # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 11
HIT, NX, NY, NZ = _ffi.ID_HIT, _ffi.ID_NX, _ffi.ID_NY, _ffi.ID_NZ


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return denoise_ref.load(tmp_path_factory.mktemp("denoise_ref"))


@functools.lru_cache(maxsize=None)
def c4(size, bounces=4):
    return scenes.c4(size, bounces=bounces)


def same_bits(a, b):
    return bool(np.all((denoise_ref.bits(a) == denoise_ref.bits(b)) | (np.isnan(a) & np.isnan(b))))


def frame(gpu, passes, sigma=0.0, spp=1, seed=SEED, **kw):
    gpu.set_denoise(passes, sigma)
    gpu.render(MODE_PATH, spp=spp, seed=seed, **kw)
    rgb, ids, _ = gpu.read_output()
    return rgb, ids


def check_denoised(ref, gpu, o, size, passes, sigma, spp=1, what=""):
    """Off, then on: the denoised frame is the reference filter over the raw one."""
    w, h = size
    raw, ids = frame(gpu, 0, spp=spp)
    got, got_ids = frame(gpu, passes, sigma, spp=spp)
    guide = gpu.read_guide()
    want_guide, want_ids = ref.guide(o, w, h)
    assert np.array_equal(ids, want_ids) and np.array_equal(got_ids, ids), f"{what}: id words"
    bad = np.argwhere(guide != want_guide)
    assert bad.size == 0, f"{what}: {len(bad)} guide words differ from the oracle's, first at (y, x) = {tuple(bad[0])}"
    want = ref.denoise(raw, ids, want_guide, passes, sigma)
    diff = denoise_ref.bits(got) != denoise_ref.bits(want)
    assert same_bits(got, want), f"{what}: {int(diff.sum())} radiance words differ from the reference filter's, max {np.nanmax(np.abs(got - want))}"
    filterable = ((ids & HIT) != 0) & ((ids & (NX | NY | NZ)) != 0)
    assert not np.array_equal(denoise_ref.bits(got)[filterable], denoise_ref.bits(raw)[filterable]), f"{what}: nothing was filtered"
    return raw, got, ids


# ---- the guide ----
def _inside_a_solid():
    sc = scenes.c2((64, 40))
    x, z = int(sc.eye[0]), int(sc.eye[2])
    from voxelraytracing_amd.world import gen_height
    eye = (x + 0.5, float(gen_height(1, x, z) - 3) + 0.5, z + 0.5)
    sc.cam = g.cam_data_create(sc.rot, eye, 70.0, (64.0, 40.0))
    return sc


GUIDE_SCENES = {
    "c1": lambda: scenes.c1_flat((256, 256)),
    "c2_640x360": lambda: scenes.c2((640, 360)),
    "water": lambda: mk.case_scene("c2_water_40x24")[0],
    "underwater": lambda: mk.case_scene("c2_underwater_24x16")[0],
    "inside_a_solid": _inside_a_solid,
}


@pytest.mark.parametrize("name", sorted(GUIDE_SCENES))
def test_the_guide_is_the_oracles(ref, orc, name):
    sc = GUIDE_SCENES[name]()
    w, h = sc.size
    gpu = gpu_for_scene(sc)
    gpu.set_denoise(1)
    gpu.render(MODE_PATH, seed=SEED)
    _, ids, _ = gpu.read_output()
    guide = gpu.read_guide()
    want, want_ids = ref.guide(orc.from_package_scene(sc), w, h)
    assert np.array_equal(ids, want_ids)
    assert np.array_equal(guide, want), f"{name}: {int((guide != want).sum())} guide words differ"
    if name == "inside_a_solid":
        assert (((ids & HIT) != 0) & ((ids & (NX | NY | NZ)) == 0)).all() and not guide.any()   # hits without a normal: guide 0
    else:
        assert (guide != 0).any()   # (the underwater camera sees a dozen faces, the others thousands)
    gpu.close()


# ---- the filter ----
@pytest.mark.parametrize("spp,passes,sigma", [(1, 5, 0.0), (4, 4, 0.5)])
def test_c4_at_full_size(ref, orc, spp, passes, sigma):
    sc = c4((1920, 1080))
    gpu = gpu_for_scene(sc)
    check_denoised(ref, gpu, orc.from_package_scene(sc), sc.size, passes, sigma, spp=spp, what=f"C4 {spp} spp, {passes} passes, sigma {sigma}")
    gpu.close()


@pytest.mark.parametrize("sigma", [0.0, 0.35])
@pytest.mark.parametrize("size", [(480, 272), (100, 60)])   # (100 x 60: neither a multiple of 8, the traced area is 96 x 56)
def test_every_number_of_passes_and_both_sigma_modes(ref, orc, size, sigma):
    sc = c4(size)
    gpu = gpu_for_scene(sc)
    o = orc.from_package_scene(sc)
    for passes in (1, 2, 3, 4, 5):
        raw, got, _ = check_denoised(ref, gpu, o, size, passes, sigma, what=f"{size} passes {passes} sigma {sigma}")
        if size == (100, 60):   # beyond the traced area: zeros, before and after
            assert not got[56:].any() and not got[:, 96:].any() and not raw[56:].any()
    gpu.close()


def test_a_band_of_c5s_shape(ref, orc):
    sc = scenes.c5((3840, 16), bounces=4, chunks=32)
    gpu = gpu_for_scene(sc)
    check_denoised(ref, gpu, orc.from_package_scene(sc), sc.size, 5, 0.35, spp=16, what="3840 x 16 of C5's world, 16 spp")
    gpu.close()


def test_with_emission(ref, orc):
    """(The table's reference is its own tests'; here the filter over whatever the frame holds.)"""
    sc = c4((256, 144))
    gpu = gpu_for_scene(sc)
    raw0, ids0 = frame(gpu, 0)
    vox = ids0[(ids0 & HIT) != 0] & _ffi.ID_VOXEL_MASK
    table = np.zeros(256, np.float32)
    table[int(np.bincount(vox).argmax())] = 2.5
    gpu.write_emission(table)
    for spp in (1, 3):
        raw, _, _ = check_denoised(ref, gpu, orc.from_package_scene(sc), sc.size, 3, 0.35, spp=spp, what=f"emission, {spp} spp")
    assert not np.array_equal(raw0, frame(gpu, 0)[0])   # (the table is in the frame)
    gpu.close()


@pytest.mark.parametrize("in_flight", [1, 2])
def test_back_to_back_frames_of_a_moving_camera(ref, orc, in_flight):
    """Frames enqueued back to back, each with its own camera, read one by one afterwards in a second run: a denoised frame in
    flight is the filter over that frame's own raw image, whichever frame set traced it."""
    size = (256, 144)
    sc = c4(size)
    o = orc.from_package_scene(sc)
    gpu = gpu_for_scene(sc)
    gpu.set_frames_in_flight(in_flight)
    cams = [g.cam_data_create((sc.rot[0] + 0.7 * k, sc.rot[1] + 2.0 * k, 0.0), (sc.eye[0] + 0.3 * k, sc.eye[1], sc.eye[2]), 70.0,
                              (float(size[0]), float(size[1]))) for k in range(5)]
    raws = []
    gpu.set_denoise(0)
    for cam in cams:
        gpu.write_cam_data(cam)
        gpu.render(MODE_PATH, seed=SEED)
        raws.append(gpu.read_output()[:2])
    gpu.set_denoise(4, 0.35)
    for last in range(len(cams)):
        for cam in cams[:last + 1]:   # back to back, nothing read in between
            gpu.write_cam_data(cam)
            gpu.render(MODE_PATH, seed=SEED)
        got, ids, _ = gpu.read_output()
        guide = gpu.read_guide()
        o.set_cam(cams[last])
        want_guide, want_ids = ref.guide(o, *size)
        assert np.array_equal(ids, want_ids) and np.array_equal(ids, raws[last][1]) and np.array_equal(guide, want_guide)
        assert same_bits(got, ref.denoise(raws[last][0], ids, want_guide, 4, 0.35)), f"in flight {in_flight}: frame {last} of a burst"
    o.set_cam(sc.cam)
    gpu.close()


def test_present_shows_the_filtered_image(orc):
    sc = c4((256, 144))
    gpu = gpu_for_scene(sc)
    raw, _ = frame(gpu, 0)
    shown_raw = gpu.present()
    got, _ = frame(gpu, 5, 0.0)
    shown = gpu.present()
    assert np.array_equal(shown, orc.present(got, sc.size)) and not np.array_equal(shown, shown_raw)
    ptr, nbytes = gpu.device_output()
    assert ptr and nbytes == 256 * 144 * 16
    gpu.close()


# ---- accumulation ----
@pytest.mark.parametrize("in_flight", [1, 2])
def test_accumulated_denoised_frames_are_one_denoised_frame_of_all_the_samples(in_flight):
    sc = c4((256, 144))
    gpu = gpu_for_scene(sc)
    gpu.set_frames_in_flight(in_flight)
    want = {n: frame(gpu, 3, 0.35, spp=n) for n in (4, 6)}
    plain6 = frame(gpu, 0, spp=6)
    gpu.set_denoise(3, 0.35)
    for _ in range(4):
        gpu.render(MODE_PATH, spp=1, seed=SEED, accumulate=True)
    rgb, ids, _ = gpu.read_output()
    assert np.array_equal(ids, want[4][1]) and same_bits(rgb, want[4][0])
    assert gpu.accumulation() == (4, SEED)
    # toggling the setting between frames does not restart the sum: off for a frame (the plain mean), then on again
    gpu.set_denoise(0)
    gpu.render(MODE_PATH, spp=1, seed=SEED, accumulate=True)
    assert gpu.accumulation() == (5, SEED)
    gpu.set_denoise(3, 0.35)
    gpu.render(MODE_PATH, spp=1, seed=SEED, accumulate=True)
    rgb, ids, _ = gpu.read_output()
    assert gpu.accumulation() == (6, SEED)
    assert same_bits(rgb, want[6][0]) and not same_bits(rgb, plain6[0])
    gpu.set_denoise(0)
    gpu.reset_accumulation()
    for spp in (2, 4):
        gpu.render(MODE_PATH, spp=spp, seed=SEED, accumulate=True)
    assert same_bits(gpu.read_output()[0], plain6[0])   # (and the sum itself was never filtered)
    gpu.close()


# ---- off is off ----
def test_off_is_off():
    sc = c4((200, 104))

    def frames(setup):
        gpu = gpu_for_scene(sc)
        setup(gpu)
        out = []
        for mode in (MODE_PATH, MODE_PRIMARY, MODE_PRIMARY_SHADOW):
            gpu.render(mode, seed=SEED)
            out.append(gpu.read_output()[:2])
        return gpu, out

    lib = _ffi.vrt()
    never, a = frames(lambda gpu: None)
    null, b = frames(lambda gpu: gpu._ck(lib.vrt_set_denoise(gpu._h, None)))
    zero, c = frames(lambda gpu: gpu.set_denoise(0, 0.7))
    for x, y, z in zip(a, b, c):
        for other in (y, z):
            assert np.array_equal(x[1], other[1]) and np.array_equal(denoise_ref.bits(x[0]), denoise_ref.bits(other[0]))
    for gpu in (never, null, zero):
        with pytest.raises(VrtError) as e:
            gpu.read_guide()   # nothing was made for a frame that is not denoised
        assert e.value.code == _ffi.VRT_ERR_STATE
    # a primary frame rendered while denoising is on is the live shader's bytes
    zero.set_denoise(5, 0.0)
    zero.render(MODE_PATH, seed=SEED)
    assert not np.array_equal(denoise_ref.bits(zero.read_output()[0]), denoise_ref.bits(a[0][0]))
    for mode, want in ((MODE_PRIMARY, a[1]), (MODE_PRIMARY_SHADOW, a[2])):
        zero.render(mode, seed=SEED)
        rgb, ids, _ = zero.read_output()
        assert np.array_equal(ids, want[1]) and np.array_equal(denoise_ref.bits(rgb), denoise_ref.bits(want[0]))
    for gpu in (never, null, zero):
        gpu.close()


# ---- refusals ----
def _refused(gpu, opts, code):
    rc = _ffi.vrt().vrt_set_denoise(gpu._h, None if opts is None else _ffi.C.byref(opts))
    assert rc == code, (rc, code)
    if code:
        assert _ffi.vrt().vrt_last_error(gpu._h)


def test_refusals_change_nothing(ref, orc):
    sc = c4((128, 72))
    gpu = gpu_for_scene(sc)
    with pytest.raises(VrtError) as e:
        gpu.read_guide()
    assert e.value.code == _ffi.VRT_ERR_STATE
    want = frame(gpu, 2, 0.35)
    D = _ffi.DenoiseOpts
    for opts in (D(6, 0.0, 0, 0), D(2, -1.0, 0, 0), D(2, float("nan"), 0, 0), D(2, float("inf"), 0, 0), D(2, 0.5, 1, 0), D(2, 0.5, 0, 1),
                 D(0, 0.0, 2, 0)):
        _refused(gpu, opts, _ffi.VRT_ERR_INVALID_ARG)
    gpu.render(MODE_PATH, seed=SEED)   # the setting is still (2, 0.35)
    rgb, ids, _ = gpu.read_output()
    assert np.array_equal(ids, want[1]) and same_bits(rgb, want[0])
    gpu.close()
    for kw in (dict(shard_rank=0, shard_count=2), dict(tile_major=True)):
        shard = gpu_for_scene(sc, **kw)
        _refused(shard, D(2, 0.0, 0, 0), _ffi.VRT_ERR_STATE)
        _refused(shard, D(0, 0.0, 0, 0), _ffi.VRT_OK)
        _refused(shard, None, _ffi.VRT_OK)
        shard.close()
    group = Gpu(sc.world.max_nodes(), sc.world.size_in_chunks(), sc.size, devices=[0, 0], texel_messages=True)
    _refused(group, D(2, 0.0, 0, 0), _ffi.VRT_ERR_STATE)
    _refused(group, None, _ffi.VRT_OK)
    with pytest.raises(VrtError) as e:
        group.read_guide()
    assert e.value.code == _ffi.VRT_ERR_STATE
    group.close()
