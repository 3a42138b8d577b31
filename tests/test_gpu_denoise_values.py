"""The five pass kernels of vrt_set_denoise (csrc/vrt_denoise.hip: denoise_pass_lds_kernel<1, 2>, denoise_pass_kernel<4, 8, 16>) on
frames nobody rendered: tests/denoise_cases.py's crafted frames through vrt_selftest_denoise — the launcher, the tap spacings and
the sigma per pass of a frame — against tests/denoise_ref.c, for every size x frame x number of passes x sigma of the table.

What the kernels add to csrc/both/denoise_math.h (which tests/test_denoise_ref.py holds to the same reference on the host) is
what these frames aim at: the halo staged through LDS, the traced width and height against the frame's stride, the texels staged
as zeros beyond the traced area, the ragged last tile and last wave, and the device's divide on denormal and overflowing operands.

The rule is tests/test_denoise_ref.py's: the same binary32 bits in every channel of every pixel, except that where one side
holds a NaN the other must hold a NaN in that same channel, of whatever sign and payload.  Id words come back as they went in,
all 32 bits; a pixel no pass stores to comes back byte for byte, NaN payloads included."""
import ctypes as C

import numpy as np
import pytest

import denoise_cases as dc
import denoise_ref
from voxelraytracing_amd import MODE_PATH, VrtError, _ffi, scenes

from util import gpu_for_scene

pytestmark = pytest.mark.gpu

ALL_PASSES = [1, 2, 3, 4, 5]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return denoise_ref.load(tmp_path_factory.mktemp("denoise_ref"))


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (denoise_ref.bits(a) == denoise_ref.bits(b)) | (np.isnan(a) & np.isnan(b))


def where_it_lies(x, y, w, h, passes):
    """'within 2S of ...' for the widest pass that ran: what a failure message says about the first differing pixel."""
    reach = 2 << (passes - 1)
    d = dc.border_distances(x, y, w, h)
    near = [f"{k} border ({v} px)" if k != "edge" else f"the traced area's edge ({v} px)" for k, v in d.items() if 0 <= v < reach]
    return f"within 2S = {reach} px of " + ", ".join(near) if near else f"not within 2S = {reach} px of a tile border, a wave border or the traced area's edge"


def compare(ref, name, size, rgb, ids, guide, passes, sigma):
    """None, or what differs between vrt_selftest_denoise and the reference on this case."""
    w, h = size
    got, got_ids = _ffi.selftest_denoise(rgb, ids, guide, passes, sigma)
    want = ref.denoise(rgb, ids, guide, passes, sigma)
    case = f"{name} {w} x {h}, passes {passes}, sigma {sigma}"
    if not np.array_equal(got_ids, ids):
        y, x = (int(v) for v in np.argwhere(got_ids != ids)[0])
        return f"{case}: {int((got_ids != ids).sum())} id words changed, first at (x, y) = ({x}, {y}): {int(ids[y, x]):#010x} -> {int(got_ids[y, x]):#010x}"
    stored = dc.filtered_mask(ids)
    kept = denoise_ref.bits(got)[~stored] == denoise_ref.bits(rgb)[~stored]
    if not kept.all():
        y, x = (int(v) for v in np.argwhere(~stored & (denoise_ref.bits(got) != denoise_ref.bits(rgb)).any(axis=2))[0])
        return (f"{case}: {int((~kept).sum())} words of pixels no pass filters (beyond the traced area, or not filterable) changed, first at "
                f"(x, y) = ({x}, {y}); {where_it_lies(x, y, w, h, passes)}")
    ok = same_bits(got, want)
    if not ok.all():
        y, x = (int(v) for v in np.argwhere(~ok.all(axis=2))[0])
        return (f"{case}: {int((~ok).sum())} colour words differ from the reference, first at (x, y) = ({x}, {y}): got {got[y, x]} "
                f"({[hex(int(v)) for v in denoise_ref.bits(got[y, x])]}), want {want[y, x]} ({[hex(int(v)) for v in denoise_ref.bits(want[y, x])]}); "
                f"{where_it_lies(x, y, w, h, passes)}")
    return None


def run_cases(ref, size, sigmas):
    """Every frame of the table at `size` under `sigmas`: for each (frame, sigma) the first number of passes that fails."""
    failures, n = [], 0
    for name in dc.FRAMES:
        rgb, ids, guide = dc.frame(name, size)
        for sigma in sigmas:
            for passes in ALL_PASSES:
                n += 1
                bad = compare(ref, name, size, rgb, ids, guide, passes, sigma)
                if bad:
                    failures.append(f"{bad} [the first number of passes at which this frame and sigma fail: {passes}]")
                    break
    assert not failures, f"{len(failures)} of {len(dc.FRAMES) * len(sigmas)} frame x sigma cases differ; the first three:\n" + "\n".join(failures[:3])
    return n


@pytest.mark.parametrize("size", dc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_pass_kernels_are_the_reference_on_every_crafted_frame(ref, size):
    assert run_cases(ref, size, dc.SIGMAS) == len(dc.FRAMES) * len(dc.SIGMAS) * 5


@pytest.mark.parametrize("size", dc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_sigma_that_underflows_or_overflows_leaves_nans_and_nothing_else(ref, size):
    """Sigma 1e-30 (sg2 = 0, the centre tap's weight 0 / 0) and 2e19 (sg2 = inf): every channel the reference filters is NaN
    (tests/test_denoise_cases.py proves it), so the kernels must hold a NaN in every one of them — and the bytes of every other pixel."""
    run_cases(ref, size, dc.EXTREME_SIGMAS)
    rgb, ids, guide = dc.frame("random_finite", size)
    got, _ = _ffi.selftest_denoise(rgb, ids, guide, 5, dc.EXTREME_SIGMAS[0])
    assert np.isnan(got[dc.filtered_mask(ids)]).all()


def test_no_passes_and_no_traced_area_return_the_input(ref):
    for name in dc.FRAMES:
        rgb, ids, guide = dc.frame(name, (76, 44))
        got, got_ids = _ffi.selftest_denoise(rgb, ids, guide, 0, 0.35)
        assert np.array_equal(denoise_ref.bits(got), denoise_ref.bits(rgb)) and np.array_equal(got_ids, ids), name
        rgb, ids, guide = dc.frame(name, dc.NO_TRACED_AREA)
        for passes in [0] + ALL_PASSES:
            got, got_ids = _ffi.selftest_denoise(rgb, ids, guide, passes, 0.35)
            assert np.array_equal(denoise_ref.bits(got), denoise_ref.bits(rgb)) and np.array_equal(got_ids, ids), (name, passes)
    # the bytes of a NaN with a payload, inside the traced area (a pixel that is not filterable) and beyond it
    rgb, ids, guide = dc.frame("random_finite", (76, 44))
    odd = np.array([0x7FC12345, 0xFFA00001, 0x7F800001], np.uint32).view(np.float32)
    sky = np.argwhere(~dc.filterable(ids)[:40, :72])[0]
    rgb[sky[0], sky[1]] = odd
    rgb[43, 75] = odd
    rgb[10, 73] = odd
    got, _ = _ffi.selftest_denoise(rgb, ids, guide, 5, 0.35)
    for y, x in ((sky[0], sky[1]), (43, 75), (10, 73)):
        assert np.array_equal(denoise_ref.bits(got[y, x]), denoise_ref.bits(odd)), (y, x)
    assert compare(ref, "random_finite with NaN payloads", (76, 44), rgb, ids, guide, 5, 0.35) is None


def test_refusals_and_a_null_ids_out(ref):
    lib = _ffi.vrt()
    w, h = 40, 24
    rgb, ids, guide = dc.frame("random_finite", (w, h))
    out = np.full_like(rgb, 7.0)
    ids_out = np.full_like(ids, 7)
    D = _ffi.DenoiseOpts
    p = lambda a: a.ctypes.data
    good = D(2, 0.35, 0, 0)

    def call(rgb_p=p(rgb), ids_p=p(ids), guide_p=p(guide), w=w, h=h, opts=good, out_p=p(out), ids_out_p=p(ids_out)):
        return lib.vrt_selftest_denoise(0, rgb_p, ids_p, guide_p, w, h, None if opts is None else C.byref(opts), out_p, ids_out_p)

    for opts in (D(6, 0.0, 0, 0), D(2, -1.0, 0, 0), D(2, float("nan"), 0, 0), D(2, float("inf"), 0, 0), D(2, 0.5, 1, 0), D(2, 0.5, 0, 1), D(0, 0.0, 2, 0)):
        assert call(opts=opts) == _ffi.VRT_ERR_INVALID_ARG, (opts.passes, opts.sigma_color, opts.flags, opts._reserved)
    for kw in (dict(rgb_p=None), dict(ids_p=None), dict(guide_p=None), dict(opts=None), dict(out_p=None), dict(w=0), dict(h=0)):
        assert call(**kw) == _ffi.VRT_ERR_INVALID_ARG, kw
    assert call(w=4097, h=4096) == _ffi.VRT_ERR_OUT_OF_RANGE     # w * h above 2^24 (refused before a byte of the arrays is read)
    assert call(w=1 << 16, h=1 << 16) == _ffi.VRT_ERR_OUT_OF_RANGE
    assert (out == 7.0).all() and (ids_out == 7).all()           # a refused call writes nothing
    with pytest.raises(VrtError) as e:
        _ffi.selftest_denoise(rgb, ids, guide, 6, 0.0)
    assert e.value.code == _ffi.VRT_ERR_INVALID_ARG
    # ids_out may be NULL
    assert call(ids_out_p=None) == _ffi.VRT_OK
    assert same_bits(out, ref.denoise(rgb, ids, guide, 2, 0.35)).all() and (ids_out == 7).all()
    assert call() == _ffi.VRT_OK and np.array_equal(ids_out, ids)


def test_the_entry_point_launches_what_a_frame_launches():
    """Dispatch: a 76 x 44 path frame rendered raw, then denoised by its context; vrt_selftest_denoise over the raw frame's texels,
    id words and the context's guide is that denoised frame — for every number of passes, with and without a colour stop."""
    size = (76, 44)
    sc = scenes.c4(size, bounces=4)
    gpu = gpu_for_scene(sc)
    gpu.set_denoise(0)
    gpu.render(MODE_PATH, seed=11)
    raw, ids, _ = gpu.read_output()
    assert dc.filtered_mask(ids).sum() > 500
    for sigma in (0.0, 0.35):
        for passes in ALL_PASSES:
            gpu.set_denoise(passes, sigma)
            gpu.render(MODE_PATH, seed=11)
            want, want_ids, _ = gpu.read_output()
            guide = gpu.read_guide()
            got, got_ids = _ffi.selftest_denoise(raw, ids, guide, passes, sigma)
            assert np.array_equal(want_ids, ids) and np.array_equal(got_ids, ids)
            assert same_bits(got, want).all(), f"passes {passes} sigma {sigma}: {int((~same_bits(got, want)).sum())} words differ from the context's frame"
            assert not np.array_equal(denoise_ref.bits(got), denoise_ref.bits(raw))
    gpu.close()
