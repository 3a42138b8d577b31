"""tests/denoise_cases.py — the crafted frames the GPU's pass kernels are held to (tests/test_gpu_denoise_values.py) — proved from
tests/denoise_ref.c alone to be what they claim: comparable by value (few or no NaNs), not vacuous (the filter changes them), and
each reaching the edge it is there for.  The host twin vrth_denoise is held to the reference on every one of them too.  No GPU."""
import numpy as np
import pytest

import denoise_cases as dc
import denoise_ref
from voxelraytracing_amd import _ffi

ALL_PASSES = [1, 2, 3, 4, 5]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return denoise_ref.load(tmp_path_factory.mktemp("denoise_ref"))


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(np.all((denoise_ref.bits(a) == denoise_ref.bits(b)) | (np.isnan(a) & np.isnan(b))))


def test_the_table_gives_the_same_frame_every_time_and_every_frame_its_size():
    for size in dc.SIZES + [dc.NO_TRACED_AREA]:
        for name in dc.FRAMES:
            a, b = dc.frame(name, size), dc.frame(name, size)
            assert a[0].shape == (size[1], size[0], 3) and a[1].shape == a[2].shape == (size[1], size[0])
            assert a[0].dtype == np.float32 and a[1].dtype == a[2].dtype == np.uint32
            assert all(np.array_equal(denoise_ref.bits(x) if x.dtype == np.float32 else x, denoise_ref.bits(y) if y.dtype == np.float32 else y)
                       for x, y in zip(a, b))


def test_the_default_share_of_special_colours_is_the_host_tests_generator():
    """random_frame's new parameter leaves the frames of tests/test_denoise_ref.py what they were: at the default the thresholds
    are the literals 0.03 .. 0.08, and the sparse share draws the same stream of random numbers."""
    a = dc.random_frame(np.random.default_rng(5), 52, 30)
    b = dc.random_frame(np.random.default_rng(5), 52, 30, share=dc.SPECIAL_SHARE)
    c = dc.random_frame(np.random.default_rng(5), 52, 30, share=dc.SPARSE_SHARE)
    assert np.array_equal(denoise_ref.bits(a[0]), denoise_ref.bits(b[0])) and np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2])
    odd = lambda rgb: float((~np.isfinite(rgb) | (rgb == 0) | (rgb == np.float32(1e-41)) | (rgb == np.float32(3e38))).mean())
    assert 0.06 < odd(a[0]) < 0.10 and 0.001 < odd(c[0]) < 0.008


@pytest.mark.parametrize("size", dc.SIZES + [dc.NO_TRACED_AREA])
def test_the_host_entry_point_is_the_reference_on_every_case(ref, size):
    for name in dc.FRAMES:
        rgb, ids, guide = dc.frame(name, size)
        for sigma in dc.SIGMAS + dc.EXTREME_SIGMAS:
            for passes in [0] + ALL_PASSES:
                got, want = _ffi.denoise(rgb, ids, guide, passes, sigma), ref.denoise(rgb, ids, guide, passes, sigma)
                assert same_bits(got, want), f"{name} {size} passes {passes} sigma {sigma}"


@pytest.mark.parametrize("size", dc.SIZES)
def test_nans_stay_few_in_the_sparse_frame_and_absent_from_the_finite_ones(ref, size):
    """A channel that is NaN on both sides compares equal whatever the kernel did to it, so NaNs must be few: at most 10 % of
    random_sparse's filterable channels under every sigma of SIGMAS and every number of passes (at the generator's own 8 % of
    special colours it is most of them, which is why the GPU comparison does not use that frame), none at all in the frames of
    finite colours."""
    for name in dc.FRAMES:
        rgb, ids, guide = dc.frame(name, size)
        m = dc.filtered_mask(ids)
        for sigma in dc.SIGMAS:
            for passes in ALL_PASSES:
                share = float(np.isnan(ref.denoise(rgb, ids, guide, passes, sigma)[m]).mean())
                print(f"{name} {size} sigma {sigma} passes {passes}: {share:.1%} of the filterable channels NaN")
                if name == "random_sparse":
                    assert share <= 0.10, f"{size} sigma {sigma} passes {passes}: {share:.1%} (another seed in denoise_cases.SPARSE_SEEDS, not another cap)"
                else:
                    assert share == 0.0, f"{name} {size} sigma {sigma} passes {passes}"


@pytest.mark.parametrize("size", dc.SIZES)
def test_the_filter_changes_more_than_half_of_the_filterable_words(ref, size):
    """Not vacuous: under sigma 0, 0.35 and 4.0 more than half of the words the passes store differ from the input, in the frames
    where pixels have neighbours that agree at every size (a lattice of a spacing the frame is too small for has none)."""
    for name in ("random_sparse", "random_finite", "stripes", "one_surface", "lattice_1", "wrong_half"):
        rgb, ids, guide = dc.frame(name, size)
        m = dc.filtered_mask(ids)
        for sigma in (0.0, 0.35, 4.0):
            out = ref.denoise(rgb, ids, guide, 5, sigma)
            share = float((denoise_ref.bits(out)[m] != denoise_ref.bits(rgb)[m]).mean())
            print(f"{name} {size} sigma {sigma}: {share:.1%} of the filterable words change")
            assert share > 0.5, f"{name} {size} sigma {sigma}: {share:.1%}"


@pytest.mark.parametrize("size", [(76, 44), (136, 72)])
def test_every_lattice_is_filtered_by_its_own_pass(ref, size):
    """lattice(S): the pass of spacing S changes the lattice's pixels (they have up to 24 neighbours that agree)."""
    for s in dc.LATTICE_SPACINGS:
        rgb, ids, guide = dc.frame(f"lattice_{s}", size)
        m = dc.filtered_mask(ids) & (guide == 20)
        i = dc.LATTICE_SPACINGS.index(s)
        before = ref.denoise(rgb, ids, guide, i, 0.0)
        after = ref.denoise(rgb, ids, guide, i + 1, 0.0)
        assert (denoise_ref.bits(after)[m] != denoise_ref.bits(before)[m]).mean() > 0.9


@pytest.mark.parametrize("size", dc.SIZES)
def test_a_denormal_sigma_keeps_its_weights(ref, size):
    """Sigma 1e-20: sg2 = 1e-40 is a denormal.  A tap of the pixel's own colour weighs sg2 / (sg2 + 0) = 1, any other tap about
    1e-40 / d2 — a denormal or 0 —, so one_surface's zeros and 1e-41s (d2 underflows to 0 among them) average with each other and
    every other pixel keeps its colour within the rounding of (w c) / w.  A divide that flushed sg2 would give 0 / 0 at the centre
    tap and NaN everywhere: the reference has no NaN in the frames of finite colours, and at least 1 % of the words it filters
    differ from the input."""
    for name in dc.NO_NAN_FRAMES:
        rgb, ids, guide = dc.frame(name, size)
        m = dc.filtered_mask(ids)
        out = ref.denoise(rgb, ids, guide, 5, 1e-20)
        share = float((denoise_ref.bits(out)[m] != denoise_ref.bits(rgb)[m]).mean())
        print(f"{name} {size} sigma 1e-20: {share:.1%} of the filterable words change, {int(np.isnan(out[m]).sum())} NaN")
        assert not np.isnan(out[m]).any()
        assert share >= 0.01, f"{name} {size}: {share:.2%}"


@pytest.mark.parametrize("sigma", dc.EXTREME_SIGMAS)
def test_a_sigma_that_underflows_or_overflows_leaves_only_nans(ref, sigma):
    """Sigma 1e-30: sg2 underflows to 0 and the centre tap's weight is 0 / 0.  Sigma 2e19: sg2 overflows to infinity on pass 0 and
    every weight is inf / inf.  Either way EVERY channel the reference filters is NaN from the first pass on, whatever the frame —
    which is why the GPU must hold a NaN in every one of them and nothing else: a kernel that took a special path around a zero or
    infinite sg2 (a clamp, a flush, a reciprocal) would leave a number somewhere."""
    for size in dc.SIZES:
        for name in dc.FRAMES:
            rgb, ids, guide = dc.frame(name, size)
            m = dc.filtered_mask(ids)
            for passes in ALL_PASSES:
                out = ref.denoise(rgb, ids, guide, passes, sigma)
                assert np.isnan(out[m]).all(), f"{name} {size} passes {passes}"
                assert np.array_equal(denoise_ref.bits(out)[~m], denoise_ref.bits(rgb)[~m])


@pytest.mark.parametrize("sigma", [0.0, 0.35])
def test_one_surface_shows_a_tap_that_leaks_past_the_traced_area(ref, sigma):
    """one_surface at 76 x 44 (traced 72 x 40): the four columns and rows beyond the traced area agree with every pixel on key and
    guide and hold colours of 50 to 100.  The right answer is the filter over the frame cropped to 72 x 40; the reference over the
    whole frame gives exactly that and hands the pixels beyond back as given; and the same frame inside a traced area that covers
    them (zero-padded to 80 x 48) gives something else in more than 1 000 words of the 72 x 40 block — what a kernel that bounded
    its taps by the frame's width, or staged them into its halo, would return."""
    w, h = 76, 44
    rgb, ids, guide = dc.frame("one_surface", (w, h))
    assert dc.filterable(ids).all() and (guide == guide[0, 0]).all() and ((ids & dc.KEY_MASK) == (ids[0, 0] & dc.KEY_MASK)).all()
    assert float(rgb[40:].min()) >= 50.0 and float(rgb[:, 72:].min()) >= 50.0 and float(rgb[:40, :72].max()) < 3.0
    assert len(np.unique(ids >> 21)) > 100    # the bits outside the key differ from pixel to pixel
    right = ref.denoise(rgb[:40, :72], ids[:40, :72], guide[:40, :72], 5, sigma)
    whole = ref.denoise(rgb, ids, guide, 5, sigma)
    assert np.array_equal(denoise_ref.bits(whole[:40, :72]), denoise_ref.bits(right))
    beyond = np.ones((h, w), bool)
    beyond[:40, :72] = False
    assert np.array_equal(denoise_ref.bits(whole)[beyond], denoise_ref.bits(rgb)[beyond])
    pad = lambda a: np.pad(a, ((0, 4), (0, 4)) + ((0, 0),) * (a.ndim - 2))
    leaked = ref.denoise(pad(rgb), pad(ids), pad(guide), 5, sigma)
    differ = int((denoise_ref.bits(leaked[:40, :72]) != denoise_ref.bits(right)).sum())
    print(f"sigma {sigma}: {differ} of {40 * 72 * 3} words differ when the junk lies inside a traced area")
    assert differ > 1000


def test_every_lattice_has_taps_that_cross_tile_and_wave_borders():
    """lattice(S) at 136 x 72, the pass of spacing S, from keys and guides alone: taps accepted between pixels of different
    32 x 32 tiles (the LDS kernels' halo) and of different 64-pixel spans (another wave's pixels) exist for every S, and — S > 1 —
    every tap at a distance that is no multiple of S is refused."""
    for s in dc.LATTICE_SPACINGS:
        _, ids, guide = dc.frame(f"lattice_{s}", (136, 72))
        n = dc.tap_counts(ids, guide, s)
        print(f"lattice({s}) at 136 x 72: {n}")
        assert n["accepted_across_tiles"] > 0 and n["accepted_across_waves"] > 0
        if s > 1:
            half = dc.tap_counts(ids, guide, s // 2)
            on = ((np.arange(72)[:, None] % s == 0) & (np.arange(136)[None, :] % s == 0))
            assert int(on.sum()) == len(range(0, 136, s)) * len(range(0, 72, s))
            assert half["refused_inside"] + half["refused_across_tiles"] > 0


@pytest.mark.parametrize("size", [(76, 44), (136, 72)])
def test_wrong_half_ends_agreement_exactly_at_tile_and_wave_borders(size):
    """wrong_half: no tap between two pixels of one tile and one wave span is refused, and taps are refused between tiles and
    between wave spans in every pass — only because of the border."""
    _, ids, guide = dc.frame("wrong_half", size)
    for s in dc.LATTICE_SPACINGS:
        n = dc.tap_counts(ids, guide, s)
        print(f"wrong_half {size} spacing {s}: {n}")
        assert n["refused_inside"] == 0
        assert n["refused_across_tiles"] > 0 and n["refused_across_waves"] > 0
