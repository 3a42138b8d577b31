"""What keeps tests/test_gpu_tone.py from being vacuous, held to the CPU path reference (tests/sun_ref.py: the oracle's path loop
with the sun term and the emission table): the main scene's luminance histogram is spread out and counts most of the frame, and
the two views the adaptation test alternates between meter exposures far apart."""
import numpy as np
import pytest

import sun_ref
import tone_cases as tc
import tone_ref as tr


@pytest.fixture(scope="module")
def sref(tmp_path_factory):
    return sun_ref.load(tmp_path_factory.mktemp("sun_ref"))


def test_the_main_scene_spans_many_bins_and_counts_most_pixels(orc, sref):
    sc = tc.scene(tc.MAIN)
    rgb, _ = sref.render(orc.from_package_scene(sc), tc.SUN, *tc.MAIN, spp=1, seed=tc.SEED, emission=tc.emission_table())
    info, bins = tr.meter(rgb, tr.Setting(flags=tr.AUTO))
    assert int((bins > 0).sum()) >= 8, "the histogram occupies fewer than 8 bins"
    assert info.counted >= tc.MAIN[0] * tc.MAIN[1] // 2, "fewer than half the traced pixels are counted"
    lum = tr.luminance(rgb)
    assert np.log2(lum[lum > 0].max() / lum[lum > 0].min()) >= 4.0, "the radiance spans fewer than four octaves"


def test_the_two_views_of_the_adaptation_test_meter_far_apart(orc, sref):
    sc = tc.scene(tc.MAIN)
    o = orc.from_package_scene(sc)
    targets = []
    for pitch in (tc.SKY_PITCH, tc.DOWN_PITCH):
        o.set_cam(tc.view(sc, pitch, tc.MAIN))
        rgb, _ = sref.render(o, tc.SUN, *tc.MAIN, spp=1, seed=tc.SEED, emission=tc.emission_table())
        info, _ = tr.meter(rgb, tr.Setting(flags=tr.AUTO))
        assert info.counted > 0
        targets.append(float(info.target))
    o.set_cam(sc.cam)
    assert max(targets) / min(targets) >= 2.0, targets
