"""Emissive materials in the path trace (vrt_write_emission, include/vrt.h) on the GPU.

Against tests/emission_ref.py (the oracle's path loop with path_tracer.wgsl's emission term) for every variant, sample count and
frames in flight; a table of zeros renders exactly as no table; emission only adds light; accumulated emissive frames are one
frame of all their samples, bit for bit; what restarts the sum and what is refused; shards and devices."""
import numpy as np
import pytest

import emission_ref
from emission_cases import _table
from voxelraytracing_amd import MODE_PATH, MODE_PRIMARY, MODE_PRIMARY_SHADOW, VrtError, _ffi, scenes

from util import assert_frame_parity, gpu_for_scene

pytestmark = pytest.mark.gpu

SEED = 11


@pytest.fixture(scope="module")
def eref(tmp_path_factory):
    return emission_ref.load(tmp_path_factory.mktemp("emission_ref"))


def _frame(gpu, spp, seed=SEED, **kw):
    gpu.render(MODE_PATH, spp=spp, seed=seed, **kw)
    rgb, ids, _ = gpu.read_output()
    return rgb, ids


def _acc(gpu, spp, seed=SEED, **kw):
    return _frame(gpu, spp, seed=seed, accumulate=True, **kw)


def _same(a, b, what):
    assert np.array_equal(a[1], b[1]), f"{what}: id words differ"
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f"{what}: radiance differs (max {np.abs(a[0] - b[0]).max()})"


_refs = {}


def _ref(eref, orc, sc, table, spp):
    key = (sc.size, spp, table.tobytes(), sc.materials[0].is_liquid)
    if key not in _refs:
        _refs[key] = eref.render(orc.from_package_scene(sc), table, sc.size[0], sc.size[1], spp=spp, seed=SEED)
    return _refs[key]


# The path trace has one kernel variant (vrt_render_opts.variant 0) and four routes through its kernels: the pool kernel over
# the march cells (plain frames), the lane = path bounce kernel (VRT_PATH_POOL=0), the literal march (air flagged liquid) and
# the counting kernels of a stats frame.
ROUTES = ["cells", "lane", "literal", "stats"]


@pytest.mark.parametrize("size", [(128, 72), (100, 60)])
@pytest.mark.parametrize("route", ROUTES)
def test_emissive_frames_match_the_reference(eref, orc, monkeypatch, size, route):
    if route == "lane":
        monkeypatch.setenv("VRT_PATH_POOL", "0")   # (read when the context is created)
    sc = scenes.c4(size)
    if route == "literal":
        sc.materials[0].is_liquid = 1
    gpu = gpu_for_scene(sc)
    table = _table(gpu)
    gpu.write_emission(table)
    for in_flight in (1, 2):
        gpu.set_frames_in_flight(in_flight)
        for spp in (1, 3, 8, 12):
            rgb, ids = _frame(gpu, spp, stats=route == "stats")
            r_rgb, r_ids = _ref(eref, orc, sc, table, spp)
            assert_frame_parity(rgb, ids, r_rgb, r_ids, f"{size} {route} in flight {in_flight} spp {spp}")
    # (the table is not a no-op here: the reference with it is not the plain path trace)
    plain, _, _, _ = orc.from_package_scene(sc).render(orc.MODE_PATH, size[0], size[1], spp=3, seed=SEED)
    assert (_ref(eref, orc, sc, table, 3)[0] > plain + 1e-3).sum() > 100
    gpu.close()


def test_one_sample_per_chain_matches_the_reference(eref, orc, monkeypatch):
    monkeypatch.setenv("VRT_PATH_SAMPLES_PER_CHAIN", "1")   # (read when the context is created)
    sc = scenes.c4((128, 72))
    gpu = gpu_for_scene(sc)
    table = _table(gpu)
    gpu.write_emission(table)
    for spp in (1, 3, 8, 12):
        rgb, ids = _frame(gpu, spp)
        r_rgb, r_ids = _ref(eref, orc, sc, table, spp)
        assert_frame_parity(rgb, ids, r_rgb, r_ids, f"one sample per chain, spp {spp}")
    # ... and the stats frames, which take the one-sample route whatever the setting
    rgb, ids = _frame(gpu, 3, stats=True)
    assert_frame_parity(rgb, ids, *_ref(eref, orc, sc, table, 3), "stats frame, 3 spp")
    gpu.close()


def _all_modes(gpu):
    out = {}
    for spp in (1, 3, 12):
        out[("path", spp)] = _frame(gpu, spp)
    out[("path stats", 3)] = _frame(gpu, 3, stats=True)
    for name, mode in (("primary", MODE_PRIMARY), ("primary+shadow", MODE_PRIMARY_SHADOW)):
        gpu.render(mode)
        rgb, ids, _ = gpu.read_output()
        out[(name, 1)] = (rgb, ids)
    return out


def test_a_table_of_zeros_is_no_table():
    sc = scenes.c4((128, 72))
    never = gpu_for_scene(sc)
    table = _table(never)
    want = _all_modes(never)
    never.close()
    zeros = gpu_for_scene(sc)
    zeros.write_emission(np.zeros(256, np.float32))
    back = gpu_for_scene(sc)
    back.write_emission(table)
    on = _all_modes(back)
    back.write_emission(np.zeros(256, np.float32))
    for name, gpu in (("written all zero", zeros), ("written and zeroed again", back)):
        got = _all_modes(gpu)
        for k in want:
            _same(got[k], want[k], f"{name}: {k}")
        gpu.close()
    for k in (("primary", 1), ("primary+shadow", 1)):
        _same(on[k], want[k], f"a non-zero table: {k}")
    assert not np.array_equal(on[("path", 3)][0], want[("path", 3)][0])


def test_emission_only_adds_light():
    sc = scenes.c4((128, 72))
    gpu = gpu_for_scene(sc)
    table = _table(gpu)
    off = _frame(gpu, 3, stats=True)
    off_steps = gpu.read_steps()
    gpu.write_emission(table)
    on = _frame(gpu, 3, stats=True)
    on_steps = gpu.read_steps()
    assert np.array_equal(on[1], off[1]), "id words"
    assert np.array_equal(on_steps, off_steps), "step counts"
    assert (on[0] >= off[0]).all(), "a pixel is darker with emission on"
    assert (on[0] > off[0]).sum() > 100
    plain_on = _frame(gpu, 3)
    _same(plain_on, on, "a plain frame and a stats frame")
    gpu.close()


@pytest.mark.parametrize("size", [(480, 272), (100, 60)])
@pytest.mark.parametrize("in_flight", [1, 2, 4])
def test_accumulated_emissive_frames_are_one_frame_of_all_their_samples(size, in_flight):
    sc = scenes.c4(size)
    gpu = gpu_for_scene(sc)
    gpu.write_emission(_table(gpu))
    gpu.set_frames_in_flight(in_flight)
    want = {n: _frame(gpu, n) for n in (1, 4, 6, 8, 12)}
    for _ in range(4):
        gpu.render(MODE_PATH, spp=1, seed=SEED, accumulate=True)
    rgb, ids, _ = gpu.read_output()
    _same((rgb, ids), want[4], f"{size} in flight {in_flight}: 4 x 1 spp")
    gpu.reset_accumulation()
    n = 0
    for spp in (1, 3, 2, 2):
        n += spp
        _same(_acc(gpu, spp), want[n], f"{size} in flight {in_flight}: 1 + 3 + 2 + 2, after {n} samples")
        assert gpu.accumulation() == (n, SEED)
    gpu.reset_accumulation()
    for spp in (8, 4):
        gpu.render(MODE_PATH, spp=spp, seed=SEED, accumulate=True)
    rgb, ids, _ = gpu.read_output()
    _same((rgb, ids), want[12], f"{size} in flight {in_flight}: 8 + 4 unread")
    assert gpu.accumulation() == (12, SEED)
    gpu.close()


def test_writes_restart_the_sum_and_refusals_change_nothing():
    sc = scenes.c4((128, 72))
    gpu = gpu_for_scene(sc)
    table = _table(gpu)
    gpu.write_emission(table)
    want = {n: _frame(gpu, n) for n in (1, 2, 3, 4)}
    for _ in range(3):
        gpu.render(MODE_PATH, spp=1, seed=SEED, accumulate=True)
    gpu.write_emission(table[:4])   # the same values: any non-empty write restarts
    _same(_acc(gpu, 1), want[1], "after a write")
    assert gpu.accumulation() == (1, SEED)
    gpu.write_emission([])          # n == 0: nothing
    _same(_acc(gpu, 1), want[2], "after an empty write")
    before = gpu.read_output()
    bad_nan, bad_neg, bad_inf = table.copy(), table.copy(), table.copy()
    bad_nan[7], bad_neg[9], bad_inf[200] = np.nan, -0.25, np.inf
    for values, first, code in ((bad_nan, 0, _ffi.VRT_ERR_INVALID_ARG), (bad_neg, 0, _ffi.VRT_ERR_INVALID_ARG),
                                (bad_inf, 0, _ffi.VRT_ERR_INVALID_ARG), (np.ones(2, np.float32), 255, _ffi.VRT_ERR_OUT_OF_RANGE),
                                (np.ones(257, np.float32), 0, _ffi.VRT_ERR_OUT_OF_RANGE), ([5.0], 256, _ffi.VRT_ERR_OUT_OF_RANGE)):
        with pytest.raises(VrtError) as e:
            gpu.write_emission(values, first=first)
        assert e.value.code == code
    after = gpu.read_output()
    for a, b in zip(before[:2], after[:2]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "a refused write enqueued something"
    assert gpu.accumulation() == (2, SEED)
    _same(_acc(gpu, 1), want[3], "the accumulation after the refused writes")
    _same(_acc(gpu, 1), want[4], "... and the next")
    gpu.close()


def test_shards_and_devices_give_the_one_device_frame():
    sc = scenes.c4((160, 96))
    whole = gpu_for_scene(sc)
    table = _table(whole)
    whole.write_emission(table)
    want = _frame(whole, 3)
    whole.close()
    acc_rgb, acc_ids = np.zeros_like(want[0]), np.zeros_like(want[1])
    sum_rgb = np.zeros_like(want[0])
    for r in range(4):
        sh = gpu_for_scene(sc, shard_rank=r, shard_count=4)
        sh.write_emission(table)
        rgb, ids = _frame(sh, 3)
        sum_rgb += rgb
        acc_ids |= ids
        sh.render(MODE_PATH, spp=1, seed=SEED, accumulate=True)
        rgb_a, _ = _acc(sh, 2)
        acc_rgb += rgb_a
        sh.close()
    _same((sum_rgb, acc_ids), want, "the union of four shards")
    _same((acc_rgb, acc_ids), want, "the union of four accumulating shards")
    grp = gpu_for_scene(sc, devices=[0, 0], texel_messages=True)
    grp.write_emission(table)
    _same(_frame(grp, 3), want, "two devices with texel messages")
    grp.render(MODE_PATH, spp=2, seed=SEED, accumulate=True)
    grp.render(MODE_PATH, spp=1, seed=SEED, accumulate=True)
    rgb, ids, _ = grp.read_output()
    assert grp.accumulation() == (3, SEED)
    _same((rgb, ids), want, "two devices, accumulated")
    grp.close()
