"""The path-trace kernel families past 256 primary workgroups, against tests/lamp_ref.py.

Every launch of the wavefront path trace hands its records — paths, sun rays, lamp rays — to the next through 256 segments
(vrt_device.h: kHitSegments): workgroup k appends to segment k % 256, and the consuming launch's workgroup `part` = k / 256 of a
segment reads its records part * 256 ... (the pool kernel part * 4E ...).  Up to 65 536 traced pixels a segment has one producer,
part is 0 and no record index reaches 256 — which is where every other suite holds the emissive, polished, translucent, sun-lit,
camera-sampled and lamp-lit kernels to a reference.  Here they go against it at tests/segment_cases.py's frames, whose segments have
two, three and four producers (tests/test_segment_cases.py shows, from the reference alone, that the records are there): every
kind of frame on every route through the kernels, one and several samples, the pools of 256 and of 320 rays, a stats frame's
counters, two shards, the buffers behind a resize, and accumulation.  util.assert_frame_parity: id words exact, radiance to 1e-4."""
import ctypes as C

import numpy as np
import pytest

import lamp_ref
import polish_ref
import segment_cases as SC
import translucent_ref
from test_gpu_lamp import ENV, ROUTES as LAMP_ROUTES
from voxelraytracing_amd import MODE_PATH, _ffi

from util import assert_frame_parity, gpu_for_scene

pytestmark = pytest.mark.gpu

SEED = SC.SEED
SPPS = (1, 3)
KINDS = ("plain", "emissive", "polished", "translucent", "sun", "lens", "lens+sun", "lamps", "everything")
# (environment, stats, literal): tests/test_gpu_lamp.py's four, the pool kernel switched off (one lane = path launch per bounce), and
# a world that keeps no derived tables (tests/test_gpu_accel.py's switch: the octree walk)
ROUTES = dict(LAMP_ROUTES, lane=({"VRT_PATH_POOL": "0"}, False, False), **{"no tables": ({"VRT_ACCEL_MAX_S": "4"}, False, False)})


@pytest.fixture(scope="module")
def refs(tmp_path_factory, orc):
    return SC.References(lamp_ref.load(tmp_path_factory.mktemp("lamp_ref")), orc)


def _gpu(monkeypatch, sc, env=None, **kw):
    """A context for the scene under exactly `env` of the backend's switches (read when the context is created)."""
    for k in ENV + ["VRT_ACCEL_MAX_S"]:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    gpu = gpu_for_scene(sc, **kw)
    monkeypatch.delenv("VRT_ACCEL_MAX_S", raising=False)
    return gpu


def _set(gpu, refs, case, kind):
    """The tables and the three settings of a kind."""
    which, sun, setting, lamp = SC.KINDS[kind]
    t = refs.tables(case)[which]
    gpu.write_emission(t[0] if t[0] is not None else np.zeros(256, np.float32))
    gpu.write_polish(t[1] if t[1] is not None else polish_ref.table())
    gpu.write_translucency(t[2] if t[2] is not None else translucent_ref.table())
    gpu.set_sun_light(sun)
    gpu.set_camera_sampling(*setting)
    gpu.set_lamp_light(*lamp)


def _frame(gpu, spp, **kw):
    gpu.render(MODE_PATH, spp=spp, seed=SEED, **kw)
    rgb, ids, _ = gpu.read_output()
    return rgb, ids


def _check(got, ref, what):
    """A GPU frame against the reference's; 1e-4 is above an ulp where the radiance stays below 512."""
    assert float(ref.rgb.max()) < 512.0, what
    err = np.abs(got[0] - ref.rgb)
    print(f"{what}: max radiance {float(ref.rgb.max()):.4g}, max error {float(err[np.isfinite(err)].max()):.3g}; {ref.counts}")
    assert_frame_parity(got[0], got[1], ref.rgb, ref.ids, what)


def _check_stats(gpu, ref, what):
    st = gpu.stats()
    print(f"    secondary_rays {st.secondary_rays} steps {st.steps}")
    assert st.secondary_rays == ref.counts.bounce_segments + ref.counts.sun_rays + ref.counts.lamp_rays, what
    assert st.steps == ref.counts.steps, what


def _frames_of_a_kind(monkeypatch, refs, case, kind, route, bounces):
    """spp 1 and 3 of one kind on one route, one context."""
    env, stats, literal = ROUTES[route]
    gpu = _gpu(monkeypatch, SC.scene(case, bounces, literal), env)
    if route == "no tables":
        if kind in SC.LAMP_KINDS:   # such a world refuses a lamp-lit frame (include/vrt.h) ...
            _set(gpu, refs, case, kind)
            assert gpu._lib.vrt_render(gpu._h, C.byref(_ffi.RenderOpts(mode=MODE_PATH, spp=1, seed=SEED))) == _ffi.VRT_ERR_STATE
            if kind != "everything":
                gpu.close()
                return
            kind = "everything but lamps"   # ... and renders everything else
    _set(gpu, refs, case, kind)
    for spp in SPPS:
        what = f"{case} {kind} {route} b{bounces} spp {spp}"
        got = _frame(gpu, spp, stats=stats)
        ref = refs.frame(case, kind, bounces, spp, literal)
        _check(got, ref, what)
        if stats:
            _check_stats(gpu, ref, what)
    if route == "directory":
        assert gpu.read_march_cells()[1] == False, "the context's march cells are in the direct layout"   # noqa: E712
    if route == "no tables":
        assert gpu.accel_info().available == 0
    gpu.close()


# ---- every kind, route by route ----

@pytest.mark.parametrize("bounces", [1, 2, 4])
@pytest.mark.parametrize("route", ["default", "lane", "stats"])
@pytest.mark.parametrize("kind", KINDS)
def test_four_parts(refs, monkeypatch, kind, route, bounces):
    """1024 workgroups, capacity 1024: every consuming launch is 4 x 256 workgroups, and most segments hold more than 512 records."""
    _frames_of_a_kind(monkeypatch, refs, "four_parts", kind, route, bounces)


@pytest.mark.parametrize("route", ["directory", "literal", "no tables"])
@pytest.mark.parametrize("kind", KINDS)
def test_three_parts(refs, monkeypatch, kind, route):
    """516 workgroups, capacity 768 — not a power of two; segments 0-3 alone have a third producer."""
    _frames_of_a_kind(monkeypatch, refs, "three_parts", kind, route, 4)


@pytest.mark.parametrize("route", ["default", "stats"])
@pytest.mark.parametrize("kind", ["translucent", "sun", "everything"])
@pytest.mark.parametrize("case", ["one_over", "one_over_ragged"])
def test_one_over(refs, monkeypatch, case, kind, route):
    """257 workgroups: segment 0 alone has a second producer — one tile's worth of records behind the first workgroup's 256."""
    _frames_of_a_kind(monkeypatch, refs, case, kind, route, 4)


def test_one_over_ragged_leaves_the_border_zero(refs, monkeypatch):
    case = "one_over_ragged"
    w, h = SC.CASES["one_over"].size
    gpu = _gpu(monkeypatch, SC.scene(case))
    _set(gpu, refs, case, "everything")
    for spp in SPPS:
        rgb, ids = _frame(gpu, spp)
        assert not rgb[h:].any() and not rgb[:, w:].any() and not ids[h:].any() and not ids[:, w:].any()
        assert ids[:h, :w].all()   # (every primary ray of the traced area hits)
    gpu.close()


# ---- frames in flight: a frame set's own buffers, the pools of 256 and of 320 rays ----

@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("kind", ["translucent", "everything"])
def test_four_parts_three_frames_back_to_back(refs, monkeypatch, kind, in_flight):
    """With two frames in flight the frames alternate between two frame sets, each with path, sun and lamp buffers of its own, and a
    direct world's pool kernel takes 320 rays a wave (4E = 1280 records a workgroup) instead of 256."""
    case = "four_parts"
    gpu = _gpu(monkeypatch, SC.scene(case))
    _set(gpu, refs, case, kind)
    gpu.set_frames_in_flight(in_flight)
    for _ in range(3):
        gpu.render(MODE_PATH, spp=3, seed=SEED)
    rgb, ids, _ = gpu.read_output()
    _check((rgb, ids), refs.frame(case, kind, 4, 3), f"{case} {kind}, the third of three frames, {in_flight} in flight")
    assert gpu.read_march_cells()[1] == True, "the context's march cells are behind a chunk directory"   # noqa: E712
    gpu.close()


# ---- two shards ----

@pytest.mark.parametrize("kind", ["everything", "everything, second lit"])
def test_the_union_of_two_shards_is_the_reference_frame(refs, monkeypatch, kind):
    """2048 tiles a shard, 512 workgroups, capacity 512; a shard's t-th tile is screen tile 2 t + rank."""
    case = "two_shards"
    sc = SC.scene(case)
    ref = refs.frame(case, kind, 4, 3)
    sum_rgb, all_ids = np.zeros_like(ref.rgb), np.zeros_like(ref.ids)
    for r in range(2):
        sh = _gpu(monkeypatch, sc, shard_rank=r, shard_count=2)
        _set(sh, refs, case, kind)
        rgb, ids = _frame(sh, 3)
        assert not (all_ids != 0)[ids != 0].any()   # (the shards' tiles are disjoint)
        sum_rgb += rgb
        all_ids |= ids
        sh.close()
    _check((sum_rgb, all_ids), ref, f"{case} {kind}: the union of two shards")


# ---- a resize: the path, sun and lamp buffers are made by the first frame that needs them, and grow ----

def test_a_context_resized_up_and_down_matches_the_reference_at_each_size(refs, monkeypatch):
    case, kind, small = "four_parts", "everything", (128, 72)
    big = SC.CASES[case].size
    sc_small, sc_big = SC.scene(case, size=small), SC.scene(case)
    gpu = _gpu(monkeypatch, sc_small)
    _set(gpu, refs, case, kind)
    for sc, size in ((sc_small, small), (sc_big, big), (sc_small, small)):
        if gpu.result_size != size:
            gpu.resize_result_texture(size)
            gpu.write_cam_data(sc.cam)
        for spp in (1, 3, 3):   # (two frames in flight by default: a frame of each frame set at least)
            _check(_frame(gpu, spp), refs.frame(case, kind, 4, spp, size=None if size == big else size), f"{case} {kind} at {size}, spp {spp}")
    gpu.close()


# ---- accumulation: kResolveIntoSum behind multi-part launches ----

@pytest.mark.parametrize("in_flight", [1, 2])
def test_four_accumulated_frames_are_the_references_four_samples(refs, monkeypatch, in_flight):
    case, kind = "four_parts", "everything"
    gpu = _gpu(monkeypatch, SC.scene(case))
    _set(gpu, refs, case, kind)
    gpu.set_frames_in_flight(in_flight)
    for _ in range(4):
        gpu.render(MODE_PATH, spp=1, seed=SEED, accumulate=True)
    rgb, ids, _ = gpu.read_output()
    assert gpu.accumulation() == (4, SEED)
    _check((rgb, ids), refs.frame(case, kind, 4, 4), f"{case} {kind}: 4 x 1 spp accumulated, {in_flight} in flight")
    gpu.close()
