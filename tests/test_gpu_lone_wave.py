"""The asm march loops with one wave resident, on cameras whose rays tie: the timed, stats-free kernels against the oracle.

The march step (vrt_march.h) and the bounce march (VBM_* in vrt_path.hip) are hand-written, and their wait states are their own
(tests/test_isa_hazards.py).  A parity frame of many waves hides issue timing; these frames are one 8x8 tile or a handful of tiles,
so each wave issues with nothing else to cover its latency.  The cameras are built for the case where the per-axis `v_cmp_eq`
results of the axis select differ: eyes on integer and half-integer lattice points, rays along (+-1, +-1, 0) and (+-1, +-1, +-1)
(exactly equal |components|: equal exit distances on two or three axes) and rays with a zero component (the |0| * inf path).
"""
import math

import numpy as np
import pytest

from voxelraytracing_amd import MODE_PATH, MODE_PRIMARY, MODE_PRIMARY_SHADOW, scenes

from util import assert_frame_parity, gpu_for_scene

pytestmark = pytest.mark.gpu

DIAG3 = math.degrees(math.atan(1.0 / math.sqrt(2.0)))   # the pitch of (1, 1, 1)
# (eye offset from the world's lattice, rotation): rays of the frame along / around these directions
CAMERAS = [
    ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),          # (+-1, +-1, 0)-like pixel rays: |x| == |y| on the frame's diagonals
    ((0.5, 0.5, 0.5), (0.0, 45.0, 0.0)),         # forward (-1, 0, -1): rows with a zero y component
    ((0.0, 0.0, 0.0), (DIAG3, 45.0, 0.0)),       # forward (-1, -1, -1): a pixel with three equal |components|
    ((0.5, 0.0, 0.5), (-DIAG3, -135.0, 0.0)),    # forward (+1, +1, +1)-like, above the terrain looking up
    ((0.0, 0.5, 0.0), (0.0, -135.0, 0.0)),       # forward (+1, 0, +1)
]
SIZES = [(8, 8), (32, 16)]   # one tile; eight tiles


@pytest.fixture(scope="module")
def worlds():
    """C1's superflat world (long air runs over a layered surface of split cells) and C2's procedural one, with an eye on each."""
    c1, c2 = scenes.c1_flat((8, 8)), scenes.c2((8, 8))
    h = float(c2.world.highest_vox_at(128, 128))
    return {"c1": (c1.world, (32.0, 14.0, 32.0)), "c2": (c2.world, (128.0, h + 2.0, 128.0))}


def _scene(worlds, key, cam, size, mode, bounces=None):
    world, base = worlds[key]
    eye = tuple(b + o for b, o in zip(base, cam[0]))
    sc = scenes._scene(f"{key} eye {eye} rot {cam[1]}", world, size, eye, cam[1], mode)
    if bounces is not None:
        sc.settings.max_ray_bounces = bounces
        scenes._diffuse(sc.materials)
    return sc


def _ties(o, size, mode):
    """Pixels of the frame whose ray has two / three exactly equal |components|, or a zero one."""
    t2 = t3 = t0 = 0
    for py in range(size[1]):
        for px in range(size[0]):
            a = np.abs(np.float32(o.trace_pixel(mode, px, py)[2]))
            eq = int(a[0] == a[1]) + int(a[1] == a[2]) + int(a[0] == a[2])
            t3 += eq == 3
            t2 += eq == 1
            t0 += bool((a == 0).any())
    return t2, t3, t0


@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("key", ["c1", "c2"])
def test_lone_waves_on_tie_cameras_match_oracle(orc, worlds, key, size, in_flight):
    """Primary, and primary + shadow: the timed kernels (the asm loop) bit for bit; then the counting kernels' per-pixel step
    counts on the same frames."""
    sc = _scene(worlds, key, CAMERAS[0], size, MODE_PRIMARY_SHADOW)
    gpu = gpu_for_scene(sc)
    gpu.set_frames_in_flight(in_flight)
    ties = [0, 0, 0]
    try:
        for cam in CAMERAS:
            sc = _scene(worlds, key, cam, size, MODE_PRIMARY_SHADOW)
            gpu.write_cam_data(sc.cam)
            o = orc.from_package_scene(sc)
            for mode in (MODE_PRIMARY, MODE_PRIMARY_SHADOW):
                gpu.render(mode, timed=True)
                gpu.render(mode, timed=True)   # two frames back to back: with two in flight the second overlaps the first
                rgb, ids, _ = gpu.read_output()
                r_rgb, r_ids, r_steps, _ = o.render(mode, *size, want_steps=True)
                assert_frame_parity(rgb, ids, r_rgb, r_ids, f"{sc.name} {size} mode {mode}, {in_flight} in flight")
                gpu.render(mode, stats=True)
                assert np.array_equal(gpu.read_steps(), r_steps), f"{sc.name} {size} mode {mode}: step counts"
            ties = [a + b for a, b in zip(ties, _ties(o, size, MODE_PRIMARY))]
    finally:
        gpu.close()
    print(f"{key} {size}: pixels with 2-axis ties {ties[0]}, 3-axis ties {ties[1]}, a zero component {ties[2]}")
    assert ties[0] > 0 and ties[1] > 0 and ties[2] > 0, "the cameras no longer give rays that tie"


@pytest.mark.parametrize("bounces", [1, 2, 3, 4])
@pytest.mark.parametrize("size", SIZES)
def test_lone_waves_bounce_march_matches_oracle(orc, worlds, size, bounces):
    """The bounce march (VBM_*) through the path trace at 1 spp on the same small frames and cameras, one and two in flight."""
    for cam in CAMERAS[:3]:
        sc = _scene(worlds, "c2", cam, size, MODE_PATH, bounces=bounces)
        o = orc.from_package_scene(sc)
        r_rgb, r_ids, _, _ = o.render(MODE_PATH, *size, spp=1, seed=3)
        gpu = gpu_for_scene(sc)
        try:
            for in_flight in (1, 2):
                gpu.set_frames_in_flight(in_flight)
                gpu.render(MODE_PATH, spp=1, seed=3, timed=True)
                gpu.render(MODE_PATH, spp=1, seed=3, timed=True)
                rgb, ids, _ = gpu.read_output()
                assert_frame_parity(rgb, ids, r_rgb, r_ids, f"{sc.name} {size} path b{bounces}, {in_flight} in flight")
        finally:
            gpu.close()
