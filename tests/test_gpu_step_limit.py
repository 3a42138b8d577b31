"""Rays that run out of lookups (kMaxSteps = 500) in the hand-written march loops, against the oracle.

The primary/shadow march (the asm block of vrt_march.h) counts its trips as iter - kMaxSteps, and the general step after it can
reach lookup 500 too; the bounce march (VBM_* in vrt_path.hip) counts per lane and reloads the voxel of a lane that ran out in a
split cell from the brick.  The scenes (tests/step_limit_scenes.py) put first solid voxels at lookups 499, 500 and 501, rays that
run out in air and in water, shadow rays that run out, and bounce segments that run out on water in split cells; which of them
a frame holds is counted on the CPU (tests/test_step_limit_classes.py).  Ids bit for bit, rgb within 1e-4, and the counting
kernels' per-pixel step counts exactly.
"""
import numpy as np
import pytest

from voxelraytracing_amd import MODE_PATH, MODE_PRIMARY, MODE_PRIMARY_SHADOW

import step_limit_scenes as L
from util import assert_frame_parity, gpu_for_scene

pytestmark = pytest.mark.gpu

VARIANTS = [0, 1, 2, 3]   # as tests/test_gpu_parity.py: grid march fused (default), literal octree walk, ancestor cache, two launches
SEED = 3


@pytest.fixture(scope="module")
def world():
    return L.build_world()


def _primary(orc, sc, gpu, what, variants=(0,)):
    w, h = sc.size
    o = orc.from_package_scene(sc)
    ran_out = False
    for mode in (MODE_PRIMARY, MODE_PRIMARY_SHADOW):
        r_rgb, r_ids, r_steps, _ = o.render(mode, w, h, want_steps=True)
        for variant in variants:
            gpu.render(mode, variant=variant, timed=True)
            gpu.render(mode, variant=variant, timed=True)   # with two in flight the second frame overlaps the first
            rgb, ids, _ = gpu.read_output()
            assert_frame_parity(rgb, ids, r_rgb, r_ids, f"{what} mode {mode} variant {variant}")
            gpu.render(mode, variant=variant, stats=True)
            assert np.array_equal(gpu.read_steps(), r_steps), f"{what} mode {mode} variant {variant}: step counts"
        ran_out |= bool(((r_steps & 0xFFFF) == 500).any() or ((r_steps >> 16) == 500).any())
    assert ran_out, f"{what}: nothing ran out"


@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("size", L.SIZES)
def test_primary_and_shadow_at_the_step_limit(orc, world, size, in_flight):
    """One 8x8 tile and eight tiles, one and two frames in flight: every camera, every march variant."""
    sc = L.scene(world, L.CAMERAS[0], size, MODE_PRIMARY_SHADOW)
    gpu = gpu_for_scene(sc)
    gpu.set_frames_in_flight(in_flight)
    try:
        for cam in L.CAMERAS:
            sc = L.scene(world, cam, size, MODE_PRIMARY_SHADOW)
            gpu.write_cam_data(sc.cam)
            _primary(orc, sc, gpu, f"{sc.name}, {in_flight} in flight", VARIANTS)
    finally:
        gpu.close()


def test_primary_and_shadow_at_the_step_limit_many_waves(orc, world):
    """256 x 144: many waves at once, exhausted and early lanes side by side."""
    for cam in L.CAMERAS:
        sc = L.scene(world, cam, L.BIG, MODE_PRIMARY_SHADOW)
        gpu = gpu_for_scene(sc)
        try:
            _primary(orc, sc, gpu, sc.name, VARIANTS)
        finally:
            gpu.close()


def _path(orc, sc, what, in_flight=(1, 2), steps=True):
    w, h = sc.size
    r_rgb, r_ids, r_steps, _ = orc.from_package_scene(sc).render(MODE_PATH, w, h, want_steps=True, spp=1, seed=SEED)
    gpu = gpu_for_scene(sc)
    try:
        for n in in_flight:
            gpu.set_frames_in_flight(n)
            gpu.render(MODE_PATH, spp=1, seed=SEED, timed=True)
            gpu.render(MODE_PATH, spp=1, seed=SEED, timed=True)
            rgb, ids, _ = gpu.read_output()
            assert_frame_parity(rgb, ids, r_rgb, r_ids, f"{what}, {n} in flight")
        if steps:
            gpu.render(MODE_PATH, spp=1, seed=SEED, stats=True)
            assert np.array_equal(gpu.read_steps(), r_steps), f"{what}: step counts"
    finally:
        gpu.close()


@pytest.mark.parametrize("bounces", [1, 2, 3, 4])
def test_bounce_march_at_the_step_limit(orc, world, bounces):
    """The path trace over the same world, mirror and diffuse, one tile to 256 x 144: bounce segments that run out, some of them
    on water in split cells (the brick reload)."""
    for sc in L.path_scenes(world, bounces):
        _path(orc, sc, f"{sc.name} b{bounces} {'diffuse' if sc.materials[4].scatter else 'mirror'}")


@pytest.mark.parametrize("env", [{"VRT_PATH_POOL": "0"}, {"VRT_PATH_CELLS": "0"}, {"VRT_PATH_POOL_K": "4"},
                                 {"VRT_PATH_POOL_K": "5"}, {"VRT_MARCH_DIRECT_MAX_S": "16"}, {"VRT_MARCH_DIRECT_MAX_S": "0"}])
def test_every_form_of_the_bounce_launch_at_the_step_limit(orc, world, monkeypatch, env):
    """Each form of the bounce launch the backend can be switched to, on the frames with the brick reload."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for bounces in (3, 4):
        for sc in L.path_scenes(world, bounces):
            if sc.size == L.BIG:
                _path(orc, sc, f"{sc.name} b{bounces} {env}", steps=False)
