"""The scene tests/test_gpu_tone.py meters and maps, and the views its adaptation test alternates between: C4's world under
vrt_set_sun_light with one emissive material, so that a frame's radiance spans many octaves.  tests/test_tone_cases.py holds the
conditions that keep those tests from being vacuous to the CPU path reference (tests/sun_ref.py); the GPU tests check them again
on the frames they read back."""
import functools

import numpy as np

from voxelraytracing_amd import _ffi, scenes
from voxelraytracing_amd import graphics as g

SEED = 11
SUN = 1.0
EMISSION = 6.0
MAIN = (64, 40)


@functools.lru_cache(maxsize=None)
def scene(size=MAIN, bounces=4):
    return scenes.c4(size, bounces=bounces)


@functools.lru_cache(maxsize=None)
def emission_table():
    """The material most of the main view's primary rays hit gives off light."""
    from oracle import orc
    sc = scene(MAIN)
    _, ids, _, _ = orc.from_package_scene(sc).render(orc.MODE_PRIMARY, *MAIN)
    vox = ids[(ids & _ffi.ID_HIT) != 0] & _ffi.ID_VOXEL_MASK
    table = np.zeros(256, np.float32)
    table[int(np.bincount(vox).argmax())] = EMISSION
    return table


def view(sc, pitch, size):
    """The scene's camera turned to `pitch` degrees (negative: up)."""
    return g.cam_data_create((pitch, sc.rot[1], 0.0), sc.eye, 70.0, (float(size[0]), float(size[1])))


SKY_PITCH, DOWN_PITCH = -50.0, 89.0
