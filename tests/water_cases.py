"""The scenes of the water tests (tests/test_water_ref.py, tests/test_gpu_water.py): a hand-built pool in a 2^3-chunk world and
C4's scene from its two lake cameras.  TEST INFRASTRUCTURE ONLY.

The pool: a slate floor (id 5) to y = 8 over the whole world; on it a basin with walls one voxel thick around x, z in [20, 44),
three voxels deep in water (id 3, y = 9, 10, 11: the surface is the plane y = 12, the walls' tops too); a slate pillar at
x, z in [30, 32) from the bed to y = 15, through the surface."""
import numpy as np

from voxelraytracing_amd import graphics as g, scenes
from voxelraytracing_amd.world import ClientWorld

WATER, SLATE = 3, 5
FLOOR_TOP, DEPTH = 9, 3            # the bed is the plane y = 9; water fills y in [9, 12)
SURFACE = FLOOR_TOP + DEPTH
X0, X1 = 20, 44                    # the water's x and z extent; the walls are the voxels around it
PILLAR = (30, 32)

SIZES = [(8, 8), (16, 8), (100, 60), (128, 72)]
BOUNCES = (1, 2, 4)
SPPS = (1, 3, 12)
SEED = 11
OPTICS = ((0.30, 0.12, 0.05), 0.04)   # (absorb, reflectance): red goes first; a little more mirror than real water's 0.02

# name -> (eye, rot): across the surface at a grazing angle; straight down from above the middle of one half of the basin; from
# inside the water down at the bed; from inside the water up and out through the surface
CAMERAS = {
    "grazing": ((12.5, 13.5, 32.5), (6.0, 270.0, 0.0)),
    "down": ((37.5, 20.5, 37.5), (90.0, 0.0, 0.0)),
    "under_bed": ((37.5, 11.5, 37.5), (60.0, 30.0, 0.0)),
    "under_up": ((37.5, 10.5, 37.5), (-50.0, 200.0, 0.0)),
}

_world = None


def pool_world() -> ClientWorld:
    """The pool's world, built once by set_voxel (2^3 chunks, world.min = (0, 0, 0))."""
    global _world
    if _world is None:
        w = ClientWorld((1, 1, 1), 1 << 20, 2)
        w.generate(1, 0)   # Superflat, as C1's world: every chunk exists
        n = 64
        # clear what the generator put there, then build (whole columns: the generator's ground is replaced)
        for x in range(n):
            for z in range(n):
                for y in range(0, 32):   # (the chunks above hold nothing: Superflat leaves them out, chunk_roots 0)
                    inside = X0 <= x < X1 and X0 <= z < X1
                    wall = (X0 - 1 <= x <= X1 and X0 - 1 <= z <= X1) and not inside
                    pillar = PILLAR[0] <= x < PILLAR[1] and PILLAR[0] <= z < PILLAR[1]
                    if y < FLOOR_TOP:
                        v = SLATE
                    elif pillar and y < 16:
                        v = SLATE
                    elif y < SURFACE and inside:
                        v = WATER
                    elif y < SURFACE and wall:
                        v = SLATE
                    else:
                        v = 0
                    if w.get_voxel((x, y, z)) != v:
                        w.set_voxel((x, y, z), v)
        _world = w
    return _world


def pool(camera: str, size, bounces=4) -> "scenes.Scene":
    eye, rot = CAMERAS[camera]
    sc = scenes._scene(f"pool {camera} {size[0]}x{size[1]}", pool_world(), size, eye, rot, g.MODE_PATH)
    sc.settings.max_ray_bounces = bounces
    scenes._diffuse(sc.materials)
    return sc


def c4_lake(camera: str, size=(128, 72), bounces=4) -> "scenes.Scene":
    """C4's scene from tests/golden/make_wgsl_fixtures.py's lake cameras: "water" (c2_water_40x24: just above the lake) or
    "underwater" (c2_underwater_24x16: the eye inside it)."""
    eye, rot = {"water": ((24.5, 76.5, 84.5), (30.0, 150.0, 0.0)), "underwater": ((22.5, 55.5, 80.5), (-20.0, 40.0, 0.0))}[camera]
    sc = scenes.c4(size, bounces=bounces)
    sc.cam = g.cam_data_create(rot, eye, 70.0, (float(size[0]), float(size[1])))
    sc.eye, sc.rot = eye, rot
    return sc
