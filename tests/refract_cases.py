"""The scenes of the refraction tests (tests/test_refract_ref.py, tests/test_refract_cases.py, tests/test_gpu_refract.py) beyond
tests/water_cases.py's: a pool with a column of water that reaches the top of its chunk, so that a wet segment leaves the water into
a chunk the generator left out.  TEST INFRASTRUCTURE ONLY.

"Column": water_cases' pool with water (id 3) over x, z in [34, 40) from the surface (y = 12) up to y = 31, the last layer of the
world's lower chunks; the chunks above hold nothing and chunk_roots holds 0 for them.  The camera "column_up" sits in the pool
under the column and looks straight up it: the paths near the axis leave through the column's top face, y = 32, into such a chunk
(vrt_get_voxels answers 0 there: no chunk), the others through its sides into air that exists."""
import water_cases as K

IOR = 1.33                         # water's
COLUMN = (34, 40)                  # the column's x and z extent
COLUMN_TOP = 32                    # its top face: the chunk boundary
CAMERAS = {"column_up": ((37.5, 10.5, 37.5), (-90.0, 0.0, 0.0))}

_worlds = {}


def column_world():
    """The pool's world with the column of water, built once."""
    if "column" not in _worlds:
        w = K.fresh_pool_world()
        for x in range(*COLUMN):
            for z in range(*COLUMN):
                for y in range(K.SURFACE, COLUMN_TOP):
                    w.set_voxel((x, y, z), K.WATER)
        _worlds["column"] = w
    return _worlds["column"]


def column(camera: str, size, bounces=4):
    from voxelraytracing_amd import graphics as g, scenes
    eye, rot = CAMERAS[camera]
    sc = scenes._scene(f"column {camera} {size[0]}x{size[1]}", column_world(), size, eye, rot, g.MODE_PATH)
    sc.settings.max_ray_bounces = bounces
    scenes._diffuse(sc.materials)
    return sc
