"""ctypes binding of tests/water_ref.c: the path trace with water optics (vrt_set_water_optics, include/vrt.h) on top of the
emission, polish and translucency tables and direct sunlight.  TEST INFRASTRUCTURE ONLY.

``load(directory)`` compiles water_ref.c with oracle/Makefile's own CFLAGS (strict IEEE: no contraction, no fast-math) into
`directory` — a pytest temporary directory, never the source tree — and loads it, once per process.  The scene struct is
oracle/orc.py's; the tables are path_ref's."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from collections import namedtuple

import numpy as np

from oracle import orc
from path_ref import _tables, oracle_cflags
from voxelraytracing_amd._ffi import WATER_ON, WaterOptics

_HERE = os.path.dirname(os.path.abspath(__file__))

# of one render or one sample, in the order of water_ref.c's enum: the lookups of every march (path segments and sun rays), the
# path segments behind the primary ones, the sun rays marched and the unoccluded ones, the surface events and how many of them
# reflected / went through, the wet segments with water_dist > 0, the wet segments that hit, the primary segments that start wet
# with water_dist > 0, the bounce segments that start wet, the passes through a translucent voxel, the bounces off a coat
Counts = namedtuple("Counts", "steps bounce_segments sun_rays sun_unoccluded surface reflected transmitted wet_w wet_hit wet_primary_w wet_bounces "
                              "passes polished_bounces")

OFF = None   # the setting off
LOAD_PATH, LOAD_SUN, LOAD_WET = 1, 2, 4   # water_ref.c's load bits


def optics(setting) -> WaterOptics:
    """setting: None (off) or (absorb, reflectance), absorb one float or three."""
    if setting is None:
        return WaterOptics((C.c_float * 3)(0, 0, 0), 0.0, 0, (C.c_uint32 * 3)(0, 0, 0))
    a = np.broadcast_to(np.asarray(setting[0], dtype=np.float32), (3,))
    return WaterOptics((C.c_float * 3)(*(float(x) for x in a)), float(setting[1]), WATER_ON, (C.c_uint32 * 3)(0, 0, 0))


class WaterRef:
    def __init__(self, so: str):
        L = C.CDLL(so)
        u32, f32, ptr = C.c_uint32, C.c_float, C.c_void_p
        settings = [C.POINTER(orc.Scene), ptr, ptr, ptr, f32, C.POINTER(WaterOptics), u32, u32, u32]   # scene, tables, sun, optics, w, h, seed
        L.ref_render_water.restype = None
        L.ref_render_water.argtypes = settings + [u32, u32, ptr, ptr, ptr, ptr]          # spp, sample_base, rgb, ids, counts, load
        L.ref_trace_pixel_water.restype = None
        L.ref_trace_pixel_water.argtypes = settings + [u32, u32, u32, ptr, ptr, ptr, ptr]  # px, py, sample, light, id, counts, thr_bed
        L.ref_water_exp_neg.restype = f32
        L.ref_water_exp_neg.argtypes = [f32]
        L.ref_voxel_at_floor.restype = u32
        L.ref_voxel_at_floor.argtypes = [C.POINTER(orc.Scene), f32, f32, f32]
        self._lib = L

    @staticmethod
    def _settings(scene, w, h, seed, water, sun, emission, polish, translucency):
        e, p, t = _tables(emission, polish, translucency)
        wo = optics(water)
        return (e, p, t, wo), (C.byref(scene.c), e.ctypes.data, p.ctypes.data, t.ctypes.data, sun, C.byref(wo), w, h, seed)

    def render(self, scene: "orc.OracleScene", w: int, h: int, water=OFF, spp: int = 1, seed: int = 0, sample_base: int = 0, sun: float = 0.0,
               emission=None, polish=None, translucency=None, load=None):
        """(rgb [h, w, 3] f32, ids [h, w] u32, Counts) of samples sample_base .. sample_base + spp - 1.  water: None or (absorb,
        reflectance); sun: vrt_set_sun_light's strength; the three 256-entry tables (None = zeros); load: None, or a zeroed uint8
        array [spp, bounces, h, w] that receives the LOAD_ bits of every sample's every segment."""
        keep, args = self._settings(scene, w, h, seed, water, sun, emission, polish, translucency)
        rgb = np.zeros((h, w, 3), dtype=np.float32)
        ids = np.zeros((h, w), dtype=np.uint32)
        n = np.zeros(len(Counts._fields), dtype=np.uint64)
        if load is not None:
            assert load.dtype == np.uint8 and load.flags.c_contiguous and load.shape == (spp, scene.c.settings.max_ray_bounces, h, w), load.shape
        self._lib.ref_render_water(*args, spp, sample_base, rgb.ctypes.data, ids.ctypes.data, n.ctypes.data, load.ctypes.data if load is not None else None)
        return rgb, ids, Counts(*(int(x) for x in n))

    def trace_pixel(self, scene: "orc.OracleScene", w: int, h: int, px: int, py: int, water=OFF, sample: int = 0, seed: int = 0, sun: float = 0.0,
                    emission=None, polish=None, translucency=None):
        """(light [3] f32, the id word of the sample's primary segment, Counts, thr_bed [3] f32: the throughput at the sample's
        first hit on a solid voxel at the end of a wet segment, NaN if it has none) of one sample of one pixel."""
        keep, args = self._settings(scene, w, h, seed, water, sun, emission, polish, translucency)
        light = np.zeros(3, dtype=np.float32)
        idw = C.c_uint32(0)
        n = np.zeros(len(Counts._fields), dtype=np.uint64)
        thr = np.full(3, np.nan, dtype=np.float32)
        self._lib.ref_trace_pixel_water(*args, px, py, sample, light.ctypes.data, C.byref(idw), n.ctypes.data, thr.ctypes.data)
        return light, int(idw.value), Counts(*(int(x) for x in n)), thr

    def voxel_at_floor(self, scene: "orc.OracleScene", o) -> int:
        """Step 1 of the contract: the voxel at floor(o), o world-local — 0 outside the world box and where there is no chunk."""
        return int(self._lib.ref_voxel_at_floor(C.byref(scene.c), float(o[0]), float(o[1]), float(o[2])))

    def eye_is_wet(self, scene: "orc.OracleScene") -> bool:
        """Whether the camera's voxel is a liquid of the scene's material table (ids >= 255 share entry 255)."""
        origin = [scene.c.cam.pos[a] - float(scene.c.world.min[a]) for a in range(3)]   # create_ray_from_screen's: world-local
        return scene.mats[min(self.voxel_at_floor(scene, origin), 255)].is_liquid == 1

    def guide(self, dref, scene: "orc.OracleScene", w: int, h: int, water=OFF):
        """(guide [h, w] u32, ids [h, w] u32) of a frame's primary segments, by tests/denoise_ref.py's ref_guide (dref: its
        library): over the scene as it is with the setting off or the camera's voxel a liquid of the table, over a copy with every
        is_liquid cleared otherwise — the march a water frame gives its primary rays."""
        if water is None or self.eye_is_wet(scene):
            return dref.guide(scene, w, h)
        return dref.guide(dry_copy(scene), w, h)

    def exp_neg(self, t) -> np.ndarray:
        """water_ref.c's own statement of vexp_neg, value by value."""
        t = np.asarray(t, dtype=np.float32)
        return np.array([self._lib.ref_water_exp_neg(float(x)) for x in t.reshape(-1)], dtype=np.float32).reshape(t.shape)


def dry_copy(scene: "orc.OracleScene") -> "orc.OracleScene":
    """The scene with every is_liquid cleared (the nodes and roots shared, the materials its own)."""
    dry = orc.OracleScene(scene.nodes, scene.roots, scene.mats, scene.c.cam, scene.c.settings, scene.c.world)
    for m in dry.mats:
        m.is_liquid = 0
    return dry


_loaded = None


def load(directory) -> WaterRef:
    """Compile tests/water_ref.c into `directory` and load it; later calls return the library of the first."""
    global _loaded
    if _loaded is None:
        so = os.path.join(str(directory), "libwater_ref.so")
        cc = os.environ.get("CC", "gcc")
        subprocess.check_call([cc, *oracle_cflags(), "-shared", "-o", so, os.path.join(_HERE, "water_ref.c"), "-lm"])
        _loaded = WaterRef(so)
    return _loaded
