"""The frames that take the path trace's record buffers past one workgroup per segment (vrt_device.h: kHitSegments;
vrt_path_common.h: append_paths, append_light_rays), for tests/test_segment_cases.py (the cases' preconditions, from the reference
alone) and tests/test_gpu_path_segments.py (the kernels against the reference).  TEST INFRASTRUCTURE ONLY.

A launch's workgroup k appends to segment k % 256 of the launch's buffers; the consuming launch gives a segment the workgroups seg,
seg + 256, ..., and workgroup `part` = k / 256 of a segment reads its records part * 256 ... (the pool kernel part * 4E ...).  A
segment holds ceil(workgroups / 256) * 256 records (hit_seg_cap) per sample of a chain.  Up to 256 primary workgroups — 1024
tiles, 65 536 traced pixels — a segment has one producer, part is 0 everywhere and no record index reaches 256: the cases here
are past that.

Every case is scenes.c4's world seen from its own eye; the cases marked with a rotation look down (every primary ray hits).
`segment_loads` is what a launch puts into each segment, from a plane of tests/lamp_ref.py's `load` output."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import emission_cases as E
import lamp_ref
import polish_ref
import translucent_ref
from voxelraytracing_amd import cam_data_create, scenes

SEED = 11
SUN = 1.0
LAMP = (1.0, 0.01)        # (strength, max_geometry)
LENS = (1.0, 0.05, 20.0)
NO_LAMP = (0.0, 0.0)
HALF = (0.5, (0.9, 0.6, 0.3))             # (chance, colour): passes half of the time, with a tint
ALWAYS = (2.0, (0.25, 0.5, 0.75))         # always passes
COAT_A = (0.5, 0.0, (1.0, 0.9, 0.8))      # (chance, scatter, colour): a mirror half of the time
DOWN = (60.0, 35.0, 0.0)
FOV = 70.0                                # scenes.py's

SEGMENTS = 256

# size; the camera's rotation (None: scenes.c4's own); shard contexts
Case = namedtuple("Case", "size rot shards")
CASES = {
    # 41 x 25 = 1025 tiles, 257 workgroups, capacity 512: only segment 0 has two producers, and the last workgroup has one tile
    "one_over": Case((328, 200), DOWN, 1),
    # the same traced area inside a frame that is not whole tiles
    "one_over_ragged": Case((332, 204), DOWN, 1),
    # 48 x 43 = 2064 tiles, 516 workgroups, capacity 768 (not a power of two): segments 0-3 have three producers
    "three_parts": Case((384, 344), DOWN, 1),
    # 4096 tiles, 1024 workgroups, capacity 1024: every consumer launch is 4 x 256 workgroups
    "four_parts": Case((1024, 256), None, 1),
    # two shard contexts of 2048 tiles each, capacity 512
    "two_shards": Case((1024, 256), None, 2),
}

# kind: (tables: a key of tables(), sun, camera sampling, lamp)
KINDS = {
    "plain": ("none", 0.0, lamp_ref.OFF, NO_LAMP),
    "emissive": ("alone", 0.0, lamp_ref.OFF, NO_LAMP),
    "polished": ("polish", 0.0, lamp_ref.OFF, NO_LAMP),
    "translucent": ("translucent", 0.0, lamp_ref.OFF, NO_LAMP),
    "sun": ("alone", SUN, lamp_ref.OFF, NO_LAMP),
    "lens": ("alone", 0.0, LENS, NO_LAMP),
    "lens+sun": ("alone", SUN, LENS, NO_LAMP),
    "lamps": ("alone", 0.0, lamp_ref.OFF, LAMP),
    "everything": ("all", SUN, LENS, LAMP),
    # "everything" as a world without derived tables renders it: such a context refuses a lamp-lit frame (include/vrt.h)
    "everything but lamps": ("all", SUN, LENS, NO_LAMP),
    # "everything" with the second material alone giving off light: the lamp rays of a shard's context.  Under "all" a shard's
    # fullest lamp segment holds 257 and 253 records of the 512 it can (lamp faces that look up are seen by few of the hits that
    # look up too, and the most-hit material is the ground); with the ground dark, 338 and 353
    "everything, second lit": ("all second", SUN, LENS, LAMP),
}
LAMP_KINDS = tuple(k for k, v in KINDS.items() if v[3][0] != 0.0)


def workgroups(case: str) -> int:
    """The primary launch's workgroups of one context of the case."""
    c = CASES[case]
    tiles = (c.size[0] // 8) * (c.size[1] // 8)
    return ((tiles + c.shards - 1) // c.shards + 3) // 4


def capacity(case: str) -> int:
    """hit_seg_cap of one context of the case (vrt_frames.hip: alloc_output)."""
    return (workgroups(case) + SEGMENTS - 1) // SEGMENTS * 256


def scene(case: str, bounces: int = 4, literal: bool = False, size=None):
    """scenes.c4 at the case's size (or `size`) with the case's camera; literal: air flagged liquid (the literal march)."""
    c = CASES[case]
    size = size or c.size
    sc = scenes.c4(size, bounces=bounces)
    if c.rot is not None:
        sc.cam = cam_data_create(c.rot, sc.eye, FOV, (float(size[0]), float(size[1])))
        sc.rot = c.rot
    if literal:
        sc.materials[0].is_liquid = 1
    return sc


def shard_tiles(w: int, h: int, rank: int, count: int) -> np.ndarray:
    """The screen tiles of shard `rank` of `count` (root weight 1: tile t belongs to rank t % count), in increasing order."""
    return np.arange(rank, (w // 8) * (h // 8), count)


def segment_loads(load_plane, w: int, h: int, tiles=None) -> np.ndarray:
    """What one launch over the frame's tiles appends to each of the 256 segments: load_plane [h, w] holds, per pixel, the records
    the pixel's lane appends (a bit of lamp_ref's load plane as 0 / 1, or several samples' summed).  Tiles are 8 x 8 pixels,
    numbered row-major; the launch's t-th tile is tiles[t] (None: every tile of the frame) — a shard's own list, in increasing
    order; four tiles make a workgroup, and workgroup k feeds segment k % 256."""
    plane = np.asarray(load_plane)
    assert plane.shape == (h, w)
    tx, ty = w // 8, h // 8
    per_tile = plane[:ty * 8, :tx * 8].astype(np.int64).reshape(ty, 8, tx, 8).sum(axis=(1, 3)).reshape(-1)
    if tiles is not None:
        tiles = np.asarray(tiles, np.int64)
        assert tiles.ndim == 1 and (np.diff(tiles) > 0).all() and (tiles.size == 0 or (0 <= tiles[0] and tiles[-1] < tx * ty))
        per_tile = per_tile[tiles]
    seg = (np.arange(per_tile.size) // 4) % SEGMENTS
    return np.bincount(seg, weights=per_tile, minlength=SEGMENTS).astype(np.int64)


def tables(ids) -> dict:
    """The tables of every kind, chosen as tests/test_gpu_lamp.py chooses them, from a frame's id words: the material the primary
    rays hit most gives off light ("alone"); in "all" the second passes half of the time with a tint and gives off light too,
    the third always passes, the fourth has coat A.  "polish" and "translucent" are "all" with one of the two lobes, "all second" is "all" with the most-hit material dark."""
    counts = E.hit_counts(ids)
    top = [int(t) for t in np.argsort(counts)[::-1][:4] if counts[t] > 0]
    assert len(top) == 4, f"the frame hits {len(top)} materials"
    alone = np.zeros(256, np.float32)
    alone[top[0]] = 1.5
    emission = alone.copy()
    emission[top[1]] = 0.75
    tr = translucent_ref.table({top[1]: HALF, top[2]: ALWAYS})
    polish = polish_ref.table()
    polish[top[3]]["chance"], polish[top[3]]["scatter"], polish[top[3]]["color"] = COAT_A
    second = emission - alone
    return {"none": (None, None, None), "alone": (alone, None, None), "polish": (emission, polish, None),
            "translucent": (emission, None, tr), "all": (emission, polish, tr), "all second": (second, polish, tr)}


Frame = namedtuple("Frame", "rgb ids counts load")


class References:
    """The reference's frames of the cases, each computed once (a test module keeps one of these)."""

    def __init__(self, lref, orc):
        self.lref, self.orc = lref, orc
        self._scenes, self._tables, self._lists, self._frames = {}, {}, {}, {}

    def oracle_scene(self, case, bounces=4, literal=False, size=None):
        k = (case, bounces, literal, size)
        if k not in self._scenes:
            sc = scene(case, bounces, literal, size)
            self._scenes[k] = (sc, self.orc.from_package_scene(sc))   # (the package scene kept alive: the oracle's points into it)
        return self._scenes[k]

    def tables(self, case):
        """tables() of the case's plain 1-spp frame at the case's own size (the id words do not depend on the bounces: 1 here)."""
        if case not in self._tables:
            sc, o = self.oracle_scene(case, 1)
            _, ids = self.lref.render(o, NO_LAMP, np.zeros(0, lamp_ref.LAMP_DTYPE), *sc.size, spp=1, seed=SEED)
            self._tables[case] = tables(ids)
        return self._tables[case]

    def lamps(self, case, literal, emission):
        k = (literal, emission.tobytes())   # (every case is the same world)
        if k not in self._lists:
            self._lists[k] = self.lref.lamps(self.oracle_scene(case, 1, literal)[1], emission)
        return self._lists[k]

    def frame(self, case, kind, bounces=4, spp=1, literal=False, load=False, sample_base=0, size=None) -> Frame:
        """The reference frame of a kind of a case; load: with its load planes [spp, bounces, h, w]; size: the case's world, camera
        and tables in a frame of another size."""
        k = (case, kind, bounces, spp, literal, load, sample_base, size)
        if k not in self._frames:
            which, sun, setting, lamp = KINDS[kind]
            t = self.tables(case)[which]
            sc, o = self.oracle_scene(case, bounces, literal, size)
            lamps = self.lamps(case, literal, t[0]) if lamp[0] != 0.0 else np.zeros(0, lamp_ref.LAMP_DTYPE)
            planes = np.zeros((spp, bounces, sc.size[1], sc.size[0]), np.uint8) if load else None
            rgb, ids = self.lref.render(o, lamp, lamps, *sc.size, spp=spp, seed=SEED, sample_base=sample_base, sun=sun, setting=setting,
                                        emission=t[0], polish=t[1], translucency=t[2], load=planes)
            self._frames[k] = Frame(rgb, ids, self.lref.counts, planes)
        return self._frames[k]
