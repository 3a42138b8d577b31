"""The tests' reference for camera sampling (vrt_set_camera_sampling) on top of direct sunlight and the emission, polish and
translucency tables: tests/path_ref.c's loop with lamp light off — a primary ray of its own for every sample, as include/vrt.h
defines it.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from collections import namedtuple

import path_ref
from path_ref import OFF  # noqa: F401

# of one render: the lookups of every march (the centre ray's, the path segments', the sun rays'), the path segments behind the
# primary ones, the sun rays marched, the samples whose own primary id word is not the centre ray's, the samples with o' != origin
Counts = namedtuple("Counts", "steps bounce_segments sun_rays jitter_changed lens_moved")


class LensRef:
    def __init__(self, ref: path_ref.PathRef):
        self._ref = ref
        self.counts = Counts(0, 0, 0, 0, 0)   # of the last render

    def render(self, scene, setting, w: int, h: int, spp: int = 1, seed: int = 0, sample_base: int = 0, strength: float = 0.0, emission=None,
               polish=None, translucency=None):
        """(rgb [h, w, 3] f32, ids [h, w] u32) of samples sample_base .. sample_base + spp - 1 under the camera sampling
        `setting` = (pixel_spread, aperture, focus_distance) (OFF: tests/sun_ref.py's frame), the sun term's factor `strength`
        and the three 256-entry tables (None = zeros)."""
        rgb, ids, n = self._ref.render(scene, w, h, spp, seed, sample_base, sun=strength, setting=setting, emission=emission, polish=polish,
                                       translucency=translucency)
        self.counts = Counts(n.steps, n.bounce_segments, n.sun_rays, n.jitter_changed, n.lens_moved)
        return rgb, ids

    def ray(self, scene, setting, px: int, py: int, u):
        """The reference's ray of one sample from the draws u[4]: [w, o', F - o' (w for a pinhole), d'] as a [4, 3] f32 array."""
        return self._ref.lens_ray(scene, setting, px, py, u)

    def trace_pixel(self, scene, setting, w: int, h: int, px: int, py: int, sample: int = 0, seed: int = 0, strength: float = 0.0, emission=None,
                    polish=None, translucency=None):
        """(light [3] f32, the id word of the sample's own primary segment, its draws u[4]) of one sample of one pixel."""
        return self._ref.trace_pixel(scene, w, h, px, py, sample, seed, sun=strength, setting=setting, emission=emission, polish=polish,
                                     translucency=translucency)[:3]


def load(directory) -> LensRef:
    return LensRef(path_ref.load(directory))
