"""The tests' reference for direct sunlight (vrt_set_sun_light) on top of the emission, polish and translucency tables:
tests/path_ref.c's loop with camera sampling and lamp light off — a sun ray from every hit, as include/vrt.h defines it.  TEST
INFRASTRUCTURE ONLY."""
from __future__ import annotations

from collections import namedtuple

import path_ref
from path_ref import _tables  # noqa: F401

# of one render: the sun rays marched, the unoccluded ones, the later segments' misses through the sun's disc, the lookups of
# every march (path segments and sun rays), the path segments behind the primary ones
Counts = namedtuple("Counts", "sun_rays unoccluded disc_misses steps bounce_segments")


def _counts(n: path_ref.Counts) -> Counts:
    return Counts(n.sun_rays, n.sun_unoccluded, n.disc_misses, n.steps, n.bounce_segments)


class SunRef:
    def __init__(self, ref: path_ref.PathRef):
        self._ref = ref
        self.counts = Counts(0, 0, 0, 0, 0)   # of the last render

    def render(self, scene, strength: float, w: int, h: int, spp: int = 1, seed: int = 0, sample_base: int = 0, emission=None, polish=None,
               translucency=None):
        """(rgb [h, w, 3] f32, ids [h, w] u32) of samples sample_base .. sample_base + spp - 1 with the sun term's factor
        `strength` (0: off) under the three 256-entry tables (None = zeros)."""
        rgb, ids, n = self._ref.render(scene, w, h, spp, seed, sample_base, sun=strength, emission=emission, polish=polish, translucency=translucency)
        self.counts = _counts(n)
        return rgb, ids

    def trace_pixel(self, scene, strength: float, w: int, h: int, px: int, py: int, sample: int = 0, seed: int = 0, emission=None, polish=None,
                    translucency=None):
        """(light [3] f32, Counts) of one sample of one pixel of a w x h frame."""
        light, _, _, n = self._ref.trace_pixel(scene, w, h, px, py, sample, seed, sun=strength, emission=emission, polish=polish,
                                               translucency=translucency)
        return light, _counts(n)


def load(directory) -> SunRef:
    return SunRef(path_ref.load(directory))
