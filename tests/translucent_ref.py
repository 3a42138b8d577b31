"""The tests' reference for the emission, polish and translucency tables (vrt_write_emission, vrt_write_polish,
vrt_write_translucency): tests/path_ref.c's loop with every later term off — the oracle's loop with path_tracer.wgsl's emission
term, its coat and the pass-through lobe as include/vrt.h defines it.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import path_ref
from path_ref import translucency_table as table  # noqa: F401


class TranslucentRef:
    def __init__(self, ref: path_ref.PathRef):
        self._ref = ref
        self.passes = 0   # of the last render: how many times a path passed through a voxel

    def render(self, scene, emission, polish, translucency, w: int, h: int, spp: int = 1, seed: int = 0, sample_base: int = 0):
        """(rgb [h, w, 3] f32, ids [h, w] u32) of samples sample_base .. sample_base + spp - 1 under the three 256-entry tables
        (emission: float32; polish: POLISH_DTYPE; translucency: TRANSLUCENCY_DTYPE; None = zeros)."""
        rgb, ids, n = self._ref.render(scene, w, h, spp, seed, sample_base, emission=emission, polish=polish, translucency=translucency)
        self.passes = n.passes
        return rgb, ids


def load(directory) -> TranslucentRef:
    return TranslucentRef(path_ref.load(directory))
