"""The tests' reference for the emission and polish tables (vrt_write_emission, vrt_write_polish): tests/path_ref.c's loop with
every later term off — the oracle's loop with path_tracer.wgsl's emission term and its coat.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import path_ref
from path_ref import polish_table as table  # noqa: F401


class PolishRef:
    def __init__(self, ref: path_ref.PathRef):
        self._ref = ref
        self.polished_bounces = 0   # of the last render: how many bounces went off a coat

    def render(self, scene, emission, polish, w: int, h: int, spp: int = 1, seed: int = 0, sample_base: int = 0):
        """(rgb [h, w, 3] f32, ids [h, w] u32) of samples sample_base .. sample_base + spp - 1 under the two 256-entry tables
        (emission: float32, None = zeros; polish: POLISH_DTYPE, None = zeros)."""
        rgb, ids, n = self._ref.render(scene, w, h, spp, seed, sample_base, emission=emission, polish=polish)
        self.polished_bounces = n.polished_bounces
        return rgb, ids


def load(directory) -> PolishRef:
    return PolishRef(path_ref.load(directory))
