"""The tests' reference for the per-material emission table (vrt_write_emission): tests/path_ref.c's loop with every later term
off — the oracle's loop with path_tracer.wgsl's emission term.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import path_ref
from path_ref import oracle_cflags  # noqa: F401  (tests/denoise_ref.py and the tests take it from here)


class EmissionRef:
    def __init__(self, ref: path_ref.PathRef):
        self._ref = ref

    def render(self, scene, emission, w: int, h: int, spp: int = 1, seed: int = 0, sample_base: int = 0):
        """(rgb [h, w, 3] f32, ids [h, w] u32) of samples sample_base .. sample_base + spp - 1 under the 256-entry table."""
        return self._ref.render(scene, w, h, spp, seed, sample_base, emission=emission)[:2]


def load(directory) -> EmissionRef:
    return EmissionRef(path_ref.load(directory))
