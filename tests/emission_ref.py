"""ctypes wrapper of tests/emission_ref.c: the path trace with the per-material emission table (vrt_write_emission), the
oracle's loop with path_tracer.wgsl's emission term.  TEST INFRASTRUCTURE ONLY.

``load(directory)`` compiles it with oracle/Makefile's own CFLAGS (strict IEEE: no contraction, no fast-math) into
`directory` — a pytest temporary directory, never the source tree — and loads it; the scene struct is oracle/orc.py's."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np

from oracle import orc

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)


def oracle_cflags() -> list[str]:
    """CFLAGS of oracle/Makefile, as written there (continuation lines joined)."""
    text = open(os.path.join(_ROOT, "oracle", "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^CFLAGS\s*=(.*)$", text, re.M)
    assert m, "oracle/Makefile has no CFLAGS line"
    return m.group(1).split()


class EmissionRef:
    def __init__(self, so: str):
        L = C.CDLL(so)
        u32 = C.c_uint32
        L.ref_render_path_emissive.restype = None
        L.ref_render_path_emissive.argtypes = [C.POINTER(orc.Scene), C.POINTER(C.c_float), u32, u32, u32, u32, u32, C.c_void_p, C.c_void_p]
        self._lib = L

    def render(self, scene: "orc.OracleScene", emission, w: int, h: int, spp: int = 1, seed: int = 0, sample_base: int = 0):
        """(rgb [h, w, 3] f32, ids [h, w] u32) of samples sample_base .. sample_base + spp - 1 under the 256-entry table."""
        e = np.zeros(256, dtype=np.float32)
        em = np.asarray(emission, dtype=np.float32).reshape(-1)
        e[:em.size] = em
        rgb = np.zeros((h, w, 3), dtype=np.float32)
        ids = np.zeros((h, w), dtype=np.uint32)
        self._lib.ref_render_path_emissive(C.byref(scene.c), e.ctypes.data_as(C.POINTER(C.c_float)), w, h, spp, seed, sample_base,
                                           rgb.ctypes.data, ids.ctypes.data)
        return rgb, ids


def load(directory) -> EmissionRef:
    """Compile tests/emission_ref.c into `directory` and load it."""
    so = os.path.join(str(directory), "libemission_ref.so")
    cc = os.environ.get("CC", "gcc")
    subprocess.check_call([cc, *oracle_cflags(), "-shared", "-o", so, os.path.join(_HERE, "emission_ref.c"), "-lm"])
    return EmissionRef(so)
