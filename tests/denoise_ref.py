"""ctypes wrapper of tests/denoise_ref.c: the a-trous filter of vrt_set_denoise as include/vrt.h words it, in plain C, and the
guide words from the oracle's primary march.  TEST INFRASTRUCTURE ONLY.

``load(directory)`` compiles it with oracle/Makefile's own CFLAGS (strict IEEE: no contraction, no fast-math) into
`directory` — a pytest temporary directory, never the source tree — and loads it; the scene struct is oracle/orc.py's."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from oracle import orc

from emission_ref import oracle_cflags

_HERE = os.path.dirname(os.path.abspath(__file__))


class DenoiseRef:
    def __init__(self, so: str):
        L = C.CDLL(so)
        u32, vp = C.c_uint32, C.c_void_p
        L.ref_guide.restype = None
        L.ref_guide.argtypes = [C.POINTER(orc.Scene), u32, u32, vp, vp]
        L.ref_denoise.restype = None
        L.ref_denoise.argtypes = [vp, vp, vp, u32, u32, u32, C.c_float, vp, vp]
        self._lib = L

    def guide(self, scene: "orc.OracleScene", w: int, h: int):
        """(guide [h, w] u32, ids [h, w] u32) of the scene's camera."""
        g = np.zeros((h, w), dtype=np.uint32)
        ids = np.zeros((h, w), dtype=np.uint32)
        self._lib.ref_guide(C.byref(scene.c), w, h, g.ctypes.data, ids.ctypes.data)
        return g, ids

    def denoise(self, rgb, ids, guide, passes: int, sigma_color: float = 0.0) -> np.ndarray:
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        h, w = rgb.shape[:2]
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(h, w)
        guide = np.ascontiguousarray(guide, dtype=np.uint32).reshape(h, w)
        out, tmp = np.empty_like(rgb), np.empty_like(rgb)
        self._lib.ref_denoise(rgb.ctypes.data, ids.ctypes.data, guide.ctypes.data, w, h, passes, float(sigma_color),
                              out.ctypes.data, tmp.ctypes.data)
        return out


def load(directory) -> DenoiseRef:
    """Compile tests/denoise_ref.c into `directory` and load it."""
    so = os.path.join(str(directory), "libdenoise_ref.so")
    cc = os.environ.get("CC", "gcc")
    subprocess.check_call([cc, *oracle_cflags(), "-shared", "-o", so, os.path.join(_HERE, "denoise_ref.c"), "-lm"])
    return DenoiseRef(so)


def bits(a) -> np.ndarray:
    """The bit patterns of an f32 array (NaNs compare by payload)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
