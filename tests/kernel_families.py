"""The path trace's kernel templates by their mangled names, for the tests that count instantiations (tests/test_*_api.py,
tests/test_abi.py): which template a symbol of libvrt.so instantiates, with which arguments, and the family it belongs to —
the word the family's kernels had in their names while each family was a set of kernels of its own.

    path_primary_kernel<MARCH, LDS_ROOTS, STATS, MULTI, EMIT, POLISH, TRANSLUCENT, SUN...>(FrameParams, SUN...)
    path_bounce_kernel<MARCH, LDS_ROOTS, STATS, EMIT, POLISH, TRANSLUCENT, SUN...>(FrameParams, SUN...)
    path_bounce_cells_kernel<DIRECT, KB, EMIT, POLISH, TRANSLUCENT>(CellsLaunch)
    path_lens_primary_kernel<MARCH, LDS_ROOTS, STATS, MULTI, SUN...>(FrameParams, LensLaunch, SUN...)

and the pair of a water frame, a family of its own ("water") whose lobes and sun are read from the launch:

    path_water_primary_kernel<MARCH, LDS_ROOTS, STATS>(FrameParams, FrameParams, WaterLaunch, SunLaunch)
    path_water_bounce_kernel<MARCH, LDS_ROOTS, STATS>(FrameParams, FrameParams, WaterLaunch, SunLaunch)
"""
import re

_SYMBOL = re.compile(r"^_ZN3vrt\d+path_(primary|bounce|bounce_cells|lens_primary)_kernelI((?:L[ibj]\d+E)+)(?:J(NS_9SunLaunchE)?E)?EEv")
_WATER = re.compile(r"^_ZN3vrt\d+path_water_(primary|bounce)_kernelI(Li\dELb\dELb\dE)EEv")
_FLAGS = {"primary": ("multi", "emit", "polish", "translucent"), "bounce": ("emit", "polish", "translucent"),
          "bounce_cells": ("emit", "polish", "translucent"), "lens_primary": ("multi",)}


def path_kernel(symbol):
    """None, or {"template", "build", "multi", "emit", "polish", "translucent", "sun"} of a symbol of the four templates above.
    build: the mangled arguments that choose the march (MARCH, LDS_ROOTS, STATS) or the pool (DIRECT, KB), e.g. "Li1ELb0ELb1E"."""
    m = _SYMBOL.match(symbol)
    if not m:
        return None
    args = re.findall(r"L[ibj]\d+E", m.group(2))
    n_build = 2 if m.group(1) == "bounce_cells" else 3
    flags = _FLAGS[m.group(1)]
    assert len(args) == n_build + len(flags), symbol
    k = {"template": m.group(1), "build": "".join(args[:n_build]), "multi": False, "emit": False, "polish": False,
         "translucent": False, "sun": m.group(3) is not None}
    for name, a in zip(flags, args[n_build:]):
        assert a in ("Lb0E", "Lb1E"), symbol
        k[name] = a == "Lb1E"
    return k


def water_kernel(symbol):
    """None, or {"template": "water_primary" | "water_bounce", "build", "march", "lds_roots", "stats"} of a symbol of the water pair."""
    m = _WATER.match(symbol)
    if not m:
        return None
    march, roots, stats = re.findall(r"L[ib](\d)E", m.group(2))
    return {"template": "water_" + m.group(1), "build": m.group(2), "march": int(march), "lds_roots": roots == "1", "stats": stats == "1"}


# the march builds vrt_path.hip's with_march_build chooses between: the grid march (0) never stages the root table in LDS, the
# literal march (1) and the octree walk (2) do where it fits; each counting (STATS) and not
MARCH_BUILDS = tuple(f"Li{m}ELb{r}ELb{s}E" for m, roots in ((0, (0,)), (1, (0, 1)), (2, (0, 1))) for r in roots for s in (0, 1))


def families(symbol):
    """The families a kernel is counted in: "polished", "translucent", "sunlit" (the trace kernels that take a SunLaunch behind
    FrameParams alone), "emissive" (the pool kernel with the emission term and no lobe besides), "lens"; "water": the water pair."""
    if water_kernel(symbol) is not None:
        return frozenset({"water"})
    k = path_kernel(symbol)
    if k is None:
        return frozenset()
    f = set()
    if k["template"] == "lens_primary":
        f.add("lens")
    elif k["sun"]:
        f.add("sunlit")
    elif k["polish"]:
        f.add("polished")
    elif k["translucent"]:
        f.add("translucent")
    elif k["template"] == "bounce_cells" and k["emit"]:
        f.add("emissive")
    return frozenset(f)


def in_family(symbol, family):
    return family in families(symbol)
