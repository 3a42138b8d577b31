"""Soundness of the voxel marks' rule (tests/lit_voxel_ref.py; docs/NUMERICS.md "Lit stops"), on the reference alone, without a GPU.

The procedural worlds of 4^3 and 8^3 chunks (the bench's), four suns: the bench's (the sun's axis is y), one beyond -x, one beyond
+z and one below the horizon.  The cell marks are the corridor rule's (tests/lit_corridor_ref.py, the whole corridor); the voxel
marks are made for 4, 8 and 16 layers.  From a fixed-seed sample of the voxels the rule lights, shadow rays are cast with the
oracle's ray_world: from the voxel's eight corners pulled in by the shadow bias, its centre, and the centres of its three faces
towards the sun.  Every ray must miss, and within the lookups the step budget leaves it: B + 1 of the cell marks (B = 6 (W / L + 1)
+ 2) plus the voxel marks' budget for the smallest layer count that lights the voxel.  More layers light no fewer voxels, the
rule without margins lights no fewer than the rule with them, and the rule lights something on every world and sun above the
horizon: the counts are printed (profiles/lit_voxels_ab.txt holds them).
"""
import numpy as np
import pytest

import lit_corridor_ref as C
import lit_voxel_ref as R
import path_ref
from test_gpu_sun_marks import suns
from voxelraytracing_amd import scenes

F = np.float32
LAYERS = (4, 8, 16)
SAMPLE = 1200          # lit voxels probed per world and sun
BIAS = 0.002           # vrt_device.h kShadowBias: where a shadow ray starts over a face
MAX_STEPS = 500


def _suns(w):
    by_name = {name: sun for name, sun, _ in suns(w)}
    return [("the bench's", tuple(scenes.SUN_POS)), ("-x", by_name["-x"]), ("+z", by_name["+z"]), ("below the horizon", by_name["below the horizon"])]


def _starts(sun_local, corner):
    """Offsets inside the unit voxel at `corner`: the eight corners pulled in by the bias, the centre, and the three faces on the sun's side."""
    e = BIAS
    pts = [[x, y, z] for x in (e, 1 - e) for y in (e, 1 - e) for z in (e, 1 - e)] + [[0.5, 0.5, 0.5]]
    for ax in range(3):
        f = [0.5, 0.5, 0.5]
        f[ax] = 1 - e if sun_local[ax] > corner[ax] else e
        pts.append(f)
    return np.array(pts, F)


@pytest.fixture(scope="module")
def worlds(orc, tmp_path_factory):
    pr = path_ref.load(tmp_path_factory.mktemp("path_ref"))
    out = {}
    for chunks in (4, 8):
        sc = scenes.procedural(chunks, (64, 40))
        o = orc.from_package_scene(sc)
        dense = pr.dense_world(o)
        out[chunks] = (o, dense, C.leaf_lo(dense), R.split_cells(dense), sc)   # (sc: the oracle reads the scene's own arrays)
    return out


def test_the_budget_leaves_room():
    # W = 256: the cell marks stop a ray below 107 trips; eight voxel layers take 60 of them
    assert R.budget(8) == 60 and R.budget(4) == 36 and MAX_STEPS - (6 * (256 // 4 + 1) + 2) - 1 - R.budget(8) == 47


@pytest.mark.parametrize("chunks", [4, 8])
def test_every_lit_voxel_sees_the_sun(orc, worlds, chunks):
    o, dense, lo, split, _ = worlds[chunks]
    n = dense.shape[0]
    G = n // 4
    wmin = o.c.world.min
    rng = np.random.default_rng(20261 + chunks)
    cand = int((np.repeat(np.repeat(np.repeat(split, 4, 0), 4, 1), 4, 2) & (dense == 0)).sum())
    assert cand > 1000
    probes = 0
    for name, sun in _suns(n):
        plan = C.plan(n, sun)
        assert plan is not None, name
        B = 6 * (n // (plan[2] + 1) + 1) + 2
        cell_lit = C.lit(lo, sun, G).astype(bool)
        lit = {k: R.lit_voxels(dense, split, cell_lit, sun, k).astype(bool) for k in LAYERS}
        free = R.lit_voxels(dense, split, cell_lit, sun, LAYERS[-1], margins=False).astype(bool)
        counts = {k: int(v.sum()) for k, v in lit.items()}
        print(f"{chunks}^3 sun {name}: air voxels of split cells {cand}, air cells lit {int(cell_lit.sum())} of {int((lo >= 0).sum())}, "
              f"voxels lit by layers {counts} ({100.0 * counts[8] / cand:.1f} % at 8), without margins {int(free.sum())}")
        for k, v in lit.items():
            assert not v[dense != 0].any(), (name, k, "a lit voxel that is not air")
            assert not (v & ~free).any(), (name, k)
        assert not (lit[4] & ~lit[8]).any() and not (lit[8] & ~lit[16]).any(), name
        if name != "below the horizon":
            assert counts[4] > 0 and counts[16] > counts[4], (name, counts)
        first_k = np.where(lit[4], 4, np.where(lit[8], 8, 16))
        sun_local = np.array([F(F(sun[a]) - F(float(wmin[a]))) for a in range(3)], F)
        at = np.argwhere(lit[16])
        if len(at) > SAMPLE:
            at = at[rng.choice(len(at), SAMPLE, replace=False)]
        for z, y, x in at:
            corner = np.array([x, y, z], F)
            allowed = B + 1 + R.budget(int(first_k[z, y, x]))
            for s in _starts(sun_local, corner):
                p = corner + s
                d = (sun_local - p).astype(np.float64)
                d = (d / np.sqrt((d * d).sum())).astype(F)
                idw, _, res = o.ray_world(p, d)
                assert not idw & orc.ID_HIT, (name, (int(x), int(y), int(z)), p, hex(idw))
                assert res[7] <= min(allowed, MAX_STEPS), (name, (int(x), int(y), int(z)), p, res[7], allowed)
                probes += 1
    print(f"{chunks}^3: {probes} probes, all missed within their budgets")
    assert probes > 10000
