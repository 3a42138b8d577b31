"""Soundness of the lit rule (tests/lit_corridor_ref.py; docs/NUMERICS.md "Lit stops"), on the reference alone, without a GPU.

For the procedural worlds of 2^3 and 4^3 chunks, every sun of test_gpu_sun_marks.suns that gets marks and slab depths 1, 4 and the
whole corridor, every cell the rule lights is probed with the oracle's ray_world: from its eight corners, its centre and a
fixed-seed handful of interior points, each pulled 1e-3 inside the cell and aimed at the sun.  Every probe must miss.  (A probe's
outcome does not depend on the depth, so a cell that several depths light is probed once.)

So that the cases show something, on the 4^3 world every depth above 1 must light at least what depth 1 lights, and strictly more
cells.  One combination cannot, whatever the implementation: the sun below the horizon at depth 4.  The bottom layers of the
world are solid ground, so a ray towards that sun can only leave through a side face; its slopes are 0.25 and 0.15, a cell at the
face needs its rays 4 voxels further out before the interval it hands over lies outside the world, which takes a rise of at
least 16 + 5 voxels: 7 layers, and a slab of 4 hands over after 4 at the most.  There the counts are 0 at depth 1, 0 at depth 4
and 187 for the whole corridor, and depth 4 is held to "no fewer" only.  (The 2^3 world lies under water: no cell of it is an air
leaf, and the rule must light nothing there.)
"""
import numpy as np
import pytest

import lit_corridor_ref as R
import path_ref
from test_gpu_sun_marks import suns
from voxelraytracing_amd import scenes

F = np.float32
DEPTHS = (1, 4, None)   # None: the whole corridor
INTERIOR = np.random.default_rng(20251).uniform(0.0, 4.0, (4, 3))


def _starts():
    e = 1e-3
    corners = np.array([[x, y, z] for x in (e, 4 - e) for y in (e, 4 - e) for z in (e, 4 - e)])
    return np.concatenate([corners, [[2.0, 2.0, 2.0]], np.clip(INTERIOR, e, 4 - e)]).astype(F)


@pytest.fixture(scope="module")
def worlds(orc, tmp_path_factory):
    pr = path_ref.load(tmp_path_factory.mktemp("path_ref"))
    out = {}
    for chunks in (2, 4):
        sc = scenes.procedural(chunks, (64, 40))
        o = orc.from_package_scene(sc)
        out[chunks] = (sc, o, R.leaf_lo(pr.dense_world(o)))
    return out


def test_the_plan_is_the_hosts():
    for w in (64, 128, 320):
        for name, sun, marks in suns(w):
            p = R.plan(w, sun)
            assert (p is not None) == marks, (w, name)
            if p:
                assert p[2] == 3
    assert R.plan(256, suns(256)[0][1]) == (1, True, 3) and R.plan(512, suns(512)[0][1])[2] == 7 and R.plan(960, suns(960)[0][1])[2] == 15
    assert R.plan(2624, (0.0, 1e6, 0.0)) is None


@pytest.mark.parametrize("chunks", [2, 4])
def test_every_lit_cell_sees_the_sun(orc, worlds, chunks):
    sc, o, lo = worlds[chunks]
    G = lo.shape[0]
    starts = _starts()
    wmin = o.c.world.min
    probes = 0
    for name, sun, marks in suns(chunks * 32):
        if not marks:
            assert not R.lit(lo, sun, G).any(), name
            continue
        lit = {d: R.lit(lo, sun, d or G).astype(bool) for d in DEPTHS}
        free = R.lit(lo, sun, G, margins=False).astype(bool)
        counts = {d: int(v.sum()) for d, v in lit.items()}
        print(f"{chunks}^3 sun {name}: air cells {int((lo >= 0).sum())}, lit {counts}, without margins {int(free.sum())}")
        for d, v in lit.items():
            assert not v[lo < 0].any() and not (v & ~free).any(), (name, d)
            assert not (lit[1] & ~v).any(), (name, d, "a cell depth 1 lights is not lit")
        if chunks == 4:
            below = R.plan(chunks * 32, sun)[:2] == (1, False)
            assert counts[None] > counts[1], (name, counts)
            assert counts[4] > counts[1] or (below and counts[4] == counts[1]), (name, counts)
        sun_local = np.array([F(F(sun[a]) - F(float(wmin[a]))) for a in range(3)], F)
        assert not ((lit[1] | lit[4] | lit[None]) & ~free).any()
        for z, y, x in np.argwhere(free):   # (every depth's cells are among them)
            for s in starts:
                p = np.array([4 * x, 4 * y, 4 * z], F) + s
                d = (sun_local - p).astype(np.float64)
                d = (d / np.sqrt((d * d).sum())).astype(F)
                idw, _, _ = o.ray_world(p, d)
                assert not idw & orc.ID_HIT, (name, (int(x), int(y), int(z)), p, hex(idw))
                probes += 1
    print(f"{chunks}^3: {probes} probes, all missed")
    assert chunks == 2 or probes > 100000
