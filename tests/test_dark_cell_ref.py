"""The dark rule (tests/dark_cell_ref.py; docs/NUMERICS.md "Dark stops") on the reference alone, without a GPU.

Hand-built dense worlds the rule must mark, mutations of them it must refuse, and soundness against the oracle: on the procedural
worlds of 3^3 and 4^3 chunks, for the suns of tests/test_gpu_dark_marks.py, shadow rays from marked cells — the corners pulled in
by the shadow bias, the centre, the centres of the faces towards the sun — must all come back `hit`.
"""
import numpy as np
import pytest

import dark_cell_ref as D
import lit_corridor_ref as C
import path_ref
from voxelraytracing_amd import scenes

F = np.float32
STONE, WATER = 4, 3
LIQUID = np.zeros(256, bool)
LIQUID[WATER] = True
N = 64   # voxels a side of the hand-built worlds: 16 cells
HIGH = (10000.0, 20000.0, 5000.0)   # the plan's axis is y, the sun above; slopes 0.5 on x, 0.25 on z
LOW = (5000.0, 1500.0, 0.0)         # ... x, the sun beyond the high face; slopes 0.3 on y, about -0.01 on z
BIAS = 0.002                        # vrt_device.h kShadowBias
# (name, sun_pos): the suns of the GPU tests
SUNS = [("low +x", (5000.0, 1500.0, 0.0)), ("low +z", (200.0, 1200.0, 3000.0)), ("below the world", (100.0, -5000.0, 100.0)),
        ("the bench's", (10000.0, 20000.0, 5000.0)), ("no plan", (20000.0, 20000.0, 5000.0))]


def marks(dense, sun, liquid=LIQUID, **kw):
    p = C.plan(dense.shape[0], sun)
    masks = D.floor_masks(dense, p[0] if p else 0, liquid)
    return D.dark(C.leaf_lo(dense), masks, sun, **kw).astype(bool)


def roof(voxel=STONE):
    """A slab roof, y = 48 .. 51 over the whole world, and a cavity of air under it."""
    dense = np.zeros((N, N, N), np.uint16)   # [z, y, x]
    dense[:, 48:52, :] = voxel
    return dense


def sheet(y_of_x=lambda x: 50):
    """One voxel layer over the whole world: the cells it crosses are split, one of their four voxel layers closed."""
    dense = np.zeros((N, N, N), np.uint16)
    for x in range(N):
        dense[:, y_of_x(x), x] = STONE
    return dense


def test_floor_masks():
    dense = sheet()
    m = D.floor_masks(dense, 1, LIQUID)
    assert (m[:, 12, :] == 1 << 2).all() and (np.delete(m, 12, axis=1) == 0).all()
    assert (D.floor_masks(dense, 0, LIQUID) == 0).all() and (D.floor_masks(dense, 2, LIQUID) == 0).all()
    m = D.floor_masks(roof(), 1, LIQUID)
    assert (m[:, 12, :] == 15).all() and (D.floor_masks(roof(), 0, LIQUID)[:, 12, :] == 15).all()
    assert (D.floor_masks(roof(WATER), 1, LIQUID) == 0).all()
    assert (D.floor_masks(roof(300), 1, LIQUID) == 15).all(axis=(0, 2))[12]   # (ids above 255 are material 255: no liquid here)


def test_a_slab_roof_over_a_cavity():
    d = marks(roof(), HIGH)
    assert d[8, 8, 8] and d[8, 11, 8] and d[8, 0, 8]            # [z, y, x]: under the roof, at any depth below it
    assert not d[:, 12:, :].any()                                # the roof itself and the air above it
    # a corridor that touches the world's side before the blocker: the rays lean towards + x and + z
    assert not d[8, 8, 15] and not d[15, 8, 8] and d[8, 11, 13] and not d[8, 11, 14] and not d[8, 0, 12]
    # depth: the cell right under the roof needs one layer, one four cells down five
    assert marks(roof(), HIGH, depth=1)[8, 11, 8] and not marks(roof(), HIGH, depth=1)[8, 10, 8]
    assert not marks(roof(), HIGH, depth=3)[8, 8, 8] and marks(roof(), HIGH, depth=4)[8, 8, 8]
    assert not marks(roof(), HIGH, depth=0).any()


def test_a_wall_towards_a_low_sun():
    dense = np.zeros((N, N, N), np.uint16)
    dense[:, :, 48:52] = STONE
    d = marks(dense, LOW)
    assert C.plan(N, LOW)[:2] == (0, True)
    assert d[8, 8, 6] and d[8, 2, 11] and not d[:, :, 12:].any()
    assert not d[0, 8, 6], "rays of a cell at the z = 0 face lean out of the world"
    assert not d[8, 15, 6], "rays of a cell at the top face climb out of the world"


def test_one_closed_voxel_layer_shared_by_split_cells():
    d = marks(sheet(), HIGH)
    assert d[8, 8, 8] and d[8, 11, 8]
    lo = C.leaf_lo(sheet())
    assert (lo[:, 12, :] < 0).all(), "the sheet's cells are not split: the case shows nothing"


def test_one_voxel_missing_from_the_shared_layer():
    dense = sheet()
    dense[36, 50, 42] = 0   # in cell [9, 12, 10], which rays of cell [8, 8, 8] can be in
    d = marks(dense, HIGH)
    assert not d[8, 8, 8] and marks(sheet(), HIGH)[8, 8, 8]
    assert d[2, 8, 2], "a cell whose rays stay clear of the hole is still dark"


def test_closed_layers_at_different_heights():
    d = marks(sheet(lambda x: 50 if x < 40 else 49), HIGH)
    assert not d[8, 8, 8], "cells 9 and 10 of the corridor have their closed layers at y = 50 and y = 49"
    assert d[8, 8, 2] and d[8, 8, 12], "corridors on one side of the step share a layer"


def test_a_blocker_of_a_liquid():
    assert not marks(roof(WATER), HIGH).any()
    none = np.zeros(256, bool)
    assert marks(roof(WATER), HIGH, liquid=none)[8, 8, 8]


def test_no_plan():
    assert C.plan(N, SUNS[4][1]) is None
    assert not marks(roof(), SUNS[4][1]).any()


def test_transitivity_adds_nothing_under_a_roof():
    assert np.array_equal(marks(roof(), HIGH), marks(roof(), HIGH, transitive=True))


@pytest.fixture(scope="module")
def worlds(orc, tmp_path_factory):
    pr = path_ref.load(tmp_path_factory.mktemp("path_ref"))
    out = {}
    for chunks in (3, 4):
        sc = scenes.procedural(chunks, (64, 40))
        o = orc.from_package_scene(sc)
        out[chunks] = (sc, o, pr.dense_world(o))
    return out


def _starts(toward):
    """toward: per axis + 1 / - 1, the side the sun lies on."""
    e = BIAS
    pts = [[x, y, z] for x in (e, 4 - e) for y in (e, 4 - e) for z in (e, 4 - e)] + [[2.0, 2.0, 2.0]]
    for a in range(3):
        p = [2.0, 2.0, 2.0]
        p[a] = 4 - e if toward[a] > 0 else e
        pts.append(p)
    return np.array(pts, F)


@pytest.mark.parametrize("chunks", [3, 4])
def test_every_ray_of_a_dark_cell_hits(orc, worlds, chunks):
    sc, o, dense = worlds[chunks]
    n = dense.shape[0]
    wmin = o.c.world.min
    assert all(float(wmin[a]) == 0.0 for a in range(3))
    liquid = np.array([bool(sc.materials[i].is_liquid) for i in range(256)])
    lo = C.leaf_lo(dense)
    rng = np.random.default_rng(20263)
    for name, sun in SUNS:
        p = C.plan(n, sun)
        if p is None:
            assert not marks(dense, sun, liquid).any()
            continue
        d = marks(dense, sun, liquid)
        t = marks(dense, sun, liquid, transitive=True)
        assert not d[lo < 0].any() and not (d & ~t).any()
        cells = np.argwhere(t)   # (every cell of the plain rule is among them)
        print(f"{chunks}^3 sun {name}: air cells {int((lo >= 0).sum())}, dark {int(d.sum())}, with transitivity {int(t.sum())}")
        if len(cells) > 1000:
            cells = cells[rng.choice(len(cells), 1000, replace=False)]
        sun_local = np.array([F(F(sun[a]) - F(float(wmin[a]))) for a in range(3)], F)
        starts = _starts([1 if sun_local[a] > n / 2 else -1 for a in range(3)])
        for z, y, x in cells:
            for s in starts:
                q = np.array([4 * x, 4 * y, 4 * z], F) + s
                dr = (sun_local - q).astype(np.float64)
                dr = (dr / np.sqrt((dr * dr).sum())).astype(F)
                idw, _, _ = o.ray_world(q, dr)
                assert idw & orc.ID_HIT, (name, (int(x), int(y), int(z)), q, hex(idw))
