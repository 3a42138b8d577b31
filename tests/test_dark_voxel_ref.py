"""The dark rule of the voxel marks (tests/dark_voxel_ref.py; docs/NUMERICS.md "Dark stops", the voxels of split cells) on the
reference alone, without a GPU.

Hand-built dense worlds the rule must mark — a plate over a pit, where no cell carries the dark cell mark — mutations of them it
must refuse (a liquid plate, a corridor that touches the world's side, K_d = 0), and soundness against the oracle: on the procedural
worlds of 3^3 and 4^3 chunks, for the suns of tests/test_dark_cell_ref.py, shadow rays from up to 1 000 marked voxels — the centre,
the eight corners pulled in by the shadow bias, the centres of the faces towards the sun — must all come back `hit`.
"""
import numpy as np
import pytest

import dark_cell_ref as D
import dark_voxel_ref as V
import lit_corridor_ref as C
import lit_voxel_ref as R
import path_ref
from test_dark_cell_ref import BIAS, HIGH, LIQUID, N, STONE, SUNS, WATER
from voxelraytracing_amd import scenes

F = np.float32
K_LIT = 8    # the lit voxel marks' layers (vrt_lit.hip: lit_voxel_layers)
K_D = 16     # voxel layers of the dark walk in these tests


def marks(dense, sun, layers=K_D, liquid=LIQUID, cell_dark=None):
    """The dark voxels of a dense world, from the marks the references give it; and its dark cells."""
    n = dense.shape[0]
    lo = C.leaf_lo(dense)
    split = R.split_cells(dense)
    p = C.plan(n, sun)
    if cell_dark is None:
        cell_dark = D.dark(lo, D.floor_masks(dense, p[0] if p else 0, liquid), sun).astype(bool)
    cell_lit = C.lit(lo, sun, n // 4).astype(bool)
    lit = R.lit_voxels(dense, split, cell_lit, sun, K_LIT).astype(bool)
    dv = V.dark_voxels(dense, split, lit, cell_dark, sun, layers, liquid).astype(bool)
    assert not dv[dense != 0].any() and not (dv & lit).any() and not dv[np.repeat(np.repeat(np.repeat(~split, 4, 0), 4, 1), 4, 2)].any()
    return dv, cell_dark


def pit(plate=STONE, lid=0, whole=False):
    """Stone below y = 32, a pit of 2 x 2 x 4 air voxels in it (inside one cell, which it splits), and one voxel layer of `plate` at
    y = 33 over x, z = 16 .. 47 (or the whole world): the cells of y = 32 .. 35 under it are split, the air between is theirs."""
    dense = np.zeros((N, N, N), np.uint16)   # [z, y, x]
    dense[:, :32, :] = STONE
    dense[25:27, 28:32, 25:27] = 0
    if whole:
        dense[:, 33, :] = plate
    else:
        dense[16:48, 33, 16:48] = plate
    if lid:
        dense[25:27, 32, 25:27] = lid   # over the pit's mouth
    return dense


def test_a_plate_over_a_pit_without_any_dark_cell():
    dv, cells = marks(pit(), HIGH)
    assert C.plan(N, HIGH)[:2] == (1, True)
    assert not cells.any(), "a cell carries the dark cell mark: the case does not show what the voxel rule adds"
    assert dv[25, 32, 25] and dv[20, 32, 20], "the air between the ground and the plate"
    assert dv[25, 31, 25] and dv[26, 28, 26], "the pit: the plate is two to five voxel layers up"
    assert not dv[:, 34:, :].any(), "nothing is above the plate"
    # rays lean towards + x (0.5 a voxel of y) and + z (0.25): a voxel near those edges of the plate has rays that pass it
    assert dv[30, 32, 40] and not dv[30, 32, 47] and not dv[47, 32, 30]
    assert dv[30, 32, 16] and dv[16, 32, 30], "... and none towards - x or - z: an interval is one-sided"
    # depth: the voxel right under the plate needs one layer, the pit's floor five
    assert marks(pit(), HIGH, layers=1)[0][25, 32, 25] and not marks(pit(), HIGH, layers=1)[0][25, 31, 25]
    assert not marks(pit(), HIGH, layers=4)[0][25, 28, 25] and marks(pit(), HIGH, layers=5)[0][25, 28, 25]


def test_no_layers_no_marks():
    assert not marks(pit(), HIGH, layers=0)[0].any()


def test_a_liquid_closes_nothing_and_stops_nothing():
    assert not marks(pit(plate=WATER), HIGH)[0].any()
    assert marks(pit(plate=WATER), HIGH, liquid=np.zeros(256, bool))[0][25, 32, 25]
    # water over the pit's mouth, under the stone plate: the pit's voxels see the plate through it
    dv, _ = marks(pit(lid=WATER), HIGH)
    assert dv[25, 31, 25] and dv[26, 28, 26] and dv[20, 32, 20] and not dv[25, 32, 25]
    assert marks(pit(plate=300), HIGH)[0][25, 32, 25]   # (ids above 255 are material 255: no liquid here)


def test_a_corridor_that_touches_the_worlds_side():
    dv, _ = marks(pit(whole=True), HIGH)
    assert dv[30, 32, 40] and dv[0, 32, 0]
    assert not dv[30, 32, 63] and not dv[30, 32, 62], "rays of a voxel at the + x face lean out of the world"
    assert not dv[63, 32, 30], "... and at the + z face"
    assert dv[25, 31, 25]


def test_a_dark_cell_closes_its_voxels():
    """No plate: the pit's cell is the only split one, and nothing closes its voxels' corridors — until the air cells over the ground
    are declared dark: a voxel inside a cell with the dark cell mark is closed."""
    dense = pit(plate=0)
    cell_dark = np.zeros((N // 4,) * 3, bool)
    assert not marks(dense, HIGH, cell_dark=cell_dark)[0].any()
    cell_dark[:, 8, :] = True
    dv, _ = marks(dense, HIGH, cell_dark=cell_dark)
    assert dv[25, 31, 25] and dv[26, 28, 26]


def test_no_plan():
    assert C.plan(N, SUNS[4][1]) is None
    assert not marks(pit(), SUNS[4][1])[0].any()


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
    pts = [[x, y, z] for x in (e, 1 - e) for y in (e, 1 - e) for z in (e, 1 - e)] + [[0.5, 0.5, 0.5]]
    for a in range(3):
        p = [0.5, 0.5, 0.5]
        p[a] = 1 - e if toward[a] > 0 else e
        pts.append(p)
    return np.array(pts, F)


@pytest.mark.parametrize("chunks", [3, 4])
def test_every_ray_of_a_dark_voxel_hits(orc, worlds, chunks):
    sc, o, dense = worlds[chunks]
    n = dense.shape[0]
    wmin = o.c.world.min
    assert all(float(wmin[a]) == 0.0 for a in range(3))
    liquid = np.array([bool(sc.materials[i].is_liquid) for i in range(256)])
    rng = np.random.default_rng(20264)
    marked = 0
    for name, sun in SUNS:
        dv, cells = marks(dense, sun, liquid=liquid)
        if C.plan(n, sun) is None:
            assert not dv.any()
            continue
        at = np.argwhere(dv)
        print(f"{chunks}^3 sun {name}: dark cells {int(cells.sum())}, dark voxels at K_d = {K_D}: {len(at)}")
        marked += len(at)
        if len(at) > 1000:
            at = at[rng.choice(len(at), 1000, replace=False)]
        sun_local = np.array([F(F(sun[a]) - F(float(wmin[a]))) for a in range(3)], F)
        starts = _starts([1 if sun_local[a] > n / 2 else -1 for a in range(3)])
        for z, y, x in at:
            for s in starts:
                q = np.array([x, y, z], F) + s
                dr = (sun_local - q).astype(np.float64)
                dr = (dr / np.sqrt((dr * dr).sum())).astype(F)
                idw, _, _ = o.ray_world(q, dr)
                assert idw & orc.ID_HIT, (name, (int(x), int(y), int(z)), q, hex(idw))
    assert marked >= 1000, "hardly a voxel is marked: the case shows nothing"
