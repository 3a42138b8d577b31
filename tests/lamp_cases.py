"""Worlds and scenes for the lamp tests (vrt_set_lamp_light): a hand-made world that holds every kind of lamp the list build has a
path for, a sealed room for the estimator test, worlds of 9^3 and 11^3 chunks whose lamps sit where the list build's scan has a
path for, random worlds with voxel ids above 255, and the cameras from which lamp rays reach every kind of the hand-made world's
lamps.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from voxelraytracing_amd import MODE_PATH, scenes
from voxelraytracing_amd import world as W
from voxelraytracing_amd.world import ClientWorld, svo_build_by_set_node

STONE, WATER, LAMP, ORE = 4, 3, 7, 9   # (ORE: a second lamp material, emissive only in some tables)
S = 2                                  # the hand-made world: 2^3 chunks, the top layer of chunks missing (root 0)


def _at(x, y, z):
    return x + 32 * (y + 32 * z)


def hand_made_blocks():
    """{chunk position: dense block} of the hand-made world.  In chunk (0, 0, 0), over a stone floor: a lone lamp voxel (a split
    cell, depth 5), an aligned 2^3 block (a size-2 leaf), an aligned 8^3 block (one leaf over eight cells: only its surface is
    listed), a lamp in the world's corner (two faces look out of the world box), a lamp under water (every face looks at a
    liquid), a lamp under the missing chunk above (its +y face looks at a chunk whose root is 0), a lamp buried in stone (no
    face) and a pair across the border to chunk (1, 0, 0) (the faces between them are not listed)."""
    a = np.zeros(32768, np.uint16)
    x, y, z = np.meshgrid(np.arange(32), np.arange(32), np.arange(32), indexing="ij")
    a[_at(x, y, z)[y < 4]] = STONE
    a[_at(5, 6, 5)] = LAMP
    a[_at(x, y, z)[(x >= 10) & (x < 12) & (y >= 6) & (y < 8) & (z >= 10) & (z < 12)]] = LAMP
    a[_at(x, y, z)[(x >= 16) & (x < 24) & (y >= 8) & (y < 16) & (z >= 16) & (z < 24)]] = LAMP
    a[_at(0, 10, 0)] = LAMP
    a[_at(x, y, z)[(abs(x - 12) <= 1) & (abs(y - 20) <= 1) & (abs(z - 12) <= 1)]] = WATER
    a[_at(12, 20, 12)] = LAMP
    a[_at(5, 31, 20)] = LAMP
    a[_at(7, 1, 7)] = ORE
    a[_at(31, 10, 5)] = LAMP
    b = np.zeros(32768, np.uint16)
    b[_at(x, y, z)[y < 4]] = STONE
    b[_at(0, 10, 5)] = LAMP
    b[_at(3, 4, 3)] = ORE
    c = np.zeros(32768, np.uint16)
    c[_at(x, y, z)[y < 4]] = STONE
    return {(0, 0, 0): a, (1, 0, 0): b, (0, 0, 1): c, (1, 0, 1): c.copy()}


def hand_made_world() -> ClientWorld:
    world = ClientWorld((S // 2,) * 3, 1 << 20, S)   # min chunk (0, 0, 0)
    for pos, dense in hand_made_blocks().items():
        world.create_chunk(pos, svo_build_by_set_node(dense))
    return world


def hand_made_scene(world, size=(8, 8), bounces=2, eye=(14.5, 12.5, 3.5), rot=(10.0, 20.0, 0.0)):
    sc = scenes._scene("hand-made lamps", world, size, eye, rot, MODE_PATH)
    sc.settings.max_ray_bounces = bounces
    scenes._diffuse(sc.materials)
    return sc


def emission(**entries):
    t = np.zeros(256, np.float32)
    for k, v in entries.items():
        t[{"lamp": LAMP, "ore": ORE, "stone": STONE, "water": WATER}[k]] = v
    return t


ROOM_R = 8.5


def room_world():
    """One chunk of solid stone with a spherical room carved around its centre and lamp voxels in the wall, through the host
    mirror's shapes (apply_shapes: a sphere of voxel 0, then points).  Returns (world, the lamp positions)."""
    dense = np.full(32768, STONE, np.uint16)
    carved = W.apply_shapes(dense, (0, 0, 0), [W.shape_sphere((16, 16, 16), ROOM_R, 0)])
    x, y, z = np.meshgrid(np.arange(32), np.arange(32), np.arange(32), indexing="ij")
    air = (carved[_at(x, y, z)] == 0)
    # wall voxels that touch the room: the first of them along a few lines from the centre
    lamps = []
    for d in ((1, 0, 0), (0, 1, 0), (0, 0, -1), (-1, 0, 0), (0, 0, 1)):
        p = np.array([16, 16, 16])
        while air[tuple(p)]:
            p = p + d
        lamps.append(tuple(int(v) for v in p))
    dense = W.apply_shapes(dense, (0, 0, 0), [W.shape_sphere((16, 16, 16), ROOM_R, 0)] + [W.shape_point(p, LAMP) for p in lamps])
    world = ClientWorld((0, 0, 0), 1 << 18, 1)
    world.create_chunk((0, 0, 0), svo_build_by_set_node(dense))
    return world, lamps


def room_scene(world, size=(8, 8), bounces=2):
    sc = scenes._scene("lamp room", world, size, (16.5, 16.5, 16.5), (10.0, 30.0, 0.0), MODE_PATH)
    sc.settings.max_ray_bounces = bounces
    scenes._diffuse(sc.materials)
    return sc


# ---- worlds for the list build's scan and cap (tests/test_gpu_lamp_list.py) ----

BIG = 300   # a voxel id above 255: it reads entry 255 of every table, and the list carries it unclamped


def _lamp_in_the_last_cell():
    """hand_made_blocks()' chunk (0, 0, 0) with a lamp in its last voxel: as the world's last chunk, that is the world's last
    depth-3 cell, and +x, +y, +z look out of the world box."""
    d = hand_made_blocks()[(0, 0, 0)].copy()
    d[_at(31, 31, 31)] = LAMP
    return d


def scan_blocks(S):
    """{chunk position: dense block} of scan_world(S): the hand-made world in the corner at (0, 0, 0), its chunk (0, 0, 0) twice
    more on top of each other in the middle of the world, and once more as the last chunk with a lamp in the world's last cell.
    Then a lamp voxel in the air of the middle chunks in each of four consecutive workgroups of the list build (256 consecutive
    depth-3 cells, x fastest over the world's (8 S)^3): whatever per = ceil(n_blocks / 1024) in 2..3 is, two of them share a
    scan thread and two neighbours do not."""
    hm = hand_made_blocks()
    m = S // 2
    blocks = {pos: d.copy() for pos, d in hm.items()}
    blocks[(m, m, m)] = hm[(0, 0, 0)].copy()
    blocks[(m, m + 1, m)] = hm[(0, 0, 0)].copy()
    blocks[(S - 1, S - 1, S - 1)] = _lamp_in_the_last_cell()
    G = 8 * S
    gz = 8 * m + 7                                         # a plane of cells above everything else in the two chunks
    rows = [(gz * G + gy) * G + 8 * m for gy in range(8 * m + 1, 8 * m + 16) if gy != 8 * m + 8]   # the first cell of each row of theirs above a floor
    by_group = {}
    for c in rows:
        by_group.setdefault(c // 256, c)
    first = next(b for b in sorted(by_group) if all(b + i in by_group for i in range(4)))
    for b in range(first, first + 4):
        c = by_group[b]
        x, y, z = 4 * (c % G) + 1, 4 * ((c // G) % G) + 1, 4 * (c // (G * G)) + 1
        d = blocks[(x >> 5, y >> 5, z >> 5)]
        assert d[_at(x & 31, y & 31, z & 31)] == 0
        d[_at(x & 31, y & 31, z & 31)] = LAMP
    return blocks


def scan_world(S) -> ClientWorld:
    """S^3 chunks, min chunk (0, 0, 0), all but seven of the roots 0: see scan_blocks."""
    world = ClientWorld((S // 2,) * 3, 1 << 20, S)
    for pos, dense in scan_blocks(S).items():
        world.create_chunk(pos, svo_build_by_set_node(dense))
    return world


def scan_scene(world, S, size=(16, 8), bounces=2):
    """The camera in the lower middle chunk, above the floor, looking down at it between the lamps."""
    m = 32.0 * (S // 2)
    sc = scenes._scene(f"lamps in {S}^3 chunks", world, size, (m + 14.5, m + 12.5, m + 3.5), (35.0, 20.0, 0.0), MODE_PATH)
    sc.settings.max_ray_bounces = bounces
    scenes._diffuse(sc.materials)
    return sc


def random_blocks(seed, S=3):
    """{chunk position: dense block}: all of the S^3 chunks but three that the seed chooses.  Each has a stone floor, scattered
    single voxels of LAMP, ORE, WATER, STONE and BIG, aligned 2^3 and 4^3 blocks of LAMP and of BIG (leaves above the bricks),
    4^3 cells filled as a LAMP / air checkerboard (32 lamps, every face listed: the most a cell can hold) and 4^3 cells of
    solid LAMP with one air voxel inside (a split cell whose lamps mostly look at lamps)."""
    rng = np.random.default_rng(seed)
    missing = set(int(i) for i in rng.choice(S ** 3, 3, replace=False))
    x, y, z = np.meshgrid(np.arange(32), np.arange(32), np.arange(32), indexing="ij")
    blocks = {}
    for i in range(S ** 3):
        if i in missing:
            continue
        d = np.zeros(32768, np.uint16)
        d[_at(x, y, z)[y < 2]] = STONE
        for voxel, n in ((LAMP, 40), (ORE, 12), (WATER, 40), (STONE, 40), (BIG, 20)):
            d[rng.integers(0, 32768, n)] = voxel
        for voxel, size, n in ((LAMP, 2, 4), (BIG, 2, 3), (LAMP, 4, 2), (BIG, 4, 1)):
            for _ in range(n):
                p = rng.integers(0, 32 // size, 3) * size
                d[_at(x, y, z)[(x >= p[0]) & (x < p[0] + size) & (y >= p[1]) & (y < p[1] + size) & (z >= p[2]) & (z < p[2] + size)]] = voxel
        for kind in ("checkerboard", "checkerboard", "hollow", "hollow"):
            p = rng.integers(0, 8, 3) * 4
            cell = (x >= p[0]) & (x < p[0] + 4) & (y >= p[1]) & (y < p[1] + 4) & (z >= p[2]) & (z < p[2] + 4)
            if kind == "checkerboard":
                d[_at(x, y, z)[cell]] = np.where((x + y + z)[cell] & 1, LAMP, 0)
            else:
                d[_at(x, y, z)[cell]] = LAMP
                q = p + rng.integers(1, 3, 3)
                d[_at(*q)] = 0
        blocks[(i % S, (i // S) % S, i // (S * S))] = d
    return blocks


def random_world(seed, S=3) -> ClientWorld:
    world = ClientWorld((S // 2,) * 3, 1 << 21, S)   # min chunk (0, 0, 0)
    for pos, dense in random_blocks(seed, S).items():
        world.create_chunk(pos, svo_build_by_set_node(dense))
    return world


def random_scene(world, S=3, size=(16, 8), bounces=2):
    c = 16.0 * S
    sc = scenes._scene(f"random lamps in {S}^3 chunks", world, size, (c + 0.5, c + 0.5, c + 0.5), (25.0, 30.0, 0.0), MODE_PATH)
    sc.settings.max_ray_bounces = bounces
    scenes._diffuse(sc.materials)
    return sc


def emission_big(**entries):
    """emission() with entry 255, which BIG reads, non-zero too."""
    t = emission(**entries)
    t[255] = 1.25
    return t


# ---- the hand-made world's lamps by kind, and cameras from which a lamp ray arrives at each (test_lamp_ref.py asserts it) ----

def hand_made_kinds():
    """{kind: a test over list entries' pos [n, 3] -> bool [n]}"""
    def at(*ps):
        return lambda p: np.any([np.all(p == np.array(q), axis=1) for q in ps], axis=0)

    def box(lo, hi):
        return lambda p: np.all((p >= np.array(lo)) & (p < np.array(hi)), axis=1)

    return {"the lone split-cell lamp": at((5, 6, 5)), "the size-2 leaf": box((10, 6, 10), (12, 8, 12)), "the 8^3 block": box((16, 8, 16), (24, 16, 24)),
            "under water": at((12, 20, 12)), "under the missing chunk": at((5, 31, 20)), "the border pair": at((31, 10, 5), (32, 10, 5)),
            "the corner": at((0, 10, 0))}


# (eye, rot): above the floor between the lamps looking down, and from beside the corner lamp across the chunk
EDGE_CAMERAS = (((8.5, 14.5, 8.5), (60.0, 45.0, 0.0)), ((3.5, 8.5, 3.5), (30.0, 230.0, 0.0)))
EDGE_SIZES = ((8, 8), (16, 8), (100, 60))
EDGE_SPPS = (1, 3)


def workgroups(lamps, S):
    """From a list alone: (b, base, count) — the list build's workgroups that have faces (256 consecutive depth-3 cells each, x
    fastest over the world's (8 S)^3), the entries in front of each and its own."""
    G = 8 * S
    p = lamps["pos"].astype(np.int64)
    cell = ((p[:, 2] >> 2) * G + (p[:, 1] >> 2)) * G + (p[:, 0] >> 2)
    assert (np.diff(cell) >= 0).all()
    b, first, count = np.unique(cell // 256, return_index=True, return_counts=True)
    return b, first, count
