"""ClientWorld::get_voxel (client/src/world.rs:352-357) and highest_vox_at (world.rs:359-366) with include/vrt.h's flags,
restated in numpy over a dense copy of a world, and the worlds and queries the column tests use.

Independent of the C++ mirror and the kernels: the reference below reads a column of the dense array whole and looks for
the highest entry that counts; it calls neither library's scan.  The worlds are built by hand (create_chunk, set_voxel) so
that every case the tests name is present, and `check_presence` asserts through the reference that it is.
"""
from __future__ import annotations

import numpy as np

from voxelraytracing_amd import ClientWorld, _ffi
from voxelraytracing_amd.world import column_queries

from cast_ray_cases import DenseWorld

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
STONE, SAND, WATER, HIGH, LAST, HUGE = 1, 2, 9, 300, 255, 1000   # HIGH, LAST and HUGE all use entry 255 of the table
FROM_Y, SOLID = _ffi.COLUMN_FROM_Y, _ffi.COLUMN_SOLID


def materials(liquid_255: bool = False, air_solid: bool = False, liquid_sand: bool = False):
    """A material table written out in full: every entry solid (all zeros) but air (is_empty), WATER (is_liquid) and what the
    arguments say — entry 255 a liquid, entry 0 not flagged empty, SAND a liquid.  HIGH & 255 = 44 and HUGE & 255 = 232
    stay solid: a look-up that masked instead of clamping would show."""
    m = (_ffi.Material * 256)()
    m[0].is_empty = 0 if air_solid else 1
    m[WATER].is_liquid = 1
    m[255].is_liquid = 1 if liquid_255 else 0
    m[SAND].is_liquid = 1 if liquid_sand else 0
    return m


def solid_table(mats) -> np.ndarray:
    """[256] bool: include/vrt.h's SOLID of every entry of a (Material * 256) table; None: nothing is solid."""
    if mats is None:
        return np.zeros(256, bool)
    return np.array([mats[i].is_empty == 0 and mats[i].is_liquid == 0 for i in range(256)], bool)


# ---- the reference ----

class Dense(DenseWorld):
    """DenseWorld plus which chunks exist (chunk_roots entry not 0)."""

    def __init__(self, world: ClientWorld):
        super().__init__(world)
        S = self.S
        self.has_chunk = (world.chunk_roots() != 0).reshape(S, S, S)   # [cz][cy][cx]


def ref_get_voxels(dw: Dense, pos) -> np.ndarray:
    """get_voxel of every (n,3) position -> VOXEL_AT_DTYPE: check_bounds against [min, min + 32 S), then the chunk, then the voxel."""
    pos = np.asarray(pos, np.int64).reshape(-1, 3)
    out = np.zeros(pos.shape[0], _ffi.VOXEL_AT_DTYPE)
    loc = pos - dw.min
    inside = np.all((loc >= 0) & (loc < dw.W), axis=1)
    out["status"] = _ffi.VOXEL_OUT_OF_BOUNDS
    li = loc[inside]
    chunk = dw.has_chunk[li[:, 2] >> 5, li[:, 1] >> 5, li[:, 0] >> 5]
    out["status"][inside] = np.where(chunk, _ffi.VOXEL_OK, _ffi.VOXEL_NO_CHUNK)
    out["voxel"][inside] = np.where(chunk, dw.v[li[:, 2], li[:, 1], li[:, 0]], 0)
    return out


def ref_column_tops(dw: Dense, q: np.ndarray, mats=None) -> np.ndarray:
    """The column top of every query of q (COLUMN_QUERY_DTYPE) -> COLUMN_TOP_DTYPE, from include/vrt.h's semantics."""
    solid = solid_table(mats)
    out = np.zeros(q.size, _ffi.COLUMN_TOP_DTYPE)
    W, min_y = dw.W, int(dw.min[1])
    lx, lz = q["x"].astype(np.int64) - dw.min[0], q["z"].astype(np.int64) - dw.min[2]
    inside = (lx >= 0) & (lx < W) & (lz >= 0) & (lz < W)
    out["status"][~inside] = _ffi.COLUMN_OUTSIDE
    idx = np.nonzero(inside)[0]
    col = dw.v[lz[idx], :, lx[idx]].astype(np.int64)                     # [k][y]
    flags = q["flags"][idx]
    counts = col != 0                                                     # voxel 0 never counts
    counts &= np.where(((flags & SOLID) != 0)[:, None], solid[np.minimum(col, 255)], True)
    start = np.where((flags & FROM_Y) != 0, np.minimum(q["from_y"][idx].astype(np.int64) - min_y, W - 1), W - 1)   # < 0: below the world
    counts &= np.arange(W)[None, :] <= start[:, None]
    found = counts.any(axis=1)
    top = W - 1 - np.argmax(counts[:, ::-1], axis=1)
    out["y"][idx] = np.where(found, min_y + top, min_y - 1)
    out["voxel"][idx] = np.where(found, col[np.arange(idx.size), top], 0)
    out["status"][idx] = np.where(found, _ffi.COLUMN_FOUND, _ffi.COLUMN_NONE)
    return out


def map_queries(dw: Dense, solid: bool) -> np.ndarray:
    """The (32 S)^2 queries of the map, [z][x] flattened."""
    x, z = np.arange(dw.W) + dw.min[0], np.arange(dw.W) + dw.min[2]
    zz, xx = np.meshgrid(z, x, indexing="ij")
    return column_queries(xx.ravel(), zz.ravel(), solid=solid)


def ref_top_map(dw: Dense, solid: bool, mats=None) -> np.ndarray:
    """The whole world from above -> TOP_ENTRY_DTYPE [z - min.z][x - min.x]."""
    r = ref_column_tops(dw, map_queries(dw, solid), mats)
    out = np.zeros((dw.W, dw.W), _ffi.TOP_ENTRY_DTYPE)
    out["y"], out["voxel"] = r["y"].reshape(dw.W, dw.W), r["voxel"].reshape(dw.W, dw.W)
    return out


def leaf_size(world: ClientWorld, p) -> int:
    """The side of the leaf find_node reaches at world position p (inside the world box); 32 for a missing chunk."""
    lo, S = world.min_voxel(), world.size_in_chunks()
    x, y, z = (int(p[a]) - int(lo[a]) for a in range(3))
    root = int(world.chunk_roots()[(x >> 5) + S * ((y >> 5) + S * (z >> 5))])
    if root == 0:
        return 32
    nodes, node, depth = world.nodes(), int(world.nodes()[root]), 0
    while node & 0x8000 and depth < 5:
        sh = 4 - depth
        node = int(nodes[root + (node & 0x7FFF) + (((x >> sh) & 1) | (((y >> sh) & 1) << 1) | (((z >> sh) & 1) << 2))])
        depth += 1
    return 32 >> depth


# ---- the worlds ----

def _uniform(v: int) -> np.ndarray:
    return np.array([v], np.uint16)   # one leaf node: the whole chunk is voxel v (0: an air leaf of side 32)


def _chunk(w: ClientWorld, cpos, fill: int, voxels=()):
    """create_chunk a uniform chunk, then set_voxel every (local position, voxel) of `voxels`."""
    w.create_chunk(cpos, _uniform(fill))
    for (x, y, z), v in voxels:
        w.set_voxel((cpos[0] * 32 + x, cpos[1] * 32 + y, cpos[2] * 32 + z), v)


# world A: where each top of the leaf columns lies (local x, y, z in chunk (-1, -1, -1)) and the side of the air leaf on top of it
LEAF_TOPS = {32: (18, 31, 2), 16: (6, 15, 2), 8: (10, 7, 2), 4: (2, 3, 10), 2: (2, 1, 18), 1: (18, 0, 18)}


def leaf_world() -> ClientWorld:
    """2^3 chunks, min voxel (-32, -32, -32).  Chunk column (-1, -1): single voxels in an air chunk under an air chunk of one
    leaf — tops directly under air leaves of side 32, 16, 8, 4, 2 and 1, the last at min.y with leaves of every size above it.
    (0, -1): an air chunk under a chunk with a voxel at the world's highest y.  (-1, 0): a uniform stone chunk under a
    missing one.  (0, 0): both chunks missing."""
    w = ClientWorld((0, 0, 0), 1 << 16, 2)
    assert tuple(w.min_voxel()) == (-32, -32, -32)
    _chunk(w, (-1, -1, -1), 0, [(p, STONE) for p in LEAF_TOPS.values()])
    _chunk(w, (-1, 0, -1), 0)
    _chunk(w, (0, -1, -1), 0)
    _chunk(w, (0, 0, -1), 0, [((5, 31, 5), STONE), ((9, 0, 9), SAND)])
    _chunk(w, (-1, -1, 0), STONE)
    return w


MIXED_CENTRE = (4, 2, -2)   # the centre chunk of the world whose min differs in value and sign on every axis


def strata_world(centre=(0, 0, 0)) -> ClientWorld:
    """3^3 chunks around `centre`, min voxel 32 * (centre - 1) — (-32, -32, -32), or (96, 32, -96) around MIXED_CENTRE:
    missing chunks above, between and below populated ones, a whole column of them, water over sand and over nothing, a 32^3
    leaf of water, voxel ids of 255 and more.  The chunk positions below are relative to the centre."""
    w = ClientWorld(centre, 1 << 17, 3)
    assert tuple(w.min_voxel()) == tuple(32 * (c - 1) for c in centre) and w.size_in_voxels() == 96

    def place(w, cpos, fill, voxels=()):
        _chunk(w, tuple(a + b for a, b in zip(cpos, centre)), fill, voxels)

    # z = -1: stone / missing / voxels of high ids;  missing / a voxel / air;  nothing at all
    place(w, (-1, -1, -1), STONE)
    place(w, (-1, 1, -1), 0, [((4, 0, 4), HIGH), ((8, 5, 8), LAST), ((12, 9, 12), HUGE), ((12, 10, 12), WATER)])
    place(w, (0, 0, -1), 0, [((3, 3, 3), STONE)])
    place(w, (0, 1, -1), 0)
    # z = 0: sand / a chunk of water / water and sand voxels;  missing / missing / a chunk of water;  stone / water and sand in split cells / missing
    place(w, (-1, -1, 0), SAND)
    place(w, (-1, 0, 0), WATER)
    place(w, (-1, 1, 0), 0, [((1, 0, 1), WATER), ((20, 4, 20), SAND), ((20, 5, 20), WATER)])
    place(w, (0, 1, 0), WATER)
    place(w, (1, -1, 0), STONE)
    place(w, (1, 0, 0), 0, [((2, 0, 2), WATER), ((2, 1, 2), WATER), ((6, 0, 6), SAND), ((6, 1, 6), WATER), ((7, 2, 6), STONE)])
    # z = 1: an air chunk alone;  stone all the way up;  the corners of the world
    place(w, (-1, -1, 1), 0)
    for cy in (-1, 0, 1):
        place(w, (0, cy, 1), STONE)
    place(w, (1, -1, 1), 0, [((31, 0, 31), SAND)])
    place(w, (1, 0, 1), 0)
    place(w, (1, 1, 1), 0, [((31, 31, 31), STONE)])
    return w


# ---- the queries ----

def column_cases(dw: Dense, mats=None) -> np.ndarray:
    """Every column of the world box and of a ring of one voxel around it, with flags 0 and SOLID; FROM_Y on, one above and one
    below each column's own top (of either kind); and on every fifth column the fixed starts: above the world, its top, min.y,
    min.y - 1, 0, INT32_MIN, INT32_MAX.  Then x and z at INT32_MIN and INT32_MAX."""
    lo, W = dw.min, dw.W
    r = np.arange(-1, W + 1)
    zz, xx = np.meshgrid(r + lo[2], r + lo[0], indexing="ij")
    xs, zs = xx.ravel(), zz.ravel()
    parts = []
    for solid in (False, True):
        base = column_queries(xs, zs, solid=solid)
        parts.append(base)
        top = ref_column_tops(dw, base, mats)["y"].astype(np.int64)
        for d in (0, 1, -1):
            parts.append(column_queries(xs, zs, from_y=np.clip(top + d, I32_MIN, I32_MAX), solid=solid))
        for y in (int(lo[1]) + W + 7, int(lo[1]) + W, int(lo[1]) + W - 1, int(lo[1]), int(lo[1]) - 1, 0, I32_MIN, I32_MAX):
            parts.append(column_queries(xs[::5], zs[::5], from_y=y, solid=solid))
    ext = [(I32_MIN, 0), (I32_MAX, 0), (0, I32_MIN), (0, I32_MAX), (I32_MIN, I32_MIN), (I32_MAX, I32_MAX)]
    parts.append(column_queries([e[0] for e in ext], [e[1] for e in ext]))
    parts.append(column_queries([e[0] for e in ext], [e[1] for e in ext], from_y=I32_MIN, solid=True))
    q = np.concatenate(parts)
    # bits without a meaning are ignored: set some on every third query
    q["flags"][::3] |= 0xFFFFFFF0
    return q


def voxel_cases(dw: Dense, seed: int = 5) -> np.ndarray:
    """(n,3) positions: the two voxels across every face of the world box along lines through it, every voxel of a few
    columns, random positions in and around the box, and coordinates at INT32_MIN and INT32_MAX."""
    lo, W = dw.min, dw.W
    rng = np.random.default_rng(seed)
    parts = [rng.integers(-40, W + 40, (6000, 3)) + lo]
    inside = rng.integers(0, W, (600, 3)) + lo
    for a in range(3):
        for edge in (-1, 0, W - 1, W, W + 30, W + 31):   # (the reference's own check_bounds ends 31 voxels further out)
            p = inside.copy()
            p[:, a] = lo[a] + edge
            parts.append(p)
    for x, z in ((18, 2), (6, 7), (37, 37), (1, 33)):   # (relative to min: columns with voxels, water and missing chunks)
        parts.append(np.stack([np.full(W + 4, lo[0] + x), np.arange(-2, W + 2) + lo[1], np.full(W + 4, lo[2] + z)], axis=1))
    ext = np.array([[I32_MIN, 0, 0], [0, I32_MIN, 0], [0, 0, I32_MIN], [I32_MAX, 0, 0], [0, I32_MAX, 0], [0, 0, I32_MAX],
                    [I32_MIN, I32_MIN, I32_MIN], [I32_MAX, I32_MAX, I32_MAX], [I32_MIN, I32_MAX, 0]], np.int64)
    parts.append(ext)
    return np.concatenate(parts).astype(np.int32)


class Case:
    """A world, its dense copy, a material table, the queries and the reference's answers — computed once, left unchanged."""

    def __init__(self, name: str, world: ClientWorld, mats, mixed: bool = False):
        self.name, self.world, self.mats, self.mixed = name, world, mats, mixed
        self.dw = Dense(world)
        self.q = column_cases(self.dw, mats)
        self.want = ref_column_tops(self.dw, self.q, mats)
        self.pos = voxel_cases(self.dw)
        self.want_voxels = ref_get_voxels(self.dw, self.pos)
        self.want_maps = {s: ref_top_map(self.dw, s, mats) for s in (False, True)}
        for a in (self.q, self.want, self.pos, self.want_voxels, *self.want_maps.values()):
            a.setflags(write=False)


def column(case: Case, x: int, z: int, from_y=None, solid=False):
    """The reference's record of one column as (y, voxel, status)."""
    r = ref_column_tops(case.dw, column_queries([x], [z], from_y=from_y, solid=solid), case.mats)[0]
    return int(r["y"]), int(r["voxel"]), int(r["status"])


def check_presence(case: Case):
    """Every case the tests name is in the world and in the queries — asserted through the reference, so that a case that
    silently vanished (a builder that changed, a chunk that was not created) fails here and not nowhere."""
    w, q, want = case.world, case.q, case.want
    lo, W = [int(v) for v in case.dw.min], case.dw.W
    top_y = lo[1] + W - 1
    st = want["status"]
    assert {0, 1, 2} <= set(np.unique(st).tolist())
    plain = (q["flags"] & 3) == 0
    assert (st[plain] == _ffi.COLUMN_NONE).sum() > 0 and (st[plain] == _ffi.COLUMN_FOUND).sum() > 0
    assert ((st == _ffi.COLUMN_FOUND) & (want["y"] == top_y)).sum() > 0      # a top at the world's highest y
    assert ((st == _ffi.COLUMN_FOUND) & (want["y"] == lo[1])).sum() > 0      # ... and at min.y
    fy = (q["flags"] & FROM_Y) != 0
    for y in (I32_MIN, I32_MAX, lo[1], lo[1] - 1, top_y + 1):
        assert (fy & (q["from_y"] == y)).sum() > 0
    assert (fy & (q["from_y"] == want["y"]) & (st == 1)).sum() > 0           # from_y on a counting voxel answers that voxel
    assert (fy & (q["from_y"] < lo[1]) & (st == 0)).sum() > 0
    assert (st[(q["x"] == I32_MIN) | (q["x"] == I32_MAX) | (q["z"] == I32_MIN) | (q["z"] == I32_MAX)] == 2).all()
    for a, f, b, g in ((lo[0], "x", lo[2], "z"), (lo[2], "z", lo[0], "x")):    # each face: one inside, one outside
        for outside in (q[f] == a - 1, q[f] == a + W):
            assert outside.sum() > 0 and (st[outside] == 2).all()
        for inside in ((q[f] == a) & (q[g] == b + 1), (q[f] == a + W - 1) & (q[g] == b + 1)):
            assert inside.sum() > 0 and (st[inside] != 2).all()
    if case.mixed:                                                            # min differs in value and in sign between the axes
        assert len(set(lo)) == 3 and min(lo) < 0 < max(lo) and lo[0] != lo[2]
    vs = case.want_voxels["status"]
    assert {0, 1, 3} <= set(np.unique(vs).tolist()) and (case.want_voxels["voxel"][vs != 0] == 0).all()
    if case.name == "leaf":
        for side, (x, y, z) in LEAF_TOPS.items():
            p = (x - 32, y - 32, z - 32)
            assert column(case, p[0], p[2]) == (p[1], STONE, 1)
            assert leaf_size(w, p) == 1 and leaf_size(w, (p[0], p[1] + 1, p[2])) == side, side
        x, y, z = LEAF_TOPS[1]
        sides, yy = [], y - 32 + 1
        while yy <= top_y:                                                    # the air over the top at min.y: every size
            sides.append(leaf_size(w, (x - 32, yy, z - 32)))
            yy += sides[-1]
        assert sides == [1, 2, 4, 8, 16, 32]
        assert column(case, 5, -27) == (top_y, STONE, 1) and column(case, 9, -23) == (0, SAND, 1)
        assert column(case, 20, -20) == (lo[1] - 1, 0, 0)                     # all air, in chunks that exist
        assert column(case, -10, 10) == (-1, STONE, 1)                        # a uniform chunk under a missing one
        assert column(case, 10, 10) == (lo[1] - 1, 0, 0)                      # a whole column of missing chunks
        assert not case.dw.has_chunk[1, :, 1].any() and not case.dw.has_chunk[1, 1, 0]
    if case.name == "strata":
        hc = case.dw.has_chunk   # [cz][cy][cx]
        o = [v + 32 for v in lo]   # the positions and heights below are those of the world with min (-32, -32, -32)

        def col(x, z, from_y=None, solid=False):
            y, v, status = column(case, x + o[0], z + o[2], None if from_y is None else from_y + o[1], solid)
            return y - o[1], v, status

        assert hc[0, :, 0].tolist() == [True, False, True]                    # a missing chunk between two populated ones
        assert hc[0, :, 1].tolist() == [False, True, True]                    # ... below one
        assert hc[1, :, 2].tolist() == [True, True, False]                    # ... above one
        assert not hc[0, :, 2].any()                                          # a whole column of them
        assert col(-10, -10) == (-1, STONE, 1)                       # through the missing chunk to the stone
        assert col(-28, -28) == (32, HIGH, 1) and col(-24, -24) == (37, LAST, 1)
        assert col(-20, -20) == (42, WATER, 1)
        assert col(3, -29) == (3, STONE, 1) and col(40, -20) == (-33, 0, 0)
        # SOLID: entry 255 of the table decides for every id from 255 up
        if case.mats[255].is_liquid:
            assert [col(x, x, solid=True) for x in (-28, -24, -20)] == [(-1, STONE, 1)] * 3
        else:
            assert [col(x, x, solid=True) for x in (-28, -24, -20)] == [(32, HIGH, 1), (37, LAST, 1), (41, HUGE, 1)]
        # water over sand: the 32^3 leaf of water is one leaf, and SOLID answers the sand under it
        assert leaf_size(w, (-20 + o[0], 10 + o[1], 12 + o[2])) == 32
        assert col(-20, 12) == (31, WATER, 1) and col(-20, 12, solid=True) == (-1, SAND, 1)
        assert col(-12, 20) == (37, WATER, 1) and col(-12, 20, solid=True) == (36, SAND, 1)
        assert col(38, 6) == (1, WATER, 1) and col(38, 6, solid=True) == (0, SAND, 1)
        assert col(34, 2) == (1, WATER, 1) and col(34, 2, solid=True) == (-1, STONE, 1)
        assert col(10, 10) == (63, WATER, 1) and col(10, 10, solid=True) == (-33, 0, 0)   # water over nothing
        assert col(20, 40) == (63, STONE, 1) and col(63, 63) == (63, STONE, 1)
        assert col(63, 63, from_y=63 - 1) == (-32, SAND, 1)
        assert col(-20, 40) == (-33, 0, 0)                     # an air chunk alone


_cases = {}


def case(name: str) -> Case:
    """The shared cases: "leaf" (world A, the plain table), "strata" (world B, the plain table), "strata255" (world B with
    entry 255 and entry 0 of the table turned round: ids from 255 up are liquid, air is not flagged empty), "mixed" (world B
    around MIXED_CENTRE, min voxel (96, 32, -96): every axis has a min of its own, of either sign)."""
    if name not in _cases:
        world, mats = {"leaf": (leaf_world, materials()), "strata": (strata_world, materials()),
                       "strata255": (strata_world, materials(liquid_255=True, air_solid=True)),
                       "mixed": (lambda: strata_world(MIXED_CENTRE), materials())}[name]
        _cases[name] = Case("leaf" if name == "leaf" else "strata", world(), mats, mixed=name == "mixed")
    return _cases[name]


def records_differ(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Indices where two arrays of one record type differ in any byte."""
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    n = a.dtype.itemsize
    return np.nonzero(np.any(a.view(np.uint8).reshape(-1, n) != b.view(np.uint8).reshape(-1, n), axis=1))[0]
