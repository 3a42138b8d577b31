"""One table of vrt_edit_chunks cases for the host mirror (tests/test_edit_cases.py) and the kernels (tests/test_gpu_edit_matrix.py).

Plain data and builders, no GPU.  A case is (name, pos, nodes, offsets, shapes) and a claim: a predicate on the restatement
alone (`restate`) that says what the case exercises.  The restatement shares nothing with csrc:
  - `read_tree` reads all 32768 voxels of a tree in numpy: from word 0, child x_bit | y_bit << 1 | z_bit << 2 per level, most
    significant bit first, until a word without bit 15;
  - the shapes are tests/shapes_ref.py's, with a sphere's or disc's loops cut to the chunk (`apply`), so that a radius of 32767.5
    can be restated on the few chunks a case holds;
  - `shape_box` / `bins` restate which (chunk, shape) pairs a call makes (include/vrt.h: the shapes whose box meets the chunk).
The expected tree of a chunk is world.svo_build_bottom_up of its restated block, the builder the interface is defined by.

`NAMES` lists the cases, `get(name)` builds one (cached), `restate(case)` answers for it, `size(case)` orders them.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from voxelraytracing_amd import world as W
from voxelraytracing_amd.world import shape_disc, shape_line, shape_point, shape_sphere

import shapes_ref as R
from test_edit_chunks_ref import CORNER_CHUNK, LEAVES, LINE_CASES, STONE, WATER, WOOD, _block, _feature, _pattern

Case = namedtuple("Case", "name pos nodes offsets shapes claim")
Restated = namedtuple("Restated", "before after nodes offsets changed")

MAX_TREE = 32761          # kEditMaxTree
BATCH = 2048              # kEditBatch
CHUNK_MAX = (1 << 17) - 1
COORD_MAX = (1 << 22) - 1
FILL = 30000              # a voxel that neither the pattern nor a tree with leaves down to depth 4 holds
POINT_INDICES = (0, 1, 2, 3, 31, 32, 1024, 32767, 12345)     # each 16-bit place of a uint2, lane 0 and 255, the last iteration

_I = np.arange(32768)
_X, _Y, _Z = _I & 31, (_I >> 5) & 31, _I >> 10


# ---- the restatement ----

def read_tree(nodes) -> np.ndarray:
    """The block dense[x + 32 * (y + 32 * z)] a tree holds, every voxel walking from word 0."""
    nodes = np.asarray(nodes, np.uint16).astype(np.int64)
    at = np.zeros(32768, np.int64)
    for bit in (4, 3, 2, 1, 0):
        w = nodes[at]
        split = (w & 0x8000) != 0
        child = ((_X >> bit) & 1) | (((_Y >> bit) & 1) << 1) | (((_Z >> bit) & 1) << 2)
        at = np.where(split, (w & 0x7FFF) + child, at)
    w = nodes[at]
    assert not (w & 0x8000).any(), "a split at depth 5"
    return w.astype(np.uint16)


def child_blocks(nodes) -> list:
    """[(depth of the parent, parent word's index, first)] of every split word a walk from word 0 reaches, each parent once."""
    nodes = np.asarray(nodes, np.uint16)
    out, seen, todo = [], set(), [(0, 0)]
    while todo:
        idx, d = todo.pop()
        if idx in seen:
            continue
        seen.add(idx)
        w = int(nodes[idx])
        if w & 0x8000:
            first = w & 0x7FFF
            out.append((d, idx, first))
            todo.extend((first + k, d + 1) for k in range(8))
    return out


def shape_box(shape):
    """(lo, hi), inclusive, of the reference's loops for a sphere or disc (`r as i32` truncates), the span of a line, a point."""
    kind, _, a, b, r, height = shape
    a = [int(v) for v in a]
    if kind == R.POINT:
        return a, a
    if kind == R.LINE:
        return [min(a[i], int(b[i])) for i in range(3)], [max(a[i], int(b[i])) for i in range(3)]
    ri = int(np.float32(r))
    lo, hi = [v - ri for v in a], [v + ri for v in a]
    if kind == R.DISC:
        lo[1], hi[1] = a[1], a[1] + int(height) - 1
    return lo, hi


def box_cells(shape) -> int:
    """The chunk cells a shape's box covers (0 for an empty box)."""
    lo, hi = shape_box(shape)
    if any(hi[i] < lo[i] for i in range(3)):
        return 0
    return int(np.prod([(hi[i] // 32) - (lo[i] // 32) + 1 for i in range(3)]))


def bins(pos, shapes) -> list:
    """For every chunk the indices of the shapes whose box meets its 32^3 voxels, ascending."""
    lo, hi = _boxes(shapes)
    return [np.flatnonzero(_meets(lo, hi, p)).tolist() for p in pos]


def _boxes(shapes):
    """shape_box of every shape: two (m, 3) arrays."""
    boxes = [shape_box(s) for s in shapes]
    return (np.array([b[0] for b in boxes], np.int64).reshape(-1, 3), np.array([b[1] for b in boxes], np.int64).reshape(-1, 3))


def _meets(lo, hi, chunk_pos):
    """Which boxes are not empty and hold a voxel of the chunk."""
    o = 32 * np.array(chunk_pos, np.int64)
    return ((lo <= o + 31) & (hi >= o) & (lo <= hi)).all(axis=1)


def _placed(shape, o, lines):
    """Local indices x + 32 * (y + 32 * z) of the voxels `shape` places in the chunk whose first voxel is o."""
    kind, _, a, b, r, height = shape
    if kind in (R.POINT, R.LINE):
        key = (kind, tuple(a), tuple(b))
        if key not in lines:
            lines[key] = np.array(R.voxels(shape), np.int64).reshape(-1, 3)
        l = lines[key] - np.array(o, np.int64)
        l = l[((l >= 0) & (l < 32)).all(axis=1)]
    else:      # fill_region_by_radius over the loops' own bounds, cut to the chunk
        lo, hi = shape_box(shape)
        lo = [max(lo[i], o[i]) for i in range(3)]
        hi = [min(hi[i], o[i] + 31) for i in range(3)]
        l = np.array(R._by_radius(tuple(int(v) for v in a), r, lo, hi), np.int64).reshape(-1, 3) - np.array(o, np.int64)
    return l[:, 0] + 32 * (l[:, 1] + 32 * l[:, 2])


def apply(dense, chunk_pos, shapes, lines=None):
    """shapes_ref.apply with every shape cut to the chunk first; returns `dense` itself when no placement lies in the chunk.
    `lines` keeps, from chunk to chunk of one call, the voxels of each line and the shapes' boxes (a shape whose box misses the
    chunk places nothing in it: the box is the loops' own bounds, or the span a line's walker stays in)."""
    lines = {} if lines is None else lines
    if lines.get("boxes of") is not shapes:
        lines["boxes of"], lines["boxes"] = shapes, _boxes(shapes)
    o = [32 * int(c) for c in chunk_pos]
    out = None
    for j in np.flatnonzero(_meets(*lines["boxes"], chunk_pos)):
        s = shapes[j]
        idx = _placed(s, o, lines)
        if idx.size:
            out = np.array(dense, np.uint16) if out is None else out
            out[idx] = s[1]
    return dense if out is None else out


_read, _built = {}, {}


def _read_cached(tree):
    key = tree.tobytes()
    if key not in _read:
        _read[key] = read_tree(tree)
        _read[key].setflags(write=False)
    return _read[key]


def canonical(block) -> np.ndarray:
    """The tree vrt_edit_chunks answers with for a block: the bottom-up builder's, or no words where it refuses."""
    try:
        return W.svo_build_bottom_up(block)
    except W.SetVoxelErr:
        return np.zeros(0, np.uint16)


def restate(case, shapes=None) -> Restated:
    """What vrt_edit_chunks has to answer (strict=False), by the restatement; `shapes` replaces the case's (an order's claim)."""
    shapes = case.shapes if shapes is None else shapes
    lines, before, after, trees, changed = {}, [], [], [], []
    for i, p in enumerate(case.pos):
        tree = case.nodes[int(case.offsets[i]):int(case.offsets[i + 1])]
        b = _read_cached(tree)
        a = apply(b, p, shapes, lines)
        if a is b:
            key = tree.tobytes()
            if key not in _built:
                _built[key] = canonical(b)
            trees.append(_built[key])
        else:
            trees.append(canonical(a))
        before.append(b)
        after.append(a)
        changed.append(int(a is not b and not np.array_equal(a, b)))
    offs = np.concatenate([[0], np.cumsum([t.size for t in trees])]).astype(np.uint64)
    return Restated(before, after, np.concatenate(trees) if trees else np.zeros(0, np.uint16), offs, np.array(changed, np.uint8))


def size(case) -> int:
    """What the call's device buffers have to hold, for ordering the cases: node words + shapes + bin entries."""
    return int(case.offsets[-1]) + len(case.shapes) + sum(len(b) for b in bins(case.pos, case.shapes))


# ---- hand-made trees ----

def cell_xyz(level, m):
    """The coordinates, in cells of its level, of the cell with Morton index m (child k = x | y << 1 | z << 2, root first)."""
    x = y = z = 0
    for l in range(level):
        k = (m >> (3 * (level - 1 - l))) & 7
        x, y, z = (x << 1) | (k & 1), (y << 1) | ((k >> 1) & 1), (z << 1) | (k >> 2)
    return x, y, z


def make_tree(cell, order="pre", gap=()) -> np.ndarray:
    """A tree from cell(level, morton) -> a voxel, or None for a split.  order "pre": a child block follows its parent's block
    (ascending addresses); "post": it comes before it (descending).  `gap`: unreachable words after every block."""
    words = [0]

    def emit(level, m):
        v = cell(level, m)
        if v is not None:
            assert 0 <= v < 0x8000 and level <= 5
            return v
        assert level < 5
        if order == "pre":
            at = len(words)
            words.extend([0] * 8)
            words.extend(gap)
            for k in range(8):
                words[at + k] = emit(level + 1, 8 * m + k)
        else:
            kids = [emit(level + 1, 8 * m + k) for k in range(8)]
            at = len(words)
            words.extend(kids)
            words.extend(gap)
        assert at + 8 <= 0x8000
        return 0x8000 | at
    words[0] = emit(0, 0)
    assert len(words) <= MAX_TREE, len(words)
    return np.array(words, np.uint16)


def _voxel5(m):
    x, y, z = cell_xyz(5, m)
    return (1 + x + 32 * y + 1024 * z) & 0x7FFF      # injective in every axis bit; 32768 folds to 0, which nothing else is


def _leaves_at(d):
    return lambda level, m: None if level < d else 1 + m


def _depth5(parity):
    """Level-4 cells of Morton parity `parity` split into voxels, the others leaves: 2048 mixed cells."""
    return lambda level, m: None if level < 4 or (level == 4 and (m & 1) == parity) else (1 + m if level == 4 else _voxel5(m))


def _most_cells(level, m):
    """Voxels in level-4 cells 0..3508 and 4095, leaves in the others."""
    if level < 4 or (level == 4 and (m < 3509 or m == 4095)):
        return None
    return 1 + m if level == 4 else _voxel5(m)


def _dag():
    """The root's children 0 and 7 are one block (9..16), whose child 3 splits once more (17..24)."""
    w = np.zeros(25, np.uint16)
    w[0] = 0x8001
    w[1:9] = [0x8009, 11, 12, 13, 14, 15, 16, 0x8009]
    w[9:17] = [21, 22, 23, 0x8000 | 17, 25, 26, 27, 28]
    w[17:25] = [31, 32, 33, 34, 35, 36, 37, 38]
    return w


def thinned_pattern(pos) -> np.ndarray:
    """test_edit_chunks_ref._pattern with its diagonal 7s kept in every other level-4 cell only: the whole pattern has 4096
    mixed level-4 cells, which the builder refuses (tests/test_edit_cases.py asserts both counts)."""
    keep = (((_X >> 1) + (_Y >> 1) + (_Z >> 1)) & 1) == 0
    full = _pattern(pos)
    return np.where(keep, full, (_Y < 9) * 4).astype(np.uint16)


def mixed_cells(block) -> int:
    b = np.asarray(block).reshape(16, 2, 16, 2, 16, 2)
    return int((b.max(axis=(1, 3, 5)) != b.min(axis=(1, 3, 5))).sum())


@functools.lru_cache(maxsize=None)
def _pattern_tree_mod5(k):
    return W.svo_build_bottom_up(thinned_pattern((k, 0, 0)))


def pattern_tree(pos) -> np.ndarray:
    return _pattern_tree_mod5(sum(int(v) for v in pos) % 5)      # (_pattern reads the position through sum(pos) % 5 alone)


@functools.lru_cache(maxsize=None)
def trees() -> dict:
    """name -> (nodes, canonical): the hand-made trees, and whether the bottom-up builder would have made these very words."""
    t = {
        "uniform": (np.array([STONE], np.uint16), True),
        "leaves at depth 1": (make_tree(_leaves_at(1)), True),
        "leaves at depth 2": (make_tree(_leaves_at(2)), None),
        "leaves at depth 3": (make_tree(_leaves_at(3)), None),
        "leaves at depth 4": (make_tree(_leaves_at(4)), None),
        "voxels in the even level-4 cells": (make_tree(_depth5(0)), None),
        "voxels in the odd level-4 cells": (make_tree(_depth5(1)), None),
        "the thinned pattern, built bottom-up": (pattern_tree((0, 0, 0)), True),
        "eight equal leaves unmerged at depth 1": (make_tree(lambda level, m: None if level < 1 else STONE), False),
        "eight equal leaves unmerged at depth 4": (make_tree(lambda level, m: None if level < 4 else (WOOD if m < 8 else 1 + m)), False),
        "a child block shared by two parents": (_dag(), False),
        "child blocks in descending order": (make_tree(lambda level, m: None if level < 3 or (level == 3 and m % 5 == 0) else 1 + m, "post"), False),
        "garbage between the blocks": (make_tree(_leaves_at(3), gap=(0xFFFF, 0x8000 | 123, 0x7FFF, 0xFFFF)), False),
        "the last block ends at len": (make_tree(lambda level, m: None if level < 2 or (level == 2 and m == 63) else 1 + m), None),
        # 3510 mixed level-4 cells, the most a tree can hold; the last cell among them, so that POINT_INDICES all lie in split cells
        # (a voxel changed in a leaf cell would make a 3511th, which the builder refuses)
        "32761 words": (make_tree(_most_cells), None),
    }
    return t


def _concat(parts):
    offs = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    return np.concatenate(parts).astype(np.uint16), offs


# ---- the table ----

_BUILDERS = {}


def _case(name):
    def reg(fn):
        assert name not in _BUILDERS, name
        _BUILDERS[name] = fn
        return fn
    return reg


def _unchanged(tree_name):
    def claim(case, r):
        nodes, is_canonical = trees()[tree_name]
        assert not r.changed.any() and r.after[0] is r.before[0]
        if is_canonical is not None:      # (the canonical tree of the block is these very words, or is not)
            assert np.array_equal(r.nodes, nodes) == is_canonical
        _TREE_CLAIMS[tree_name](nodes, r.before[0])
    return claim


def _depth_claim(d, cells=None):
    def claim(nodes, block):
        blocks = child_blocks(nodes)
        assert max([p[0] for p in blocks], default=-1) == d - 1, "the deepest split"
        if cells is not None:
            assert np.unique(block).size == cells, "every cell a value of its own"
    return claim


def _claim_depth5(nodes, block):
    assert sum(1 for p in child_blocks(nodes) if p[0] == 4) == 2048 and mixed_cells(block) == 2048
    b = block.reshape(16, 2, 16, 2, 16, 2)
    split = b.max(axis=(1, 3, 5)) != b.min(axis=(1, 3, 5))
    vox = block[np.repeat(np.repeat(np.repeat(split, 2, axis=0), 2, axis=1), 2, axis=2).reshape(-1)]
    assert np.unique(vox).size == vox.size == 2048 * 8, "every voxel of a split cell a value of its own"


def _claim_unmerged(d):
    def claim(nodes, block):
        eq = [p for p in child_blocks(nodes) if p[0] == d - 1 and len(set(nodes[p[2]:p[2] + 8].tolist())) == 1 and not nodes[p[2]] & 0x8000]
        assert eq, "a block of eight equal leaves"
    return claim


def _claim_dag(nodes, block):
    firsts = [p[2] for p in child_blocks(nodes)]
    assert len(firsts) != len(set(firsts)), "two parents of one block"
    assert block[0] == 21 and block[32767] == 28 and block[8 + 32 * 8] == 31      # octant 0, octant 7, and the split below child 3


def _claim_descending(nodes, block):
    blocks = child_blocks(nodes)
    assert len(blocks) > 100 and all(first < idx for _, idx, first in blocks if idx), "every child block before its parent's"
    assert max(p[0] for p in blocks) == 3


def _claim_garbage(nodes, block):
    reach = np.zeros(nodes.size, bool)
    reach[0] = True
    for _, _, first in child_blocks(nodes):
        reach[first:first + 8] = True
    junk = nodes[~reach]
    assert junk.size >= 4 * 73 and (junk == 0xFFFF).any() and not reach[-1], "unreachable words, 0xFFFF among them, and after the last block"


def _claim_ends_at_len(nodes, block):
    assert max(first for _, _, first in child_blocks(nodes)) + 8 == nodes.size


def _claim_max(nodes, block):
    assert nodes.size == MAX_TREE and max(first for _, _, first in child_blocks(nodes)) + 8 == MAX_TREE
    assert mixed_cells(block) == 3510


def _claim_pattern(nodes, block):
    assert set(np.unique(block)) == {0, 4, 7, 11} and 2000 < mixed_cells(block) < 3510
    assert nodes.size == 4681 + 8 * mixed_cells(block)      # (every level above is mixed too: the diagonals cross every cell)


_TREE_CLAIMS = {
    "uniform": lambda nodes, block: (_depth_claim(0)(nodes, block), np.testing.assert_array_equal(block, STONE)),
    "leaves at depth 1": _depth_claim(1, 8),
    "leaves at depth 2": _depth_claim(2, 64),
    "leaves at depth 3": _depth_claim(3, 512),
    "leaves at depth 4": _depth_claim(4, 4096),
    "voxels in the even level-4 cells": _claim_depth5,
    "voxels in the odd level-4 cells": _claim_depth5,
    "the thinned pattern, built bottom-up": _claim_pattern,
    "eight equal leaves unmerged at depth 1": _claim_unmerged(1),
    "eight equal leaves unmerged at depth 4": _claim_unmerged(4),
    "a child block shared by two parents": _claim_dag,
    "child blocks in descending order": _claim_descending,
    "garbage between the blocks": _claim_garbage,
    "the last block ends at len": _claim_ends_at_len,
    "32761 words": _claim_max,
}

TREE_NAMES = list(_TREE_CLAIMS)
_NINE = [(3 + i, -2, 5 - 2 * i) for i in range(len(POINT_INDICES))]


def _points_claim(case, r):
    assert r.changed.tolist() == [1] * len(POINT_INDICES)
    for i, at in enumerate(POINT_INDICES):
        assert np.flatnonzero(r.after[i] != r.before[i]).tolist() == [at], at


def _tree_cases(tname):
    @_case(f"tree, {tname}: no shapes")
    def _():
        nodes = trees()[tname][0]
        return [(3, -2, 5)], nodes, [0, nodes.size], [], _unchanged(tname)

    @_case(f"tree, {tname}: one voxel changed in each of nine copies")
    def _():
        nodes = trees()[tname][0]
        block = read_tree(nodes)
        shapes = [shape_point((32 * p[0] + (at & 31), 32 * p[1] + ((at >> 5) & 31), 32 * p[2] + (at >> 10)), (int(block[at]) + 1) & 0x7FFF)
                  for p, at in zip(_NINE, POINT_INDICES)]
        allnodes, offs = _concat([nodes] * len(_NINE))
        return _NINE, allnodes, offs, shapes, _points_claim


for _t in TREE_NAMES:
    _tree_cases(_t)


@_case("nothing changes: a point writes the value already there")
def _():
    nodes = trees()["leaves at depth 3"][0]
    block = read_tree(nodes)
    at = 7 + 32 * (9 + 32 * 21)
    def claim(case, r):
        assert not r.changed.any() and r.after[0] is not r.before[0], "a placement that lands and changes nothing"
    return [(-4, 0, 2)], nodes, [0, nodes.size], [shape_point((-128 + 7, 9, 64 + 21), int(block[at]))], claim


@_case("nothing changes: a sphere of air in an air chunk")
def _():
    def claim(case, r):
        assert not r.changed.any() and r.after[0] is not r.before[0] and r.nodes.tolist() == [0]
    return [(0, 0, 0)], np.zeros(1, np.uint16), [0, 1], [shape_sphere((16, 16, 16), 9.9, 0)], claim


def _over_pattern(shapes, chunks, claim):
    """The case whose chunks hold the thinned pattern."""
    chunks = [tuple(int(v) for v in p) for p in chunks]
    nodes, offs = _concat([pattern_tree(p) for p in chunks])
    return chunks, nodes, offs, shapes, claim


def _carves_and_overwrites(case, r):
    """Some voxel that was air is written, and some voxel that was not."""
    was = np.concatenate(r.before)
    now = np.concatenate(r.after)
    moved = was != now
    assert (moved & (was == 0)).any() and (moved & (was != 0)).any()


def _line_case(name):
    @_case(f"line, {name}")
    def _():
        a, b = LINE_CASES[name]
        s = [shape_line(a, b, WOOD)]
        def claim(case, r):
            assert r.changed.all() and len(case.pos) == len(R.touched_chunks(s))
            assert sum(int((x != y).sum()) for x, y in zip(r.before, r.after)) == max(abs(b[i] - a[i]) for i in range(3)) + 1
        return _over_pattern(s, R.touched_chunks(s), claim)


for _n in sorted(LINE_CASES):
    _line_case(_n)


@_case("line of dist 4096, every chunk it touches in one call")
def _():
    s = [shape_line((-2048, 3, 5), (2048, 900, -700), WOOD)]
    def claim(case, r):
        assert len(case.pos) >= 129 and r.changed.all()
        assert sum(int((y == WOOD).sum()) for y in r.after) == 4097
    return _over_pattern(s, R.touched_chunks(s), claim)


def _sphere_case(r_):
    @_case(f"sphere, r = {r_}")
    def _():
        s = [shape_sphere((16, 16, 16), r_, LEAVES), shape_sphere((-1, 31, -33), r_, STONE)]
        chunks = sorted(set(R.touched_chunks(s)) | {(0, 0, 0), (-1, 0, -2)})
        def claim(case, r):
            n = [len(R.voxels(x)) for x in s]
            assert n[0] == n[1] == {0.0: 0, 0.4: 1, 1.0: 1}.get(r_, n[0]) and (n[0] > 50 or r_ <= 1.0)
            assert sum(int((y == LEAVES).sum()) for y in r.after) == n[0] and sum(int((y == STONE).sum()) for y in r.after) == n[1]
            assert (len(case.pos) == 2) == (r_ < 2) and (len(case.pos) >= 8 or r_ < 2)      # one chunk, or across faces
        return _over_pattern(s, chunks, claim)


for _r in (0.0, 0.4, 1.0, 3.0, 4.9, 5.0, 9.9):
    _sphere_case(_r)


@_case("sphere, r = 40: the whole chunk and six clipped neighbours")
def _():
    c = (2, -1, 3)
    s = [shape_sphere(tuple(32 * v + 16 for v in c), 40.0, FILL)]
    chunks = [c] + [tuple(c[i] + (d if i == ax else 0) for i in range(3)) for ax in range(3) for d in (-1, 1)]
    def claim(case, r):
        assert (r.after[0] == FILL).all() and r.offsets[1] == 1, "total == 32768, and every voxel inside"
        lo, hi = shape_box(s[0])
        for p, y in zip(case.pos[1:], r.after[1:]):
            o = [32 * v for v in p]
            n = [min(hi[i], o[i] + 31) - max(lo[i], o[i]) + 1 for i in range(3)]
            assert sorted(n)[1:] == [32, 32] and min(n) in (24, 25) and 0 < (y == FILL).sum() < min(n) * 1024, "a clipped box that is no cube"
        assert box_cells(s[0]) == 27 > len(case.pos), "more cells than chunks: every chunk is tested"
    return _over_pattern(s, chunks, claim)


@_case("sphere, r = 23.5 on a chunk corner")
def _():
    s = [shape_sphere((64, -32, 96), 23.5, FILL)]
    def claim(case, r):
        assert len(case.pos) == 8 and r.changed.all() and len({int((y == FILL).sum()) for y in r.after}) > 1
        _carves_and_overwrites(case, r)
    return _over_pattern(s, R.touched_chunks(s), claim)


def _big_sphere(r_, cut, inside, outside):
    @_case(f"sphere, r = {r_} at the origin")
    def _():
        s = [shape_sphere((0, 0, 0), r_, FILL)]
        def claim(case, r):
            filled = [int((y == FILL).sum()) for y in r.after]
            assert all(0 < f < 32768 for f in filled[:len(cut)]), f"chunks the surface cuts: {filled[:len(cut)]}"
            assert filled[len(cut):] == [32768, 0] and r.changed.tolist() == [1] * (len(cut) + 1) + [0]
            lo, hi = shape_box(s[0])
            assert all(lo[i] <= 32 * outside[i] <= hi[i] for i in range(3)), "the chunk outside the sphere is inside its box"
            assert box_cells(s[0]) > len(case.pos)
        return _over_pattern(s, list(cut) + [inside, outside], claim)


# The chunks the surface cuts were found by counting, with `apply` on an empty block, the voxels the sphere fills in the chunks
# along each axis ((r // 32, k, 0) for k = 0, 1, ...) and along the diagonals (r / sqrt(3) // 32 and r / sqrt(2) // 32 per axis) and
# keeping some with a count strictly between 0 and 32768; the claim asserts that of each, so a wrong entry fails on the host.
# (The chunk at -1024 is cut by the box alone: `r as i32` ends the loops at -32767, and the sphere would take the layer at -32768)
_big_sphere(32767.5, [(1023, 36, 0), (0, -1024, 0), (36, 0, 1023), (591, 591, 591), (-592, 591, -592), (723, 0, 724)], (100, -200, 300), (1023, 1023, 1023))
_big_sphere(20000.3, [(625, 3, 0), (0, -625, 20), (3, 0, 625), (360, 360, 360), (360, -361, 360), (441, 442, 0)], (-300, 10, 200), (625, 625, 625))


def _disc_case(height, w):
    r_ = float(np.float32(w) * np.float32(0.5) - np.float32(0.1))
    @_case(f"disc, height {height}, r = {w} * 0.5 - 0.1")
    def _():
        s = [shape_disc((30, 30, 1), r_, height, STONE), shape_disc((-40, -1, 70), r_, height, FILL)]     # the second astride y = 0
        ys = {0: ([0, 1], [-1, 0]), 1: ([0, 1], [-1, 0]), 3: ([0, 1], [-1, 0]), 40: ([0, 1, 2, 3], [-1, 0, 1, 2]),
              32768: ([0, 1, 511, 1024, 1025], [-1, 0, 1023, 1024])}[height]
        chunks = [(x, y, z) for y in ys[0] for x, z in ((0, 0), (1, 0), (0, -1), (1, -1))] + [(-2, y, 2) for y in ys[1]]
        def claim(case, r):
            """The distance is three-dimensional: layer k above the centre's holds voxels only while k < r, so a tall disc's box
            covers chunks it places nothing in (the kernel's "the bin was generous")."""
            got = {p: (int((y == STONE).sum()), int((y == FILL).sum())) for p, y in zip(case.pos, r.after)}
            b = dict(zip(case.pos, bins(case.pos, s)))
            if height == 0:
                assert not r.changed.any() and box_cells(s[0]) == 0 and not any(b.values())
                return
            n = [len(R.voxels(x)) for x in s]      # (at most 5 x 32768 x 5 cells of the loops)
            assert n[0] == n[1] > 0 and sum(g[0] for g in got.values()) == n[0] and sum(g[1] for g in got.values()) == n[1]
            assert got[(0, 0, 0)][0] > 0 and got[(-2, -1, 2)][1] > 0
            if height >= 3 and w >= 3:
                assert got[(-2, 0, 2)][1] > 0, "both sides of the face y = 0"
            if height >= 3 and w >= 5:
                assert got[(0, 1, 0)][0] > 0, "both sides of the face y = 32"
            if w >= 5:
                assert got[(1, 0, 0)][0] > 0 and got[(0, 0, -1)][0] > 0, "across the faces in x and z"
            if height == 40:
                assert b[(0, 2, 0)] == [0] and b[(0, 3, 0)] == [] and b[(-2, 1, 2)] == [1] and b[(-2, 2, 2)] == [], "taller than a chunk"
                assert got[(0, 2, 0)] == got[(-2, 1, 2)] == (0, 0)
            if height == 32768:
                assert b[(0, 511, 0)] == [0] and b[(0, 1024, 0)] == [0] and b[(0, 1025, 0)] == [] and b[(-2, 1023, 2)] == [1] and b[(-2, 1024, 2)] == []
                assert got[(0, 1024, 0)] == got[(-2, 1023, 2)] == (0, 0)
        return _over_pattern(s, chunks, claim)


for _h in (0, 1, 3, 40, 32768):
    for _w in range(1, 7):
        _disc_case(_h, _w)

_C = (64, -32, 96)      # the common corner of eight chunks
_ORDERS = {
    "point, sphere, point": [shape_point(_C, STONE), shape_sphere(_C, 3.0, LEAVES), shape_point((_C[0] + 1, _C[1], _C[2]), WOOD)],
    "sphere, line through it": [shape_sphere(_C, 4.9, LEAVES), shape_line((_C[0] - 9, _C[1] - 6, _C[2] - 3), (_C[0] + 9, _C[1] + 6, _C[2] + 3), WOOD)],
    "disc of water, disc of air": [shape_disc((_C[0], _C[1] - 1, _C[2]), 3.9, 2, WATER), shape_disc((_C[0], _C[1] - 1, _C[2]), 3.9, 2, 0)],
}


def _order_case(name, backwards):
    @_case(f"order, {name}{', backwards' if backwards else ''}")
    def _():
        s = _ORDERS[name][::-1] if backwards else _ORDERS[name]
        def claim(case, r):
            other = restate(case, s[::-1])
            differ = [not np.array_equal(x, y) for x, y in zip(r.after, other.after)]
            assert any(differ), "the other order gives other blocks"
            assert any(len(b) == len(s) for b in bins(case.pos, s)), "every shape in one chunk's bin"
        return _over_pattern(s, R.touched_chunks(s), claim)


for _n in _ORDERS:
    _order_case(_n, False)
    _order_case(_n, True)


def _limit_case(sign):
    @_case(f"limits, chunk_pos and coordinates at {'+' if sign > 0 else '-'}(2^17 - 1) and (2^22 - 1)")
    def _():
        m = sign * CHUNK_MAX
        chunks = [(m, 1, -1), (-1, m, 1), (1, -1, m), (m, m, m)]
        shapes = []
        for p in chunks:
            o = [32 * v for v in p]
            far = [sign * COORD_MAX if v == m else o[i] + 5 for i, v in enumerate(p)]      # the last coordinate a shape may have
            near = [o[i] + (31 if sign > 0 else 0) if v == m else o[i] + 5 for i, v in enumerate(p)]      # the chunk's outermost voxel
            inward = [near[i] - sign * 6 if v == m else near[i] + 3 for i, v in enumerate(p)]
            shapes += [shape_sphere(far, 60.0, FILL), shape_line(far, inward, WOOD), shape_sphere(inward, 4.9, LEAVES), shape_point(near, STONE)]
        def claim(case, r):
            assert r.changed.all()
            for y in r.after:
                assert all((y == v).any() for v in (FILL, WOOD, LEAVES, STONE)), "a sphere and a line from the limit, a small sphere and a point in every chunk"
            assert max(abs(v) for p in case.pos for v in p) == CHUNK_MAX
            assert max(abs(v) for s in shapes for v in s[2]) == COORD_MAX
        return _over_pattern(shapes, chunks, claim)


_limit_case(1)
_limit_case(-1)


@_case("one position twice, with different trees")
def _():
    a, b = trees()["leaves at depth 3"][0], pattern_tree((1, 1, 1))
    nodes, offs = _concat([a, b, a])
    s = [shape_sphere((48, 48, 48), 6.9, FILL), shape_point((33, 33, 33), WOOD)]
    def claim(case, r):
        assert case.pos[0] == case.pos[1] and r.changed.tolist() == [1, 1, 0]
        assert not np.array_equal(r.after[0], r.after[1]) and np.array_equal(r.after[0] == FILL, r.after[1] == FILL)
        assert bins(case.pos, s) == [[0, 1], [0, 1], []]
    return [(1, 1, 1), (1, 1, 1), (1, 2, 1)], nodes, offs, s, claim


@_case("bins, both ways of making them in one call")
def _():
    c = (2, -1, 3)
    around = [(c[0] + dx, c[1] + dy, c[2] + dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    chunks = around + [(40, 40, 40)]
    s = [shape_sphere(tuple(32 * v + 16 for v in c), 40.0, FILL),                      # 27 cells <= 28 chunks: looked up
         shape_disc((32 * c[0] + 16, 32 * c[1], 32 * c[2] + 16), 2000.5, 3, WATER),    # 125 x 1 x 126 cells: every chunk tested
         shape_point((32 * 40 + 1, 32 * 40 + 2, 32 * 40 + 3), STONE)]                  # 1 cell
    def claim(case, r):
        assert [box_cells(x) > len(case.pos) for x in s] == [False, True, False]
        b = bins(case.pos, s)
        assert sorted(map(tuple, b)).count((0, 1)) == 9 and b[-1] == [2] and sum(len(x) for x in b) == 27 + 9 + 1
        assert r.changed.all() and (r.after[13] == FILL).sum() + (r.after[13] == WATER).sum() == 32768
    return _over_pattern(s, chunks, claim)


def _batch_case(n):
    @_case(f"batches, {n} chunks in a row with hand-made trees")
    def _():
        t = trees()
        small = [t[k][0] for k in ("uniform", "leaves at depth 1", "leaves at depth 2", "a child block shared by two parents", "leaves at depth 3",
                                   "eight equal leaves unmerged at depth 1", "child blocks in descending order", "garbage between the blocks",
                                   "the last block ends at len")]
        big = {5: "leaves at depth 4", 700: "voxels in the even level-4 cells", BATCH - 2: "eight equal leaves unmerged at depth 4",
               BATCH - 1: "leaves at depth 4", BATCH: "voxels in the odd level-4 cells", BATCH + 1: "leaves at depth 3", BATCH + 2: "leaves at depth 4"}
        parts = [t[big[i]][0] if i in big else small[(i * 7 + i // 9) % len(small)] for i in range(n)]
        nodes, offs = _concat(parts)
        pos = [(i, 0, 0) for i in range(n)]
        x0 = 32 * BATCH
        shapes = [shape_point((32 * 7 + 3, 4, 5), FILL), shape_sphere((32 * 101, 16, 16), 9.9, FILL),        # in the first batch
                  shape_disc((32 * 700 + 16, 30, 16), 5.9, 2, FILL),
                  shape_point((x0 - 1, 31, 0), FILL),                                                          # its last chunk
                  shape_point((x0, 0, 31), FILL),                                                              # the second's first
                  shape_line((x0 - 5, 3, 3), (x0 + 6, 9, 3), FILL),                                            # both at once
                  shape_sphere((x0, 16, 16), 4.9, LEAVES)]
        if n > BATCH + 1:
            shapes += [shape_point((x0 + 32 + 9, 9, 9), FILL), shape_line((x0 + 60, 1, 1), (x0 + 70, 1, 30), FILL)]
        def claim(case, r):
            b = bins(case.pos, shapes)
            start = np.concatenate([[0], np.cumsum([len(x) for x in b])])
            assert start[BATCH] >= 5 and int(case.offsets[BATCH]) > 500000, "the second batch's first bin and first word are far from 0"
            assert len(set(np.diff(case.offsets.astype(np.int64)).tolist())) >= 10, "trees of many lengths"
            want = {7, 100, 101, 700, BATCH - 1, BATCH} | ({BATCH + 1, BATCH + 2} if n > BATCH + 1 else set())
            assert set(np.flatnonzero(r.changed).tolist()) == want
            assert len(b[BATCH - 1]) == 3 and len(b[BATCH]) == 3
            for i in range(BATCH + 1, n):      # past the second batch's first chunk: node_off relative to the batch, and not 0
                assert int(case.offsets[i] - case.offsets[BATCH]) > 0 and start[i] > start[BATCH] and len(b[i]) >= 1
            assert int(case.offsets[-1]) < 4 << 20 and start[-1] < 64
        return pos, nodes, offs, shapes, claim


_batch_case(BATCH + 1)
_batch_case(BATCH + 3)      # one chunk more than a batch has no second chunk in the second batch: here node_off is not 0 there


@_case("everything large at once: 180 chunks, 1100 shapes, 8800 bin entries")
def _():
    """Above the floors of the call's three device buffers (2^20 node words, 1024 shapes, 4096 bin entries), and the largest
    case of the table in each."""
    chunks = [(x, y, z) for z in range(-3, 2) for y in range(6) for x in range(-2, 4)]
    rng = np.random.default_rng(11)
    corners = [(32 * int(rng.integers(-1, 4)), 32 * int(rng.integers(1, 6)), 32 * int(rng.integers(-2, 2))) for _ in range(1100)]
    s = [shape_sphere(tuple(int(v) + int(d) for v, d in zip(c, rng.integers(-1, 1, 3))), 2.9, int(rng.choice([FILL, WOOD, 0]))) for c in corners]
    def claim(case, r):
        b = bins(case.pos, s)
        assert len(s) > 1024 and sum(len(x) for x in b) == 8 * len(s) > 4096 and int(case.offsets[-1]) > 3 * (1 << 20)
        assert max(len(x) for x in b) > 40 and r.changed.sum() > 100, "long bins, in order"
        _carves_and_overwrites(case, r)
    return _over_pattern(s, chunks, claim)


@_case("a tree and a lake at the corner of eight generated chunks")
def _():
    pos, nodes, offs, _ = _block(CORNER_CHUNK)
    def claim(case, r):
        assert 4 <= r.changed.sum() < 8
    return pos, nodes, offs, _feature(CORNER_CHUNK), claim


NAMES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def get(name) -> Case:
    pos, nodes, offs, shapes, claim = _BUILDERS[name]()
    pos = [tuple(int(v) for v in p) for p in pos]
    nodes = np.ascontiguousarray(nodes, np.uint16)
    nodes.setflags(write=False)
    return Case(name, pos, nodes, np.asarray(offs, np.uint64), list(shapes), claim)
