"""tests/tile_order_ref.py held to itself (no GPU): hand-worked orders, the canonical block order through the checker on every shape
and pattern of tests/tile_order_cases.py, the mutations the checker and the exact reference must refuse, and that the cases show
something: enough classes, a hot region that ends inside the grid."""
import numpy as np
import pytest

import tile_order_cases as cases
import tile_order_ref as ref


# ---- hand-worked ----

def test_classes_by_hand():
    assert ref.cost_class(np.array([0, 1, 2, 3, 125, 126, 127, 128, 0xFFFFFFFF], dtype=np.uint32)).tolist() == [0, 0, 1, 1, 62, 63, 63, 63, 63]


def test_exact_order_by_hand():
    #                classes 1  0  2  1  0  2  63  63
    cost = np.array([2, 0, 5, 3, 1, 4, 126, 4000000000], dtype=np.uint32)
    assert ref.exact_order(cost).tolist() == [6, 7, 2, 5, 0, 3, 1, 4]
    assert ref.check_exact_order(cost, np.array([6, 7, 2, 5, 0, 3, 1, 4], dtype=np.uint32)) == []


def test_five_by_five_tiles_by_hand():
    """2 x 2 blocks of 4 x 4, 1 x 4, 4 x 1 and 1 x 1 tiles; one hot tile, radius 1: every block is within one block of it, one class, the
    blocks in turn and each row by row."""
    cost = np.zeros(25, dtype=np.uint32)
    cost[24] = 100
    assert ref.block_costs(cost, 5, 5).tolist() == [[0, 0], [0, 100]]
    assert ref.block_classes(cost, 5, 5, 1).tolist() == [13, 13, 13, 13]
    want = [0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 12, 13, 15, 16, 17, 18,   4, 9, 14, 19,   20, 21, 22, 23,   24]
    assert ref.canonical_block_order(cost, 5, 5, 1).tolist() == want
    assert ref.check_block_order(cost, 5, 5, 1, np.array(want, dtype=np.uint32)) == []
    # the blocks of one key in any order
    other = [24, 20, 21, 22, 23, 4, 9, 14, 19, 0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 12, 13, 15, 16, 17, 18]
    assert ref.check_block_order(cost, 5, 5, 1, np.array(other, dtype=np.uint32)) == []


def test_strips_by_hand():
    """One tile wide: a block is four tiles of the column.  8 tiles: two blocks, each within one of the other.  16 tiles, the last one
    hot, radius 1: blocks 2 and 3 first (class' 63 - 50), then blocks 0 and 1 (class' 63)."""
    cost = np.zeros(8, dtype=np.uint32)
    cost[5] = 100
    assert ref.block_classes(cost, 1, 8, 1).tolist() == [13, 13]
    assert ref.canonical_block_order(cost, 1, 8, 1).tolist() == list(range(8))
    cost = np.zeros(16, dtype=np.uint32)
    cost[15] = 100
    assert ref.block_classes(cost, 1, 16, 1).tolist() == [63, 63, 13, 13]
    assert ref.canonical_block_order(cost, 1, 16, 1).tolist() == [8, 9, 10, 11, 12, 13, 14, 15, 0, 1, 2, 3, 4, 5, 6, 7]
    assert ref.check_block_order(cost, 1, 16, 1, np.arange(16, dtype=np.uint32)) != []   # screen order: the cheap blocks first
    # ... and lying down it is the same blocks, each one row of four
    assert ref.canonical_block_order(cost, 16, 1, 1).tolist() == [8, 9, 10, 11, 12, 13, 14, 15, 0, 1, 2, 3, 4, 5, 6, 7]


def test_dilation_reaches_exactly_radius_blocks_and_is_clipped():
    """9 x 7 blocks, block (6, 1) hot, radius 2: the blocks 4..8 x 0..3 and no others."""
    cost = np.zeros(36 * 28, dtype=np.uint32)
    cost[(4 * 1 + 2) * 36 + 4 * 6 + 1] = 100
    cls = ref.block_classes(cost, 36, 28, 2).reshape(7, 9)
    hot = cls == 13
    assert hot[0:4, 4:9].all() and hot.sum() == 20 and (cls[~hot] == 63).all()


# ---- the canonical order passes everywhere ----

@pytest.mark.parametrize("shape,radius", cases.BLOCK_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"r{v}")
def test_canonical_block_order_passes(shape, radius):
    tx, ty = shape
    for name in cases.pattern_names(tx, ty):
        cost = cases.costs(name, tx, ty)
        assert ref.check_block_order(cost, tx, ty, radius, ref.canonical_block_order(cost, tx, ty, radius)) == [], name


# ---- mutations of a passing block order ----

TX, TY, RADIUS = 25, 13, 1


@pytest.fixture(scope="module")
def passing():
    cost = cases.costs("random field", TX, TY)
    order = ref.canonical_block_order(cost, TX, TY, RADIUS)
    assert ref.check_block_order(cost, TX, TY, RADIUS, order) == []
    return cost, order


def _runs(cost, order):
    """(start, block, class') of every run of a passing order."""
    cls = ref.block_classes(cost, TX, TY, RADIUS)
    block_of = ref.tile_blocks(TX, TY)
    out, p = [], 0
    while p < order.size:
        b = int(block_of[order[p]])
        out.append((p, b, int(cls[b])))
        p += ref.block_tiles(b, TX, TY).size
    return out


def _refused(cost, order, word):
    got = ref.check_block_order(cost, TX, TY, RADIUS, order)
    assert got and any(word in v for v in got), got


def test_checker_refuses_a_tile_dropped_for_a_duplicate(passing):
    cost, order = passing
    bad = order.copy()
    bad[6] = bad[5]
    _refused(cost, bad, "not a permutation")


def test_checker_refuses_an_entry_out_of_range(passing):
    cost, order = passing
    bad = order.copy()
    bad[3] = TX * TY
    _refused(cost, bad, f">= {TX * TY}")


def test_checker_refuses_an_entry_nobody_wrote(passing):
    cost, order = passing
    bad = order.copy()
    bad[7] = 0xFFFFFFFF
    _refused(cost, bad, "nobody wrote")


def test_checker_refuses_two_runs_of_different_classes_swapped(passing):
    cost, order = passing
    runs = _runs(cost, order) + [(order.size, -1, -1)]
    k = next(k for k in range(len(runs) - 2) if runs[k][2] != runs[k + 1][2])
    a, b, c = runs[k][0], runs[k + 1][0], runs[k + 2][0]
    bad = np.concatenate([order[:a], order[b:c], order[a:b], order[c:]])
    _refused(cost, bad, "the keys go down")


def test_checker_refuses_a_block_with_its_rows_transposed(passing):
    cost, order = passing
    p = next(p for p, b, _ in _runs(cost, order) if ref.block_tiles(b, TX, TY).size == 16)
    bad = order.copy()
    bad[p:p + 16] = order[p:p + 16].reshape(4, 4).T.reshape(-1)
    _refused(cost, bad, "row by row")


def test_checker_refuses_a_block_split_across_two_runs(passing):
    cost, order = passing
    runs = _runs(cost, order) + [(order.size, -1, -1)]
    k = next(k for k in range(len(runs) - 2) if runs[k + 1][0] - runs[k][0] == 16)
    a, b, c = runs[k][0], runs[k + 1][0], runs[k + 2][0]
    bad = np.concatenate([order[:a], order[a:b - 4], order[b:c], order[b - 4:b], order[c:]])   # its last row behind the next block
    _refused(cost, bad, "row by row")


def _order_of_dilation(cost, dilated):
    return ref.order_from_block_classes((ref.CLASSES - 1 - ref.cost_class(dilated)).reshape(-1), TX, TY)


def test_checker_refuses_a_dilation_of_radius_less_one():
    cost = cases.costs("random field", TX, TY)
    for radius in (2, 3):
        bad = ref.canonical_block_order(cost, TX, TY, radius - 1)
        assert ref.check_block_order(cost, TX, TY, radius - 1, bad) == []
        assert ref.check_block_order(cost, TX, TY, radius, bad) != []
    cost = cases.costs("hot 0", TX, TY)
    assert ref.check_block_order(cost, TX, TY, 5, ref.canonical_block_order(cost, TX, TY, 4)) != []


@pytest.mark.parametrize("pattern,which", [("ramp back", 0), ("hot 2", 0), ("ramp", 1), ("hot 1", 1), ("hot 3", 1)])
def test_checker_refuses_a_dilation_clamped_on_one_side_only(pattern, which):
    """Two ways of it: x + r not clamped at all on the right (0: the index runs on into the next row of blocks, or past the last block
    into nothing), and clamped one block early (1)."""
    cost = cases.costs(pattern, TX, TY)
    blocks = ref.block_costs(cost, TX, TY)
    bh, bw = blocks.shape
    flat = np.concatenate([blocks.reshape(-1), np.zeros(RADIUS + 1, dtype=blocks.dtype)])
    runs_on, early = np.zeros_like(blocks), np.zeros_like(blocks)
    for by in range(bh):
        for bx in range(bw):
            for dy in range(-RADIUS, RADIUS + 1):
                y = min(max(by + dy, 0), bh - 1)
                for dx in range(-RADIUS, RADIUS + 1):
                    runs_on[by, bx] = max(runs_on[by, bx], flat[y * bw + max(bx + dx, 0)])
                    early[by, bx] = max(early[by, bx], blocks[y, min(max(bx + dx, 0), bw - 2)])
    bad = _order_of_dilation(cost, (runs_on, early)[which])
    assert ref.check_block_order(cost, TX, TY, RADIUS, bad) != []


def test_checker_refuses_classes_of_the_undilated_maximum(passing):
    cost, _ = passing
    bad = ref.canonical_block_order(cost, TX, TY, 0)
    assert ref.check_block_order(cost, TX, TY, RADIUS, bad) != []


# ---- what the exact reference refuses ----

def test_exact_reference_refuses_an_unstable_and_an_ascending_sort():
    cost = cases.costs("pairs", 200, 1)
    cls = ref.cost_class(cost)
    good = ref.exact_order(cost)
    assert ref.check_exact_order(cost, good) == []
    unstable = np.lexsort((-np.arange(cost.size), ref.CLASSES - 1 - cls)).astype(np.uint32)   # the right classes, a class's tiles backwards
    assert sorted(unstable.tolist()) == list(range(200)) and (cls[unstable] == cls[good]).all()
    assert ref.check_exact_order(cost, unstable) != []
    ascending = np.argsort(cls, kind="stable").astype(np.uint32)
    assert ref.check_exact_order(cost, ascending) != []


@pytest.mark.parametrize("n", [4097, 8191, 32400])
def test_exact_reference_refuses_a_lost_scan_carry(n):
    """A scan of a class's chunks that forgets, from its second piece of 64 chunks on, what the pieces before it held: the tiles behind
    tile 4 096 land one piece's total of their class too early, on top of other tiles, and the end of the class is never written."""
    cost = cases.costs("uniform 0..255", n, 1)
    cls = ref.cost_class(cost)
    good = ref.exact_order(cost)
    place = np.empty(n, dtype=np.int64)
    place[good] = np.arange(n)
    bad = np.full(n, ref.UNWRITTEN, dtype=np.uint32)
    for t in range(n):
        piece = t // 4096
        lost = int((cls[(piece - 1) * 4096:piece * 4096] == cls[t]).sum()) if piece else 0
        bad[place[t] - lost] = t
    assert (bad == ref.UNWRITTEN).any()
    assert ref.check_exact_order(cost, bad) != []


def test_an_order_of_the_wrong_size_is_refused():
    cost = cases.costs("uniform 0..7", 5, 5)
    assert ref.check_exact_order(cost, np.arange(24, dtype=np.uint32)) != []
    assert ref.check_block_order(cost, 5, 5, 1, np.arange(24, dtype=np.uint32)) != []


# ---- every case shows something ----

@pytest.mark.parametrize("n", cases.EXACT_SIZES)
def test_the_exact_patterns_show_what_they_are_for(n):
    cls = {name: ref.cost_class(cases.costs(name, n, 1)) for name in cases.PATTERNS}
    ident = np.arange(n)
    assert ref.exact_order(cases.costs("constant", n, 1)).tolist() == ident.tolist()
    # a class a tile; beyond 64 tiles the last class holds the rest, in screen order
    assert ref.exact_order(cases.costs("ascending", n, 1)).tolist() == (ident[::-1].tolist() if n <= 64 else list(range(63, n)) + list(range(62, -1, -1)))
    assert ref.exact_order(cases.costs("descending", n, 1)).tolist() == ident.tolist()
    if n >= 64:
        assert len(set(cls["ascending"].tolist())) == 64 and len(set(cls["descending"].tolist())) == 64
    pairs = cls["pairs"]
    assert (pairs[0:n - n % 2:2] == pairs[1:n:2]).all()
    if n >= 63:
        assert len(set(cls["uniform 0..7"].tolist())) == 4            # ... and long ties
        assert len(set(cls["uniform 0..255"].tolist())) >= 8
        sat = cases.costs("full 32 bits, saturated", n, 1)
        assert (cls["full 32 bits, saturated"] == 63).all() and all((sat == v).any() for v in (126, 127, 128, 0xFFFFFFFF))
        assert not np.array_equal(ref.exact_order(cases.costs("uniform 0..255", n, 1)), ident)


@pytest.mark.parametrize("shape", cases.SMALL_SHAPES + cases.LARGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_block_patterns_show_what_they_are_for(shape):
    """The random field and the ramps give at least 8 dilated classes at the smallest radius a shape is run at (a shape of fewer than 28
    blocks: at least 2, it has no room for more); a hot tile in a corner gives two, and its region ends inside the grid on a side.
    (Independent random trips do not: a block and its neighbours are hundreds of draws, and their maximum is the same almost
    everywhere.  5 x 5 tiles are 2 x 2 blocks, all within one block of each other: that shape is there for its blocks one tile wide
    and high, and any dilation gives it one class.)"""
    tx, ty = shape
    bw, bh = ref.block_grid(tx, ty)
    radius = min(r for s, r in cases.BLOCK_CASES if s == shape)
    if shape != (5, 5):
        for name in ("random field", "ramp", "ramp back"):
            assert len(set(ref.block_classes(cases.costs(name, tx, ty), tx, ty, radius).tolist())) >= (8 if bw * bh >= 28 else 2), name
        for k, (x, y) in enumerate(cases.hot_positions(tx, ty)):
            if x not in (0, tx - 1) or y not in (0, ty - 1):
                continue
            cls = ref.block_classes(cases.costs(f"hot {k}", tx, ty), tx, ty, radius).reshape(bh, bw)
            hot = cls == 63 - 50
            assert set(cls.reshape(-1).tolist()) == {13, 63}
            cols, rows = np.flatnonzero(hot.any(axis=0)), np.flatnonzero(hot.any(axis=1))
            assert hot[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1].all()      # a rectangle ...
            assert cols.size == min(radius + 1, bw) and rows.size == min(radius + 1, bh)   # ... of exactly radius blocks beyond the corner's
            assert cols.size < bw or rows.size < bh
    else:
        assert set(ref.block_classes(cases.costs("hot 0", tx, ty), tx, ty, radius).tolist()) == {13}


# ---- the scenes of the frame tests have classes to sort ----

@pytest.mark.parametrize("size,mode", [((128, 64), "shadow"), ((200, 104), "shadow"), ((640, 360), "shadow"), ((640, 360), "primary"), ((1920, 1080), "shadow")],
                         ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_the_resting_views_have_eight_classes(orc, size, mode):
    """The oracle's per-tile step maxima (a bound on, and close to, the trips a tile's wave notes: tests/test_gpu_sun_marks.py) of the
    views tests/test_gpu_tile_order.py rests on: at least 8 cost classes, and not in screen order."""
    from voxelraytracing_amd import MODE_PRIMARY, MODE_PRIMARY_SHADOW, scenes
    sc = scenes.c2(size)
    w, h = size
    _, _, steps, _ = orc.from_package_scene(sc).render(MODE_PRIMARY_SHADOW if mode == "shadow" else MODE_PRIMARY, w, h, want_steps=True)
    steps = steps[:h // 8 * 8, :w // 8 * 8]
    tiles = (steps & 0xFFFF).reshape(h // 8, 8, w // 8, 8).max(axis=(1, 3)) + (steps >> 16).reshape(h // 8, 8, w // 8, 8).max(axis=(1, 3))
    cls = ref.cost_class(tiles.reshape(-1))
    assert len(set(cls.tolist())) >= 8, sorted(set(cls.tolist()))
    assert not np.array_equal(ref.exact_order(tiles.reshape(-1)), np.arange(tiles.size))
