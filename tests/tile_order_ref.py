"""The order a one-frame-at-a-time context launches its 8 x 8 tiles in, from the rule alone (numpy and integers; include/vrt.h:
vrt_read_tile_order, vrt_selftest_tile_order).  tests/test_tile_order_ref.py holds this file to itself, tests/test_gpu_tile_order.py
holds the kernels to it.

    class of a trip count        min(trips >> 1, 63)
    the exact order              tiles by descending class, screen order within a class: ONE array
    the block order              blocks of 4 x 4 tiles (ragged at the right and bottom edges), block b = by * bw + bx; a block's cost is
                                 the maximum over its own tiles, its dilated cost the maximum over the blocks within `radius` in x and
                                 in y, clipped to the grid; class' = 63 - class(dilated cost).  The order is a permutation of the tiles
                                 cut into runs, one per block, each the block's tiles row by row, the runs' keys (class', b >> 6)
                                 non-decreasing.  Within one key any order of the blocks is right (the kernel places them with an LDS
                                 atomic), so this is a checker, and the canonical order (blocks ascending inside a key) one that passes.
"""
import numpy as np

CLASSES = 64
UNWRITTEN = 0xFFFFFFFF


def cost_class(cost):
    return np.minimum(np.asarray(cost, dtype=np.uint64) >> np.uint64(1), np.uint64(CLASSES - 1)).astype(np.int64)


# ---- the exact order ----

def exact_order(cost):
    return np.argsort(CLASSES - 1 - cost_class(cost).reshape(-1), kind="stable").astype(np.uint32)


def check_exact_order(cost, order):
    """Violations (strings) of `order` against the exact order of `cost`; none: it is that order, entry for entry."""
    want = exact_order(cost)
    order = np.asarray(order)
    if order.shape != want.shape:
        return [f"{order.shape} entries for {want.size} tiles"]
    bad = np.flatnonzero(order.astype(np.int64) != want.astype(np.int64))
    if bad.size == 0:
        return []
    p = int(bad[0])
    return [f"{bad.size} of {want.size} entries differ, the first at position {p}: tile {int(order[p])} where tile {int(want[p])} belongs"]


# ---- the block order ----

def block_grid(tiles_x, tiles_y):
    return (tiles_x + 3) // 4, (tiles_y + 3) // 4


def block_tiles(b, tiles_x, tiles_y):
    """The tiles of block b, row by row."""
    bw, _ = block_grid(tiles_x, tiles_y)
    by, bx = divmod(b, bw)
    xs = np.arange(4 * bx, min(4 * bx + 4, tiles_x), dtype=np.int64)
    ys = np.arange(4 * by, min(4 * by + 4, tiles_y), dtype=np.int64)
    return (ys[:, None] * tiles_x + xs[None, :]).reshape(-1)


def block_costs(cost, tiles_x, tiles_y):
    """[bh, bw]: the maximum over each block's own tiles."""
    c = np.asarray(cost, dtype=np.uint64).reshape(tiles_y, tiles_x)
    bw, bh = block_grid(tiles_x, tiles_y)
    out = np.empty((bh, bw), dtype=np.uint64)
    for by in range(bh):
        for bx in range(bw):
            out[by, bx] = c[4 * by:4 * by + 4, 4 * bx:4 * bx + 4].max()
    return out


def dilate(blocks, radius):
    """[bh, bw]: the maximum over the blocks within `radius` in x and in y, clipped to the grid (radius 0: the blocks themselves)."""
    bh, bw = blocks.shape
    out = np.empty_like(blocks)
    for by in range(bh):
        for bx in range(bw):
            out[by, bx] = blocks[max(by - radius, 0):by + radius + 1, max(bx - radius, 0):bx + radius + 1].max()
    return out


def block_classes(cost, tiles_x, tiles_y, radius):
    """class'[bh * bw] of every block: 0 is the most expensive."""
    return (CLASSES - 1 - cost_class(dilate(block_costs(cost, tiles_x, tiles_y), radius))).reshape(-1)


def block_keys(classes):
    """(class', b >> 6) of every block as one integer."""
    classes = np.asarray(classes, dtype=np.int64)
    return classes * (1 << 32) + (np.arange(classes.size, dtype=np.int64) >> 6)


def order_from_block_classes(classes, tiles_x, tiles_y):
    """The tiles of the blocks by ascending (class', b), each block row by row."""
    blocks = np.argsort(np.asarray(classes, dtype=np.int64), kind="stable")
    return np.concatenate([block_tiles(int(b), tiles_x, tiles_y) for b in blocks]).astype(np.uint32)


def canonical_block_order(cost, tiles_x, tiles_y, radius):
    return order_from_block_classes(block_classes(cost, tiles_x, tiles_y, radius), tiles_x, tiles_y)


def tile_blocks(tiles_x, tiles_y):
    """[tiles]: the block of every tile."""
    bw, _ = block_grid(tiles_x, tiles_y)
    t = np.arange(tiles_x * tiles_y, dtype=np.int64)
    return (t // tiles_x // 4) * bw + (t % tiles_x) // 4


def check_block_order(cost, tiles_x, tiles_y, radius, order):
    """Violations (strings) of `order` against the rule above; none: it is a block order of `cost` dilated over `radius` blocks."""
    n = tiles_x * tiles_y
    order = np.asarray(order)
    if order.shape != (n,):
        return [f"{order.shape} entries for {n} tiles"]
    order = order.astype(np.int64)
    out = []
    unwritten = np.flatnonzero(order == UNWRITTEN)
    if unwritten.size:
        out.append(f"{unwritten.size} entries nobody wrote (0xFFFFFFFF), the first at position {int(unwritten[0])}")
    beyond = np.flatnonzero((order >= n) & (order != UNWRITTEN))
    if beyond.size:
        out.append(f"{beyond.size} entries >= {n}, the first at position {int(beyond[0])}: {int(order[beyond[0]])}")
    seen = np.bincount(order[(order >= 0) & (order < n)], minlength=n)
    if (seen != 1).any():
        twice, never = np.flatnonzero(seen > 1), np.flatnonzero(seen == 0)
        out.append(f"not a permutation: {twice.size} tiles more than once (first: {twice[:1].tolist()}), {never.size} missing (first: {never[:1].tolist()})")
    if out:
        return out
    classes = block_classes(cost, tiles_x, tiles_y, radius)
    keys = block_keys(classes)
    block_of = tile_blocks(tiles_x, tiles_y)
    p, before, before_b = 0, -1, -1
    while p < n:
        b = int(block_of[order[p]])
        tiles = block_tiles(b, tiles_x, tiles_y)
        if not np.array_equal(order[p:p + tiles.size], tiles):
            return [f"position {p}: the {tiles.size} tiles of block {b} are not there contiguous and row by row: {order[p:p + tiles.size].tolist()}"]
        if keys[b] < before:
            return [f"position {p}: block {b} (class' {int(classes[b])}, chunk {b >> 6}) behind block {before_b} (class' {int(classes[before_b])}, "
                    f"chunk {before_b >> 6}): the keys go down"]
        before, before_b = int(keys[b]), b
        p += tiles.size
    return []


def position_keys(cost, tiles_x, tiles_y, radius, order):
    """[tiles]: the key (class', chunk) of the block whose tile stands at each position of `order` (a permutation)."""
    keys = block_keys(block_classes(cost, tiles_x, tiles_y, radius))
    return keys[tile_blocks(tiles_x, tiles_y)[np.asarray(order).astype(np.int64)]]


def sorted_within_keys(order, keys):
    """`order` with the tiles of every key in ascending order: equal for two orders exactly when the multisets per key are."""
    order = np.asarray(order).astype(np.int64)
    return order[np.lexsort((order, keys))]
