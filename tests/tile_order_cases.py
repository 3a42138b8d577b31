"""The synthetic costs the tile-order kernels are held to (tests/test_gpu_tile_order.py, through vrt_selftest_tile_order) and the
reference is held to itself with (tests/test_tile_order_ref.py): sizes, shapes, radii and cost patterns, from a seeded generator."""
import numpy as np

# tiles in a row for the exact sort: one tile, around one chunk of 64, two chunks, exactly one scan piece of 64 chunks, a second piece of
# one chunk, 8 191, and 1080p's 32 400 (507 chunks, 8 pieces)
EXACT_SIZES = [1, 63, 64, 65, 128, 4096, 4097, 8191, 32400]

# (tiles_x, tiles_y) for the block order.  1 x 128 and 4 x 32: one block a row (the branch beside the magic multiply), per-word and
# 16-byte loads; 5 x 5: blocks one tile wide and one tile high, bw a power of two; 7 x 9: blocks three tiles wide; 6 x 10: two wide, two
# high; 25 x 13: a 200 x 104 frame; 1020 x 4 and 4 x 1020: 255 blocks a side; 240 x 135: 1080p, 2 040 blocks; 480 x 270: 4K, 8 160 blocks
SMALL_SHAPES = [(1, 128), (4, 32), (5, 5), (7, 9), (6, 10), (25, 13), (1020, 4), (4, 1020)]
LARGE_SHAPES = [(240, 135), (480, 270)]
BLOCK_CASES = [(s, r) for s in SMALL_SHAPES for r in (1, 5, 6)] + [(s, 5) for s in LARGE_SHAPES]
# what the block order refuses: 256 blocks a side, 8 228 blocks, a radius of 7
REFUSED = [((1024, 4), 5), ((484, 272), 5), ((25, 13), 7)]

HOT = 100


def hot_positions(tiles_x, tiles_y):
    """Where the one hot tile goes in turn: the corners, then the last column and the last row (partial blocks unless the size is a
    multiple of four) half way along."""
    at = [(0, 0), (tiles_x - 1, 0), (0, tiles_y - 1), (tiles_x - 1, tiles_y - 1), (tiles_x - 1, tiles_y // 2), (tiles_x // 2, tiles_y - 1)]
    return list(dict.fromkeys(at))


# (independent random trips have one dilated maximum almost everywhere — a block and its neighbours are hundreds of draws —: the ramps and
# the random field are what gives the block order many classes)
PATTERNS = ("constant", "ascending", "descending", "pairs", "uniform 0..7", "full 32 bits, saturated", "uniform 0..255", "ramp", "ramp back", "random field")


def pattern_names(tiles_x, tiles_y):
    return list(PATTERNS) + [f"hot {k}" for k in range(len(hot_positions(tiles_x, tiles_y)))]


def costs(name, tiles_x, tiles_y):
    """cost[tiles_x * tiles_y] (uint32) of the pattern `name`; the same array whenever it is asked for."""
    n = tiles_x * tiles_y
    i = np.arange(n, dtype=np.uint64)
    rng = np.random.default_rng([tiles_x, tiles_y, PATTERNS.index(name) if name in PATTERNS else 99])
    if name == "constant":
        c = np.full(n, 37, dtype=np.uint64)
    elif name == "ascending":       # steps of two: a class a tile, up to the last class
        c = 2 * i
    elif name == "descending":
        c = 2 * (n - 1 - i)
    elif name == "pairs":           # 2k, 2k + 1: each pair is one class (again from 0 after 128 tiles, so that a large frame has no class of thousands)
        c = i % 128
    elif name == "uniform 0..7":    # four classes and long ties
        c = rng.integers(0, 8, n, dtype=np.uint64)
    elif name == "full 32 bits, saturated":   # every one of them class 63: the values around the last class's start and the largest word
        c = rng.integers(0, 1 << 32, n, dtype=np.uint64)
        some = rng.permutation(n)[:n // 10]
        c[some] = np.array([126, 127, 128, 0xFFFFFFFF], dtype=np.uint64)[np.arange(some.size) % 4]
    elif name == "uniform 0..255":  # every class, half of the tiles in the last one
        c = rng.integers(0, 256, n, dtype=np.uint64)
    elif name in ("ramp", "ramp back"):   # up (down) to the right and to the bottom: a dilated maximum comes from one side alone
        x, y = i % tiles_x, i // tiles_x
        if name == "ramp back":
            x, y = tiles_x - 1 - x, tiles_y - 1 - y
        c = (126 * (x * max(tiles_y - 1, 1) + y * max(tiles_x - 1, 1))) // max((tiles_x > 1) + (tiles_y > 1), 1) // (max(tiles_x - 1, 1) * max(tiles_y - 1, 1))
    elif name == "random field":    # random trips 0..127 every 32 tiles, interpolated: neighbouring blocks differ by little, distant ones by much
        gx, gy = (tiles_x + 31) // 32 + 1, (tiles_y + 31) // 32 + 1
        g = rng.integers(0, 128, (gy, gx)).astype(np.int64)
        x, y = (i % tiles_x).astype(np.int64), (i // tiles_x).astype(np.int64)
        x0, y0, fx, fy = x // 32, y // 32, x % 32, y % 32
        c = ((g[y0, x0] * (32 - fx) + g[y0, x0 + 1] * fx) * (32 - fy) + (g[y0 + 1, x0] * (32 - fx) + g[y0 + 1, x0 + 1] * fx) * fy) // 1024
        c = c.astype(np.uint64)
    elif name.startswith("hot "):
        x, y = hot_positions(tiles_x, tiles_y)[int(name[4:])]
        c = np.zeros(n, dtype=np.uint64)
        c[y * tiles_x + x] = HOT
    else:
        raise KeyError(name)
    return (c & np.uint64(0xFFFFFFFF)).astype(np.uint32)
