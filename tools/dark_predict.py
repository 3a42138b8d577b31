"""tools/dark_predict.py [tiles] — what the dark marks should take out of the headline frame, from the CPU oracle alone.

The bench's standing camera over the 8^3-chunk world at 1920 x 1080; `tiles` whole 8 x 8 tiles (default 2000) drawn with the seed
of tools/lit_voxel_predict.py, whose march this tool uses: the oracle gives every pixel's primary hit, the shadow ray from it is
marched in numpy binary32 lookup by lookup over a dense copy of the world, and for every lookup today's marks (the lit cells, the
lit voxels at K = 8 with their budget) and the dark rule of tests/dark_cell_ref.py say whether the lane would stop there.  A wave
makes as many trips through its shadow loop as its slowest lane; the table is the sum over the tiles.  Rules: closed voxel layers
of full solid cells only, the rule as it is ("floors": split cells count by their closed layers), the same with transitivity, and
the same at smaller depths.

Prints the table that opens profiles/dark_marks_ab.txt, and the sanity counts, which must be 0.  No GPU."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dark_cell_ref as D      # noqa: E402
import lit_corridor_ref as C   # noqa: E402
import lit_voxel_ref as R      # noqa: E402
import path_ref                # noqa: E402
from lit_voxel_predict import TILES_PER_LAUNCH, VALU_PER_TRIP, leaf_sizes, march   # noqa: E402
from oracle import orc         # noqa: E402
from voxelraytracing_amd import scenes  # noqa: E402

F = np.float32
K = 8                     # today's voxel layers at 64^3 cells
VALU_PER_LAUNCH = 55.4e6  # profiles/lit_voxels_ab.txt: the marked launch
OTHER_SUNS = [(200.0, 1200.0, 3000.0), (5000.0, 1500.0, 0.0), (100.0, -5000.0, 100.0)]


def main():
    n_tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    sc = scenes.c2((1920, 1080))
    o = orc.from_package_scene(sc)
    with tempfile.TemporaryDirectory() as tmp:   # (the library stays loaded; its file need not stay)
        dense = path_ref.load(tmp).dense_world(o)
    n = dense.shape[0]
    G = n // 4
    sun = np.array([F(F(sc.settings.sun_pos[a]) - F(float(o.c.world.min[a]))) for a in range(3)], F)
    sun_t = tuple(float(s) for s in sun)
    liquid = np.array([bool(sc.materials[i].is_liquid) for i in range(256)])
    lo = C.leaf_lo(dense)
    plan = C.plan(n, sun_t)
    cell_lit = C.lit(lo, sun_t, G).astype(bool)
    masks = D.floor_masks(dense, plan[0], liquid)
    full = np.where(masks == 15, 15, 0).astype(np.uint8)
    rules = [("full solid cells, whole corridor", D.dark(lo, full, sun_t)),
             ("floors, whole corridor", D.dark(lo, masks, sun_t)),
             ("floors, transitive", D.dark(lo, masks, sun_t, transitive=True))]
    rules += [(f"floors, depth {d}", D.dark(lo, masks, sun_t, depth=d)) for d in (4, 8, 16, 32)]
    up = lambda cells: np.repeat(np.repeat(np.repeat(cells.astype(bool), 4, 0), 4, 1), 4, 2)   # noqa: E731
    lit_cells = up(cell_lit)
    lit_voxels = R.lit_voxels(dense, R.split_cells(dense), cell_lit, sun_t, K).astype(bool)
    stops = [lit_cells, lit_voxels] + [up(d) for _, d in rules]
    cell_trips = 500 - (6 * (n // (plan[2] + 1) + 1) + 2) - 1
    voxel_trips = cell_trips - R.budget(K)

    rng = np.random.default_rng(20262)
    tiles = rng.choice((1080 // 8) * (1920 // 8), n_tiles, replace=False)
    origins, lanes, prim = [], [], np.zeros(n_tiles, np.int64)
    for ti, t in enumerate(tiles):
        ty, tx = divmod(int(t), 1920 // 8)
        for ly in range(8):
            for lx in range(8):
                idw, _, _, out = o.trace_pixel(orc.MODE_PRIMARY_SHADOW, tx * 8 + lx, ty * 8 + ly)
                prim[ti] = max(prim[ti], int(out[7]))
                if idw & orc.ID_SHADOW_RAY:
                    origins.append([F(out[a]) + F(out[3 + a]) * F(0.002) for a in range(3)])
                    lanes.append(ti)
    origins, lanes = np.array(origins, F), np.array(lanes)
    total, first, hit = march(dense, leaf_sizes(dense), liquid, origins, sun, stops)

    def wave_trips(stop_at):
        stop = np.where(stop_at > 0, stop_at, total)
        w = np.zeros(n_tiles, np.int64)
        np.maximum.at(w, lanes, stop)
        return w

    def earliest(*fs):
        big = np.iinfo(np.int32).max
        m = np.minimum.reduce([np.where(f > 0, f, big) for f in fs])
        return np.where(m == big, 0, m)

    # today's marks: a voxel's mark stops a lane up to voxel_trips, a cell's up to cell_trips
    today = earliest(np.where(first[1] <= voxel_trips, first[1], 0), np.where(first[0] <= cell_trips, first[0], 0))
    base, none = wave_trips(today), wave_trips(np.zeros_like(total))
    occluded = hit
    print(f"{n_tiles} tiles of 8 x 8 (seed 20262) of the 1920 x 1080 frame, {len(lanes)} shadow rays, {int(occluded.sum())} of them occluded "
          f"({int((occluded & (total > 20)).sum())} after more than 20 lookups; mean lookups occluded {total[occluded].mean():.1f}, not {total[~occluded].mean():.1f})")
    print(f"primary wave trips {prim.sum()} ({prim.mean():.2f} a tile); shadow wave trips without marks {none.sum()} ({none.mean():.2f} a tile)")
    all_stop = wave_trips(np.where(occluded, 1, today))
    print(f"every occluded ray stopped at its first lookup: shadow wave trips {100 * (all_stop.sum() - base.sum()) / base.sum():.1f}%")
    print(f"air cells {int((lo >= 0).sum())}, lit {int(cell_lit.sum())}")
    print(f"{'rule':<36}{'dark cells':>11}{'shadow trips':>13}{'a tile':>8}{'shadow':>9}{'all trips':>11}{'VALU / launch':>15}")
    print(f"{'today: lit cells + voxels, K = 8':<36}{'':>11}{base.sum():>13}{base.mean():>8.2f}")
    for (what, cells), f in zip(rules, first[2:]):
        w = wave_trips(earliest(today, np.where(f <= cell_trips, f, 0)))
        ds = (w.sum() - base.sum()) / base.sum()
        da = (w.sum() - base.sum()) / (base.sum() + prim.sum())
        dv = (w.sum() - base.sum()) / n_tiles * TILES_PER_LAUNCH * VALU_PER_TRIP / VALU_PER_LAUNCH
        wrong = int(((f > 0) & ~occluded).sum())
        print(f"{what:<36}{int(cells.sum()):>11}{w.sum():>13}{w.mean():>8.2f}{100 * ds:>8.1f}%{100 * da:>10.1f}%{100 * dv:>14.1f}%"
              f"   dark stops on rays that miss: {wrong}")
    print(f"lit stops on rays that hit: {int(((today > 0) & occluded).sum())}")
    print(f"(VALU: {VALU_PER_TRIP} wave-instructions a fast trip against {VALU_PER_LAUNCH / 1e6:.1f} M a launch; a trip on the split path costs more, so the change is at least this)")
    print("dark cells of this world under other suns (floors, whole corridor / full solid cells):")
    for s in OTHER_SUNS:
        p = C.plan(n, s)
        m = D.floor_masks(dense, p[0], liquid)
        print(f"  {s}: {int(D.dark(lo, m, s).sum())} / {int(D.dark(lo, np.where(m == 15, 15, 0).astype(np.uint8), s).sum())}")


if __name__ == "__main__":
    main()
