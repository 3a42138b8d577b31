"""tools/dark_voxel_predict.py [tiles] — what the dark voxel marks should take out of the headline frame, from the CPU oracle alone.

The set-up is tools/dark_predict.py's: the bench's standing camera over the 8^3-chunk world at 1920 x 1080, `tiles` whole 8 x 8 tiles
(default 800) drawn with its seed, every pixel's primary hit from the oracle, the shadow ray marched in numpy binary32 lookup by
lookup (tools/lit_voxel_predict.py's march) over a dense copy of the world.  The base is today's marks: the lit cells, the lit
voxels at K = 8 with their budget, the dark cells at depth 32.  On top of them the dark voxel rule of tests/dark_voxel_ref.py at
K_d = 8, 16, 32, 64: a lane that looks up a dark voxel while the wave still reads the shadow pool stops there.

Prints the table that opens profiles/dark_voxels_ab.txt: dark voxels per depth, shadow and total wave trips, the look-ups the walk
makes per candidate (the voxels of REACH_1 .. REACH_k up to the layer that decides, or to the world's side), and the sanity count
"dark stops on rays that miss", which must be 0.  No GPU."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dark_cell_ref as D      # noqa: E402
import dark_voxel_ref as V     # noqa: E402
import lit_corridor_ref as C   # noqa: E402
import lit_voxel_ref as R      # noqa: E402
import path_ref                # noqa: E402
from lit_voxel_predict import TILES_PER_LAUNCH, VALU_PER_TRIP, leaf_sizes, march   # noqa: E402
from oracle import orc         # noqa: E402
from voxelraytracing_amd import scenes  # noqa: E402

F = np.float32
K = 8                      # today's lit voxel layers at 64^3 cells
DARK_DEPTH = 32            # today's dark cell depth there
DEPTHS = (8, 16, 32, 64)
VALU_PER_LAUNCH = 50.24e6  # profiles/dark_marks_ab.txt: the marked launch


def main():
    n_tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 800
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
    split = R.split_cells(dense)
    cell_lit = C.lit(lo, sun_t, G).astype(bool)
    cell_dark = D.dark(lo, D.floor_masks(dense, plan[0], liquid), sun_t, depth=DARK_DEPTH).astype(bool)
    up = lambda cells: np.repeat(np.repeat(np.repeat(cells.astype(bool), 4, 0), 4, 1), 4, 2)   # noqa: E731
    lit_voxels = R.lit_voxels(dense, split, cell_lit, sun_t, K).astype(bool)
    candidates = int((up(split) & (dense == 0) & ~lit_voxels).sum())
    rules = [(f"voxel layers K_d = {d}", V.dark_voxels(dense, split, lit_voxels, cell_dark, sun_t, d, liquid).astype(bool)) for d in DEPTHS]
    stops = [up(cell_lit), lit_voxels, up(cell_dark)] + [v for _, v in rules]
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

    # today's marks: a voxel's mark stops a lane up to voxel_trips, a cell's (lit or dark) up to cell_trips
    today = earliest(np.where(first[1] <= voxel_trips, first[1], 0), np.where(first[0] <= cell_trips, first[0], 0),
                     np.where(first[2] <= cell_trips, first[2], 0))
    base = wave_trips(today)
    print(f"{n_tiles} tiles of 8 x 8 (seed 20262) of the 1920 x 1080 frame, {len(lanes)} shadow rays, {int(hit.sum())} of them occluded")
    print(f"primary wave trips {prim.sum()} ({prim.mean():.2f} a tile)")
    all_stop = wave_trips(np.where(hit, 1, today))
    print(f"every occluded ray stopped at its first lookup: shadow wave trips {100 * (all_stop.sum() - base.sum()) / base.sum():.1f}%")
    print(f"split cells {int(split.sum())}, their air voxels without a lit mark (the candidates) {candidates}, dark cells {int(cell_dark.sum())}")
    print(f"{'rule':<36}{'dark voxels':>12}{'shadow trips':>13}{'a tile':>8}{'shadow':>9}{'all trips':>11}{'VALU / launch':>15}")
    print(f"{'today: lit marks, dark cells':<36}{'':>12}{base.sum():>13}{base.mean():>8.2f}")
    for (what, voxels), f in zip(rules, first[3:]):
        # (a dark voxel stops a lane while the wave reads the shadow pool: up to the lit voxel marks' trip count)
        w = wave_trips(earliest(today, np.where(f <= voxel_trips, f, 0)))
        ds = (w.sum() - base.sum()) / base.sum()
        da = (w.sum() - base.sum()) / (base.sum() + prim.sum())
        dv = (w.sum() - base.sum()) / n_tiles * TILES_PER_LAUNCH * VALU_PER_TRIP / VALU_PER_LAUNCH
        wrong = int(((f > 0) & ~hit).sum())
        print(f"{what:<36}{int(voxels.sum()):>12}{w.sum():>13}{w.mean():>8.2f}{100 * ds:>8.1f}%{100 * da:>10.1f}%{100 * dv:>14.1f}%"
              f"   dark stops on rays that miss: {wrong}")
    print(f"lit stops on rays that hit: {int(((today > 0) & hit & (earliest(first[0], first[1]) == today)).sum())}")
    print(f"(VALU: {VALU_PER_TRIP} wave-instructions a fast trip against {VALU_PER_LAUNCH / 1e6:.2f} M a launch; a trip on the split path costs more, so the change is at least this)")
    print("look-ups of the walk per candidate (whole layers up to the one that decides or the world's side; the kernel leaves a layer at its first open voxel):")
    for d in DEPTHS:
        print(f"  K_d = {d}: {V.walk_lookups(dense, split, lit_voxels, cell_dark, sun_t, d, liquid) / max(candidates, 1):.0f}")


if __name__ == "__main__":
    main()
