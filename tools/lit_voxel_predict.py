"""tools/lit_voxel_predict.py [tiles] — what the voxel marks should take out of the headline frame, from the CPU oracle alone.

The bench's standing camera over the 8^3-chunk world at 1920 x 1080; `tiles` whole 8 x 8 tiles (default 2000) drawn with a fixed
seed.  The oracle gives every pixel's primary hit; the shadow ray from it is marched here, in numpy binary32 with the shader's own
step (the literal form, vrt_march.h march_literal), lookup by lookup over a dense copy of the world, and for every lookup the rule
of tests/lit_corridor_ref.py (today's marks) and of tests/lit_voxel_ref.py (K voxel layers) says whether the lane would stop
there.  A wave makes as many trips through its shadow loop as its slowest lane; the table is the sum over the tiles.

Prints the table that profiles/lit_voxels_ab.txt holds.  No GPU."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lit_corridor_ref as C   # noqa: E402
import lit_voxel_ref as R      # noqa: E402
import path_ref                # noqa: E402
from oracle import orc         # noqa: E402
from voxelraytracing_amd import scenes  # noqa: E402

F = np.float32
LAYERS = (4, 8, 16, 32)
VALU_PER_TRIP, VALU_PER_LAUNCH, TILES_PER_LAUNCH = 37, 57.0e6, 32400


def leaf_sizes(dense):
    """u8 [n, n, n]: the size of the octree leaf over every voxel (a canonical octree: an aligned uniform cube is one leaf)."""
    n = dense.shape[0]
    size = np.ones(dense.shape, np.uint8)
    s = 1
    while s < 32:
        s *= 2
        g = n // s
        c = dense.reshape(g, s, g, s, g, s)
        u = (c == c[:, :1, :, :1, :, :1]).all(axis=(1, 3, 5))
        size[np.repeat(np.repeat(np.repeat(u, s, 0), s, 1), s, 2)] = s
    return size


def march(dense, size, liquid, origin, sun, stops, max_steps=500):
    """Lookups per ray until it ends (hit, left the world, ran out), and per stop mask the lookup at which the ray first stands on
    a marked voxel (0: never); and whether the ray is occluded (it ended on a solid voxel, or ran out: march_literal's `hit`)."""
    n = dense.shape[0]
    N = len(origin)
    d = (sun[None, :] - origin).astype(F)
    d = (d / np.sqrt((d * d).sum(axis=1, dtype=F), dtype=F)[:, None]).astype(F)
    pos = origin.copy()
    frac = pos - np.floor(pos)
    nudge = (frac < F(0.001)).any(axis=1)
    pos[nudge] += F(0.001) * d[nudge]
    with np.errstate(all="ignore"):
        unit = np.stack([np.sqrt(F(1) + (d[:, (a + 1) % 3] / d[:, a]) ** 2 + (d[:, (a + 2) % 3] / d[:, a]) ** 2, dtype=F) for a in range(3)], axis=1).astype(F)
    up = d >= 0
    total = np.zeros(N, np.int32)
    first = [np.zeros(N, np.int32) for _ in stops]
    hit = np.zeros(N, bool)
    act = np.nonzero(((pos > 0) & (pos < n)).all(axis=1))[0]
    it = 0
    while len(act) and it < max_steps:
        it += 1
        p = pos[act]
        v = np.floor(p).astype(np.int64)
        vox = dense[v[:, 2], v[:, 1], v[:, 0]]
        total[act] = it
        liq = liquid[np.minimum(vox, 255)]
        for f, m in zip(first, stops):
            here = m[v[:, 2], v[:, 1], v[:, 0]] & (f[act] == 0)
            f[act[here]] = it
        go = (vox == 0) | liq
        hit[act[~go]] = True
        act, p, v = act[go], p[go], v[go]
        s = size[v[:, 2], v[:, 1], v[:, 0]].astype(np.int64)
        lo = v & ~(s[:, None] - 1)
        t = np.where(up[act], (lo + s[:, None]).astype(F) - p, p - lo.astype(F)).astype(F)
        ad = (t * unit[act]).astype(F)
        with np.errstate(all="ignore"):
            nz = np.where(ad == 0, F(np.inf), ad)
            step = np.nanmin(np.where(np.isnan(nz), F(np.inf), nz), axis=1).astype(F)
        zero = (ad == 0).all(axis=1)
        step[zero] = ad[zero, 2]
        add = np.where(ad == step[:, None], step[:, None] + F(0.001), step[:, None]).astype(F)
        p = (p + d[act] * add).astype(F)
        pos[act] = p
        inside = ((p >= 0) & (np.floor(p) < n)).all(axis=1)
        act = act[inside]
    hit[act] = True   # (still marching after max_steps lookups)
    return total, first, hit


def main():
    n_tiles = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    sc = scenes.c2((1920, 1080))
    o = orc.from_package_scene(sc)
    with tempfile.TemporaryDirectory() as tmp:   # (the library stays loaded; its file need not stay)
        dense = path_ref.load(tmp).dense_world(o)
    n = dense.shape[0]
    sun = np.array([F(F(sc.settings.sun_pos[a]) - F(float(o.c.world.min[a]))) for a in range(3)], F)
    sun_t = tuple(float(s) for s in sun)
    liquid = np.array([bool(sc.materials[i].is_liquid) for i in range(256)])
    lo = C.leaf_lo(dense)
    cell_lit = C.lit(lo, sun_t, n // 4).astype(bool)
    cells = np.repeat(np.repeat(np.repeat(cell_lit, 4, 0), 4, 1), 4, 2)
    split = R.split_cells(dense)
    stops = [cells] + [cells | R.lit_voxels(dense, split, cell_lit, sun_t, k).astype(bool) for k in LAYERS]
    plan = C.plan(n, sun_t)
    cell_trips = 500 - (6 * (n // (plan[2] + 1) + 1) + 2) - 1

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
    total, first, _ = march(dense, leaf_sizes(dense), liquid, origins, sun, stops)

    def wave_trips(f, limit):
        stop = np.where((f > 0) & (f <= limit), f, total)
        w = np.zeros(n_tiles, np.int64)
        np.maximum.at(w, lanes, stop)
        return w

    base = wave_trips(first[0], cell_trips)
    none = wave_trips(np.zeros_like(total), 0)
    print(f"{n_tiles} tiles of 8 x 8 (seed 20262) of the 1920 x 1080 frame, {len(lanes)} shadow rays; the cell marks stop a ray below {cell_trips} trips")
    print(f"primary wave trips {prim.sum()} ({prim.mean():.2f} a tile); shadow wave trips without marks {none.sum()} ({none.mean():.2f} a tile)")
    print(f"{'marks':<34}{'shadow trips':>13}{'a tile':>8}{'shadow':>9}{'all trips':>11}{'VALU / launch':>15}")
    print(f"{'today: cells':<34}{base.sum():>13}{base.mean():>8.2f}{'':>9}{'':>11}{'':>15}")
    for k, f in zip(LAYERS, first[1:]):
        for what, limit in ((f"+ voxels, K = {k}, budget {R.budget(k)}", cell_trips - R.budget(k)), (f"+ voxels, K = {k}, no budget", cell_trips)):
            if limit <= 0:
                print(f"{what:<34}{'the budget leaves no trips: no voxel marks':>56}")
                continue
            # (a voxel's mark stops a lane up to `limit`, a cell's up to cell_trips)
            stop_at = np.where((f > 0) & (f <= limit), f, np.where((first[0] > 0) & (first[0] <= cell_trips), first[0], 0))
            w = wave_trips(stop_at, cell_trips)
            ds = (w.sum() - base.sum()) / base.sum()
            da = (w.sum() - base.sum()) / (base.sum() + prim.sum())
            dv = (w.sum() - base.sum()) / n_tiles * TILES_PER_LAUNCH * VALU_PER_TRIP / VALU_PER_LAUNCH
            print(f"{what:<34}{w.sum():>13}{w.mean():>8.2f}{100 * ds:>8.1f}%{100 * da:>10.1f}%{100 * dv:>14.1f}%")
    print(f"(VALU: {VALU_PER_TRIP} wave-instructions a fast trip against {VALU_PER_LAUNCH / 1e6:.1f} M a launch; a trip on the split path costs more, so the change is at least this)")


if __name__ == "__main__":
    main()
