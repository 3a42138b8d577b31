"""The dark rule of the voxel marks (docs/NUMERICS.md "Dark stops", the voxels of split cells; vrt_lit.hip:
accel_dark_voxels_kernel), stated in numpy, float64, over a dense copy of the world.

An AIR voxel (id 0) of a SPLIT cell that is not lit is DARK when some k with 1 <= k <= `layers` satisfies both:
  1. REACH_j lies wholly inside the world for every j in 0 .. k — no ray of the voxel can have left the world sideways before layer k
     — and layer i_a + k is inside the world;
  2. every voxel of REACH_k is CLOSED: a solid voxel that is no liquid (ids above 255 are material 255; an air-leaf cell is air
     throughout, a solid leaf cell solid throughout), or a voxel inside a cell that carries the dark cell mark (tests/dark_cell_ref.py).
REACH is the lit voxel rule's (tests/lit_voxel_ref.py): the voxel widened by a voxel gives the slopes (lit_corridor_ref._slopes),
layer k towards the sun is reached after a rise of max(0, k - 2) .. k + 2 voxels, the allowance is lit_corridor_ref.allowance(k),
an interval is one-sided where no ray of the voxel points the other way, and the world is mirrored so that the sun is "above".
A ray with a point of its path in the voxel rises monotonely, so unless it ends before — a hit, or its lookups spent, which the
reference reports as a hit — it looks up a voxel of REACH_k: a solid one, or one of a cell all of whose rays hit.  No step budget:
every way the ray can end before layer k is a hit too.  Liquids on the way stop nothing, and close nothing.

    dark_voxels(dense, split, lit, cell_dark, sun, layers, liquid)
        dense [n, n, n] uint16 = [z, y, x]; split, cell_dark [G, G, G] bool; lit [n, n, n]: the lit voxel marks; liquid: bool[256]
        -> [n, n, n] uint8 indexed [z, y, x]: 1 for a dark air voxel of a split cell
    walk_lookups(the same)                      the voxel look-ups such a walk makes, whole layers counted (tools/dark_voxel_predict.py)

Written from the text, not from the kernel; the kernel computes its intervals in binary64 in this file's order.
"""
import numpy as np

import lit_corridor_ref as C
from lit_voxel_ref import _reach

DARK_VOXEL = 0x7FFE   # the id the shadow pool holds for a dark air voxel: a solid voxel of material 255, one below the lit mark's


def dark_voxels(dense, split, lit, cell_dark, sun, layers, liquid):
    return _walk(dense, split, lit, cell_dark, sun, layers, liquid)[0]


def walk_lookups(dense, split, lit, cell_dark, sun, layers, liquid):
    """The voxels of REACH_1 .. REACH_k summed over the candidates, k: the layer that decides, the last inside the world, or `layers`."""
    return _walk(dense, split, lit, cell_dark, sun, layers, liquid)[1]


def _walk(dense, split, lit, cell_dark, sun, layers, liquid):
    n = dense.shape[0]
    out = np.zeros((n, n, n), np.uint8)
    looked = 0
    p = C.plan(n, sun)
    if p is None or layers < 1:
        return out, looked
    a, up, _ = p
    u, v = (1 if a == 0 else 0), (1 if a == 2 else 2)
    sun = [float(np.float32(s)) for s in sun]
    order = (2 - a, 2 - v, 2 - u)   # array axes are [z, y, x]
    rep = lambda m: np.repeat(np.repeat(np.repeat(m, 4, 0), 4, 1), 4, 2)
    liquid = np.asarray(liquid, bool)
    solid = (dense != 0) & ~liquid[np.minimum(dense, 255)]
    closed = np.transpose(solid | rep(np.asarray(cell_dark, bool)), order)
    cand = np.transpose(rep(np.asarray(split, bool)) & (dense == 0) & ~np.asarray(lit, bool), order)
    sun_a = sun[a]
    if not up:   # mirror: the sun above
        closed, cand = closed[::-1], cand[::-1]
        sun_a = n - sun[a]
    ia, iv, iu = [x.astype(np.float64) for x in np.nonzero(cand)]
    d_lo, d_hi = sun_a - (ia + 2.0), sun_a - (ia - 1.0)
    us = C._slopes(sun[u] - (iu + 2.0), sun[u] - (iu - 1.0), d_lo, d_hi)
    vs = C._slopes(sun[v] - (iv + 2.0), sun[v] - (iv - 1.0), d_lo, d_hi)
    la0, lv0, lu0 = ia.astype(np.int64), iv.astype(np.int64), iu.astype(np.int64)
    inside = np.ones(ia.shape, bool)   # REACH_0 .. REACH_k inside the world
    dark = np.zeros(ia.shape, bool)
    for k in range(layers + 1):
        al = C.allowance(k, True)
        r_lo, r_hi = max(0.0, k - 2.0), k + 2.0
        uf, ul = _reach(iu, us[0], us[1], r_lo, r_hi, al)
        vf, vl = _reach(iv, vs[0], vs[1], r_lo, r_hi, al)
        la = la0 + k
        inside &= (la < n) & (uf >= 0) & (ul < n) & (vf >= 0) & (vl < n)
        if k == 0:
            continue
        todo = inside & ~dark
        shut = todo.copy()
        looked += int(((vl - vf + 1) * (ul - uf + 1))[todo].sum())
        for dv in range(int((vl - vf)[todo].max(initial=-1)) + 1):
            for du in range(int((ul - uf)[todo].max(initial=-1)) + 1):
                m = todo & (vf + dv <= vl) & (uf + du <= ul)
                shut[m] &= closed[la[m], (vf + dv)[m], (uf + du)[m]]
        dark |= shut
    res = np.zeros(cand.shape, bool)
    res[la0[dark], lv0[dark], lu0[dark]] = True
    if not up:
        res = res[::-1]
    out[...] = np.transpose(res, np.argsort(order))
    return out, looked
