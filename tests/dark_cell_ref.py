"""The dark rule of the sun marks (docs/NUMERICS.md "Dark stops"; vrt_lit.hip: accel_dark_kernel), stated in numpy, float64.

An all-air cell C of layer c_a is DARK when some k >= 1 (c_a + k inside the world, k <= depth) satisfies both:
  1. REACH_j(C) lies wholly inside the world for every j in 0 .. k — no ray of C can have left the world sideways before;
  2. the cells of REACH_k(C) share a closed voxel layer: every cell has a 4-bit floor mask, bit j set when its 16 voxels of voxel
     layer j across the sun's axis are all solid and no liquid (a full solid cell: all four; an air cell: none), and the masks of
     the cells of REACH_k(C) have a non-zero AND.
The plan, REACH, the widened cell and the allowance are the lit rule's (tests/lit_corridor_ref.py), whose helpers this file
imports.  Written from the text, not from the kernel: the world is mirrored so that the sun is "above", whole layers are tested
with summed-area tables.

    floor_masks(dense, axis, liquid)            [G, G, G] uint8 indexed [z, y, x]; liquid: bool[256]
    dark(lo, masks, sun, depth=None)            [G, G, G] uint8 like vrt_get_dark_marks' `dark`; lo: lit_corridor_ref.leaf_lo
    dark(..., transitive=True)                  cells of REACH_k that are themselves DARK do not count (layers decided from the sun's side)
"""
import numpy as np

import lit_corridor_ref as C


def floor_masks(dense, axis, liquid):
    """dense: u16 [n, n, n] = [z, y, x] voxel ids; axis: 0, 1, 2 = x, y, z; ids above 255 are material 255."""
    n = dense.shape[0]
    G = n // 4
    liquid = np.asarray(liquid, bool)
    blocks = (dense != 0) & ~liquid[np.minimum(dense, 255)]
    ax = 2 - axis                       # the array axis of the world axis
    r = blocks.reshape(G, 4, G, 4, G, 4)
    others = tuple(i for i in (1, 3, 5) if i != 2 * ax + 1)
    closed = np.moveaxis(r.all(axis=others), ax + 1, -1)   # [G, G, G, 4]: voxel layer j of the cell, j = coordinate & 3
    return (closed.astype(np.uint8) << np.arange(4, dtype=np.uint8)).sum(axis=-1).astype(np.uint8)


def _reach(c4, s_min, s_max, r_lo, r_hi, allow, G):
    """C._cells, and whether the interval lies wholly inside the world: [first, end) clipped, inside."""
    b_lo = c4 + np.where(s_min < 0, r_hi, r_lo) * s_min - allow
    b_hi = c4 + 4.0 + np.where(s_max > 0, r_hi, r_lo) * s_max + allow
    first, last = np.floor(b_lo / 4.0).astype(np.int64), np.floor(b_hi / 4.0).astype(np.int64)
    own = (c4 / 4.0).astype(np.int64)   # (monotone coordinates, as C._cells)
    first = np.where(s_min < 0, first, np.maximum(first, own))
    last = np.where(s_max > 0, last, np.minimum(last, own))
    clipped = C._cells(c4, s_min, s_max, r_lo, r_hi, allow, G)
    return clipped[0], clipped[1], (first >= 0) & (last <= G - 1)


def dark(lo, masks, sun, depth=None, transitive=False):
    G = lo.shape[0]
    W = 4 * G
    out = np.zeros((G, G, G), np.uint8)
    p = C.plan(W, sun)
    if p is None:
        return out
    a, up, _ = p
    u, v = (1 if a == 0 else 0), (1 if a == 2 else 2)
    sun = [float(np.float32(s)) for s in sun]
    order = (2 - a, 2 - v, 2 - u)   # array axes are [z, y, x]
    lo_t, m_t = np.transpose(lo, order), np.transpose(masks, order)
    sun_a = sun[a]
    if not up:   # mirror: the sun above
        lo_t, m_t = lo_t[::-1], m_t[::-1]
        sun_a = W - sun[a]
    air = lo_t >= 0
    depth = G if depth is None else max(0, min(int(depth), G))
    dark_t = np.zeros((G, G, G), bool)
    c4 = 4.0 * np.arange(G)
    for i in range(G - 1, -1, -1):   # from the sun's side: the layers above are decided
        d_lo, d_hi = sun_a - (4.0 * i + 5.0), sun_a - (4.0 * i - 1.0)
        us = C._slopes(sun[u] - (c4 + 5.0), sun[u] - (c4 - 1.0), d_lo, d_hi)
        vs = C._slopes(sun[v] - (c4 + 5.0), sun[v] - (c4 - 1.0), d_lo, d_hi)
        inside = np.ones((G, G), bool)
        found = np.zeros((G, G), bool)
        for k in range(0, min(depth, G - 1 - i) + 1):
            r_lo, r_hi, al = max(0.0, 4.0 * k - 5.0), 4.0 * k + 5.0, C.allowance(k, True)
            uf, ue, u_in = _reach(c4, us[0], us[1], r_lo, r_hi, al, G)
            vf, ve, v_in = _reach(c4, vs[0], vs[1], r_lo, r_hi, al, G)
            inside &= v_in[:, None] & u_in[None, :]
            if k == 0:
                continue
            m = m_t[i + k]
            if transitive:
                m = np.where(dark_t[i + k], 15, m)
            shared = np.zeros((G, G), bool)
            for j in range(4):
                shared |= C._count(C._sat(((m >> j) & 1) == 0), vf, ve, uf, ue) == 0
            found |= inside & shared
        dark_t[i] = found & air[i]
    if not up:
        dark_t = dark_t[::-1]
    out[...] = np.transpose(dark_t, np.argsort(order))
    return out
