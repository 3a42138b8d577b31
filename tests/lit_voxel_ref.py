"""The lit rule of the voxel marks (docs/NUMERICS.md "Lit stops", the voxels of split cells; vrt_lit.hip:
accel_lit_voxels_kernel), stated in numpy over a dense copy of the world.

An AIR voxel (id 0) of a SPLIT cell is lit when every shadow ray with a point of its path in the voxel meets only air voxels
until its path is inside cells that carry the cell-level lit mark (tests/lit_corridor_ref.py), whose proof takes over from
there.  It is the cell rule with a cell of ONE voxel: the voxel widened by a voxel gives the slopes, layer k towards the sun is
reached after a rise of max(0, k - 2) .. k + 2 voxels, the allowance is the cell rule's (a voxel layer has fewer faces than a
cell layer), an interval is one-sided where no ray of the voxel points the other way.  Layer 0 is the voxel's own: a ray crosses
into its neighbours there before it has risen a voxel.

    walk, for k = 0, 1, ... `layers`:
        a voxel of REACH_k beyond the world on any axis        -> unlit  (the world's border)
        a voxel of REACH_k that is not air                     -> unlit  (an air-leaf cell is air throughout)
        every voxel of REACH_k in a cell with the lit mark     -> lit
    no verdict after layer `layers`                            -> unlit

    split_cells(dense)                                   [G, G, G] bool: cells that are not one leaf (canonical octrees)
    lit_voxels(dense, split, cell_lit, sun, layers, margins=True, extra=0.0)
                                                         [n, n, n] uint8 indexed [z, y, x]: 1 for a lit air voxel of a split cell
    budget(layers)                                       lookups a ray may spend between a lit voxel and the lit cells

`extra` widens (or, negative, narrows) every allowance: the lit set shrinks as the allowance grows, which is how the GPU test
brackets a binary32 kernel between two float64 statements.  Written from the text, not from the kernel.
"""
import numpy as np

import lit_corridor_ref as C

LIT_VOXEL = 0x7FFF   # the id the shadow pool holds for a lit air voxel: the highest a brick's 16-bit entry (voxel << 1 | lo) can carry


def budget(layers):
    """Planes of voxels a ray crosses from a lit voxel to the first lit cell, at most `layers` voxel layers further: `layers` + 1
    on the sun's axis, and on each other axis what a slope below 1 over a rise of at most `layers` + 2 crosses, plus one: three a
    layer, plus six in all (the issue's "plus three", and one more per axis for the widened voxel); and one re-step per plane
    (docs/NUMERICS.md, the step budget)."""
    return 2 * (3 * layers + 6)


def split_cells(dense):
    n = dense.shape[0]
    G = n // 4
    c = dense.reshape(G, 4, G, 4, G, 4)
    first = c[:, :1, :, :1, :, :1]
    return ~(c == first).all(axis=(1, 3, 5))


def _reach(i, s_min, s_max, r_lo, r_hi, allow):
    b_lo = i + np.where(s_min < 0, r_hi, r_lo) * s_min - allow
    b_hi = i + 1.0 + np.where(s_max > 0, r_hi, r_lo) * s_max + allow
    first, last = np.floor(b_lo).astype(np.int64), np.floor(b_hi).astype(np.int64)
    own = i.astype(np.int64)
    first = np.where(s_min < 0, first, np.maximum(first, own))
    last = np.where(s_max > 0, last, np.minimum(last, own))
    return first, last


def lit_voxels(dense, split, cell_lit, sun, layers, margins=True, extra=0.0):
    n = dense.shape[0]
    out = np.zeros((n, n, n), np.uint8)
    p = C.plan(n, sun)
    if p is None or layers < 1:
        return out
    a, up, _ = p
    u, v = (1 if a == 0 else 0), (1 if a == 2 else 2)
    sun = [float(np.float32(s)) for s in sun]
    order = (2 - a, 2 - v, 2 - u)   # array axes are [z, y, x]
    rep = lambda m: np.repeat(np.repeat(np.repeat(m, 4, 0), 4, 1), 4, 2)
    air = np.transpose(dense == 0, order)
    in_lit = np.transpose(rep(cell_lit.astype(bool)), order)
    cand = np.transpose(rep(split.astype(bool)), order) & air
    sun_a = sun[a]
    if not up:   # mirror: the sun above
        air, in_lit, cand = air[::-1], in_lit[::-1], cand[::-1]
        sun_a = n - sun[a]
    ia, iv, iu = [x.astype(np.float64) for x in np.nonzero(cand)]
    d_lo, d_hi = sun_a - (ia + 2.0), sun_a - (ia - 1.0)
    us = C._slopes(sun[u] - (iu + 2.0), sun[u] - (iu - 1.0), d_lo, d_hi)
    vs = C._slopes(sun[v] - (iv + 2.0), sun[v] - (iv - 1.0), d_lo, d_hi)
    la0, lv0, lu0 = ia.astype(np.int64), iv.astype(np.int64), iu.astype(np.int64)
    open_ = np.ones(ia.shape, bool)    # no verdict yet
    lit = np.zeros(ia.shape, bool)
    for k in range(layers + 1):
        al = C.allowance(k, margins) + (extra if margins else 0.0)
        r_lo, r_hi = max(0.0, k - 2.0), k + 2.0
        uf, ul = _reach(iu, us[0], us[1], r_lo, r_hi, al)
        vf, vl = _reach(iv, vs[0], vs[1], r_lo, r_hi, al)
        la = la0 + k
        inside = (la < n) & (uf >= 0) & (ul < n) & (vf >= 0) & (vl < n)
        open_ &= inside                                   # the world's border: unlit
        all_air, all_lit = open_.copy(), open_.copy()
        for dv in range(int((vl - vf)[open_].max(initial=-1)) + 1):
            for du in range(int((ul - uf)[open_].max(initial=-1)) + 1):
                m = open_ & (vf + dv <= vl) & (uf + du <= ul)
                at = (la[m], (vf + dv)[m], (uf + du)[m])
                own = (k == 0) & (at[1] == lv0[m]) & (at[2] == lu0[m])   # the voxel itself: air, in a split cell
                all_air[m] &= air[at]
                all_lit[m] &= in_lit[at] & ~own
        open_ &= all_air
        done = open_ & all_lit
        lit |= done
        open_ &= ~done
    res = np.zeros(cand.shape, bool)
    res[la0[lit], lv0[lit], lu0[lit]] = True
    if not up:
        res = res[::-1]
    out[...] = np.transpose(res, np.argsort(order))
    return out
