"""The lit rule of the sun marks (docs/NUMERICS.md "Lit stops"; vrt_lit.hip: accel_lit_kernel), stated in numpy.

A cell of the grid (4^3 voxels) is LIT when every shadow ray with a position in it leaves the world through air.  The rule tests,
layer by layer towards the sun, the cells such a ray can be in — REACH_k(C), from the smallest and largest slope of a line to the
sun through the cell widened by a voxel, times the rise to layer c_a + k — over a slab of `depth` layers, and behind the slab the
marks of the cells the ray can enter the next layer in.  This file is written from the text, not from the kernel: it mirrors the
world so that the sun is always "above", works on whole layers with summed-area tables, and computes in float64.

    plan(world_size, sun)                 (axis, up, min_lo) or None — vrt_lit.hip: lit_plan
    leaf_lo(dense)                        [G, G, G] int: leaf size - 1 of every all-air cell, -1 for any other (canonical octrees)
    lit(lo, sun, depth, margins=True)     [G, G, G] uint8, indexed [z, y, x] like vrt_get_sun_marks' `lit`

margins=False drops every allowance (nudges, roundings, the kernel's binary32 slack): the geometric rule alone, which no
implementation with margins may light more than.
"""
import numpy as np


def plan(world_size, sun):
    F = np.float32
    sun = [F(s) for s in sun]
    if not all(np.isfinite(s) for s in sun):
        return None
    lo, hi = F(-1.0), F(world_size) + F(1.0)
    best, axis, up = F(0.0), 0, False
    for a in range(3):
        for u in (0, 1):
            clear = sun[a] - hi if u else lo - sun[a]
            if clear > best:
                best, axis, up = clear, a, bool(u)
    if not best > 0:
        return None
    for b in range(3):
        if b != axis and not max(abs(sun[b] - lo), abs(sun[b] - hi)) <= F(0.99) * best:
            return None
    L = 4
    while L <= 32:
        if 6 * (world_size // L + 1) + 2 + 2 <= 500:
            return axis, up, L - 1
        L *= 2
    return None


def leaf_lo(dense):
    """dense: u16 [n, n, n] = [z, y, x] voxel ids (path_ref's dense_world).  An aligned all-air cube of 4, 8, 16 or 32 voxels is a
    leaf of at least that size in a canonical octree (a chunk is 32 voxels: no leaf is larger)."""
    n = dense.shape[0]
    G = n // 4
    air = (dense == 0).reshape(G, 4, G, 4, G, 4).all(axis=(1, 3, 5))
    lo = np.where(air, 3, -1).astype(np.int32)
    size, full = 1, air
    while size < 8:   # 2, 4, 8 cells a side
        g = full.shape[0] // 2
        full = full.reshape(g, 2, g, 2, g, 2).all(axis=(1, 3, 5))
        size *= 2
        big = np.repeat(np.repeat(np.repeat(full, size, 0), size, 1), size, 2)
        lo[big] = 4 * size - 1
    return lo


def allowance(k, margins):
    return (min(0.015 * (k + 1), 1.0) + 0.01) if margins else 0.0


def _slopes(n_lo, n_hi, d_lo, d_hi):
    return n_lo / np.where(n_lo < 0, d_lo, d_hi), n_hi / np.where(n_hi > 0, d_lo, d_hi)


def _cells(c4, s_min, s_max, r_lo, r_hi, allow, G):
    """[first, last + 1) of the cells overlapping the interval, clipped to the world (empty: first == last + 1)."""
    b_lo = c4 + np.where(s_min < 0, r_hi, r_lo) * s_min - allow
    b_hi = c4 + 4.0 + np.where(s_max > 0, r_hi, r_lo) * s_max + allow
    first, last = np.floor(b_lo / 4.0).astype(np.int64), np.floor(b_hi / 4.0).astype(np.int64)
    own = (c4 / 4.0).astype(np.int64)   # a ray's coordinates are monotone: not below its cell unless some ray of the cell points there
    first = np.where(s_min < 0, first, np.maximum(first, own))
    last = np.where(s_max > 0, last, np.minimum(last, own))
    first, end = np.clip(first, 0, G), np.clip(last + 1, 0, G)
    return first, np.maximum(end, first)


def _sat(bad):
    P = np.zeros((bad.shape[0] + 1, bad.shape[1] + 1), np.int64)
    P[1:, 1:] = bad.astype(np.int64).cumsum(0).cumsum(1)
    return P


def _count(P, vf, ve, uf, ue):
    vf, ve, uf, ue = vf[:, None], ve[:, None], uf[None, :], ue[None, :]
    return P[ve, ue] - P[vf, ue] - P[ve, uf] + P[vf, uf]


def lit(lo, sun, depth, margins=True):
    G = lo.shape[0]
    W = 4 * G
    p = plan(W, sun)
    out = np.zeros((G, G, G), np.uint8)
    if p is None:
        return out
    a, up, min_lo = p
    u, v = (1 if a == 0 else 0), (1 if a == 2 else 2)
    sun = [float(np.float32(s)) for s in sun]
    order = (2 - a, 2 - v, 2 - u)   # array axes are [z, y, x]
    lo_t = np.transpose(lo, order)
    sun_a = sun[a]
    if not up:   # mirror: the sun above
        lo_t = lo_t[::-1]
        sun_a = W - sun[a]
    ok = lo_t >= min_lo
    sats = [_sat(~ok[i]) for i in range(G)]
    lit_t = np.zeros((G, G, G), bool)
    c4 = 4.0 * np.arange(G)
    depth = max(1, min(int(depth), G))
    hi = G - 1
    while hi >= 0:
        behind = _sat(~lit_t[hi + 1]) if hi + 1 < G else None
        for i in range(hi, max(hi - depth, -1), -1):
            m = hi - i + 1
            d_lo, d_hi = sun_a - (4.0 * i + 5.0), sun_a - (4.0 * i - 1.0)
            us = _slopes(sun[u] - (c4 + 5.0), sun[u] - (c4 - 1.0), d_lo, d_hi)
            vs = _slopes(sun[v] - (c4 + 5.0), sun[v] - (c4 - 1.0), d_lo, d_hi)
            good = ok[i].copy()
            for k in range(m):
                r_lo, r_hi, al = max(0.0, 4.0 * k - 5.0), 4.0 * k + 5.0, allowance(k, margins)
                uf, ue = _cells(c4, us[0], us[1], r_lo, r_hi, al, G)
                vf, ve = _cells(c4, vs[0], vs[1], r_lo, r_hi, al, G)
                good &= _count(sats[i + k], vf, ve, uf, ue) == 0
            if behind is not None:
                r_lo, r_hi, al = max(0.0, 4.0 * m - 5.0), 4.0 * m + 1.0 + (0.01 if margins else 0.0), allowance(m, margins)
                uf, ue = _cells(c4, us[0], us[1], r_lo, r_hi, al, G)
                vf, ve = _cells(c4, vs[0], vs[1], r_lo, r_hi, al, G)
                good &= _count(behind, vf, ve, uf, ue) == 0
            lit_t[i] = good
        hi -= depth
    if not up:
        lit_t = lit_t[::-1]
    out[...] = np.transpose(lit_t, np.argsort(order))
    return out
