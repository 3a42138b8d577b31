"""The operand sets tests/test_gpu_math_values.py gives vrt_selftest_math_values, op family by op family: the smallest at which
each function can still go wrong.  Everything is a uint32 array of bit patterns, deterministic (a fixed generator per family), and
composed in WHOLE WAVES of 64 consecutive sets where the function chooses its form per wave.  tests/test_math_cases.py counts, on
the CPU and from tests/math_ref.py alone, that each set holds what it claims."""
import functools

import numpy as np

import math_ref as R

U32, F32 = np.uint32, np.float32
LO, HI = R.BAND_LO, R.BAND_HI
SPECIAL_LANES = (0, 31, 32, 63)
NAN, INF, FLT_MAX = 0x7FC00000, 0x7F800000, 0x7F7FFFFF
# what puts a lane outside the band, in one component: the band's outer neighbours, +-0, denormals, 2^31, 2^127, FLT_MAX, +inf, NaN
OUT_OF_BAND = (LO - 1, HI + 1, 0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x4F000000, 0x7F000000, FLT_MAX, INF, NAN)


def f32_bits(x):
    return int(np.array([x], dtype=F32).view(U32)[0])


def _rng(seed):
    return np.random.default_rng(seed)


def rand_fields(g, n, lo_field, hi_field, signed=True):
    """n floats with a random mantissa, an exponent field in [lo_field, hi_field] and (signed) a random sign"""
    b = g.integers(0, 1 << 23, n, dtype=np.uint64) | (g.integers(lo_field, hi_field + 1, n, dtype=np.uint64) << 23)
    if signed:
        b |= g.integers(0, 2, n, dtype=np.uint64) << 31
    return b.astype(U32)


def rand_in_band(g, n):
    return rand_fields(g, n, 97, 156)    # (field 156 is [2^29, 2^30); 2^30 itself is HI, placed by hand)


# ------------------------------------------------------------------------------------------------
# unit_steps / normalize_wave: three planes x, y, z
# ------------------------------------------------------------------------------------------------
# integer vectors whose dot product is a perfect square: (1,2,2) 9, (2,3,6) 49, (1,4,8) 81, (4,4,7) 81, (2,6,9) 121, (3,4,12) 169,
# (6,6,7) 121, (2,10,11) 225, (8,9,12) 289
QUADRUPLES = ((1, 2, 2), (2, 3, 6), (1, 4, 8), (4, 4, 7), (2, 6, 9), (3, 4, 12), (6, 6, 7), (2, 10, 11), (8, 9, 12))


@functools.lru_cache(maxsize=None)
def vectors():
    """-> (xyz [3, n] bit patterns, kind [n / 64] per wave: 'band', 'edge', 'square', 'out', 'zero')"""
    g = _rng(0xB0)
    waves, kinds = [], []

    def band_wave():
        return np.stack([rand_in_band(g, 64) for _ in range(3)])

    for _ in range(48):                   # wholly in band, random
        waves.append(band_wave()); kinds.append("band")
    for k in range(16):                   # wholly in band, components exactly at the two ends (either sign)
        w = band_wave()
        for lane in range(64):
            sign = U32(((lane >> 2) & 1) << 31)     # (component (lane / 4 + k) % 3, sign (lane / 4) % 2: all six within six lanes of four)
            if lane % 4 == 0: w[(lane // 4 + k) % 3, lane] = U32(LO) | sign
            if lane % 4 == 1: w[(lane // 4 + k) % 3, lane] = U32(HI) | sign
            if lane % 16 == 2: w[:, lane] = U32(LO) | sign
            if lane % 16 == 3: w[:, lane] = U32(HI) | sign
            if lane % 16 == 6: w[:, lane] = (U32(LO), U32(HI) | sign, U32(LO))
        waves.append(w); kinds.append("edge")
    # dot products that are perfect squares, and the vectors one ulp either side in x, at scales 2^-20 .. 2^20
    sq = []
    for (a, b, c) in QUADRUPLES:
        for e in range(-20, 21, 5):
            v = np.array([a, b, c], dtype=F32) * F32(2.0 ** e)
            vb = v.view(U32)
            for dx in (-1, 0, 1):
                for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
                    p = vb[list(perm)].copy()
                    p[0] = U32(int(p[0]) + dx)
                    sq.append(p)
    sq = np.array(sq, dtype=U32).T
    pad = (-sq.shape[1]) % 64
    sq = np.concatenate([sq, np.stack([rand_in_band(g, pad) for _ in range(3)])], axis=1)
    for k in range(sq.shape[1] // 64):
        waves.append(sq[:, 64 * k:64 * k + 64]); kinds.append("square")
    # exactly one lane out of band, in one component
    for i, special in enumerate(OUT_OF_BAND):
        for lane in SPECIAL_LANES:
            w = band_wave()
            w[(i + lane) % 3, lane] = U32(special)
            waves.append(w); kinds.append("out")
    for lane in SPECIAL_LANES:            # the zero vector (NaN out), and its negative
        w = band_wave()
        w[:, lane] = U32(0x80000000 if lane & 1 else 0)
        waves.append(w); kinds.append("zero")
    return np.concatenate(waves, axis=1), tuple(kinds)


# ------------------------------------------------------------------------------------------------
# sqrt_banded (one plane) and the lens ray's guarded form (whole waves)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sqrt_args():
    g = _rng(0xB1)
    fours = []
    for k in range(-48, 64):              # 4^k = 2^(2k): exponent field 127 + 2k in [31, 253]
        b = (127 + 2 * k) << 23
        fours += [b - 1, b, b + 1] if k > -48 else [b, b + 1]     # (below 2^-96 is outside the claimed range)
    return np.concatenate([rand_fields(g, 1 << 16, 31, 254, signed=False), np.array(fours + [31 << 23, FLT_MAX], dtype=U32)])


# what sends a wave of lens_sqrt_of to sqrtf: the lower neighbour of 1e-28f, zeros, a denormal, a negative number, NaN
LENS_SQRT_BELOW = (f32_bits(1.0e-28) - 1, 0x00000000, 0x80000000, 0x00000001, 0xBF800000, NAN)


@functools.lru_cache(maxsize=None)
def lens_sqrt_args():
    """-> (x [n], refined [n / 64] per wave as composed)"""
    g = _rng(0xB2)
    lo = f32_bits(1.0e-28)
    waves, refined = [], []
    for k in range(8):
        w = rand_fields(g, 64, (lo >> 23) + 1, 254, signed=False)
        w[k], w[8 + k], w[16 + k] = U32(lo), U32(INF), U32(FLT_MAX)
        waves.append(w); refined.append(True)
    for special in LENS_SQRT_BELOW:
        for lane in SPECIAL_LANES:
            w = rand_fields(g, 64, (lo >> 23) + 1, 254, signed=False)
            w[lane] = U32(special)
            w[(lane + 7) % 64], w[(lane + 9) % 64] = U32(INF), U32(lo)
            waves.append(w); refined.append(False)
    return np.concatenate(waves), tuple(refined)


# ------------------------------------------------------------------------------------------------
# div_refined (two planes) and the lens ray's guarded form (whole waves)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def div_args():
    g = _rng(0xB3)
    edges = list(DIV_EDGES) + [e | 0x80000000 for e in DIV_EDGES]
    nn = edges + [0x00000000, 0x80000000]
    n = np.array([a for a in nn for _ in edges], dtype=U32)
    d = np.array([b for _ in nn for b in edges], dtype=U32)
    # a band end against random operands, each way round
    r = 1 << 12
    ends = np.array([LO, HI, LO | 0x80000000, HI | 0x80000000], dtype=U32)[g.integers(0, 4, r)]
    n = np.concatenate([n, ends, rand_in_band(g, r), rand_in_band(g, 1 << 16)])
    d = np.concatenate([d, rand_in_band(g, r), ends, rand_in_band(g, 1 << 16)])
    return n, d


DIV_EDGES = (LO, LO + 1, HI - 1, HI, 0x3F800000, 0x3F800001, 0x3FFFFFFF)


@functools.lru_cache(maxsize=None)
def lens_div_args():
    """-> (n, d, refined [waves] as composed)"""
    g = _rng(0xB4)
    wn, wd, refined = [], [], []
    for k in range(8):                    # in range: zero numerators of either sign over either sign, the band's ends, random operands
        n, d = rand_in_band(g, 64), rand_in_band(g, 64)
        n[k], n[k + 8], n[k + 16], n[k + 24] = U32(0), U32(0), U32(LO), U32(HI)
        n[k + 48], n[k + 56] = U32(0x80000000), U32(0x80000000)
        d[k], d[k + 8], d[k + 48], d[k + 56] = d[k] & U32(0x7FFFFFFF), d[k + 8] | U32(0x80000000), d[k + 48] & U32(0x7FFFFFFF), d[k + 56] | U32(0x80000000)
        d[k + 16], d[k + 32], d[k + 40] = U32(HI), U32(LO), U32(HI | 0x80000000)
        wn.append(n); wd.append(d); refined.append(True)
    for i, special in enumerate(OUT_OF_BAND):
        for lane in SPECIAL_LANES:
            for which in ("n", "d"):
                if which == "n" and special in (0x00000000, 0x80000000):
                    continue              # (a zero numerator is in range: composed above)
                n, d = rand_in_band(g, 64), rand_in_band(g, 64)
                (n if which == "n" else d)[lane] = U32(special)
                n[(lane + 5) % 64] = U32(0)
                wn.append(n); wd.append(d); refined.append(False)
    return np.concatenate(wn), np.concatenate(wd), tuple(refined)


# ------------------------------------------------------------------------------------------------
# rng_next: states by their output word
# ------------------------------------------------------------------------------------------------
LCG_A, LCG_C, OUT_MUL, M32 = 747796405, 2891336453, 277803737, 0xFFFFFFFF


def state_before(state, draws=1):
    """the state from which `draws` draws lead to `state` (the LCG is invertible)"""
    inv = pow(LCG_A, -1, 1 << 32)
    for _ in range(draws):
        state = ((state - LCG_C) * inv) & M32
    return state


def state_yielding(word):
    """the state whose next rng_next has the output word `word`: every step of the output permutation inverted"""
    w = word ^ (word >> 22)                                   # r = (w >> 22) ^ w
    v = (w * pow(OUT_MUL, -1, 1 << 32)) & M32                 # w = v * 277803737
    k = (v >> 28) + 4                                         # v = (s >> k) ^ s, k = (s >> 28) + 4: s and v share their top 4 bits
    s = v
    for _ in range(8):
        s = v ^ (s >> k)
    return state_before(s)


# the states whose next draw has the output word 0, 0xFFFFFFFF .. 0xFFFFFF80 (the top 128 words: (float)r is 2^32, u == 1) and
# 0xFFFFFF7F (the first below: u < 1) — state_yielding of each, kept as constants; tests/test_math_cases.py proves what they yield
STATE_WORD_ZERO = 0x1ACE07EF
STATES_WORD_TOP = (
    0x8471B9D7, 0x4568AD8E, 0xA3FC34F1, 0xF1073194, 0xB6B9F799, 0x24FB5FB0, 0x2B0E1CE3, 0x67C50FB0,
    0xFDE3BCBF, 0xA26B7A40, 0x9C543F20, 0x754DDC24, 0x78B1791B, 0x7164CD3B, 0x891B3927, 0xAA4271A0,
    0x151EB3C3, 0x91CA9F3F, 0xFB41CB65, 0xC3E19B70, 0x4D0949E3, 0xC439BE71, 0x7C6983E9, 0x238C99D0,
    0x68E31AD5, 0x2E4A3697, 0xE002F8F0, 0x3905E880, 0xED10B925, 0x7E8D9F73, 0xFFFA4B4E, 0x7BC7789F,
    0x14F0F479, 0xA752B253, 0xB9E4D391, 0x33BCD7BE, 0xAC546D14, 0x547B1F7D, 0x85E5ACBB, 0x1ADE1304,
    0x2AEBD59B, 0x21585329, 0x39FE446C, 0x6AA59EF1, 0x5D2164BC, 0xCD918988, 0xEA777D1C, 0x086A4B73,
    0xCAE39F78, 0x6923EA5C, 0xEA71FE20, 0xAA3C18E5, 0x63B581EC, 0xCAB5B7E6, 0x382FFA3B, 0xDD51CC32,
    0xD9481FFF, 0x70041A3F, 0x1F60613B, 0x68900E8C, 0x1FAA4E61, 0x5E70345C, 0x55A0965F, 0xA0EF3361,
    0xAB6955B2, 0x05981491, 0xD1215A69, 0x32043108, 0x9CC81B4B, 0xA1F266C7, 0xB3C06FDF, 0x7D514286,
    0x2E152D67, 0xC0BC3480, 0x76BC05CA, 0x58EDD0E0, 0xB7081997, 0x34191459, 0xF867B1AE, 0x64F4E8B9,
    0xB00321E4, 0x4A073438, 0x172D276E, 0xF19D8496, 0x965E6E01, 0x2D7A852D, 0x7604A3D4, 0x3F7E7BF3,
    0x84708C5C, 0xFF80A22C, 0xE164D3C1, 0x06FD52A3, 0xC81B0C3D, 0x6E8D176F, 0xA64852EB, 0x89567CCC,
    0x4625D23B, 0xD7F3BCB6, 0xFF092B81, 0x0DFF977B, 0x4F1928F4, 0xBCE9CB20, 0x163D79DA, 0xE14E7C0E,
    0x8B077244, 0x15C0F36B, 0x64B534E5, 0xF5C8CEA1, 0x4041F7E2, 0x1274F47B, 0xD24AF104, 0x0399EB07,
    0x2B49A8F9, 0xF17B8748, 0x104D2A45, 0x864DB765, 0x944BEB76, 0x77E18FE7, 0x757CF518, 0x5C1273C6,
    0x6D811F69, 0x8FFA44CA, 0xBBC89BB4, 0x334B46A8, 0xB3FAF406, 0x35C187C8, 0x045E1A55, 0x803048B2)
STATE_WORD_BELOW_TOP = 0xBFE98117


@functools.lru_cache(maxsize=None)
def rng_states():
    g = _rng(0xB5)
    special = np.array((STATE_WORD_ZERO,) + STATES_WORD_TOP + (STATE_WORD_BELOW_TOP,), dtype=U32)
    return np.concatenate([special, g.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(U32)])


@functools.lru_cache(maxsize=None)
def rng_dir_states():
    """-> (states [n], special: a tuple of (wave, lane, draw, 'one' | 'zero')).  2^20 random states in whole waves, then waves of
    random states in which one lane's draw 1, 3 or 5 (the u2 of x, y, z) is exactly 1 — its square root's argument is -0 — or 0."""
    g = _rng(0xB6)
    n_random = 1 << 20
    waves, special = [g.integers(0, 1 << 32, n_random, dtype=np.uint64).astype(U32)], []
    wave = n_random // 64
    for kind, firsts in (("one", STATES_WORD_TOP[::37] + (STATES_WORD_TOP[-1],)), ("zero", (STATE_WORD_ZERO,))):
        for i, first in enumerate(firsts):
            for lane in SPECIAL_LANES:
                draw = (1, 3, 5)[(i + lane) % 3]
                w = g.integers(0, 1 << 32, 64, dtype=np.uint64).astype(U32)
                w[lane] = U32(state_before(first, draw))
                waves.append(w); special.append((wave, lane, draw, kind))
                wave += 1
    return np.concatenate(waves), tuple(special)


# ------------------------------------------------------------------------------------------------
# vlog, vcos2pi
# ------------------------------------------------------------------------------------------------
LOG_THRESHOLD = f32_bits(1.41421354)     # m > this: m is halved


@functools.lru_cache(maxsize=None)
def log_args():
    g = _rng(0xB7)
    parts = [np.arange(0x3F000000, 0x3F800000, dtype=U32)]                      # every mantissa of [0.5, 1)
    for field in range(93, 127):                                                # what a draw can be: 1e-10 .. 1
        parts.append((g.integers(0, 1 << 23, 4096, dtype=np.uint64) | (field << 23)).astype(U32))
    near = [f32_bits(1.0), f32_bits(1.0e-10)]
    for field in (93, 100, 120, 125, 126, 127):                                 # the threshold's four neighbours in several binades
        m = (LOG_THRESHOLD & 0x7FFFFF) | (field << 23)
        near += [m - 1, m, m + 1, m + 2]
    parts.append(np.array(near, dtype=U32))
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def cos_args():
    g = _rng(0xB8)
    _, uniforms = R.rng_next(g.integers(0, 1 << 32, 1 << 22, dtype=np.uint64).astype(U32))
    near = [0x00000000, f32_bits(1.0), 0x00800000, 0x00000001, 0x00400000]      # 0, 1, the smallest normal, two denormals
    for edge in (0.25, 0.5, 0.75, 1.0):
        e = f32_bits(edge)
        near += [e + k for k in range(-4, 5) if e + k <= f32_bits(1.0)]
    near += list(range(1, 5))                                                   # 0 + 4 ulp
    return np.concatenate([np.arange(0x3F000000, 0x3F800000, dtype=U32), uniforms, np.array(near, dtype=U32)])


# ------------------------------------------------------------------------------------------------
# the one-instruction helpers
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cvt_args():
    """trunc2i / flr2i: NaN, +-inf, +-2^31, +-(2^31 - 128), -0.0, -0.5, -1.0, -1.0 + ulp, around 2^23 and 2^24, random"""
    g = _rng(0xB9)
    v = [NAN, 0xFFC00000, 0x7FC00001, INF, INF | 0x80000000, 0x4F000000, 0xCF000000, 0x4EFFFFFF, 0xCEFFFFFF, 0x4F000001, 0xCF000001,
         0x80000000, 0x00000000, f32_bits(-0.5), f32_bits(0.5), f32_bits(-1.0), f32_bits(-1.0) - 1, f32_bits(-1.0) + 1, f32_bits(1.0) - 1,
         0x00000001, 0x80000001, FLT_MAX, FLT_MAX | 0x80000000, f32_bits(-0.001), f32_bits(255.999)]
    for p in (0x4B000000, 0x4B800000):    # 2^23, 2^24
        for k in range(-3, 4):
            v += [p + k, (p + k) | 0x80000000]
    return np.concatenate([np.array(v, dtype=U32), rand_fields(g, 1 << 14, 110, 160)])


@functools.lru_cache(maxsize=None)
def abs_mul_args():
    g = _rng(0xBA)
    v = [0x3FC00000, 0xBFC00000, 0x40490FDB, 0xC0490FDB, 0, 0x80000000, INF, INF | 0x80000000, NAN, 0xFFC00000, 0x00000001, 0x80000001, 0x007FFFFF,
         0x00800000, 0x3F800000, 0x7F7FFFFF, 0x33800000]
    a = np.array([x for x in v for _ in v], dtype=U32)
    b = np.array([y for _ in v for y in v], dtype=U32)
    r = 1 << 14
    return (np.concatenate([a, rand_fields(g, r, 100, 150), rand_fields(g, r, 1, 60)]),
            np.concatenate([b, rand_fields(g, r, 100, 150), rand_fields(g, r, 60, 130)]))


@functools.lru_cache(maxsize=None)
def min3_args():
    """min3_f32: quiet NaNs in every position (one, two, three), +-0 ties, infinities, random numbers"""
    g = _rng(0xBB)
    pool = [NAN, 0xFFC00000, 0, 0x80000000, 0x3F800000, 0xBF800000, 0x00000001, INF, INF | 0x80000000, 0x40000000]
    a = np.array([x for x in pool for _ in pool for _ in pool], dtype=U32)
    b = np.array([y for _ in pool for y in pool for _ in pool], dtype=U32)
    c = np.array([z for _ in pool for _ in pool for z in pool], dtype=U32)
    r = 1 << 14
    return tuple(np.concatenate([p, rand_fields(g, r, 90, 160)]) for p in (a, b, c))


@functools.lru_cache(maxsize=None)
def step_args():
    """row c': every pattern of zero / non-zero / NaN over the three axis distances (what abs_mul of a |unit step| makes: +0, a
    number above zero — a denormal, inf too — or a NaN of either sign), ties among the non-zero ones included"""
    g = _rng(0xBC)
    pool = [0, NAN, 0xFFC00000, 0x7FC00001, 0x00000001, 0x3F800000, 0x3F800001, 0x40000000, INF]
    a = np.array([x for x in pool for _ in pool for _ in pool], dtype=U32)
    b = np.array([y for _ in pool for y in pool for _ in pool], dtype=U32)
    c = np.array([z for _ in pool for _ in pool for z in pool], dtype=U32)
    r = 1 << 14
    rnd = [rand_fields(g, r, 90, 160, signed=False) for _ in range(3)]
    for p in rnd:                         # zeros and NaNs among random distances
        p[g.integers(0, r, r // 4)] = U32(0)
        p[g.integers(0, r, r // 16)] = U32(NAN)
    return tuple(np.concatenate([p, q]) for p, q in zip((a, b, c), rnd))


@functools.lru_cache(maxsize=None)
def word_args():
    """bfi / low_bits_of / or_and: all-ones, zero, 2^16 random words in each position"""
    g = _rng(0xBD)
    pool = [0, M32, 0x4B000000, 0xFF800003, 0xFFC0001F, 0x0000001F, 0x55555555, 0xAAAAAAAA]
    planes = [np.array([x for x in pool for _ in pool for _ in pool], dtype=U32), np.array([y for _ in pool for y in pool for _ in pool], dtype=U32),
              np.array([z for _ in pool for _ in pool for z in pool], dtype=U32)]
    return tuple(np.concatenate([p, g.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(U32)]) for p in planes)


# mad_i24 in the march: a is a voxel coordinate shifted down — flr2i(pos) >> 2 for the cell grid (vrt_march.h lookup), >> 3 and
# >> 5 for the direct cells (vrt_path_cells.h, vrt_path_sun.h) — so -1 (just beyond a low face) .. a few hundred; b is a wave-uniform
# byte stride: row_bytes = (grid_dim + 1) * 4 and slab_bytes = (grid_dim + 1) * row_bytes with grid_dim <= 800 (both < 2^23), or the
# direct cells' row / slab strides; c is the byte offset so far, an unsigned word
MARCH_GRID_DIMS = (8, 64, 200, 800)


@functools.lru_cache(maxsize=None)
def mad_args():
    """-> (a, b, c): whole waves; b is the wave's first set's (the other sets of a wave hold other values, which must not be read)"""
    g = _rng(0xBE)
    sa, sb, sc = [], [], []

    def wave(a, b, c):
        bb = g.integers(0, 1 << 32, 64, dtype=np.uint64).astype(U32)
        bb[0] = U32(b & M32)
        sa.append(np.asarray(a).astype(np.int64).astype(np.int32).view(U32)); sb.append(bb); sc.append(np.asarray(c, dtype=U32))

    ext = [-(1 << 23), (1 << 23) - 1, 0, 1, -1]
    for b in ext + [int(x) for x in g.integers(-(1 << 23), 1 << 23, 59)]:      # the whole signed 24-bit range, both factors
        a = g.integers(-(1 << 23), 1 << 23, 64)
        a[:5] = ext
        wave(a, b, g.integers(0, 1 << 32, 64, dtype=np.uint64).astype(U32))
    for dim in MARCH_GRID_DIMS:                                                 # what the march passes
        row = (dim + 1) * 4
        for b in (row, (dim + 1) * row):
            a = g.integers(-1, dim + 1, 64)
            a[:3] = (-1, 0, dim)
            wave(a, b, g.integers(0, (dim + 1) * row, 64, dtype=np.uint64).astype(U32))
    return np.concatenate(sa), np.concatenate(sb), np.concatenate(sc)
