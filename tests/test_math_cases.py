"""tests/math_cases.py holds what it claims: counted on the CPU, from the predicates and functions of tests/math_ref.py alone.  A case
set that lost its edges — a wave meant to run the refined form that holds a stray operand outside the band, a state that no longer
draws u2 == 1 — would let tests/test_gpu_math_values.py pass while looking at nothing."""
import numpy as np

import math_cases as K
import math_ref as R

U32, F32 = np.uint32, np.float32


def _has(arr, *patterns):
    return all(bool((np.asarray(arr, dtype=U32) == U32(p)).any()) for p in patterns)


def test_python_names_the_ops_as_the_header_numbers_them():
    import os
    import re
    from voxelraytracing_amd import graphics
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vrt.h")).read()
    defined = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define VRT_MATH_(\w+) (\d+)u\n", hdr)}
    assert defined.pop("ops") == len(graphics.MATH_OPS) == len(defined)
    assert defined == {name: op for name, (op, _, _) in graphics.MATH_OPS.items()}


def test_vectors_hold_refined_and_general_waves_where_they_say():
    xyz, kinds = K.vectors()
    assert xyz.shape[1] == 64 * len(kinds)
    inb = R.in_band(xyz).all(axis=0)
    refined = R.wave_all(inb).reshape(-1, 64)
    assert (refined.all(axis=1) | ~refined.any(axis=1)).all()
    refined = refined[:, 0]
    kinds = np.array(kinds)
    assert refined[np.isin(kinds, ("band", "edge", "square"))].all() and not refined[np.isin(kinds, ("out", "zero"))].any()
    assert refined.mean() >= 0.25, "at least a quarter of the waves run the refined form"
    per_wave = xyz.reshape(3, -1, 64)
    # an 'out' wave: exactly one lane outside the band, in exactly one component, at lane 0, 31, 32 or 63 — every special value at every lane
    seen = set()
    for w in np.flatnonzero(kinds == "out"):
        outside = ~R.in_band(per_wave[:, w, :])
        assert outside.sum() == 1
        comp, lane = (int(v[0]) for v in np.nonzero(outside))
        seen.add((int(per_wave[comp, w, lane]), lane))
    assert seen == {(s, lane) for s in K.OUT_OF_BAND for lane in K.SPECIAL_LANES}
    for w in np.flatnonzero(kinds == "zero"):
        zero = ((per_wave[:, w, :] & U32(0x7FFFFFFF)) == 0).all(axis=0)
        assert zero.sum() == 1 and int(np.flatnonzero(zero)[0]) in K.SPECIAL_LANES
    zero_sets = ((xyz & U32(0x7FFFFFFF)) == 0).all(axis=0)
    assert all(R.is_nan(p)[zero_sets].all() for p in R.normalize(*xyz)[:3])
    # the band's two ends, either sign, in every component, inside refined waves
    edge = per_wave[:, kinds == "edge", :]
    for comp in range(3):
        assert _has(edge[comp], K.LO, K.HI, K.LO | 0x80000000, K.HI | 0x80000000)
    assert ((edge == U32(K.HI)).all(axis=0)).any() and ((edge == U32(K.LO)).all(axis=0)).any()
    # perfect squares: dot products whose root is exact, with a neighbour either side
    sq = R.flt(per_wave[:, kinds == "square", :].reshape(3, -1)).astype(np.float64)
    root = np.sqrt((sq * sq).sum(axis=0))
    exact = root == np.round(root * 2.0 ** 20) / 2.0 ** 20
    assert exact.sum() >= len(K.QUADRUPLES) * 9 * 3 and (~exact).sum() >= 2 * len(K.QUADRUPLES) * 9 * 3


def test_square_root_arguments():
    x = K.sqrt_args()
    f = x >> U32(23)
    assert f.min() == 31 and f.max() == 254 and not (x >> U32(31)).any()
    assert set(range(31, 255)) <= set(f.tolist())
    for k in range(-48, 64):
        b = (127 + 2 * k) << 23
        assert _has(x, b, b + 1) and (k == -48 or _has(x, b - 1)), k
    assert _has(x, 31 << 23, K.FLT_MAX) and R.flt(np.array([31 << 23], dtype=U32))[0] == F32(2.0 ** -96)
    x, refined = K.lens_sqrt_args()
    flags = R.lens_sqrt(x)[1].reshape(-1, 64)
    assert (flags == np.array(refined, dtype=U32)[:, None]).all() and 0 < sum(refined) < len(refined)
    lo = K.f32_bits(1.0e-28)
    in_refined = x.reshape(-1, 64)[np.array(refined)]
    assert _has(in_refined, K.INF, lo, K.FLT_MAX)
    general = x.reshape(-1, 64)[~np.array(refined)]
    below = ~(R.flt(general) >= R.SQRT_BAND_LO)
    assert (below.sum(axis=1) == 1).all()
    assert {(int(general[w, l]), int(l)) for w, l in zip(*np.nonzero(below))} == {(s, lane) for s in K.LENS_SQRT_BELOW for lane in K.SPECIAL_LANES}
    assert _has(general, K.INF, lo)


def test_division_operands():
    n, d = K.div_args()
    assert R.in_band(d).all() and (R.in_band(n) | ((n & U32(0x7FFFFFFF)) == 0)).all()
    for end_n in (K.LO, K.HI, K.LO | 0x80000000, K.HI | 0x80000000, 0, 0x80000000):
        for end_d in (K.LO, K.HI, K.LO | 0x80000000, K.HI | 0x80000000):
            assert ((n == U32(end_n)) & (d == U32(end_d))).any(), (hex(end_n), hex(end_d))
    n, d, refined = K.lens_div_args()
    flags = R.lens_div(n, d)[1].reshape(-1, 64)
    refined = np.array(refined)
    assert (flags == refined.astype(U32)[:, None]).all() and refined.any()
    nw, dw = n.reshape(-1, 64), d.reshape(-1, 64)
    for zero in (0, 0x80000000):          # either zero over either sign, in refined waves
        for sign in (0, 1):
            assert ((nw[refined] == U32(zero)) & (dw[refined] >> U32(31) == sign)).any(), (zero, sign)
    assert _has(nw[refined], K.LO, K.HI) and _has(dw[refined], K.LO, K.HI, K.HI | 0x80000000)
    bad_n = ~(R.in_band(nw) | ((nw & U32(0x7FFFFFFF)) == 0))[~refined]
    bad_d = ~R.in_band(dw)[~refined]
    assert ((bad_n.sum(axis=1) + bad_d.sum(axis=1)) == 1).all()
    got_n = {(int(nw[~refined][w, l]), int(l)) for w, l in zip(*np.nonzero(bad_n))}
    got_d = {(int(dw[~refined][w, l]), int(l)) for w, l in zip(*np.nonzero(bad_d))}
    assert got_d == {(s, lane) for s in K.OUT_OF_BAND for lane in K.SPECIAL_LANES}
    assert got_n == {(s, lane) for s in K.OUT_OF_BAND if s & 0x7FFFFFFF for lane in K.SPECIAL_LANES}
    assert (nw[~refined] == 0).any(axis=1).all()      # a numerator of +0 beside the lane that is outside


def test_rng_states_yield_the_words_they_are_kept_for():
    def word(state):   # rng_next's output word, path_tracer.wgsl:56-60, in Python integers
        s = (state * K.LCG_A + K.LCG_C) & K.M32
        r = (((s >> ((s >> 28) + 4)) ^ s) * K.OUT_MUL) & K.M32
        return (r >> 22) ^ r
    assert word(K.STATE_WORD_ZERO) == 0 and word(K.STATE_WORD_BELOW_TOP) == 0xFFFFFF7F
    assert [word(s) for s in K.STATES_WORD_TOP] == [0xFFFFFFFF - i for i in range(128)]
    for w in (0, 1, 0xFFFFFFFF, 0x80000000, 0xDEADBEEF):
        assert word(K.state_yielding(w)) == w
    # ... and, through the oracle: the top 128 words are u == 1 exactly, the next one is below 1, word 0 is u == 0
    one = K.f32_bits(1.0)
    s = np.array((K.STATE_WORD_ZERO, K.STATE_WORD_BELOW_TOP) + K.STATES_WORD_TOP, dtype=U32)
    u = R.rng_next(s)[1]
    assert u[0] == 0 and u[1] == one - 1 and (u[2:] == one).all()
    assert R.rng_next_u2(s)[1][0] == K.f32_bits(1.0e-10)
    states = K.rng_states()
    assert states.size >= 1 << 20 and np.isin(s, states).all()


def test_direction_states_draw_the_ones_and_zeros_they_say():
    states, special = K.rng_dir_states()
    assert states.size % 64 == 0 and states.size >= (1 << 20) + 64 * len(special)
    assert {(lane, kind) for _, lane, _, kind in special} == {(lane, kind) for lane in K.SPECIAL_LANES for kind in ("one", "zero")}
    assert {draw for _, _, draw, _ in special} == {1, 3, 5}
    picked = np.array([64 * w + lane for w, lane, _, _ in special])
    s = states[picked]
    for j in range(6):
        s, u = R.rng_next(s)
        for i, (_, _, draw, kind) in enumerate(special):
            if draw == j:
                assert u[i] == (K.f32_bits(1.0) if kind == "one" else 0), (i, j)
    # a u2 of exactly 1 makes the square root's argument -0: its wave takes sqrtf and the general normalisation, the lane's component is 0
    _, dx, dy, dz, flags = R.rng_dir(states)
    d = np.stack([dx, dy, dz])
    for w, lane, draw, kind in special:
        if kind == "one":
            assert (flags[64 * w:64 * w + 64] == 0).all() and (d[draw // 2, 64 * w + lane] & U32(0x7FFFFFFF)) == 0
        else:
            assert not R.is_nan(d[:, 64 * w + lane]).any()
    assert (flags[:1 << 20] == 3).mean() > 0.9, "ordinary waves take both refined forms"


def test_log_and_cos_arguments():
    x = K.log_args()
    assert np.array_equal(x[:1 << 23], np.arange(0x3F000000, 0x3F800000, dtype=U32))
    fields = (x[1 << 23:] >> U32(23)).astype(np.int64)
    assert all((fields == f).sum() >= 4096 for f in range(93, 127))
    assert _has(x, K.f32_bits(1.0), K.f32_bits(1.0e-10))
    assert (x >= U32(0x00800000)).all() and (x < U32(0x7F800000)).all()        # normal, positive: vlog's domain
    t = K.LOG_THRESHOLD & 0x7FFFFF
    for field in (93, 126, 127):
        assert _has(x, *[((field << 23) | t) + k for k in (-1, 0, 1, 2)])
    mant = R.flt((x & U32(0x7FFFFF)) | U32(0x3F800000))
    assert (mant > F32(1.41421354)).any() and (mant <= F32(1.41421354)).any()
    u = K.cos_args()
    assert np.array_equal(u[:1 << 23], np.arange(0x3F000000, 0x3F800000, dtype=U32)) and u.size >= (1 << 23) + (1 << 22)
    assert (R.flt(u) >= 0).all() and (R.flt(u) <= 1).all()
    for edge in (0.25, 0.5, 0.75):
        assert _has(u, *[K.f32_bits(edge) + k for k in range(-4, 5)])
    assert _has(u, 0, 1, 4, K.f32_bits(1.0), K.f32_bits(1.0) - 4, 0x00800000, 0x00400000)
    quadrant = np.floor(R.flt(u) * F32(4.0)).astype(np.int64)
    assert set(quadrant.tolist()) == {0, 1, 2, 3, 4}


def test_helper_operands():
    x = K.cvt_args()
    f = lambda v: K.f32_bits(v)                                                # noqa: E731
    assert _has(x, K.NAN, K.INF, K.INF | 0x80000000, f(2.0 ** 31), f(-2.0 ** 31), f(2.0 ** 31 - 128), f(-(2.0 ** 31 - 128)), 0x80000000,
                f(-0.5), f(-1.0), f(-1.0) - 1, f(2.0 ** 23), f(2.0 ** 23) + 1, f(2.0 ** 23) - 1, f(2.0 ** 24), f(2.0 ** 24) + 1, f(2.0 ** 24) - 1)
    assert (R.trunc2i(x) != R.flr2i(x)).sum() > 1000          # negative non-integers and NaN: where the two conversions part
    a, b = K.abs_mul_args()
    sign = lambda v: (v >> U32(31)).astype(int)                                # noqa: E731
    finite = ~R.is_nan(a) & ~R.is_nan(b)
    assert {(sa, sb) for sa, sb in zip(sign(a[finite])[:289].tolist(), sign(b[finite])[:289].tolist())} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert (R.is_nan(a) | R.is_nan(b)).any() and ((a == U32(K.INF)) & (b == 0)).any() and ((a == 0) & (b == U32(K.INF))).any()
    denormal = lambda v: ((v & U32(0x7F800000)) == 0) & ((v & U32(0x7FFFFF)) != 0)    # noqa: E731
    assert denormal(a).any() and denormal(b).any() and denormal(R.abs_mul(a, b)).sum() > 100
    p = K.min3_args()
    nans = sum(R.is_nan(v).astype(int) for v in p)
    assert all((R.is_nan(p[i]) & (nans == 1)).any() for i in range(3)) and (nans == 2).any() and (nans == 3).any()
    assert all(R.is_nan(p[i]) .any() and ((p[i] & U32(0x003FFFFF)) == 0)[R.is_nan(p[i])].all() for i in range(3))   # quiet, all of them
    zero = [(v & U32(0x7FFFFFFF)) == 0 for v in p]
    assert ((p[0] == 0) & (p[1] == U32(0x80000000))).any() and ((p[0] == U32(0x80000000)) & (p[2] == 0) & ~zero[1]).any()
    p = K.step_args()
    kind = sum(np.where(R.is_nan(v), 2, np.where(v == 0, 0, 1)) * 3 ** i for i, v in enumerate(p))
    assert set(kind.tolist()) == set(range(27)), "every pattern of zero / non-zero / NaN"
    assert all(((v >> U32(31)) == 0)[~R.is_nan(v)].all() for v in p), "axis distances are not negative"
    assert ((p[0] == p[1]) & (p[0] != 0) & ~R.is_nan(p[0])).any()              # a tie between two non-zero distances
    for v in K.word_args():
        assert _has(v, 0, 0xFFFFFFFF) and v.size >= 1 << 16
    a, b, c = K.mad_args()
    assert a.size % 64 == 0 and a.size == b.size == c.size
    sa, sb = R._sext24(a), R._sext24(b[::64])
    assert (sa == a.view(np.int32)).all() and (sb == b[::64].view(np.int32)).all(), "factors inside the signed 24-bit range"
    for ext in (-(1 << 23), (1 << 23) - 1, 0, 1, -1):
        assert (sa == ext).any() and (sb == ext).any()
    for dim in K.MARCH_GRID_DIMS:
        row = (dim + 1) * 4
        for stride in (row, (dim + 1) * row):
            assert stride < 1 << 23 and (sb == stride).any()
    # the other sets of a wave hold a b of their own, which nothing may read
    assert (b.reshape(-1, 64)[:, 1:] != b.reshape(-1, 64)[:, :1]).mean() > 0.99
