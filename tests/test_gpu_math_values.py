"""The kernels' exact arithmetic, value for value against references that are not the GPU (tests/math_ref.py: float32 restatements,
the oracle's functions, the helpers' stated contracts) over the operand sets of tests/math_cases.py, through
vrt_selftest_math_values — the kernel calls the functions the frame kernels call.  The rule is math_ref.equal: bits are equal, two
NaNs are equal whatever their payload; for min3_f32 and the step's minimum +0 equals -0 as well.  No tolerances.  Where a function
chooses its form per wave the flag word must say refined and general exactly where the cases composed such waves."""
import ctypes as C

import numpy as np
import pytest

import math_cases as K
import math_ref as R
from voxelraytracing_amd import _ffi
from voxelraytracing_amd import graphics as g

pytestmark = pytest.mark.gpu

U32 = np.uint32
ERR_INVALID_ARG = -1


def _check(op, got, want, inputs, rule=R.equal):
    """got [words, n] from the GPU against the reference's tuple of words; reports the first few operand sets that differ"""
    want = np.stack([np.asarray(w, dtype=U32) for w in want])
    assert got.shape == want.shape, (op, got.shape, want.shape)
    bad = ~rule(got, want)
    if bad.any():
        where = np.flatnonzero(bad.any(axis=0))
        rows = [f"set {i} (wave {i // 64} lane {i % 64}) in {[hex(int(w[i])) for w in inputs]}: got {[hex(int(v)) for v in got[:, i]]}"
                f" want {[hex(int(v)) for v in want[:, i]]}" for i in where[:8]]
        pytest.fail(f"{op}: {where.size} of {got.shape[1]} operand sets differ\n" + "\n".join(rows))


def _run(op, ref, *inputs, rule=R.equal):
    got = g.selftest_math_values(op, *inputs)
    _check(op, got, ref, inputs, rule)
    return got


def test_division_and_square_root():
    n, d = K.div_args()
    _run("div", (R.div(n, d),), n, d)
    x = K.sqrt_args()
    _run("sqrt", (R.sqrt(x),), x)


def test_unit_steps_and_normalize_wave():
    xyz, kinds = K.vectors()
    for op, ref in (("unit_steps", R.unit_steps), ("normalize", R.normalize)):
        got = _run(op, ref(*xyz), *xyz)
        flags = got[3].reshape(-1, 64)
        refined = np.isin(np.array(kinds), ("band", "edge", "square"))
        assert (flags == refined.astype(U32)[:, None]).all(), op
        assert refined.mean() >= 0.25


def test_lens_divide_and_square_root():
    n, d, refined = K.lens_div_args()
    got = _run("lens_div", R.lens_div(n, d), n, d)
    assert (got[1].reshape(-1, 64) == np.array(refined, dtype=U32)[:, None]).all()
    x, refined = K.lens_sqrt_args()
    got = _run("lens_sqrt", R.lens_sqrt(x), x)
    assert (got[1].reshape(-1, 64) == np.array(refined, dtype=U32)[:, None]).all()


def test_rng_next():
    s = K.rng_states()
    _run("rng_next", R.rng_next(s), s)
    _run("rng_next_u2", R.rng_next_u2(s), s)


def test_log_both_forms():
    x = K.log_args()
    want = (R.log(x),)
    _run("log_banded", want, x)
    _run("log_general", want, x)


def test_cos2pi():
    u = K.cos_args()
    _run("cos2pi", (R.cos2pi(u),), u)


def test_rng_next_dir():
    s, special = K.rng_dir_states()
    want = R.rng_dir(s)
    got = _run("rng_dir", want, s)
    for w, lane, _, kind in special:      # (reported apart: the waves with a u2 of exactly 1 — the general forms — or 0 — the clamp)
        i = slice(64 * w, 64 * w + 64)
        assert R.equal(got[:, i], np.stack(want)[:, i]).all(), (w, lane, kind)
        if kind == "one":
            assert (got[4, i] == 0).all()


def test_conversions_and_float_helpers():
    x = K.cvt_args()
    _run("trunc2i", (R.trunc2i(x),), x)
    _run("flr2i", (R.flr2i(x),), x)
    a, b = K.abs_mul_args()
    _run("abs_mul", (R.abs_mul(a, b),), a, b)
    p = K.min3_args()
    _run("min3_f32", (R.min3_f32(*p),), *p, rule=R.equal_zero_sign)
    p = K.step_args()
    _run("min3_bits", (R.step_tree(*p),), *p, rule=R.equal_zero_sign)


def test_integer_helpers():
    m, a, b = K.word_args()
    _run("bfi", (R.bfi(m, a, b),), m, a, b)
    _run("low_bits", R.low_bits(a, b), a, b)
    _run("or_and", (R.or_and(m, a, b),), m, a, b)
    a, b, c = K.mad_args()
    _run("mad_i24", (R.mad_i24(a, b, c),), a, b, c)


def test_refusals_write_nothing():
    lib = _ffi.vrt()
    src = np.full(3 * 64, 0x3F800000, dtype=U32)
    out = np.full(8 * 64, 0xDEADBEEF, dtype=U32)
    ps, po = src.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    for args in ((0, 64, None, po), (0, 64, ps, None), (0, 0, ps, po), (len(g.MATH_OPS), 64, ps, po), (0xFFFFFFFF, 64, ps, po),
                 (0, (1 << 26) + 1, ps, po)):
        assert lib.vrt_selftest_math_values(0, *args) == ERR_INVALID_ARG, args
        assert (out == 0xDEADBEEF).all(), args
    with pytest.raises(ValueError):
        g.selftest_math_values("div", src[:64])
    with pytest.raises(g.VrtError):
        g.selftest_math_values("sqrt", np.zeros(0, dtype=U32))
    # ... and a call that is not refused writes exactly its own words: one output word for each of the 64 sets of a division
    assert lib.vrt_selftest_math_values(0, 0, 64, ps, po) == 0
    assert (out[:64] == 0x3F800000).all() and (out[64:] == 0xDEADBEEF).all()
