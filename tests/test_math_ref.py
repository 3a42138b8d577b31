"""tests/math_ref.py, the reference tests/test_gpu_math_values.py holds the GPU to, held to something else in turn, on the CPU:
the float32 restatements to the same operations in float64 rounded once; the oracle's array forms to its scalar functions; the
oracle's rng_next to the reference shader's (tests/golden/wgsl_rng.npz); the oracle's log and cos(2 pi u) to float64 over the whole
case set, within twice the error measured there (docs/ORACLE.md) — a bound on the oracle, never on the device, which is held to the
oracle bit for bit."""
import ctypes as C
import os

import numpy as np

import math_cases as K
import math_ref as R
from oracle import orc

U32, F32, F64 = np.uint32, np.float32, np.float64
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# measured over math_cases.log_args() / cos_args() (this test prints them; docs/ORACLE.md records them)
LOG_MAX_ULP = 1.654          # |orc_log(x) - ln x| in ulps of the float32 nearest ln x
COS_MAX_ABS = 2.081e-7      # |orc_cos2pi(u) - cos(2 pi u)|


def _same(a, b):
    return bool(np.all(R.equal(a, b)))


def test_float32_restatements_equal_float64_rounded_once():
    xyz, _ = K.vectors()
    for fn in (R.unit_steps, R.normalize):
        a, b = fn(*xyz, A=R.A32), fn(*xyz, A=R.A64R)
        assert all(_same(p, q) for p, q in zip(a, b)), fn.__name__
    n, d = K.div_args()
    assert _same(R.div(n, d, R.A32), R.div(n, d, R.A64R))
    n, d, _ = K.lens_div_args()
    assert _same(R.lens_div(n, d, R.A32)[0], R.lens_div(n, d, R.A64R)[0])
    for x in (K.sqrt_args(), K.lens_sqrt_args()[0]):
        assert _same(R.sqrt(x, R.A32), R.sqrt(x, R.A64R))


def test_restatements_on_values_worked_by_hand():
    one, two, three, four, twelve = (R.bits(F32(v)) for v in (1.0, 2.0, 3.0, 4.0, 12.0))
    nx, ny, nz, flag = R.normalize(three, four, twelve)          # |(3, 4, 12)| = 13
    assert (R.flt(nx)[0], R.flt(ny)[0], R.flt(nz)[0]) == (F32(3) / F32(13), F32(4) / F32(13), F32(12) / F32(13)) and flag[0] == 1
    ux, uy, uz, flag = R.unit_steps(one, two, two)               # sqrt(1 + 4 + 4), sqrt(1 + 1/4 + 1), the same
    assert (R.flt(ux)[0], R.flt(uy)[0], R.flt(uz)[0]) == (F32(3), F32(1.5), F32(1.5)) and flag[0] == 1
    zero = R.bits(F32(0.0))
    assert all(R.is_nan(w)[0] for w in R.normalize(zero, zero, zero)[:3]) and R.normalize(zero, zero, zero)[3][0] == 0
    # the band is [2^-30, 2^30], ends included; one set outside it takes its whole wave with it, and no other wave
    edge = np.array([0x307FFFFF, 0x30800000, 0x4E800000, 0x4E800001, 0, 0x7F800000, 0x7FC00000, 0x00000001], dtype=U32)
    assert R.in_band(edge).tolist() == [False, True, True, False, False, False, False, False]
    assert R.in_band(edge | U32(0x80000000)).tolist() == R.in_band(edge).tolist()
    pred = np.ones(200, dtype=bool)
    pred[70] = False
    assert R.wave_all(pred).tolist() == [True] * 64 + [False] * 64 + [True] * 72


def test_helper_references_on_values_worked_by_hand():
    f = lambda *v: R.bits(np.array(v, dtype=F32))                # noqa: E731
    i32 = lambda w: w.view(np.int32).tolist()                    # noqa: E731
    x = f(np.nan, np.inf, -np.inf, 2147483648.0, -2147483648.0, 2147483520.0, -0.0, -0.5, -1.0, 2.5, -2.5)
    assert i32(R.trunc2i(x)) == [0, 2147483647, -2147483648, 2147483647, -2147483648, 2147483520, 0, 0, -1, 2, -2]
    assert i32(R.flr2i(x)) == [2147483647, 2147483647, -2147483648, 2147483647, -2147483648, 2147483520, 0, -1, -1, 2, -3]
    neg_nan = np.array([0xFFC00000, 0xFFFFFFFF], dtype=U32)
    assert i32(R.trunc2i(neg_nan)) == [0, 0] and i32(R.flr2i(neg_nan)) == [-2147483648, -2147483648]
    assert R.flt(R.abs_mul(f(-3.0, 3.0, -3.0), f(2.0, -2.0, -2.0))).tolist() == [6.0, -6.0, -6.0]
    assert R.is_nan(R.abs_mul(f(np.inf), f(0.0)))[0]
    assert R.flt(R.min3_f32(f(np.nan, 5.0, np.nan), f(2.0, np.nan, np.nan), f(3.0, np.nan, 7.0))).tolist() == [2.0, 5.0, 7.0]
    assert R.is_nan(R.min3_f32(f(np.nan), f(np.nan), f(np.nan)))[0]
    # the step: the smallest non-zero distance; a NaN only where nothing else is non-zero; zero where all three are
    got = R.flt(R.step_tree(f(0.0, 0.0, 2.0, np.nan, 0.0, 3.0), f(0.0, 5.0, 0.0, 0.0, np.nan, 1.0), f(0.0, 4.0, 7.0, 6.0, 0.0, 2.0)))
    assert got[:4].tolist() == [0.0, 4.0, 2.0, 6.0] and np.isnan(got[4]) and got[5] == 1.0
    w = lambda *v: np.array(v, dtype=U32)                        # noqa: E731
    assert R.bfi(w(0x0000FFFF), w(0x12345678), w(0x9ABCDEF0)).tolist() == [0x9ABC5678]
    assert [int(p[0]) for p in R.low_bits(w(0xFFFFFFFF), w(0x100))] == [0x103, 0x107, 0x10F, 0x11F]
    assert R.or_and(w(0x1), w(0xF0), w(0x30)).tolist() == [0x31]
    a, b, c = w(0x00FFFFFF, 3), w(5, 999), w(10, 0xFFFFFFFF)       # -1 * 5 + 10; 3 * 5 - 1: the second set's own b is not read
    assert R.mad_i24(a, b, c).tolist() == [5, 14]
    assert R.mad_i24(w(0x800000), w(0x800000), w(0)).tolist() == [0]    # 2^46: the low 32 bits


def test_oracle_array_forms_equal_the_scalar_functions():
    L = orc.lib()
    g = np.random.default_rng(7)
    pick = lambda a, n=1500: np.concatenate([a[-64:], a[g.integers(0, a.size, n)]])    # noqa: E731  (the hand-placed ends too)
    x = pick(K.log_args())
    assert np.array_equal(R.log(x), R.bits(np.array([L.orc_test_log(float(v)) for v in R.flt(x)], dtype=F32)))
    u = pick(K.cos_args())
    assert np.array_equal(R.cos2pi(u), R.bits(np.array([L.orc_test_cos2pi(float(v)) for v in R.flt(u)], dtype=F32)))
    s = pick(K.rng_states()[:256], 300)
    states, uniforms = R.rng_next(s)
    for i, s0 in enumerate(s):
        st = C.c_uint32(int(s0))
        v = L.orc_rng_next(C.byref(st))
        assert st.value == states[i] and R.bits(F32(v))[0] == uniforms[i]
    all_states, special = K.rng_dir_states()
    s = np.concatenate([all_states[:300], all_states[[64 * w + lane for w, lane, _, _ in special]]])
    states, dx, dy, dz, _ = R.rng_dir(s)
    d = (C.c_float * 3)()
    for i, s0 in enumerate(s):
        st = C.c_uint32(int(s0))
        L.orc_test_rng_dir(C.byref(st), d)
        assert st.value == states[i] and R.equal(R.bits(np.array(list(d), dtype=F32)), np.array([dx[i], dy[i], dz[i]], dtype=U32)).all(), hex(s0)


def test_oracle_rng_next_is_the_reference_shaders():
    f = np.load(os.path.join(GOLD, "wgsl_rng.npz"))
    s = f["seeds"].astype(U32)
    for j in range(16):
        s, u = R.rng_next(s)
        assert np.array_equal(s, f["states"][:, j].astype(U32)) and np.array_equal(u, f["uniforms"][:, j].astype(F32).view(U32)), j


def test_oracle_log_and_cos2pi_within_twice_their_measured_error():
    x = K.log_args()
    want = np.log(R.flt(x).astype(F64))
    ulp = np.spacing(np.abs(want).astype(F32)).astype(F64)
    log_ulp = float((np.abs(R.flt(R.log(x)).astype(F64) - want) / ulp).max())
    u = K.cos_args()
    cos_abs = float(np.abs(R.flt(R.cos2pi(u)).astype(F64) - np.cos(2.0 * np.pi * R.flt(u).astype(F64))).max())
    print(f"orc_log: {log_ulp:.4f} ulp over {x.size} values; orc_cos2pi: {cos_abs:.4e} absolute over {u.size} values")
    assert log_ulp <= 2.0 * LOG_MAX_ULP and cos_abs <= 2.0 * COS_MAX_ABS
    assert log_ulp >= 0.5 * LOG_MAX_ULP and cos_abs >= 0.5 * COS_MAX_ABS, "the recorded figures are no longer what is measured: measure again"
