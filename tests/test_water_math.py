"""vexp_neg (csrc/both/water_math.h), the transmittance of vrt_set_water_optics, without a GPU: the host build
(_ffi.water_transmittance) is bit for bit a numpy restatement of the same operation sequence and the reference's own C statement
(tests/water_ref.c); the edges are what the header says; and against float64 exp it stays within the recorded bound.

The bound: a sweep of every binary32 t in [0, 104] (1 121 976 321 values, a small C program over the same header, float64 exp as
the truth, the error in units of binary32's spacing at the true value — 2^-149 below 2^-126) found 1.3176 ulp at t = 28.0643654
(docs/NUMERICS.md).  This test runs every 4099th of those values and asserts that maximum rounded up to the next power of two, 2
ulp: the margin covers nothing but the sampling."""
import numpy as np
import pytest

import water_ref
from voxelraytracing_amd import _ffi

F32, U32, I32 = np.float32, np.uint32, np.int32
MAX_ULP_RECORDED = 1.3176
BOUND_ULP = 2.0   # the next power of two


def exp_neg_numpy(t):
    """water_math.h's operation sequence in numpy float32, value for value."""
    t = np.asarray(t, dtype=F32)
    out = np.empty(t.shape, dtype=F32)
    nan, neg, big = np.isnan(t), t < 0, t >= F32(128.0)
    out[nan] = t[nan]
    out[neg] = F32(1.0)
    out[big] = F32(0.0)
    m = ~(nan | neg | big)
    x = -t[m]
    with np.errstate(all="ignore"):
        kf = np.floor(x * F32(1.44269502) + F32(0.5)).astype(F32)
        r = ((x - kf * F32(0.693359375)) - kf * F32(-2.12194442e-4)).astype(F32)
        q = F32(0.00138888892) + r * F32(1.98412701e-4)
        for c in (0.00833333377, 0.0416666679, 0.166666672, 0.5):
            q = (F32(c) + r * q).astype(F32)
        p = ((F32(1.0) + r) + (r * r) * q).astype(F32)
    k = kf.astype(np.int64)
    bp = p.view(U32).astype(np.int64)
    E = (bp >> 23) + k
    bits = np.zeros(p.shape, dtype=np.int64)
    normal = E >= 1
    bits[normal] = bp[normal] + (k[normal] << 23)
    sub = ~normal
    shift = 1 - E[sub]
    mant = (bp[sub] & 0x007FFFFF) | 0x00800000
    keep = shift <= 24
    sh = np.where(keep, shift, 1)
    half = np.int64(1) << (sh - 1)
    rem = mant & ((half << 1) - 1)
    b = mant >> sh
    b = b + ((rem > half) | ((rem == half) & ((b & 1) == 1)))
    bits[sub] = np.where(keep, b, 0)
    out[m] = bits.astype(U32).view(F32)
    return out


def _bits(a):
    return np.asarray(a, dtype=F32).view(U32)


def _same(a, b):
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    return bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


EDGES = np.array([0.0, -0.0, 1e-45, 1e-38, 1e-10, 0.34657, 0.34658, 0.6931472, 1.0, 28.0643654, 87.0, 87.3365, 87.3366, 88.0, 100.0, 103.27, 103.28, 103.9, 103.97,
                  103.98, 104.0, 127.99, 128.0, 1e30, np.inf, -1.0, -np.inf, np.nan], dtype=F32)


def _sample():
    top = int(F32(104.0).view(U32))
    return np.append(np.arange(0, top + 1, 4099, dtype=np.int64), top).astype(U32).view(F32)   # (every 4099th bit pattern, and 104 itself)


def test_the_host_build_is_the_numpy_restatement_bit_for_bit(tmp_path):
    rng = np.random.default_rng(5)
    t = np.concatenate([EDGES, _sample()[::7], rng.uniform(0, 110, 20000).astype(F32), rng.uniform(80, 105, 20000).astype(F32)])
    got = _ffi.water_transmittance(t, F32(1.0))
    assert _same(got, exp_neg_numpy(t))
    ref = water_ref.load(tmp_path)
    assert _same(ref.exp_neg(t[:4000]), got[:4000])


def test_the_product_is_formed_in_binary32():
    rng = np.random.default_rng(6)
    a, w = rng.uniform(0, 2, 5000).astype(F32), rng.uniform(0, 60, 5000).astype(F32)
    a[:4], w[:4] = (0.0, 1e-30, 1e-20, 3.0), (5.0, 1e-10, 1e-25, 0.0)   # a zero, a denormal product, a product that underflows to 0
    assert _same(_ffi.water_transmittance(a, w), exp_neg_numpy((a * w).astype(F32)))


def test_the_edges_are_what_the_header_states():
    f = lambda x: _ffi.water_transmittance(np.array([x], F32), np.array([1.0], F32))[0]   # noqa: E731
    assert _bits(f(0.0)) == 0x3F800000 and _bits(f(-0.0)) == 0x3F800000          # exactly 1
    assert _bits(f(1e-45)) == 0x3F800000
    for t in (104.0, 127.99, 128.0, 1e30, np.inf):
        assert _bits(f(t)) == 0, t                                                # +0
    assert np.isnan(f(np.nan))
    assert _bits(f(-1.0)) == 0x3F800000                                           # outside the contract: 1
    assert _bits(f(103.27)) == 1                                                  # the smallest denormal, by rounding
    assert 0 < float(f(88.0)) < 2.0 ** -126                                       # a denormal result, not flushed
    t = _sample()
    v = _ffi.water_transmittance(t, F32(1.0))
    assert np.all(np.diff(v.astype(np.float64)) <= 0), "not increasing in t"


def test_against_float64_exp_within_the_recorded_bound():
    t = _sample()
    assert t.size > 270000 and t[0] == 0 and t[-1] == 104.0
    got = _ffi.water_transmittance(t, F32(1.0)).astype(np.float64)
    exact = np.exp(-t.astype(np.float64))
    _, e = np.frexp(exact)
    ulp = np.ldexp(1.0, np.maximum(e - 1, -126) - 23)
    err = np.abs(got - exact) / ulp
    worst = int(np.argmax(err))
    print(f"max error {err[worst]:.4f} ulp at t = {t[worst]!r} over {t.size} values (recorded over all of them: {MAX_ULP_RECORDED})")
    assert float(err.max()) <= BOUND_ULP
