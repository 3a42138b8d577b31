"""References for the kernels' exact arithmetic (csrc/vrt_march.h, vrt_path_common.h; docs/NUMERICS.md rows b'', c', h, n, p, q), none
of them the GPU.  tests/test_gpu_math_values.py holds vrt_selftest_math_values to this file word for word; tests/test_math_ref.py holds
this file to float64 and to the oracle's scalar functions on the CPU.

  * divide, square root, unit_steps, normalize_wave, the lens forms: the texts restated operation by operation in an arithmetic
    `A` — F32 (numpy float32: IEEE binary32, round to nearest even, denormals kept) or F64R (the same operation in float64,
    rounded to float32 once: for a single + - * / sqrt the double rounding is harmless, 53 >= 2 * 24 + 2 bits);
  * rng_next, vlog, vcos2pi, rng_next_dir: the oracle's own functions (oracle/vrt_oracle.c), through their array forms;
  * the one-instruction helpers: the contract their comments state, in numpy integer and float code; the step's branch tree
    (row c') as the oracle's step has it.

Everything takes and returns uint32 bit patterns (arrays of n operand sets); `equal` / `equal_zero_sign` are the comparison rule."""
import numpy as np

from oracle import orc

U32, F32, F64 = np.uint32, np.float32, np.float64
BAND_LO, BAND_HI = 0x30800000, 0x4E800000     # in_band: 2^-30 .. 2^30, both included
SQRT_BAND_LO = F32(1.0e-28)                    # kSqrtBandLo
U2_MIN = F32(1.0e-10)


def bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(U32)


def flt(b):
    return np.ascontiguousarray(b, dtype=U32).view(F32)


def is_nan(b):
    b = np.asarray(b, dtype=U32)
    return (b & U32(0x7FFFFFFF)) > U32(0x7F800000)


def equal(a, b):
    """The comparison rule: bits are equal, except that two NaNs are equal whatever their payload."""
    a, b = np.asarray(a, dtype=U32), np.asarray(b, dtype=U32)
    return (a == b) | (is_nan(a) & is_nan(b))


def equal_zero_sign(a, b):
    """... and +0 equals -0: min3_f32 and the step's minimum, where the sign of a zero is never observed (NUMERICS.md b'')."""
    a, b = np.asarray(a, dtype=U32), np.asarray(b, dtype=U32)
    return equal(a, b) | (((a | b) & U32(0x7FFFFFFF)) == 0)


# ---- the two arithmetics ----
class _F32:
    @staticmethod
    def add(a, b): return a + b
    @staticmethod
    def mul(a, b): return a * b
    @staticmethod
    def div(a, b): return a / b
    @staticmethod
    def sqrt(a): return np.sqrt(a)


class _F64R:
    @staticmethod
    def add(a, b): return (a.astype(F64) + b.astype(F64)).astype(F32)
    @staticmethod
    def mul(a, b): return (a.astype(F64) * b.astype(F64)).astype(F32)
    @staticmethod
    def div(a, b): return (a.astype(F64) / b.astype(F64)).astype(F32)
    @staticmethod
    def sqrt(a): return np.sqrt(a.astype(F64)).astype(F32)


A32, A64R = _F32, _F64R


def _quiet(fn):
    def wrapped(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    wrapped.__doc__, wrapped.__name__ = fn.__doc__, fn.__name__
    return wrapped


# ---- the band ----
def in_band(b):
    """in_band of vrt_march.h on bit patterns: one unsigned compare, so NaN, inf, 0 and denormals are outside."""
    b = np.asarray(b, dtype=U32)
    return ((b & U32(0x7FFFFFFF)) - U32(BAND_LO)) <= U32(BAND_HI - BAND_LO)     # (uint32 arithmetic wraps, as the device's)


def wave_all(pred):
    """A per-set predicate -> per set, whether every set of its wave (64 consecutive sets; the last may be short) satisfies it."""
    pred = np.asarray(pred, dtype=bool)
    n = pred.size
    padded = np.ones((n + 63) // 64 * 64, dtype=bool)
    padded[:n] = pred
    return np.repeat(padded.reshape(-1, 64).all(axis=1), 64)[:n]


# ---- divide, square root and the composites ----
@_quiet
def div(n, d, A=A32):
    """n / d, correctly rounded: what div_refined(n, d, rcp_refined(d)) claims inside the band and for a numerator of +-0."""
    return bits(A.div(flt(n), flt(d)))


@_quiet
def sqrt(x, A=A32):
    return bits(A.sqrt(flt(x)))


@_quiet
def unit_steps(x, y, z, A=A32):
    """ray_tracer.wgsl:209-213: |sqrt(1 + (b/a)^2 + (c/a)^2)| per axis, the sum left to right.  -> (ux, uy, uz, refined flag)"""
    x, y, z = flt(x), flt(y), flt(z)
    one = np.ones_like(x)

    def axis(a, b, c):
        ba, ca = A.div(b, a), A.div(c, a)
        return np.abs(A.sqrt(A.add(A.add(one, A.mul(ba, ba)), A.mul(ca, ca))))
    flag = wave_all(in_band(bits(x)) & in_band(bits(y)) & in_band(bits(z)))
    return bits(axis(x, y, z)), bits(axis(y, x, z)), bits(axis(z, x, y)), flag.astype(U32)


@_quiet
def normalize(x, y, z, A=A32):
    """v / sqrt(dot(v, v)), the dot x*x + y*y + z*z left to right.  -> (nx, ny, nz, refined flag)"""
    x, y, z = flt(x), flt(y), flt(z)
    ln = A.sqrt(A.add(A.add(A.mul(x, x), A.mul(y, y)), A.mul(z, z)))
    flag = wave_all(in_band(bits(x)) & in_band(bits(y)) & in_band(bits(z)))
    return bits(A.div(x, ln)), bits(A.div(y, ln)), bits(A.div(z, ln)), flag.astype(U32)


@_quiet
def lens_div(n, d, A=A32):
    """lens_div: n / d; refined when every set of the wave has n +-0 or in band, and d in band.  -> (quotient, flag)"""
    flag = wave_all(((np.asarray(n, dtype=U32) & U32(0x7FFFFFFF)) == 0) | in_band(n)) & wave_all(in_band(d))
    return div(n, d, A), flag.astype(U32)


@_quiet
def lens_sqrt(x, A=A32):
    """lens_sqrt_of: sqrt(x); refined when every set of the wave has x >= 1e-28 (+inf too; not -0, not NaN).  -> (root, flag)"""
    flag = wave_all(flt(x) >= SQRT_BAND_LO)
    return sqrt(x, A), flag.astype(U32)


# ---- the path trace's draws: the oracle's functions ----
def rng_next(state):
    """-> (state after the draw, bits of the uniform)"""
    s, u = orc.rng_next_n(state)
    return s, bits(u)


def rng_next_u2(state):
    s, u = orc.rng_next_n(state)
    return s, bits(np.where(u < U2_MIN, U2_MIN, u))


def log(x):
    return bits(orc.log_n(x))


def cos2pi(u):
    return bits(orc.cos2pi_n(u))


@_quiet
def rng_dir(state):
    """-> (state after the six draws, x, y, z, flags).  flags as vrt_selftest_math_values reports them: bit 0 — every set of the
    wave has its three square-root arguments -2 ln u2 >= 1e-28; bit 1 — every set's vector rho * cos(2 pi u1) is in the band."""
    s, d = orc.rng_dir_n(state)
    t = np.ascontiguousarray(state, dtype=U32).copy()
    ts, vs = [], []
    for _ in range(3):
        t, u1 = orc.rng_next_n(t)
        t, u2 = orc.rng_next_n(t)
        u2 = np.where(u2 < U2_MIN, U2_MIN, u2)
        arg = F32(-2.0) * orc.log_n(u2)
        ts.append(arg)
        vs.append(np.sqrt(arg) * orc.cos2pi_n(u1))
    assert np.array_equal(t, s)
    roots = wave_all(np.fmin(np.fmin(ts[0], ts[1]), ts[2]) >= SQRT_BAND_LO)
    norm = wave_all(in_band(bits(vs[0])) & in_band(bits(vs[1])) & in_band(bits(vs[2])))
    return s, bits(d[:, 0]), bits(d[:, 1]), bits(d[:, 2]), roots.astype(U32) | (norm.astype(U32) << U32(1))


# ---- the one-instruction helpers ----
def _cvt(x, rounded, nan, nan_signed):
    f = flt(x).astype(F64)
    with np.errstate(all="ignore"):
        r = np.clip(rounded(f), -2147483648.0, 2147483647.0)
    r = np.where(np.isnan(f), np.where(np.asarray(x, dtype=U32) >> U32(31) == 1, float(nan_signed), float(nan)), r)
    return r.astype(np.int64).astype(np.int32).view(U32)


def trunc2i(x):
    """v_cvt_i32_f32: towards zero, NaN -> 0, +-inf and |x| >= 2^31 saturate (WGSL's i32(f32))."""
    return _cvt(x, np.trunc, 0, 0)


def flr2i(x):
    """v_cvt_flr_i32_f32: towards -inf, saturating; a NaN saturates by its sign bit, INT_MAX or INT_MIN (vrt_march.h, at flr2i:
    the comment said INT_MAX for every NaN until the GPU returned INT_MIN for 0xFFC00000)."""
    return _cvt(x, np.floor, 2147483647, -2147483648)


@_quiet
def abs_mul(a, b):
    """|a| * b, one rounding (row b'')."""
    return bits(np.abs(flt(a)) * flt(b))


@_quiet
def min3_f32(a, b, c):
    """The minimum of the numbers among a, b, c: a quiet NaN operand is ignored, NaN only if all three are.  Compare with
    equal_zero_sign: which zero a +-0 tie returns is not part of the contract."""
    return bits(np.fmin(np.fmin(flt(a), flt(b)), flt(c)))


def _orc_min(a, b):
    return np.where((a < b) | (b != b), a, b)


@_quiet
def step_tree(x, y, z):
    """The step's branch tree (ray_tracer.wgsl:247-270) as the oracle's march has it, for axis distances that are non-negative
    or NaN: what row c', min3_u32(bits - 1) + 1, claims to equal.  Compare with equal_zero_sign."""
    x, y, z = flt(x), flt(y), flt(z)
    x0, y0, z0 = x == 0, y == 0, z == 0
    if_x0 = np.where(y0, z, np.where(z0, y, _orc_min(y, z)))
    if_y0 = np.where(z0, x, _orc_min(x, z))
    rest = np.where(z0, _orc_min(y, x), _orc_min(x, _orc_min(y, z)))
    return bits(np.where(x0, if_x0, np.where(y0, if_y0, rest)))


def bfi(mask, a, b):
    mask, a, b = (np.asarray(v, dtype=U32) for v in (mask, a, b))
    return (mask & a) | (~mask & b)


def low_bits(a, b):
    """low_bits_of<3>, <7>, <15>, <31>(a, b): the low bits of a over the rest of b"""
    return tuple(bfi(np.full_like(np.asarray(a, dtype=U32), m), a, b) for m in (3, 7, 15, 31))


def or_and(a, b, c):
    a, b, c = (np.asarray(v, dtype=U32) for v in (a, b, c))
    return a | (b & c)


def _sext24(v):
    v = np.asarray(v, dtype=U32).astype(np.int64) & 0xFFFFFF
    return v - ((v & 0x800000) << 1)


def mad_i24(a, b, c):
    """v_mad_i32_i24: the low 32 bits of a * b + c, a and b taken as signed 24-bit.  b is a scalar operand in the march (a
    wave-uniform stride): every set of a wave uses the b of the wave's first set."""
    b = np.asarray(b, dtype=U32)
    b_wave = np.repeat(b[::64], 64)[:b.size]
    return ((_sext24(a) * _sext24(b_wave) + np.asarray(c, dtype=U32).astype(np.int64)) & 0xFFFFFFFF).astype(U32)
