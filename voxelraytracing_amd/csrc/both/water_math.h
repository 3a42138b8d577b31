// water_math.h — the transmittance of vrt_set_water_optics (include/vrt.h), once: vexp_neg(t) = e^-t for t >= 0.  The water forms of
// the path kernels (vrt_path_water.h) and host_capi.cpp's vrth_water_transmittance both compile this text.  Only f32 add, subtract
// and multiply, floorf, conversions between float and int and integer operations occur: no libm, no ocml, no hardware
// transcendental.  It relies on -ffp-contract=off on both sides (both.h), as vlog does.
//
//   x = -t, k = floor(x * log2(e) + 0.5)            the nearest power of two, k <= 0
//   r = (x - k * ln2_hi) - k * ln2_lo               |r| <= 0.35; k * ln2_hi is exact (ln2_hi has 9 significant bits, |k| < 2^8)
//   p = 1 + r + r^2 (1/2 + r (1/6 + ... + r/5040))  Taylor's terms up to r^7: what is left out is below 6e-9
//   e^-t = p * 2^k                                  by an insert into p's exponent field where the result is normal; below that the
//                                                   significand is shifted out and rounded to nearest even in integer operations,
//                                                   so that the result does not depend on how a unit treats denormals
//
// What it gives at the edges:
//   t = +0 or -0        exactly 1 (k = 0, r = 0, p = 1)
//   t NaN               that NaN
//   t < 0               1: no caller has one (absorb >= 0 and water_dist >= 0)
//   t >= 128, t = +inf  +0; from about 103.98 (e^-t below 2^-150) the rounding gives +0 already
// Against float64 exp over every binary32 t in [0, 104]: docs/NUMERICS.md.
#pragma once
#include "both.h"

namespace vrt {

VRT_BOTH float vexp_neg(float t) {
    if (!(t >= 0.0f)) return t != t ? t : 1.0f;
    if (t >= 128.0f) return 0.0f;
    const float x = -t;
    const float kf = floorf(x * 1.44269502f + 0.5f);
    const float r = (x - kf * 0.693359375f) - kf * -2.12194442e-4f;
    const float q = 0.5f + r * (0.166666672f + r * (0.0416666679f + r * (0.00833333377f + r * (0.00138888892f + r * 1.98412701e-4f))));
    const float p = (1.0f + r) + (r * r) * q;   // in [0.70, 1.42]
    const int k = (int)kf;                      // in [-185, 0]
    uint32_t bp;
    memcpy(&bp, &p, 4);
    const int E = (int)(bp >> 23) + k;          // the result's biased exponent
    uint32_t bits;
    if (E >= 1) {
        bits = bp + ((uint32_t)k << 23);
    } else {   // below 2^-126: the 24-bit significand, shifted right by 1 - E and rounded to nearest even
        const uint32_t shift = (uint32_t)(1 - E);
        if (shift > 24u) return 0.0f;
        const uint32_t m = (bp & 0x007FFFFFu) | 0x00800000u;
        const uint32_t half = 1u << (shift - 1u), rem = m & ((half << 1) - 1u);
        bits = m >> shift;
        if (rem > half || (rem == half && (bits & 1u))) bits += 1u;
    }
    float out;
    memcpy(&out, &bits, 4);
    return out;
}

}  // namespace vrt
