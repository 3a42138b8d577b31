// haze_math.h — the arithmetic of vrt_set_haze (include/vrt.h), once: the distance a segment's draw reaches in the haze and the
// distance at which a segment that hits nothing leaves the world box.  The haze forms of the path kernels (vrt_path_haze.h) and
// host_capi.cpp's vrth_haze_distance / vrth_haze_exit both compile this text.  Only f32 add, subtract, multiply and divide, fminf,
// compares and integer operations occur: no libm, no ocml, no hardware transcendental.  It relies on -ffp-contract=off and a
// correctly rounded divide on both sides (both.h).
//
//   haze_log(x)   vrt_path_common.h's vlog in its plain-division form (vlog_t<false>), which vrt_selftest_exact_math holds equal to
//                 the banded form the other kernels call, over every mantissa
//   t = (-haze_log(uc)) * inv, uc = u < 1e-10f ? 1e-10f : u     rng_next_u2's clamp; inv = 1.0f / density, formed once on the host
//
// What it gives at the edges:
//   u = 0 (and below 1e-10)   the clamp's distance, about 23.03 * inv
//   u = 1                     -0 * inv = -0: an event at the origin wherever the segment has a length
//   u NaN                     what the integer text makes of the NaN's bits: some finite number, the same on either side (rng_next has none)
//   an origin on or beyond a face of the box, or a NaN: exit 0 — the origin ray_world treats as outside
//   d.k = +0 / -0 / NaN       that axis never exits (+inf); all three: +inf
#pragma once
#include "both.h"

namespace vrt {

VRT_BOTH float haze_log(float x) {
    uint32_t b;
    memcpy(&b, &x, 4);
    int e = (int)(b >> 23) - 127;
    const uint32_t mb = (b & 0x007FFFFFu) | 0x3F800000u;
    float m;
    memcpy(&m, &mb, 4);
    if (m > 1.41421354f) { m = m * 0.5f; e += 1; }
    const float num = m - 1.0f, den = m + 1.0f;
    const float s = num / den;
    const float z = s * s;
    const float p = z * (0.333333343f + z * (0.2f + z * (0.142857149f + z * (0.111111112f + z * 0.0909090936f))));
    return (float)e * 0.693147182f + (s + s * p) * 2.0f;
}

VRT_BOTH float haze_distance(float u, float inv) {
    const float uc = u < 1.0e-10f ? 1.0e-10f : u;
    return (-haze_log(uc)) * inv;
}

// the origin is strictly inside the world box (false for a NaN): where a segment has a length in the haze at all
VRT_BOTH bool haze_inside(float ox, float oy, float oz, float world_max) {
    return (ox > 0.0f && oy > 0.0f && oz > 0.0f) && (ox < world_max && oy < world_max && oz < world_max);
}

VRT_BOTH float haze_exit_axis(float o, float d, float world_max) {
    if (d > 0.0f) return (world_max - o) / d;
    if (d < 0.0f) return (0.0f - o) / d;
    return __builtin_inff();
}

VRT_BOTH float haze_exit(const float o[3], const float d[3], float world_max) {
    if (!haze_inside(o[0], o[1], o[2], world_max)) return 0.0f;
    const float ex = haze_exit_axis(o[0], d[0], world_max), ey = haze_exit_axis(o[1], d[1], world_max), ez = haze_exit_axis(o[2], d[2], world_max);
    return fminf(ex, fminf(ey, ez));
}

}  // namespace vrt
