// tone_math.h — exposure and tone mapping of presented path frames (include/vrt.h: vrt_set_tone_map), once: the luminance bin of
// a pixel, the one-thread step behind a metered frame's histogram (rank, luminance, target, adaptation) and the map of one colour
// channel.  vrt_tone.hip's metering kernels, vrt_kernels.hip's mapped blits and host_capi.cpp's vrth_tone_meter / vrth_tone_map
// all compile this text.  Only f32 add, subtract, multiply, divide and square root occur, in the order include/vrt.h states; it
// relies on -ffp-contract=off on both sides (both.h).
#pragma once
#include "both.h"

namespace vrt {

// include/vrt.h VRT_TONE_* (restated: a header of both/ includes nothing of the project)
constexpr uint32_t kToneOff = 0u, kToneLinear = 1u, kToneReinhard = 2u, kToneFilmic = 3u;
constexpr uint32_t kToneAuto = 1u, kToneGamma2 = 2u;
constexpr uint32_t kToneBins = 256u;
constexpr int kToneBinBase = 888;   // bits(2^-16) >> 20: eight bins an octave from 2^-16 to 2^16

VRT_BOTH uint32_t tone_bits(float x) { uint32_t u; memcpy(&u, &x, sizeof u); return u; }
VRT_BOTH float tone_float(uint32_t u) { float x; memcpy(&x, &u, sizeof x); return x; }

// Whether vrt_set_tone_map takes the setting (O: vrt_tone_map).  Every float is finite and >= 0 whatever the curve; what a curve or
// the metering reads must also be usable: exposure > 0 with a curve, key > 0 and adapt in (0, 1] with AUTO.
template <class O>
VRT_BOTH bool tone_setting_ok(const O &o) {
    if (o.curve > kToneFilmic || (o.flags & ~(kToneAuto | kToneGamma2))) return false;
    if (o._reserved[0] || o._reserved[1] || o._reserved[2]) return false;
    const float f[6] = {o.exposure, o.white, o.key, o.adapt, o.min_auto, o.max_auto};
    for (int i = 0; i < 6; i++)
        if (!(f[i] >= 0.0f) || f[i] - f[i] != 0.0f) return false;   // (negative, NaN, infinite)
    if (o.percentile > 1000u) return false;
    if (o.min_auto != 0.0f && o.max_auto != 0.0f && o.min_auto > o.max_auto) return false;
    if (o.curve == kToneOff) return (o.flags & kToneAuto) == 0u;
    if (!(o.exposure > 0.0f)) return false;
    if ((o.flags & kToneAuto) && (!(o.key > 0.0f) || !(o.adapt > 0.0f) || o.adapt > 1.0f)) return false;
    return true;
}

// ---- metering ----
VRT_BOTH float tone_luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
// The histogram bin of a luminance, or -1: left out (zero, negative, NaN, infinite)
VRT_BOTH int tone_bin(float lum) {
    const uint32_t u = tone_bits(lum);
    if (!(lum > 0.0f) || u == 0x7F800000u) return -1;
    const int b = (int)(u >> 20) - kToneBinBase;
    return b < 0 ? 0 : (b > (int)kToneBins - 1 ? (int)kToneBins - 1 : b);
}

VRT_BOTH uint64_t tone_rank(uint64_t n, uint32_t percentile) {
    const uint64_t r = n * (uint64_t)percentile / 1000u;
    return r < n - 1u ? r : n - 1u;
}

struct ToneMeter { float exposure, key, adapt, min_auto, max_auto; uint32_t percentile; };
struct ToneMetered { float exposure, target, luminance; uint32_t bin; };

// The one-thread step.  n: the histogram's sum; when it is not 0: rank = tone_rank(n), b the lowest bin whose inclusive prefix
// sum exceeds rank, before the prefix sum below b, in_bin = bins[b].  prev: the adapted exposure of the metered frame before
// this one (has_prev: there is one since the adaptation started).
VRT_BOTH ToneMetered tone_finish(const ToneMeter &m, uint64_t n, uint64_t rank, uint32_t b, uint64_t before, uint32_t in_bin, bool has_prev, float prev) {
    ToneMetered r;
    r.luminance = 0.0f;
    r.bin = 0u;
    if (n == 0u) {
        r.target = has_prev ? prev : m.exposure;
    } else {
        const float lo = tone_float((b + (uint32_t)kToneBinBase) << 20), hi = tone_float((b + (uint32_t)kToneBinBase + 1u) << 20);
        const float frac = ((float)(uint32_t)(rank - before) + 0.5f) / (float)in_bin;
        const float L = lo + (hi - lo) * frac;
        float target = (m.key / L) * m.exposure;
        if (m.min_auto != 0.0f && target < m.min_auto) target = m.min_auto;
        if (m.max_auto != 0.0f && target > m.max_auto) target = m.max_auto;
        r.target = target;
        r.luminance = L;
        r.bin = b;
    }
    r.exposure = (!has_prev || m.adapt == 1.0f) ? r.target : prev + (r.target - prev) * m.adapt;
    return r;
}

// ---- the map ----
struct ToneCurve { uint32_t curve, gamma2; float white, w2; };   // w2 = white * white, the host's product

VRT_BOTH ToneCurve tone_curve_of(uint32_t curve, uint32_t flags, float white) {
    return ToneCurve{curve, (flags & kToneGamma2) ? 1u : 0u, white, white * white};
}

VRT_BOTH float tone_clamp01(float y) {
    const float m = (y > 0.0f) ? y : 0.0f;   // (a NaN: 0, as the quantisation's own clamp makes it)
    return m < 1.0f ? m : 1.0f;
}

// encode(curve(c * E)) of one colour channel: what the blit quantises in place of c
VRT_BOTH float tone_map_channel(const ToneCurve &t, float E, float c) {
    const float x = c * E;
    float y = x;
    if (t.curve == kToneReinhard) y = t.white != 0.0f ? (x * (1.0f + x / t.w2)) / (1.0f + x) : x / (1.0f + x);
    if (t.curve == kToneFilmic) y = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
    if (t.gamma2) y = sqrtf(tone_clamp01(y));
    return y;
}

}  // namespace vrt
