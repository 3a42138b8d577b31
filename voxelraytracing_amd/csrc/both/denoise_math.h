// denoise_math.h — the edge-stopped à-trous filter of vrt_set_denoise (include/vrt.h; Dammertz et al. 2010), once: one output
// pixel of one pass, given a way to fetch a tap.  vrt_denoise.hip's kernels (taps from LDS or from the frame itself) and
// host_capi.cpp's vrth_denoise (taps from the caller's arrays) both compile this text.  Only f32 add, subtract, multiply and
// divide occur, in the order include/vrt.h states; it relies on -ffp-contract=off on both sides (both.h).
#pragma once
#include "both.h"

namespace vrt {

// the id word's bits (include/vrt.h VRT_ID_*; restated: a header of both/ includes nothing of the project)
constexpr uint32_t kDnHit = 1u << 16, kDnNX = 1u << 17, kDnNY = 1u << 18, kDnNZ = 1u << 19, kDnWater = 1u << 20;
constexpr uint32_t kDnKeyMask = 0x7FFFu | kDnHit | kDnNX | kDnNY | kDnNZ | kDnWater;
constexpr uint32_t kDnMaxPasses = 5u;

// Two pixels see the same surface when they agree on this and on the guide word
VRT_BOTH uint32_t denoise_key(uint32_t id) { return id & kDnKeyMask; }
// A pixel is filtered when its primary ray hit a face: everything else (sky, the eye inside a solid, a ray out of steps) is copied
VRT_BOTH bool denoise_filterable(uint32_t id) { return (id & kDnHit) != 0u && (id & (kDnNX | kDnNY | kDnNZ)) != 0u; }

// The guide word of a filterable pixel: the integer coordinate of the hit face's plane, from the hit position on the
// lowest-numbered axis whose normal bit is set (the position lies within rounding of the plane)
VRT_BOTH uint32_t denoise_guide(float pos_x, float pos_y, float pos_z, uint32_t id) {
    const float p = (id & kDnNX) ? pos_x : ((id & kDnNY) ? pos_y : pos_z);
    return (uint32_t)(int32_t)floorf(p + 0.5f);
}

// h = {1, 4, 6, 4, 1} / 16 (as a select: after unrolling a constant, and no array for a kernel to index)
VRT_BOTH float denoise_h(int t) { return t == 2 ? 0.375f : ((t == 1 || t == 3) ? 0.25f : 0.0625f); }

// The colour stop of pass i squared: sigma_color halves every pass
VRT_BOTH float denoise_sigma2(float sigma_color, uint32_t pass) {
    const float sg = sigma_color / (float)(1u << pass);
    return sg * sg;
}

struct DnColor { float r, g, b; };

#ifdef __HIPCC__
#define VRT_DN_UNROLL _Pragma("unroll")
#else
#define VRT_DN_UNROLL
#endif

// One filterable pixel p = (x, y) of a pass with tap spacing s.  fetch(qx, qy, c) says whether tap q is inside the traced
// area and agrees with p on key and guide, and then leaves its colour in c.  stop: sigma_color != 0 (sg2 from denoise_sigma2).
template <class Fetch>
VRT_BOTH DnColor denoise_pixel(Fetch &&fetch, int x, int y, int s, DnColor cp, bool stop, float sg2) {
    float sr = 0.0f, sgn = 0.0f, sb = 0.0f, wsum = 0.0f;
    VRT_DN_UNROLL
    for (int dy = -2; dy <= 2; dy++) {
        VRT_DN_UNROLL
        for (int dx = -2; dx <= 2; dx++) {
            DnColor cq;
            if (!fetch(x + s * dx, y + s * dy, cq)) continue;
            float w = denoise_h(dy + 2) * denoise_h(dx + 2);
            if (stop) {
                const float dr = cq.r - cp.r, dg = cq.g - cp.g, db = cq.b - cp.b;
                const float d2 = (dr * dr + dg * dg) + db * db;
                w = w * (sg2 / (sg2 + d2));
            }
            sr = sr + w * cq.r;
            sgn = sgn + w * cq.g;
            sb = sb + w * cq.b;
            wsum = wsum + w;
        }
    }
    return DnColor{sr / wsum, sgn / wsum, sb / wsum};
}

}  // namespace vrt
