// refract_math.h — the arithmetic of vrt_set_water_refraction (include/vrt.h), once: the bend of a path that enters the water
// (A), the walk of a wet segment through the body of liquid to the face it leaves by (B) and the choice at that face (C).  The
// kernels of vrt_path_refract.h and host_capi.cpp's vrth_water_refract / vrth_world_water_span both compile this text.  Only f32
// add, subtract, multiply, divide and square root, each written once and in the contract's order; it relies on -ffp-contract=off
// on both sides and, on the device, on correctly rounded divide and square root (csrc/Makefile, both.h).
#pragma once
#include "both.h"
#include "cast_dda.h"

namespace vrt {

constexpr uint32_t kRefractSpanDefault = 64u, kRefractSpanMax = 1024u;   // max_span 0, and the most a setting may ask

// which way a path went at a water face
enum : int { kRefractEntered = 0, kRefractTotal = 1, kRefractMirrored = 2, kRefractLeft = 3 };

// the path kernels' vnormalize (oracle: orc_normalize): v / sqrt(dot(v, v)), the dot in vdot's order
VRT_BOTH void refract_normalize(float v[3]) {
    const float len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    v[0] = v[0] / len; v[1] = v[1] / len; v[2] = v[2] / len;
}

// A: the transmitted branch of a surface event.  eta = 1 / ior, norm the hit's face normal (it may be zero: normalize(eta * d))
VRT_BOTH void refract_enter(float eta, const float d[3], const float norm[3], float out[3]) {
    const float dn = norm[0] * d[0] + norm[1] * d[1] + norm[2] * d[2];
    const float c = fabsf(dn);
    const float s2 = (eta * eta) * (1.0f - c * c);
    const float ct = sqrtf(1.0f - s2);
    const float g = eta * c - ct;
    for (int k = 0; k < 3; k++) {
        const float nn = dn < 0.0f ? norm[k] : -norm[k];
        out[k] = eta * d[k] + g * nn;
    }
    refract_normalize(out);
}

// C: the underside event's direction.  n the face's normal, back into the water; u the event's draw.  Returns kRefractTotal,
// kRefractMirrored (out: the mirrored direction, as it is) or kRefractLeft (out: the bent one, normalised)
VRT_BOTH int refract_leave(float ior, float reflectance, const float d[3], const float n[3], float u, float out[3]) {
    const float dn = n[0] * d[0] + n[1] * d[1] + n[2] * d[2];
    const float c = fabsf(dn);
    const float s2 = (ior * ior) * (1.0f - c * c);
    int branch = kRefractTotal;
    float ct = 0.0f;
    if (s2 < 1.0f) {   // (a NaN: total)
        ct = sqrtf(1.0f - s2);
        const float mm = 1.0f - ct, m5 = (mm * mm) * (mm * mm) * mm;
        const float F = reflectance + (1.0f - reflectance) * m5;
        branch = u < F ? kRefractMirrored : kRefractLeft;
    }
    if (branch == kRefractLeft) {
        const float g = ior * c - ct;
        for (int k = 0; k < 3; k++) out[k] = ior * d[k] + g * n[k];
        refract_normalize(out);
    } else {
        for (int k = 0; k < 3; k++) out[k] = d[k] - 2.0f * n[k] * dn;
    }
    return branch;
}

// B: what the walk of a wet segment found
struct WaterSpan {
    float dist;                // the last step's dist
    int32_t prev[3], m[3];     // the voxel the walk ended in and the one before it
    uint32_t v;                // the voxel at m (a liquid of the table: the walk ran into max_span)
    uint32_t steps;            // the steps taken
    bool ended, event;         // the walk met a voxel that is no liquid within max_span steps; the underside event
};

// cast_ray's DDA (cast_dda.h) from o along d, at most max_span steps, to the first voxel that is not a liquid.  voxel_at(x, y, z):
// vrt_get_voxels' answer, 0 outside the world box and where there is no chunk; liquid(v): of the material table
template <class VoxelAt, class Liquid>
VRT_BOTH WaterSpan water_span(const float o[3], const float d[3], uint32_t max_span, VoxelAt voxel_at, Liquid liquid) {
    WaterSpan s;
    CastDda dda = cast_setup(o, d);
    s.dist = 0.0f; s.v = 0u; s.steps = 0u; s.ended = false;
    s.prev[0] = s.m[0] = dda.mx; s.prev[1] = s.m[1] = dda.my; s.prev[2] = s.m[2] = dda.mz;
    for (uint32_t i = 0; i < max_span && !s.ended; i++) {
        s.prev[0] = dda.mx; s.prev[1] = dda.my; s.prev[2] = dda.mz;
        s.dist = cast_step(dda);
        s.v = voxel_at(dda.mx, dda.my, dda.mz);
        s.ended = !liquid(s.v);
        s.steps = i + 1u;
    }
    s.m[0] = dda.mx; s.m[1] = dda.my; s.m[2] = dda.mz;
    s.event = s.ended && s.v == 0u && s.dist >= 0.0f && s.dist < INFINITY;
    return s;
}

}  // namespace vrt
