// aabb_clip.h — the Aabb arithmetic of the client's collisions (common/src/math.rs:3-115), once, axis by axis: host/collide.hpp's
// Aabb and vrt_clip.hip's clip_pass both compile this text.  Only f32 add, subtract and compare occur, in the reference's order;
// it relies on -ffp-contract=off on both sides (both.h): every operation is one correctly rounded binary32 operation.
#pragma once
#include "both.h"

namespace vrt {

constexpr float EPSILON = 0.00001f;  // math.rs:3

// What a box query may hold (include/vrt.h): beyond 2^23 the sums of expand and translate could leave the exact integers of f32
VRT_BOTH bool clip_in_range(float v) { return fabsf(v) < 8388608.0f; }

// The cap on get_collisions_w's loops, nx * ny * nz voxels, all positive (the reference would allocate without bound); the
// sides are differences of values below 2^24 + 2 in magnitude after clip_in_range
VRT_BOTH bool clip_range_over(int32_t nx, int32_t ny, int32_t nz, uint32_t cap) {
    return nx > (int32_t)cap || ny > (int32_t)cap || nz > (int32_t)cap || (uint64_t)nx * (uint64_t)ny * (uint64_t)nz > (uint64_t)cap;
}

// Aabb::expand, math.rs:18-44, on one axis
VRT_BOTH void aabb_expand(float &from, float &to, float a) {
    if (a < 0.0f) from += a;
    if (a > 0.0f) to += a;
}

// One of the two tests a clip_*_collide starts with (math.rs:51-56): boxes w and b overlap on this axis
VRT_BOTH bool aabb_overlap(float w_from, float w_to, float b_from, float b_to) { return !(b_to <= w_from || b_from >= w_to); }

// clip_{x,y,z}_collide after its two overlap tests (math.rs:58-70): the move a of b along this axis, stopped at w
VRT_BOTH float clip_axis(float a, float w_from, float w_to, float b_from, float b_to) {
    if (a > 0.0f && b_to <= w_from) {
        const float max = w_from - b_to - EPSILON;
        if (max < a) a = max;
    }
    if (a < 0.0f && b_from >= w_to) {
        const float max = w_to - b_from + EPSILON;
        if (max > a) a = max;
    }
    return a;
}

}  // namespace vrt
