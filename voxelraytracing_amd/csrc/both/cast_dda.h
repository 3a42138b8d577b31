// cast_dda.h — the parts of common::math::cast_ray (common/src/math.rs:153-226), once: host/host_capi.cpp's vrth_world_cast_ray
// and vrt_cast.hip's cast_rays_kernel both compile this text.  Each keeps its own loop around them, a dozen lines: the loop
// shared as a template over a probe of the world cost the kernel 1.9 % on long rays (profiles/host_device_shared_ab.txt).
// The DDA is the reference's text in strict binary32, every float operation in the order the reference writes it; it relies
// on -ffp-contract=off on both sides and, on the device, on correctly rounded divide and square root and on denormals kept
// (csrc/Makefile, both.h).
#pragma once
#include "both.h"

namespace vrt {

// Rejected (include/vrt.h): the reference loops forever on max_dist = inf, and start.floor().as_ivec3() / map_check += step leave
// i32 (or the exact integers of f32) beyond 2^24: such a query is not run.
VRT_BOTH bool cast_rejected(const float start[3], float max_dist) {
    return max_dist > 1048576.0f || !(fabsf(start[0]) < 16777216.0f) || !(fabsf(start[1]) < 16777216.0f) || !(fabsf(start[2]) < 16777216.0f);
}

// The state of math.rs:163-190: unit step sizes, the voxel, the step signs, the len of each axis
struct CastDda {
    float usx, usy, usz, lx, ly, lz;
    int32_t mx, my, mz, stx, sty, stz;
    bool x_frozen, z_frozen;
};

VRT_BOTH CastDda cast_setup(const float start[3], const float dir[3]) {
    CastDda d;
    const float sx0 = start[0], sy0 = start[1], sz0 = start[2];
    const float dx = dir[0], dy = dir[1], dz = dir[2];
    // math.rs:163-167, in the order written: ((1 + (b/a)*(b/a)) + (c/a)*(c/a)), correctly rounded / and sqrt
    d.usx = sqrtf(1.0f + (dy / dx) * (dy / dx) + (dz / dx) * (dz / dx));
    d.usy = sqrtf(1.0f + (dx / dy) * (dx / dy) + (dz / dy) * (dz / dy));
    d.usz = sqrtf(1.0f + (dx / dz) * (dx / dz) + (dy / dz) * (dy / dz));
    d.mx = (int32_t)floorf(sx0); d.my = (int32_t)floorf(sy0); d.mz = (int32_t)floorf(sz0);
    d.stx = dx < 0.0f ? -1 : 1; d.sty = dy < 0.0f ? -1 : 1; d.stz = dz < 0.0f ? -1 : 1;
    d.lx = dx < 0.0f ? (sx0 - (float)d.mx) * d.usx : ((float)(d.mx + 1) - sx0) * d.usx;
    d.ly = dy < 0.0f ? (sy0 - (float)d.my) * d.usy : ((float)(d.my + 1) - sy0) * d.usy;
    d.lz = dz < 0.0f ? (sz0 - (float)d.mz) * d.usz : ((float)(d.mz + 1) - sz0) * d.usz;
    // x and z move only in their own branch, which needs their len below the others': a len that starts NaN or +inf (it only
    // grows) keeps its axis where it is for the whole ray
    d.x_frozen = !(d.lx < INFINITY); d.z_frozen = !(d.lz < INFINITY);
    return d;
}

// One step of the loop (math.rs:192-206): the voxel moves along the axis whose len is lowest; returns the new dist
VRT_BOTH float cast_step(CastDda &d) {
    float dist;
    if (d.lx < d.ly && d.lx < d.lz) {
        d.mx += d.stx;
        dist = d.lx;
        d.lx += d.usx;
    } else if (d.lz < d.lx && d.lz < d.ly) {
        d.mz += d.stz;
        dist = d.lz;
        d.lz += d.usz;
    } else {
        d.my += d.sty;
        dist = d.ly;
        d.ly += d.usy;
    }
    return dist;
}

// The hit at d's voxel, entered from (px, py, pz) at dist, into a vrt_ray_hit's pos, face, dist
template <class Hit>
VRT_BOTH void cast_hit(Hit &r, const CastDda &d, int32_t px, int32_t py, int32_t pz, float dist) {
    r.pos[0] = d.mx; r.pos[1] = d.my; r.pos[2] = d.mz;
    r.face[0] = px - d.mx; r.face[1] = py - d.my; r.face[2] = pz - d.mz;
    const uint32_t nan = 0x7FC00000u;   // (one NaN for every platform: include/vrt.h)
    if (dist == dist) r.dist = dist;
    else memcpy(&r.dist, &nan, sizeof nan);
}

// The early miss, for a voxel outside the world (the cube of W voxels at wmin): true where no later step can bring the ray
// back.  Not in the reference, and no change to any result: an axis moves only by its own step (its sign fixed for the ray), so
// once the voxel is beyond the world on an axis whose step leads away from it — or on x / z, whose len is NaN or inf and
// which never move — every voxel still to come is outside, none collides, and the reference's loop ends in None whatever it
// does meanwhile (the NaN / inf branches included: only `dist` and the positions change there, and the result of a miss carries
// neither).  Inside the world it is false by construction, so asking it only outside is asking it after every miss.
// (World-local coordinates: outside <=> W or above as unsigned; |map| < 2^24 + 3 * 2^21, far from wrapping onto [0, W).)
VRT_BOTH bool cast_gone(const CastDda &d, const int32_t wmin[3], uint32_t W) {
    const uint32_t ux = (uint32_t)d.mx - (uint32_t)wmin[0], uy = (uint32_t)d.my - (uint32_t)wmin[1], uz = (uint32_t)d.mz - (uint32_t)wmin[2];
    const bool bx = (int64_t)d.mx < (int64_t)wmin[0], by = (int64_t)d.my < (int64_t)wmin[1], bz = (int64_t)d.mz < (int64_t)wmin[2];
    return (ux >= W && ((bx && (d.stx < 0 || d.x_frozen)) || (!bx && (d.stx > 0 || d.x_frozen)))) ||
           (uy >= W && ((by && d.sty < 0) || (!by && d.sty > 0))) ||
           (uz >= W && ((bz && (d.stz < 0 || d.z_frozen)) || (!bz && (d.stz > 0 || d.z_frozen))));
}

}  // namespace vrt
