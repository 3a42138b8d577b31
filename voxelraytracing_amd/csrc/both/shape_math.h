// shape_math.h — the voxel sets of the server's feature shapes (server/src/world/gen.rs:312-354: BuiltFeature::set_voxel,
// place_line, place_sphere, place_disc; common/src/math.rs:228-324: walk_line), once: the host mirror's vrth_apply_shapes and
// vrt_edit.hip's apply_shapes_kernel both compile this text.  A shape is include/vrt.h's vrt_shape (the functions are templates
// over it, as cast_dda.h's are over the hit record, so that nothing of the C ABI is included here).
//  - A sphere or disc takes p when d2 < r * r, d = ((float)p + 0.5f) - ((float)a + 0.5f) per axis and
//    d2 = (d.x * d.x + d.y * d.y) + d.z * d.z (fill_region_by_radius, gen.rs:324-340; glam's length_squared is dot(self, self)).
//    Every coordinate is below 2^22 + 2^15 in magnitude (shape_ok, kShapeCoordLimit), so (float)p + 0.5f is exact; the
//    products and sums round, and they round the same on both sides under -ffp-contract=off (both.h).
//  - A line is the reference's LineWalker: its state, and one step of it.
#pragma once
#include "both.h"

namespace vrt {

constexpr uint32_t kShapePoint = 0, kShapeLine = 1, kShapeSphere = 2, kShapeDisc = 3;   // VRT_SHAPE_*
constexpr int32_t kShapeCoordLimit = 1 << 22;   // |a|, |b|, |32 * chunk_pos| below this
constexpr int32_t kShapeLineMax = 4096;         // a line's largest dist
constexpr float kShapeRadiusLimit = 32768.0f;   // 0 <= r < this
constexpr uint32_t kShapeHeightMax = 32768;     // a disc's height

struct ShapeBox {
    int32_t lo[3], hi[3];   // inclusive; empty when hi < lo on an axis (a disc of height 0)
};

VRT_BOTH bool shape_coord_ok(int32_t v) { return v > -kShapeCoordLimit && v < kShapeCoordLimit; }

// What vrt_edit_chunks accepts of one shape (include/vrt.h)
template <class S>
VRT_BOTH bool shape_ok(const S &s) {
    if (s.kind > kShapeDisc || s.voxel > 0x7FFFu) return false;
    for (int i = 0; i < 3; i++)
        if (!shape_coord_ok(s.a[i])) return false;
    if (s.kind == kShapeLine)
        for (int i = 0; i < 3; i++) {
            if (!shape_coord_ok(s.b[i])) return false;
            const int32_t d = s.b[i] - s.a[i];
            if (d > kShapeLineMax || d < -kShapeLineMax) return false;
        }
    if (s.kind == kShapeSphere || s.kind == kShapeDisc)
        if (!(s.r >= 0.0f) || !(s.r < kShapeRadiusLimit)) return false;   // (a NaN fails both)
    if (s.kind == kShapeDisc && s.height > kShapeHeightMax) return false;
    return true;
}

// The box a shape's voxels lie in: the loops' own bounds for a sphere (gen.rs:344-345) and a disc (:351-352, `r as i32`
// truncates), the span of a and b for a line (each axis of the walker moves from a towards b and never past it).
template <class S>
VRT_BOTH ShapeBox shape_box(const S &s) {
    ShapeBox bx;
    const int32_t ri = (s.kind == kShapeSphere || s.kind == kShapeDisc) ? (int32_t)s.r : 0;
    for (int i = 0; i < 3; i++) {
        bx.lo[i] = s.a[i] - ri;
        bx.hi[i] = s.a[i] + ri;
        if (s.kind == kShapeLine) {
            bx.lo[i] = s.a[i] < s.b[i] ? s.a[i] : s.b[i];
            bx.hi[i] = s.a[i] < s.b[i] ? s.b[i] : s.a[i];
        }
    }
    if (s.kind == kShapeDisc) {
        bx.lo[1] = s.a[1];
        bx.hi[1] = s.a[1] + ((int32_t)s.height - 1);
    }
    return bx;
}

// bx cut to the 32^3 voxels from (x0, y0, z0): false when nothing is left
VRT_BOTH bool shape_box_clip(ShapeBox &bx, int32_t x0, int32_t y0, int32_t z0) {
    const int32_t o[3] = {x0, y0, z0};
    bool any = true;
    for (int i = 0; i < 3; i++) {
        if (bx.lo[i] < o[i]) bx.lo[i] = o[i];
        if (bx.hi[i] > o[i] + 31) bx.hi[i] = o[i] + 31;
        any = any && bx.lo[i] <= bx.hi[i];
    }
    return any;
}

// fill_region_by_radius's test for voxel (x, y, z) against the centre voxel (ax, ay, az); r2 = r * r
VRT_BOTH bool shape_within(int32_t ax, int32_t ay, int32_t az, float r2, int32_t x, int32_t y, int32_t z) {
    const float dx = ((float)x + 0.5f) - ((float)ax + 0.5f);
    const float dy = ((float)y + 0.5f) - ((float)ay + 0.5f);
    const float dz = ((float)z + 0.5f) - ((float)az + 0.5f);
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    return d2 < r2;
}

// LineWalker (math.rs:228-236) after walk_line set it up (:298-322): (x, y, z) is the voxel last given out, a at first
struct LineWalk {
    int32_t x, y, z;
    int32_t bx, by, bz;
    int32_t dx, dy, dz;   // dist
    int32_t sx, sy, sz;   // step: +1 towards a larger b, else -1 (also where they are equal: that axis then never moves)
    int32_t p1, p2;
    uint32_t mode;
};

template <class S>
VRT_BOTH LineWalk line_begin(const S &s) {
    LineWalk w;
    w.x = s.a[0]; w.y = s.a[1]; w.z = s.a[2];
    w.bx = s.b[0]; w.by = s.b[1]; w.bz = s.b[2];
    w.dx = w.bx > w.x ? w.bx - w.x : w.x - w.bx;
    w.dy = w.by > w.y ? w.by - w.y : w.y - w.by;
    w.dz = w.bz > w.z ? w.bz - w.z : w.z - w.bz;
    w.sx = w.bx > w.x ? 1 : -1;
    w.sy = w.by > w.y ? 1 : -1;
    w.sz = w.bz > w.z ? 1 : -1;
    if (w.dx >= w.dy && w.dx >= w.dz) {
        w.mode = 0u; w.p1 = 2 * w.dy - w.dx; w.p2 = 2 * w.dz - w.dx;
    } else if (w.dy >= w.dx && w.dy >= w.dz) {
        w.mode = 1u; w.p1 = 2 * w.dx - w.dy; w.p2 = 2 * w.dz - w.dy;
    } else {
        w.mode = 2u; w.p1 = 2 * w.dy - w.dz; w.p2 = 2 * w.dx - w.dz;   // p1 goes with y, p2 with x
    }
    return w;
}

// LineWalker::next (math.rs:240-292): false when the major axis has reached b, else (x, y, z) is the next voxel
VRT_BOTH bool line_next(LineWalk &w) {
    if (w.mode == 0u) {
        if (w.x == w.bx) return false;
        w.x += w.sx;
        if (w.p1 >= 0) { w.y += w.sy; w.p1 -= 2 * w.dx; }
        if (w.p2 >= 0) { w.z += w.sz; w.p2 -= 2 * w.dx; }
        w.p1 += 2 * w.dy;
        w.p2 += 2 * w.dz;
    } else if (w.mode == 1u) {
        if (w.y == w.by) return false;
        w.y += w.sy;
        if (w.p1 >= 0) { w.x += w.sx; w.p1 -= 2 * w.dy; }
        if (w.p2 >= 0) { w.z += w.sz; w.p2 -= 2 * w.dy; }
        w.p1 += 2 * w.dx;
        w.p2 += 2 * w.dz;
    } else {
        if (w.z == w.bz) return false;
        w.z += w.sz;
        if (w.p1 >= 0) { w.y += w.sy; w.p1 -= 2 * w.dz; }
        if (w.p2 >= 0) { w.x += w.sx; w.p2 -= 2 * w.dz; }
        w.p1 += 2 * w.dy;
        w.p2 += 2 * w.dx;
    }
    return true;
}

}  // namespace vrt
