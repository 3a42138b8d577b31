// collide.hpp — the client's collisions on the host: Aabb (common/src/math.rs:5-126), ClientWorld::get_collisions_w
// (client/src/world.rs:369-391) and clip_aabb_movement (client/src/player.rs:202-244), restated line for line over
// ClientWorld::get_voxel.  The CPU twin of vrt_clip_moves (include/vrt.h): same rejections, same record, and the same text for
// the Aabb arithmetic (../both/aabb_clip.h, which vrt_clip.hip compiles too); the list here and the kernel's fused walk stay apart.  Built with
// -ffp-contract=off (Makefile): every float operation is one correctly rounded binary32 operation, in the reference's order.
#pragma once
#include <cmath>
#include <vector>

#include "../both/aabb_clip.h"
#include "graphics.hpp"
#include "../both/material.h"

namespace vrt {

struct Aabb {  // math.rs:5-126, over ../both/aabb_clip.h's axes
    Vec3 from, to;

    Aabb expand(Vec3 a) const {
        Aabb r = *this;
        aabb_expand(r.from.x, r.to.x, a.x);
        aabb_expand(r.from.y, r.to.y, a.y);
        aabb_expand(r.from.z, r.to.z, a.z);
        return r;
    }
    Aabb translate(Vec3 a) const { return {{from.x + a.x, from.y + a.y, from.z + a.z}, {to.x + a.x, to.y + a.y, to.z + a.z}}; }

    bool overlap_x(const Aabb &c) const { return aabb_overlap(from.x, to.x, c.from.x, c.to.x); }
    bool overlap_y(const Aabb &c) const { return aabb_overlap(from.y, to.y, c.from.y, c.to.y); }
    bool overlap_z(const Aabb &c) const { return aabb_overlap(from.z, to.z, c.from.z, c.to.z); }
    float clip_x_collide(const Aabb &c, float a) const { return overlap_y(c) && overlap_z(c) ? clip_axis(a, from.x, to.x, c.from.x, c.to.x) : a; }
    float clip_y_collide(const Aabb &c, float a) const { return overlap_x(c) && overlap_z(c) ? clip_axis(a, from.y, to.y, c.from.y, c.to.y) : a; }
    float clip_z_collide(const Aabb &c, float a) const { return overlap_x(c) && overlap_y(c) ? clip_axis(a, from.z, to.z, c.from.z, c.to.z) : a; }
};

// voxelpack.get(voxel).is_solid() (common/src/resources/mod.rs:309) as the material table holds it: ../both/material.h's,
// the text the GPU's queries compile too
inline bool is_solid(const Material *mats256, Voxel v) { return material_solid(mats256, v.as_data()); }

// get_collisions_w, world.rs:369-391: the solid voxels' positions in gather order (each stands for Aabb [p, p + 1])
inline std::vector<VoxelPos> get_collisions_w(const ClientWorld &w, const Aabb &aabb, const Material *mats256) {
    std::vector<VoxelPos> out;
    const int32_t fx = (int32_t)std::floor(aabb.from.x), fy = (int32_t)std::floor(aabb.from.y), fz = (int32_t)std::floor(aabb.from.z);
    const int32_t tx = (int32_t)std::ceil(aabb.to.x), ty = (int32_t)std::ceil(aabb.to.y), tz = (int32_t)std::ceil(aabb.to.z);
    for (int32_t x = fx; x < tx; x++)
        for (int32_t y = fy; y < ty; y++)
            for (int32_t z = fz; z < tz; z++) {
                Voxel voxel;   // get_voxel(pos).unwrap_or(Voxel::EMPTY)
                if (w.get_voxel(VoxelPos{x, y, z}, voxel) != SetVoxelErr::Ok) voxel = Voxel();
                if (is_solid(mats256, voxel)) out.push_back(VoxelPos{x, y, z});
            }
    return out;
}

// get_collisions_w's loops for `aabb` would gather more than VRT_BOX_MAX_VOXELS voxels (every coordinate passed clip_in_range)
inline bool collisions_over_cap(const Aabb &aabb) {
    const int32_t nx = (int32_t)ceilf(aabb.to.x) - (int32_t)floorf(aabb.from.x), ny = (int32_t)ceilf(aabb.to.y) - (int32_t)floorf(aabb.from.y),
                  nz = (int32_t)ceilf(aabb.to.z) - (int32_t)floorf(aabb.from.z);
    return nx > 0 && ny > 0 && nz > 0 && clip_range_over(nx, ny, nz, VRT_BOX_MAX_VOXELS);   // an empty or inverted range: no boxes
}

// clip_aabb_movement, player.rs:202-244, with world = |bb| get_collisions_w(bb); the record is include/vrt.h's
inline void clip_aabb_movement(const ClientWorld &w, const Material *mats256, const vrt_box_query &q, vrt_box_move &r) {
    std::memset(&r, 0, sizeof r);
    r.status = VRT_BOX_REJECTED;
    for (int a = 0; a < 3; a++)
        if (!clip_in_range(q.from[a]) || !clip_in_range(q.to[a]) || !clip_in_range(q.mv[a])) return;
    Aabb bbox{{q.from[0], q.from[1], q.from[2]}, {q.to[0], q.to[1], q.to[2]}};
    const Vec3 mv{q.mv[0], q.mv[1], q.mv[2]};
    const bool autojump = (q.flags & VRT_BOX_AUTOJUMP) != 0u;
    if (collisions_over_cap(bbox.expand(mv))) return;   // (the reference would allocate without bound)

    auto to_aabb = [](VoxelPos p) {
        const Vec3 min{(float)p.x, (float)p.y, (float)p.z};
        return Aabb{min, {min.x + 1.0f, min.y + 1.0f, min.z + 1.0f}};
    };
    const std::vector<VoxelPos> world_bboxs = get_collisions_w(w, bbox.expand(mv), mats256);
    Vec3 mv_clipped = mv;
    for (const VoxelPos &p : world_bboxs) {
        const Aabb world_bbox = to_aabb(p);
        mv_clipped.y = world_bbox.clip_y_collide(bbox, mv_clipped.y);
        mv_clipped.x = world_bbox.clip_x_collide(bbox, mv_clipped.x);
        mv_clipped.z = world_bbox.clip_z_collide(bbox, mv_clipped.z);
    }
    const bool eq_x = mv_clipped.x == mv.x, eq_y = mv_clipped.y == mv.y, eq_z = mv_clipped.z == mv.z;
    r.flags = (eq_x ? 0u : VRT_BOX_CLIPPED_X) | (eq_y ? 0u : VRT_BOX_CLIPPED_Y) | (eq_z ? 0u : VRT_BOX_CLIPPED_Z);
    r.boxes[0] = (uint32_t)world_bboxs.size();

    if (autojump && (!eq_x || !eq_z)) {
        bbox = bbox.translate(Vec3{0.0f, 1.1f, 0.0f});
        const std::vector<VoxelPos> jump_bboxs = get_collisions_w(w, bbox.expand(mv), mats256);
        Vec3 jmp_clipped = mv;
        for (const VoxelPos &p : jump_bboxs) {
            const Aabb world_bbox = to_aabb(p);
            jmp_clipped.y = world_bbox.clip_y_collide(bbox, jmp_clipped.y);
            jmp_clipped.x = world_bbox.clip_x_collide(bbox, jmp_clipped.x);
            jmp_clipped.z = world_bbox.clip_z_collide(bbox, jmp_clipped.z);
        }
        jmp_clipped.y = 0.0f;
        r.boxes[1] = (uint32_t)jump_bboxs.size();
        if (std::fabs(jmp_clipped.x) > std::fabs(mv_clipped.x) || std::fabs(jmp_clipped.y) > std::fabs(mv_clipped.y) ||
            std::fabs(jmp_clipped.z) > std::fabs(mv_clipped.z)) {
            mv_clipped.y += 1.0f;
            mv_clipped.x = jmp_clipped.x;
            mv_clipped.z = jmp_clipped.z;
            r.flags |= VRT_BOX_STEPPED_UP;
        }
    }
    r.mv[0] = mv_clipped.x; r.mv[1] = mv_clipped.y; r.mv[2] = mv_clipped.z;
    r.status = VRT_BOX_MOVED;
}

}  // namespace vrt
