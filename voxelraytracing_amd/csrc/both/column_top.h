// column_top.h — what the column queries (include/vrt.h: vrt_get_voxels, vrt_column_tops, vrt_read_top_map) are made of, once:
// which voxels count (solid ones are material.h's), where a scan starts and how its record is filled.  host/host_capi.cpp's
// vrth_world_column_top and vrt_column.hip's kernels both compile this text; each keeps its own loop over y around it — the host
// mirror's visits every voxel as ClientWorld::highest_vox_at does (client/src/world.rs:359-366), the kernels' jumps leaves.
// Only integer operations occur.  The including file has include/vrt.h.
#pragma once
#include "both.h"
#include "material.h"

namespace vrt {

// The solid set of a material table (material.h's material_solid, vrt_clip_moves's SOLID) as 256 bits, bit v of word v >> 5;
// null (no query asks for SOLID): the empty set
inline void solid_set(const vrt_material *mats256, uint32_t set[8]) {
    for (int w = 0; w < 8; w++) set[w] = 0u;
    if (!mats256) return;
    for (uint32_t v = 0; v < 256u; v++)
        if (material_solid(mats256, v)) set[v >> 5] |= 1u << (v & 31u);
}

// A voxel counts (include/vrt.h): never voxel 0; otherwise every voxel, or with VRT_COLUMN_SOLID the solid ones
VRT_BOTH bool column_counts(uint32_t v, uint32_t flags, const uint32_t set[8]) {
    if (v == 0u) return false;
    if (!(flags & VRT_COLUMN_SOLID)) return true;
    const uint32_t e = v < 255u ? v : 255u;
    return ((set[e >> 5] >> (e & 31u)) & 1u) != 0u;
}

// Where the scan of a column starts, as a world-local y in [0, W) (W = 32 S voxels above min_y): the top of the world, or with
// VRT_COLUMN_FROM_Y min(from_y, top).  False: from_y lies below the world and nothing is scanned.
VRT_BOTH bool column_start(uint32_t flags, int32_t from_y, int32_t min_y, uint32_t W, uint32_t &uy) {
    uy = W - 1u;
    if (!(flags & VRT_COLUMN_FROM_Y)) return true;
    if (from_y < min_y) return false;
    const uint32_t d = (uint32_t)from_y - (uint32_t)min_y;   // exact: from_y >= min_y
    if (d < uy) uy = d;
    return true;
}

// The three records
VRT_BOTH void column_found(vrt_column_top &r, int32_t min_y, uint32_t uy, uint32_t voxel) {
    r.y = (int32_t)((uint32_t)min_y + uy);
    r.voxel = voxel;
    r.status = VRT_COLUMN_FOUND;
    r._reserved = 0u;
}

VRT_BOTH void column_none(vrt_column_top &r, int32_t min_y) {
    r.y = (int32_t)((uint32_t)min_y - 1u);
    r.voxel = 0u;
    r.status = VRT_COLUMN_NONE;
    r._reserved = 0u;
}

VRT_BOTH void column_outside(vrt_column_top &r) {
    r.y = 0;
    r.voxel = 0u;
    r.status = VRT_COLUMN_OUTSIDE;
    r._reserved = 0u;
}

}  // namespace vrt
