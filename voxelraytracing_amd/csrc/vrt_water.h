// vrt_water.h — what the kernels of a frame with vrt_set_water_optics on share (vrt_path_water.h: the trace; vrt_denoise.hip: the
// guide words): whether a segment starts in a liquid, and the liquid set its march is given.
//
// march<> learns what a liquid is from two places: the 256-bit set in LDS (march_literal, march_fast, the general step of
// march_grid through is_liquid_ranged) and — march_grid only — FrameParams' liquid_is_range / liquid_lo / liquid_span, which its
// loop compares a voxel against before it ever asks the set.  A dry segment is marched with both empty: eight zero words, and the
// range the uploads keep for a material table without liquids (is_range 1, lo 2^31, span 0: no voxel id is in it; dry_params).  The derived
// tables a march reads (the cell grid, the bricks) hold voxel ids and leaf sizes and do not depend on the liquid set; the march
// cells and the sun marks do, and no kernel here reads either.  docs/KERNELS.md, "Water".
#pragma once

#include "vrt_march.h"

namespace vrt {

// The voxel at floor(o), o world-local, as vrt_get_voxels answers for it (vrt_column.hip: get_voxels_kernel over vrt_query.h's
// cast_voxel): 0 outside the world box (a NaN is outside), 0 where chunk_roots holds no chunk, else the cell grid's entry and the
// brick's — or, for a frame without the derived tables, find_node's walk from the chunk's root.
__device__ __forceinline__ uint32_t water_voxel_at(const FrameParams &P, V3 o) {
    const float fx = floorf(o.x), fy = floorf(o.y), fz = floorf(o.z);
    const float wmax = (float)P.world.size;
    if (!(fx >= 0.0f && fy >= 0.0f && fz >= 0.0f && fx < wmax && fy < wmax && fz < wmax)) return 0u;
    const uint32_t x = (uint32_t)fx, y = (uint32_t)fy, z = (uint32_t)fz;
    const uint32_t S = P.world.size_in_chunks;
    const uint32_t ch = (x >> 5) + S * ((y >> 5) + S * (z >> 5));
    const uint32_t root = ch < P.n_roots ? P.roots[ch] : 0u;
    if (root == 0u) return 0u;
    if (P.grid) {
        const uint32_t G1 = P.grid_dim + 1u;
        const uint32_t gi = ((z >> 2) * G1 + (y >> 2)) * G1 + (x >> 2);
        const uint32_t e = gi < P.grid_bytes / 4u ? P.grid[gi] : 0u;
        if (e >= kAirLeaf) return 0u;
        if (is_split_entry(e)) {
            const uint32_t i = (e & 0x7FFFFFFFu) + ((x & 3u) | ((y & 3u) << 2) | ((z & 3u) << 4));
            return i < P.brick_bytes / 2u ? (uint32_t)P.bricks[i] >> 1 : 0u;
        }
        return e >> 16;
    }
    auto node_at = [&](uint32_t idx) { return idx < P.n_nodes ? (uint32_t)P.nodes[idx] : 0u; };   // past the end: an air leaf, as in the march
    uint32_t node = node_at(root), depth = 0u;
    while ((node & 0x8000u) && depth < 5u) {
        const uint32_t sh = 4u - depth;
        const uint32_t sel = ((x >> sh) & 1u) | (((y >> sh) & 1u) << 1) | (((z >> sh) & 1u) << 2);
        node = node_at(root + (node & 0x7FFFu) + sel);
        depth += 1u;
    }
    return node & 0x7FFFu;
}

// The parameters a dry segment is marched with: the frame's own with the empty liquid set, as the uploads keep it for a material
// table without liquids.  A kernel argument of its own beside the frame's (the launchers make it): march_grid reads the range as
// scalar operands of its loop, which a kernel argument is and a struct patched inside the kernel is not.
inline FrameParams dry_params(const FrameParams &P) {
    FrameParams D = P;
    for (uint32_t &w : D.liquid) w = 0u;
    D.liquid_is_range = 1u;
    D.liquid_lo = 0x80000000u;
    D.liquid_span = 0u;
    return D;
}

}  // namespace vrt
