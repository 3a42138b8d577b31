// material.h — what the material table says of a voxel, once: host/collide.hpp's is_solid, vrt_clip.hip's clip_solid and
// both/column_top.h's solid set all compile this text.  The including file has include/vrt.h.
#pragma once
#include "both.h"

namespace vrt {

// voxelpack.get(v).is_solid() (common/src/resources/mod.rs:309) as the material table holds it: Material::construct
// (graphics/mod.rs:38-46) sets is_empty for Gas and is_liquid for Liquid; ids >= 255 share entry 255 as everywhere else
VRT_BOTH bool material_solid(const vrt_material *mats256, uint32_t v) {
    const vrt_material *m = &mats256[v < 255u ? v : 255u];
    return m->is_empty == 0u && m->is_liquid == 0u;
}

}  // namespace vrt
