// worldgen_math.h — the world generator's arithmetic, once: host/worldgen.hpp's WorldGen (fill_dense) and vrt_gen.hip's
// gen_chunks_kernel both compile this text.  Everything is integer arithmetic on (seed, x, y, z), so it relies on no float flag of
// csrc/Makefile (both.h); it relies on >> of a negative int32 being arithmetic, which both compilers give.
#pragma once
#include "both.h"

namespace vrt {

// voxel ids from stdrespack/voxels.ron (index in the list = id)
namespace vox {
constexpr uint16_t AIR = 0, LAVA = 2, WATER = 3, LIMESTONE = 4, SLATE = 5, DIRT = 39, GRASS = 40, SNOW = 45,
                   SAND = 47, OAK_WOOD = 53, OAK_LEAVES = 62;
}

namespace gen {

constexpr int32_t kHMin = 40, kHMax = 200, kSeaLevel = 70, kSnowLine = 172;

VRT_BOTH uint32_t mix(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    // PCG-style output permutation over a 4-word key
    uint32_t h = a * 747796405u + 2891336453u;
    h = (h ^ b) * 277803737u; h ^= h >> 15;
    h = (h ^ c) * 2246822519u; h ^= h >> 13;
    h = (h ^ d) * 3266489917u; h ^= h >> 16;
    return h;
}
// lattice value in [0, 65535]
VRT_BOTH uint32_t lattice(uint32_t seed, int32_t ix, int32_t iz, uint32_t octave) { return mix(seed, (uint32_t)ix, (uint32_t)iz, octave) >> 16; }

// value noise at (x,z) with cell size `cell` (power of two), 16.16 fixed point result in [0, 65536); 64-bit smoothstep products
VRT_BOTH uint32_t value_noise(uint32_t seed, int32_t x, int32_t z, uint32_t cell_log2, uint32_t octave) {
    const int32_t ix = x >> cell_log2, iz = z >> cell_log2;  // floor for negatives too
    const uint32_t m = (1u << cell_log2) - 1u;
    const uint64_t tx = ((uint64_t)((uint32_t)x & m) << 16) >> cell_log2, tz = ((uint64_t)((uint32_t)z & m) << 16) >> cell_log2;
    const uint64_t sx = (tx * tx * (3u * 65536u - 2u * tx)) >> 32, sz = (tz * tz * (3u * 65536u - 2u * tz)) >> 32;  // smoothstep, 0..65536
    const uint64_t v00 = lattice(seed, ix, iz, octave), v10 = lattice(seed, ix + 1, iz, octave), v01 = lattice(seed, ix, iz + 1, octave),
                   v11 = lattice(seed, ix + 1, iz + 1, octave);
    const uint64_t a = (v00 * (65536u - sx) + v10 * sx) >> 16, b = (v01 * (65536u - sx) + v11 * sx) >> 16;
    return (uint32_t)((a * (65536u - sz) + b * sz) >> 16);
}

// terrain surface height at (x,z): y <= height is ground
VRT_BOTH int32_t height(uint32_t seed, int32_t x, int32_t z) {
    const uint64_t f = (8ull * value_noise(seed, x, z, 7, 0) + 4ull * value_noise(seed, x, z, 6, 1) + 2ull * value_noise(seed, x, z, 5, 2) +
                        1ull * value_noise(seed, x, z, 4, 3)) / 15ull;  // 0..65535
    // contrast stretch around the middle (x2.25), clamped
    int64_t g = ((int64_t)f - 32768) * 9 / 4 + 32768;
    if (g < 0) g = 0;
    if (g > 65535) g = 65535;
    return kHMin + (int32_t)(((int64_t)(kHMax - kHMin) * g) >> 16);
}

// terrain + water only (no trees); a voxel id, as the word the kernel packs two of
VRT_BOTH uint32_t terrain_at(int32_t h, int32_t y) {
    if (y > h) return y <= kSeaLevel ? vox::WATER : vox::AIR;
    // h - y in wrapping int32 (chunks within 6 of -2^26 in y see the wrap): spelled unsigned, where the wrap is defined
    const int32_t layer = (int32_t)((uint32_t)h - (uint32_t)y);
    if (layer == 0) return h <= kSeaLevel + 1 ? vox::SAND : (h >= kSnowLine ? vox::SNOW : vox::GRASS);
    if (layer <= 4) return h <= kSeaLevel + 1 ? vox::SAND : vox::DIRT;
    return vox::SLATE;
}

struct Tree { bool present; int32_t x, z, base, top; };   // the trunk stands on y = base + 1 .. top, the crown is centred on top
// one candidate tree per 16x16 cell; offsets 3..12 keep the radius-3 crown inside its cell
VRT_BOTH Tree tree_in_cell(uint32_t seed, int32_t cx16, int32_t cz16) {
    const uint32_t h = mix(seed ^ 0x9E3779B9u, (uint32_t)cx16, (uint32_t)cz16, 77u);
    Tree t;
    t.x = cx16 * 16 + 3 + (int32_t)((h >> 4) % 10u);
    t.z = cz16 * 16 + 3 + (int32_t)((h >> 12) % 10u);
    t.base = height(seed, t.x, t.z);
    t.top = t.base + 5 + (int32_t)((h >> 20) & 3u);   // a trunk of 5 .. 8
    t.present = (h & 3u) != 0u && t.base > kSeaLevel + 1 && t.base < kSnowLine - 8;
    return t;
}

}  // namespace gen

}  // namespace vrt
