// worldgen.hpp — deterministic world generator and bottom-up SVO builder.
//
// Stands where the reference's server-side generator does (server/src/world/gen.rs:171-286: per-column
// terrain layers, water up to sea level, tree features), but is build-defined: the reference's generator
// cannot be reproduced even by itself (third-party Perlin + an unseeded global fastrand, gen.rs:11,263,274).
// Everything here is integer arithmetic on (seed, x, y, z), so every platform produces the same world — the GPU included, whose
// generator (vrt_gen.hip) compiles the same text: ../both/worldgen_math.h.
// The SVO is built bottom-up from a dense 32^3 block and laid out breadth-first: the root, its 8
// children and their 64 children occupy the first 73 node slots (146 B, two cache lines), which is what
// every ray's descent touches first.
#pragma once

#include <cstdint>
#include <vector>

#include "../both/worldgen_math.h"
#include "world.hpp"

namespace vrt {

// The generator over csrc/both/worldgen_math.h, where its arithmetic (mix .. tree_in_cell), its constants and the voxel ids are
// written once for this file and for vrt_gen.hip's kernel.
struct WorldGen {
    uint32_t seed = 1;
    using Tree = gen::Tree;

    int32_t height(int32_t x, int32_t z) const { return gen::height(seed, x, z); }
    uint16_t terrain_at(int32_t h, int32_t y) const { return (uint16_t)gen::terrain_at(h, y); }
    Tree tree_in_cell(int32_t cx16, int32_t cz16) const { return gen::tree_in_cell(seed, cx16, cz16); }

    // dense[x + 32*(y + 32*z)] for chunk cp; returns true if the block is uniform (value in dense[0])
    bool fill_dense(ChunkPos cp, uint16_t *dense) const {
        const int32_t x0 = cp.x * 32, y0 = cp.y * 32, z0 = cp.z * 32;
        for (int32_t z = 0; z < 32; z++)
            for (int32_t x = 0; x < 32; x++) {
                const int32_t h = height(x0 + x, z0 + z);
                for (int32_t y = 0; y < 32; y++) dense[x + 32 * (y + 32 * z)] = terrain_at(h, y0 + y);
            }
        for (int32_t cz = 0; cz < 2; cz++)
            for (int32_t cx = 0; cx < 2; cx++) {
                const Tree t = tree_in_cell((x0 >> 4) + cx, (z0 >> 4) + cz);
                if (!t.present) continue;
                const int32_t top = t.top;
                for (int32_t dy = -3; dy <= 3; dy++)
                    for (int32_t dz = -3; dz <= 3; dz++)
                        for (int32_t dx = -3; dx <= 3; dx++) {
                            if (dx * dx + dy * dy + dz * dz > 11) continue;
                            const int32_t x = t.x + dx - x0, y = top + dy - y0, z = t.z + dz - z0;
                            if (x < 0 || y < 0 || z < 0 || x >= 32 || y >= 32 || z >= 32) continue;
                            uint16_t &v = dense[x + 32 * (y + 32 * z)];
                            if (v == vox::AIR) v = vox::OAK_LEAVES;
                        }
                for (int32_t y = t.base + 1; y <= top; y++) {
                    const int32_t ly = y - y0;
                    if (ly < 0 || ly >= 32) continue;
                    dense[(t.x - x0) + 32 * (ly + 32 * (t.z - z0))] = vox::OAK_WOOD;
                }
            }
        bool uniform = true;
        for (int i = 1; i < 32 * 32 * 32 && uniform; i++) uniform = dense[i] == dense[0];
        return uniform;
    }
};

// Minimal octree of a dense 32^3 block (dense[x + 32*(y + 32*z)]), breadth-first node order, 8-blocks
// starting at index 1 exactly where NodeAlloc::new(0..1, 1..cap) would hand out its first block
// (server/src/world/gen.rs:177).  Returns false if the tree needs more than 32767 addressable nodes
// (the 15-bit child index, common/src/world/mod.rs:416).
inline bool build_svo_bottom_up(const uint16_t *dense, std::vector<Node> &out) {
    // level L has (1<<L)^3 cells; val >= 0: uniform voxel id, -1: mixed
    std::vector<int32_t> lv[6];
    lv[5].resize(32768);
    for (int i = 0; i < 32768; i++) lv[5][i] = dense[i];
    for (int L = 4; L >= 0; L--) {
        const int n = 1 << L, c = n * 2;
        lv[L].resize((size_t)n * n * n);
        for (int z = 0; z < n; z++)
            for (int y = 0; y < n; y++)
                for (int x = 0; x < n; x++) {
                    const int32_t first = lv[L + 1][(2 * x) + c * ((2 * y) + c * (2 * z))];
                    int32_t v = first;
                    for (int k = 1; k < 8 && v >= 0; k++) {
                        const int32_t ch = lv[L + 1][(2 * x + (k & 1)) + c * ((2 * y + ((k >> 1) & 1)) + c * (2 * z + (k >> 2)))];
                        if (ch != first) v = -1;
                    }
                    lv[L][x + n * (y + n * z)] = v;
                }
    }
    struct Item { uint8_t L, x, y, z; uint32_t idx; };
    std::vector<Item> q;
    q.push_back({0, 0, 0, 0, 0});
    out.assign(1, Node());
    for (size_t head = 0; head < q.size(); head++) {
        const Item it = q[head];
        const int n = 1 << it.L;
        const int32_t v = lv[it.L][it.x + n * (it.y + n * it.z)];
        if (v >= 0) { out[it.idx] = Node::make(Voxel((uint16_t)v)); continue; }
        const uint32_t base = (uint32_t)out.size();
        if (base + 8 > 32767u) return false;
        out.resize(base + 8);
        out[it.idx] = Node::new_split((uint16_t)base);
        for (uint32_t k = 0; k < 8; k++)
            q.push_back({(uint8_t)(it.L + 1), (uint8_t)(2 * it.x + (k & 1)), (uint8_t)(2 * it.y + ((k >> 1) & 1)),
                         (uint8_t)(2 * it.z + (k >> 2)), base + k});
    }
    return true;
}

// The reference's way (gen.rs:171-286 reduced to its SVO loop): NodeAlloc::new(0..1, 1..cap), then
// Svo::set_node for x, then z, then y ascending, skipping air. Returns nodes in use (last_used_addr+1), 0 on OOM.
inline uint32_t build_svo_by_set_node(const uint16_t *dense, Node *nodes, uint32_t cap) {
    NodeAlloc alloc({0, 1}, {1, cap});
    for (uint32_t i = 0; i < cap; i++) nodes[i] = Node();
    const Svo svo{0, CHUNK_SIZE};
    for (uint32_t x = 0; x < 32; x++)
        for (uint32_t z = 0; z < 32; z++)
            for (uint32_t y = 0; y < 32; y++) {
                const uint16_t v = dense[x + 32 * (y + 32 * z)];
                if (v == 0) continue;
                if (svo.set_node(nodes, {x, y, z}, Voxel(v), CHUNK_DEPTH, alloc) != SetVoxelErr::Ok) return 0;
            }
    return alloc.last_used_addr + 1;
}

// "Superflat" rule (stdrespack/world_gen.ron:214-249: height 12, layers grass x1 / dirt x3, earth
// limestone): y <= 8 limestone, 9..11 dirt, 12 grass, in world coordinates.
inline void fill_dense_superflat(ChunkPos cp, uint16_t *dense) {
    for (int32_t z = 0; z < 32; z++)
        for (int32_t y = 0; y < 32; y++) {
            const int32_t wy = cp.y * 32 + y;
            const uint16_t v = wy <= 8 ? vox::LIMESTONE : (wy <= 11 ? vox::DIRT : (wy == 12 ? vox::GRASS : vox::AIR));
            for (int32_t x = 0; x < 32; x++) dense[x + 32 * (y + 32 * z)] = v;
        }
}

}  // namespace vrt
