// edit_check.hpp — what vrt_edit_chunks (vrt_edit.hip, host side) and its mirror vrth_edit_chunks (host_capi.cpp) do before any
// voxel is touched, in one text so that both refuse the same calls with the same status: the argument checks of include/vrt.h
// and the bins — for every chunk the shapes whose box (both/shape_math.h) meets its 32^3 voxels, in call order.
// Host code only (it allocates); includes nothing of the world mirror.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../both/shape_math.h"

namespace vrt {

constexpr uint32_t kEditMaxShapes = 65535;          // a bin entry is a u16 shape index
constexpr uint64_t kEditMaxPairs = 1ull << 20;      // (chunk, shape) pairs of one call
constexpr uint64_t kEditMaxTree = 32761;            // words of one input tree (the largest build_svo_bottom_up makes)

enum class EditFault : int {
    None = 0,
    Null,          // a pointer that is needed
    TooManyShapes, // m > kEditMaxShapes (VRT_ERR_OUT_OF_RANGE; every other fault is VRT_ERR_INVALID_ARG)
    Shape,         // shape `index` (shape_ok)
    ChunkPos,      // chunk `index`: 32 * chunk_pos outside (-2^22, 2^22)
    Offsets,       // chunk `index`: offsets_in decreasing, or a range that is empty or longer than kEditMaxTree
    Tree,          // chunk `index`: a child block that leaves the chunk's range, or a split node at depth 5
    TooManyPairs,  // more than kEditMaxPairs (VRT_ERR_OUT_OF_RANGE)
};

struct EditBins {
    std::vector<uint32_t> start;   // n + 1: chunk i's shapes are list[start[i] .. start[i + 1]), ascending
    std::vector<uint16_t> list;
};

// The BadChunkData rule of ClientWorld::create_chunk (world.hpp chunk_payload_ok: no child block may leave the payload) on the
// nodes a walk from node 0 can reach, and no split node where a voxel has to be (depth 5 = CHUNK_DEPTH: find_node would read its
// child index as a voxel id).  The walk is bounded by the depth, whatever the words are: at most 37449 nodes.
inline bool edit_tree_ok(const uint16_t *nodes, uint32_t len) {
    if (len == 0) return false;
    uint32_t stack[64], depth_of[64], top = 0;   // (at most 7 waiting per level above + 8)
    stack[top] = 0; depth_of[top++] = 0;
    while (top) {
        const uint32_t idx = stack[--top], d = depth_of[top];
        const uint16_t w = nodes[idx];
        if (!(w & 0x8000u)) continue;
        if (d == 5u) return false;
        const uint32_t first = w & 0x7FFFu;
        if (first + 8u > len) return false;
        for (uint32_t k = 0; k < 8u; k++) { stack[top] = first + k; depth_of[top++] = d + 1u; }
    }
    return true;
}

// Everything that rejects a call, and the bins when nothing does.  *index: the shape or chunk a fault names.
inline EditFault edit_check(const int32_t *chunk_pos, uint32_t n, const uint16_t *nodes_in, const uint64_t *offsets_in,
                            const void *shapes_v, uint32_t m, const void *nodes_out, uint64_t cap_nodes, const void *offsets_out,
                            const void *changed, EditBins &bins, uint64_t *index) {
    struct Shape { uint32_t kind, voxel; int32_t a[3], b[3]; float r; uint32_t height; };   // include/vrt.h vrt_shape
    const Shape *shapes = static_cast<const Shape *>(shapes_v);
    *index = 0;
    if (!offsets_out || (m && !shapes)) return EditFault::Null;
    if (n && (!chunk_pos || !nodes_in || !offsets_in || !changed || (cap_nodes && !nodes_out))) return EditFault::Null;
    if (m > kEditMaxShapes) return EditFault::TooManyShapes;
    for (uint32_t j = 0; j < m; j++)
        if (!shape_ok(shapes[j])) { *index = j; return EditFault::Shape; }
    constexpr int32_t kChunkLimit = kShapeCoordLimit / 32;
    for (uint32_t i = 0; i < n; i++) {
        *index = i;
        for (int a = 0; a < 3; a++)
            if (chunk_pos[3ull * i + a] <= -kChunkLimit || chunk_pos[3ull * i + a] >= kChunkLimit) return EditFault::ChunkPos;
    }
    for (uint32_t i = 0; i < n; i++) {
        *index = i;
        if (offsets_in[i + 1] <= offsets_in[i] || offsets_in[i + 1] - offsets_in[i] > kEditMaxTree) return EditFault::Offsets;
    }
    for (uint32_t i = 0; i < n; i++) {
        *index = i;
        if (!edit_tree_ok(nodes_in + offsets_in[i], (uint32_t)(offsets_in[i + 1] - offsets_in[i]))) return EditFault::Tree;
    }
    *index = 0;

    // the bins.  A shape whose box covers few chunk cells looks them up among the chunks sorted by position; one that covers
    // more cells than there are chunks is tested against every chunk.
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    auto pos_less = [&](const int32_t *p, const int32_t *q) {
        return p[2] != q[2] ? p[2] < q[2] : p[1] != q[1] ? p[1] < q[1] : p[0] < q[0];
    };
    std::sort(order.begin(), order.end(), [&](uint32_t p, uint32_t q) {
        const int32_t *a = chunk_pos + 3ull * p, *b = chunk_pos + 3ull * q;
        return pos_less(a, b) || (!pos_less(b, a) && p < q);
    });
    std::vector<std::pair<uint32_t, uint16_t>> pairs;   // (chunk, shape), shape ascending
    auto push = [&](uint32_t chunk, uint32_t shape) {
        pairs.emplace_back(chunk, (uint16_t)shape);
        return pairs.size() <= kEditMaxPairs;
    };
    for (uint32_t j = 0; j < m && n; j++) {
        const ShapeBox bx = shape_box(shapes[j]);
        if (bx.hi[0] < bx.lo[0] || bx.hi[1] < bx.lo[1] || bx.hi[2] < bx.lo[2]) continue;
        int32_t c0[3], c1[3];
        uint64_t cells = 1;
        for (int a = 0; a < 3; a++) {
            c0[a] = bx.lo[a] >> 5;   // (floor: the chunk of voxel -1 is chunk -1)
            c1[a] = bx.hi[a] >> 5;
            cells *= (uint64_t)(c1[a] - c0[a] + 1);
        }
        if (cells > n) {
            for (uint32_t i = 0; i < n; i++) {
                const int32_t *p = chunk_pos + 3ull * i;
                if (p[0] >= c0[0] && p[0] <= c1[0] && p[1] >= c0[1] && p[1] <= c1[1] && p[2] >= c0[2] && p[2] <= c1[2])
                    if (!push(i, j)) return EditFault::TooManyPairs;
            }
        } else {
            for (int32_t cz = c0[2]; cz <= c1[2]; cz++)
                for (int32_t cy = c0[1]; cy <= c1[1]; cy++)
                    for (int32_t cx = c0[0]; cx <= c1[0]; cx++) {
                        const int32_t key[3] = {cx, cy, cz};
                        auto it = std::lower_bound(order.begin(), order.end(), key,
                                                   [&](uint32_t p, const int32_t *k) { return pos_less(chunk_pos + 3ull * p, k); });
                        for (; it != order.end() && !pos_less(key, chunk_pos + 3ull * *it); ++it)   // (a position given twice)
                            if (!push(*it, j)) return EditFault::TooManyPairs;
                    }
        }
    }
    bins.start.assign((size_t)n + 1, 0u);
    for (const auto &p : pairs) bins.start[p.first + 1]++;
    for (uint32_t i = 0; i < n; i++) bins.start[i + 1] += bins.start[i];
    bins.list.resize(pairs.size());
    std::vector<uint32_t> at(bins.start.begin(), bins.start.end() - 1);
    for (const auto &p : pairs) bins.list[at[p.first]++] = p.second;   // pairs come shape by shape: each bin ascends
    return EditFault::None;
}

inline bool edit_fault_is_range(EditFault f) { return f == EditFault::TooManyShapes || f == EditFault::TooManyPairs; }

inline const char *edit_fault_text(EditFault f) {
    switch (f) {
        case EditFault::Null: return "a null pointer";
        case EditFault::TooManyShapes: return "more than 65535 shapes";
        case EditFault::Shape: return "a shape with an unknown kind, voxel > 0x7FFF, a coordinate outside (-2^22, 2^22), a line longer than 4096, "
                                      "r negative, NaN or >= 32768, or height > 32768: shape";
        case EditFault::ChunkPos: return "32 * chunk_pos outside (-2^22, 2^22): chunk";
        case EditFault::Offsets: return "offsets_in decreasing, or a range that is empty or longer than 32761: chunk";
        case EditFault::Tree: return "a tree whose child block leaves its range or that splits at depth 5: chunk";
        case EditFault::TooManyPairs: return "more than 2^20 (chunk, shape) pairs whose boxes intersect";
        default: return "";
    }
}

}  // namespace vrt
