// vrt_edit.hip — vrt_edit_chunks: the server's feature shapes (server/src/world/gen.rs:312-354) onto chunks that exist, for a
// batch of chunks, one workgroup per chunk.  The specification is the host mirror's vrth_edit_chunks (host_capi.cpp):
// vrth_svo_to_dense -> the shapes in order -> build_svo_bottom_up.  This file is the middle of that:
//  - expand_chunks_kernel writes a chunk's 32^3 block into its slot of d_gen_dense, level by level from the root: the words of
//    levels 0..4 go to LDS in Morton order (the children of cell c are cells 8c .. 8c + 7, child k = x | y<<1 | z<<2, as in a
//    node's 8-block), a cell below a leaf repeating the leaf, so no voxel walks the tree again; the voxels are then written in the
//    block's own order, 4 to a lane.  Every node read is checked against the chunk's own length (a word past it reads 0, the
//    cast kernel's rule) and a word at depth 5 is a voxel whatever its top bit says (find_node's max_depth), so no input can
//    make the kernel read outside its buffers; that the tree is well-formed is the host's check (host/edit_check.hpp).
//  - apply_shapes_kernel runs the chunk's bin — the shapes whose box meets the chunk, in call order (the host makes the bins:
//    edit_check.hpp) — with a workgroup barrier between shapes, lanes over the voxels of box ∩ chunk alone; a line is walked by
//    one lane (both/shape_math.h's walker is sequential, and at most 4097 voxels long).  It ends by expanding the input tree
//    once more and comparing: changed[i].
//  - vrt_gen.hip's builder, scan and gather then run unchanged on the blocks (vrt_ctx.h gen_build_device_blocks).
// The voxel sets are the mirror's because they are the same text: both/shape_math.h.
#include "vrt_ctx.h"
#include "both/shape_math.h"
#include "host/edit_check.hpp"

namespace vrt {

namespace {

constexpr uint32_t kEditBlock = 256;
constexpr uint32_t kEditBatch = 2048;     // vrt_gen.hip's kGenBatch: the slots of d_gen_dense
constexpr uint32_t kEditLvWords = 4681;   // levels 0..4: 1 + 8 + 64 + 512 + 4096

struct EditChunk {
    int32_t x0, y0, z0;    // the chunk's first voxel
    uint32_t node_off;     // its tree in the batch's nodes
    uint32_t node_len;
    uint32_t bin_off;      // its shapes in the call's bins
    uint32_t bin_cnt;
    uint32_t _pad;
};

struct EditParams {
    const EditChunk *chunks;
    const uint16_t *nodes;
    const vrt_shape *shapes;
    const uint16_t *bins;
    uint16_t *dense;       // 32768 per chunk
    uint8_t *changed;
};

__host__ __device__ constexpr uint32_t edit_lv_off(uint32_t L) { return ((1u << (3u * L)) - 1u) / 7u; }   // 0, 1, 9, 73, 585

__device__ __forceinline__ uint32_t edit_node(const uint16_t *nodes, uint32_t len, uint32_t idx) { return idx < len ? nodes[idx] : 0u; }

// The words of levels 0..4 (Morton order) into lv; ends on a barrier
__device__ __forceinline__ void expand_levels(const uint16_t *nodes, uint32_t len, uint16_t *lv, uint32_t tid) {
    if (tid == 0u) lv[0] = (uint16_t)edit_node(nodes, len, 0u);
    __syncthreads();
    for (uint32_t L = 1; L <= 4u; L++) {
        const uint32_t n = 1u << (3u * L);
        for (uint32_t c = tid; c < n; c += kEditBlock) {
            const uint32_t pw = lv[edit_lv_off(L - 1u) + (c >> 3)];
            lv[edit_lv_off(L) + c] = (uint16_t)((pw & 0x8000u) ? edit_node(nodes, len, (pw & 0x7FFFu) + (c & 7u)) : pw);
        }
        __syncthreads();
    }
}

// A coordinate of a level-4 cell (4 bits) -> its bits of the Morton index, x's place
__device__ __forceinline__ uint32_t spread4(uint32_t v) { return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4) | ((v & 8u) << 6); }

// Voxels (4 q', y, z) .. (4 q' + 3, y, z) of the input tree, q = q' + 8 (y + 32 z): the two words at dense[4 q]
__device__ __forceinline__ uint2 expand_run(const uint16_t *nodes, uint32_t len, const uint16_t *lv, uint32_t q) {
    const uint32_t x = (q & 7u) * 4u, y = (q >> 3) & 31u, z = q >> 8;
    const uint32_t cyz = (spread4(y >> 1) << 1) | (spread4(z >> 1) << 2), k = ((y & 1u) << 1) | ((z & 1u) << 2);
    uint32_t w[2];
    for (uint32_t j = 0; j < 2u; j++) {
        const uint32_t pw = lv[edit_lv_off(4) + (spread4((x >> 1) + j) | cyz)];
        uint32_t v0 = pw, v1 = pw;
        if (pw & 0x8000u) {
            const uint32_t base = (pw & 0x7FFFu) + k;
            v0 = edit_node(nodes, len, base) & 0x7FFFu;        // depth 5: a voxel, whatever its top bit
            v1 = edit_node(nodes, len, base + 1u) & 0x7FFFu;
        }
        w[j] = v0 | (v1 << 16);
    }
    return make_uint2(w[0], w[1]);
}

__global__ __launch_bounds__(kEditBlock) void expand_chunks_kernel(EditParams P) {
    __shared__ uint16_t lv[kEditLvWords];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const EditChunk ch = P.chunks[b];
    const uint16_t *nodes = P.nodes + ch.node_off;
    expand_levels(nodes, ch.node_len, lv, tid);
    uint2 *out = reinterpret_cast<uint2 *>(P.dense + (size_t)b * 32768u);
    for (uint32_t it = 0; it < 32u; it++) {
        const uint32_t q = it * kEditBlock + tid;
        out[q] = expand_run(nodes, ch.node_len, lv, q);
    }
}

__global__ __launch_bounds__(kEditBlock) void apply_shapes_kernel(EditParams P) {
    __shared__ uint16_t lv[kEditLvWords];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const EditChunk ch = P.chunks[b];
    uint16_t *dense = P.dense + (size_t)b * 32768u;
    for (uint32_t i = 0; i < ch.bin_cnt; i++) {
        const vrt_shape s = P.shapes[P.bins[ch.bin_off + i]];
        const uint16_t v = (uint16_t)s.voxel;
        if (s.kind == kShapePoint || s.kind == kShapeLine) {
            if (tid == 0u) {
                auto put = [&](int32_t x, int32_t y, int32_t z) {
                    const uint32_t lx = (uint32_t)(x - ch.x0), ly = (uint32_t)(y - ch.y0), lz = (uint32_t)(z - ch.z0);
                    if (lx < 32u && ly < 32u && lz < 32u) dense[lx + 32u * (ly + 32u * lz)] = v;
                };
                if (s.kind == kShapePoint) {
                    put(s.a[0], s.a[1], s.a[2]);
                } else {
                    LineWalk w = line_begin(s);
                    do put(w.x, w.y, w.z);
                    while (line_next(w));
                }
            }
        } else {
            ShapeBox bx = shape_box(s);
            if (shape_box_clip(bx, ch.x0, ch.y0, ch.z0)) {   // (else the bin was generous: nothing to do)
                const uint32_t nx = (uint32_t)(bx.hi[0] - bx.lo[0] + 1), ny = (uint32_t)(bx.hi[1] - bx.lo[1] + 1),
                               nz = (uint32_t)(bx.hi[2] - bx.lo[2] + 1);
                const uint32_t total = nx * ny * nz;   // <= 32768
                const float r2 = s.r * s.r;
                for (uint32_t t = tid; t < total; t += kEditBlock) {
                    const uint32_t u = t / nx;
                    const int32_t x = bx.lo[0] + (int32_t)(t - u * nx), y = bx.lo[1] + (int32_t)(u % ny), z = bx.lo[2] + (int32_t)(u / ny);
                    if (shape_within(s.a[0], s.a[1], s.a[2], r2, x, y, z))
                        dense[(uint32_t)(x - ch.x0) + 32u * ((uint32_t)(y - ch.y0) + 32u * (uint32_t)(z - ch.z0))] = v;
                }
            }
        }
        __syncthreads();   // the next shape overwrites this one's voxels
    }
    // changed: the block against the input tree's voxels, after all shapes
    const uint16_t *nodes = P.nodes + ch.node_off;
    expand_levels(nodes, ch.node_len, lv, tid);
    const uint2 *now = reinterpret_cast<const uint2 *>(dense);
    uint32_t diff = 0;
    for (uint32_t it = 0; it < 32u; it++) {
        const uint32_t q = it * kEditBlock + tid;
        const uint2 was = expand_run(nodes, ch.node_len, lv, q), is = now[q];
        diff |= (was.x ^ is.x) | (was.y ^ is.y);
    }
    const int any = __syncthreads_or(diff != 0u);
    if (tid == 0u) P.changed[b] = any ? 1 : 0;
}

static_assert(sizeof(vrt_shape) == 40 && sizeof(EditChunk) == 32, "the records the kernels read");

// What one call carries from batch to batch (gen_build_device_blocks's fill_arg)
struct EditCall {
    const int32_t *pos;
    const uint16_t *nodes_in;
    const uint64_t *offs_in;
    const EditBins *bins;
    uint8_t *changed;
    std::vector<EditChunk> recs;   // the batch's records (alive until the batch's wait)
};

// One batch: its trees and records up, the two kernels, its changed flags down (they arrive with the builder's offsets)
int edit_fill(vrt_ctx *c, void *arg, uint32_t b0, uint32_t nb) {
    EditCall &E = *static_cast<EditCall *>(arg);
    hipStream_t st = c->stream;
    const uint64_t first = E.offs_in[b0], words = E.offs_in[b0 + nb] - first;
    // (the batch before has been waited for: nothing reads the old buffer)
    if (words > c->d_edit_nodes.cap()) HIP_TRY(c, c->d_edit_nodes.grow(std::max<uint64_t>(words, 1ull << 20)));
    E.recs.resize(nb);
    for (uint32_t i = 0; i < nb; i++) {
        const uint32_t g = b0 + i;
        EditChunk &r = E.recs[i];
        r.x0 = E.pos[3ull * g] * 32;
        r.y0 = E.pos[3ull * g + 1] * 32;
        r.z0 = E.pos[3ull * g + 2] * 32;
        r.node_off = (uint32_t)(E.offs_in[g] - first);
        r.node_len = (uint32_t)(E.offs_in[g + 1] - E.offs_in[g]);
        r.bin_off = E.bins->start[g];
        r.bin_cnt = E.bins->start[g + 1] - E.bins->start[g];
        r._pad = 0;
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_edit_nodes, E.nodes_in + first, (size_t)words * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(c->d_edit_chunks, E.recs.data(), (size_t)nb * sizeof(EditChunk), hipMemcpyHostToDevice, st));
    EditParams P;
    P.chunks = reinterpret_cast<const EditChunk *>(c->d_edit_chunks.get());
    P.nodes = c->d_edit_nodes;
    P.shapes = c->d_edit_shapes;
    P.bins = c->d_edit_bins;
    P.dense = c->d_gen_dense;
    P.changed = c->d_edit_changed;
    expand_chunks_kernel<<<dim3(nb), dim3(kEditBlock), 0, st>>>(P);
    HIP_TRY(c, hipGetLastError());
    apply_shapes_kernel<<<dim3(nb), dim3(kEditBlock), 0, st>>>(P);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(E.changed + b0, c->d_edit_changed, (size_t)nb, hipMemcpyDeviceToHost, st));
    return VRT_OK;
}

}  // namespace

}  // namespace vrt

extern "C" {

int vrt_edit_chunks(vrt_ctx *c, const int32_t *chunk_pos, uint32_t n, const uint16_t *nodes_in, const uint64_t *offsets_in,
                    const vrt_shape *shapes, uint32_t m, uint16_t *nodes_out, uint64_t cap_nodes, uint64_t *offsets_out, uint8_t *changed) {
    using namespace vrt;
    GRP_ROOT(c, vrt_edit_chunks(d, chunk_pos, n, nodes_in, offsets_in, shapes, m, nodes_out, cap_nodes, offsets_out, changed));
    if (!c) return VRT_ERR_INVALID_ARG;
    EditBins bins;
    uint64_t index = 0;
    const EditFault f = edit_check(chunk_pos, n, nodes_in, offsets_in, shapes, m, nodes_out, cap_nodes, offsets_out, changed, bins, &index);
    if (f != EditFault::None)
        return fail(c, edit_fault_is_range(f) ? VRT_ERR_OUT_OF_RANGE : VRT_ERR_INVALID_ARG, "vrt_edit_chunks: %s %llu", edit_fault_text(f),
                    (unsigned long long)index);
    if (n == 0u) {
        offsets_out[0] = 0;
        return VRT_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIP_TRY(c, c->d_edit_chunks.once((size_t)kEditBatch * sizeof(EditChunk)));
    HIP_TRY(c, c->d_edit_changed.once(kEditBatch));
    // (every earlier call has waited for its work)
    if (m > c->d_edit_shapes.cap()) HIP_TRY(c, c->d_edit_shapes.grow(std::max(m, 1024u)));
    if (bins.list.size() > c->d_edit_bins.cap()) HIP_TRY(c, c->d_edit_bins.grow(std::max<uint64_t>(bins.list.size(), 4096)));
    if (m) HIP_TRY(c, hipMemcpyAsync(c->d_edit_shapes, shapes, (size_t)m * sizeof(vrt_shape), hipMemcpyHostToDevice, st));
    if (!bins.list.empty())
        HIP_TRY(c, hipMemcpyAsync(c->d_edit_bins, bins.list.data(), bins.list.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    EditCall E;
    E.pos = chunk_pos;
    E.nodes_in = nodes_in;
    E.offs_in = offsets_in;
    E.bins = &bins;
    E.changed = changed;
    const int rc = gen_build_device_blocks(c, edit_fill, &E, n, nodes_out, cap_nodes, offsets_out, "vrt_edit_chunks");
    if (rc != VRT_OK) (void)hipStreamSynchronize(st);   // (a call that ended early: nothing may still read this call's host memory)
    return rc;
}

}  // extern "C"
