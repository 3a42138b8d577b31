// vrt_gen.hip — vrt_generate_chunks / vrt_build_chunks: the build's world generator (host/worldgen.hpp WorldGen::fill_dense)
// and its bottom-up SVO builder (build_svo_bottom_up) for a batch of chunks, one workgroup per chunk, word for word.
//
// worldgen.hpp's fill_dense and build_svo_bottom_up are the specification of what stays apart: the walk over a chunk and the
// builder.  What the kernel relies on:
//  - Node order.  build_svo_bottom_up lays nodes out breadth-first, and the children of a cell come in k = x | y<<1 | z<<2
//    order, so each level is in Morton order.  A mixed level-L cell of global breadth-first rank r (mixed cells of levels
//    0..L-1, then its rank among the mixed cells of level L in Morton order) has its 8 children at 1 + 8 r.  A mixed cell's
//    ancestors are all mixed, so every child of a mixed cell has a node; the ranks are one exclusive scan of 75 ballot words
//    (level 0, 1, 2: one word each; level 3: 8; level 4: 64).
//  - The tree is refused (count 0) when it has 4096 mixed cells or more: 1 + 8 * 4095 = 32761 nodes is the largest tree whose
//    every 8-block ends below node 32767.
//  - Uniformity compares the full 16-bit id (0x0001 next to 0x8001 is a split whose leaves both read 1); a level cell holds a
//    16-bit id or kMixed = 0x10000, which no id equals.
//  - Every voxel of a generated chunk is a pure function of its column's height, its y and the one tree of its 16 x 16 cell:
//    a crown stays inside its cell, leaves replace only AIR, the trunk overwrites.  So no dense block is kept: the heights of the
//    32 x 32 columns go to LDS once, and each 2^3 block of voxels is made where it is needed (twice for a mixed level-4 cell: to
//    reduce it, and to write its 8 leaves).  The build kernel reads the caller's dense block the same way, from device memory.
//  - The arithmetic is WorldGen's because it is the same text: both/worldgen_math.h (heights, terrain_at, tree_in_cell and
//    their constants), compiled here and into the host mirror.
//
// The nodes of chunk b go to staging slot b (kGenSlot u16, node i at slot[7 + i], so every 8-block is 16-byte aligned) and its
// node count to counts[b]; a scan kernel and a gather kernel then compact the batch.
#include "vrt_ctx.h"
#include "both/worldgen_math.h"

#include <vector>

namespace vrt {

namespace {

constexpr uint32_t kGenBlock = 256;
constexpr uint32_t kGenBatch = 2048;             // chunks per batch (include/vrt.h); staging = kGenBatch * 64 KiB
constexpr uint32_t kGenSlot = 32768;             // u16 per staging slot
constexpr uint32_t kGenMaxMixed = 4095;          // most mixed cells a tree may have (32761 nodes)
constexpr uint32_t kMixed = 0x10000u;            // a level cell's value: a 16-bit voxel id, or mixed
constexpr uint32_t kLvCells = 4688;              // levels 0..4 at lv_off(L): 8-aligned, so 8 children are two 16-byte reads
constexpr uint32_t kWords = 75;                  // mixed-flag ballot words of levels 0..4, breadth-first order
constexpr int32_t kCoordLimit = 1 << 26;         // |chunk coordinate| below this: fill_dense's cp * 32 stays in int32

__host__ __device__ constexpr uint32_t lv_off(uint32_t L) { return L == 0 ? 0u : L == 1 ? 8u : L == 2 ? 16u : L == 3 ? 80u : 592u; }
__host__ __device__ constexpr uint32_t word_off(uint32_t L) { return L < 4 ? L : 11u; }

struct GenTree {
    int32_t present, lx, lz, base, top;   // lx, lz: chunk-local (a chunk's 2 x 2 cells hold its trees); base, top: world y
};

struct GenParams {
    const int32_t *pos;       // generate: x, y, z per chunk
    const uint16_t *dense;    // build: 32768 per chunk
    uint16_t *stage;          // kGenSlot per chunk
    uint32_t *counts;         // node count per chunk, 0 = refused
    uint32_t seed;
};

// The 8 voxels of level-4 cell (x4, y4, z4) as 4 words: word j = voxels k = 2j (low half) and 2j + 1 (high half),
// k = x | y<<1 | z<<2 — each word one x-pair of dense[x + 32*(y + 32*z)].
template <bool kGen>
__device__ __forceinline__ void cell_voxels(const uint16_t *dense, const int32_t *hgt, const GenTree *trees, int32_t y0,
                                            uint32_t x4, uint32_t y4, uint32_t z4, uint32_t w[4]) {
    if constexpr (!kGen) {
        const uint32_t *d32 = reinterpret_cast<const uint32_t *>(dense);
        for (uint32_t j = 0; j < 4; j++) w[j] = d32[(32u * ((2u * y4 + (j & 1u)) + 32u * (2u * z4 + (j >> 1))) + 2u * x4) >> 1];
    } else {
        const GenTree t = trees[(x4 >> 3) + 2u * (z4 >> 3)];
        for (uint32_t j = 0; j < 4; j++) {
            const int32_t ly = (int32_t)(2u * y4 + (j & 1u)), lz = (int32_t)(2u * z4 + (j >> 1));
            const int32_t wy = y0 + ly;
            uint32_t v2[2];
            for (uint32_t i = 0; i < 2; i++) {
                const int32_t lx = (int32_t)(2u * x4 + i);
                uint32_t v = gen::terrain_at(hgt[lz * 32 + lx], wy);
                if (t.present) {
                    const int32_t dx = lx - t.lx, dz = lz - t.lz;
                    const int64_t dy = (int64_t)wy - t.top;
                    if (dx == 0 && dz == 0 && wy > t.base && wy <= t.top) v = vox::OAK_WOOD;
                    else if (v == 0u && dy >= -3 && dy <= 3 && dx * dx + (int32_t)(dy * dy) + dz * dz <= 11) v = vox::OAK_LEAVES;
                }
                v2[i] = v;
            }
            w[j] = v2[0] | (v2[1] << 16);
        }
    }
}

__device__ __forceinline__ uint32_t mixed_rank(const unsigned long long *words, const uint32_t *prefix, uint32_t L, uint32_t c) {
    const uint32_t wi = word_off(L) + (c >> 6);
    return prefix[wi] + (uint32_t)__popcll(words[wi] & ((1ull << (c & 63u)) - 1ull));
}

__device__ __forceinline__ uint32_t node_word(const unsigned long long *words, const uint32_t *prefix, uint32_t L, uint32_t c, uint32_t v) {
    return v == kMixed ? 0x8000u | (1u + 8u * mixed_rank(words, prefix, L, c)) : v & 0x7FFFu;
}

// Level-4 Morton index c (12 bits, x lowest) -> cell coordinates
__device__ __forceinline__ uint32_t morton_axis(uint32_t c) {
    return (c & 1u) | ((c >> 2) & 2u) | ((c >> 4) & 4u) | ((c >> 6) & 8u);
}

template <bool kGen>
__global__ __launch_bounds__(kGenBlock) void gen_chunks_kernel(GenParams P) {
    __shared__ __attribute__((aligned(16))) uint32_t lv[kLvCells];
    __shared__ unsigned long long words[kWords];
    __shared__ uint32_t prefix[kWords + 1];
    __shared__ int32_t hgt[kGen ? 1024 : 1];
    __shared__ GenTree trees[4];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const uint16_t *dense = nullptr;
    int32_t y0 = 0;
    if constexpr (kGen) {
        const int32_t x0 = P.pos[3u * b] * 32, z0 = P.pos[3u * b + 2u] * 32;   // |pos| < 2^26 (checked on the host)
        y0 = P.pos[3u * b + 1u] * 32;
        for (uint32_t i = tid; i < 1024u; i += kGenBlock) hgt[i] = gen::height(P.seed, x0 + (int32_t)(i & 31u), z0 + (int32_t)(i >> 5));
        if (tid < 4u) {   // the trees of the chunk's 2 x 2 cells, cell cx + 2 cz (fill_dense's loop)
            const gen::Tree g = gen::tree_in_cell(P.seed, (x0 >> 4) + (int32_t)(tid & 1u), (z0 >> 4) + (int32_t)(tid >> 1));
            GenTree t;
            t.base = g.base;
            t.top = g.top;
            t.present = g.present;
            t.lx = g.x - x0;
            t.lz = g.z - z0;
            trees[tid] = t;
        }
        __syncthreads();
    } else {
        dense = P.dense + (size_t)b * 32768u;
    }

    // level 4 from the voxels: wave w of pass it covers Morton cells [256 it + 64 w, + 64), one ballot word
#pragma unroll 4
    for (uint32_t it = 0; it < 16u; it++) {
        const uint32_t c = it * kGenBlock + tid;
        uint32_t w[4];
        cell_voxels<kGen>(dense, hgt, trees, y0, morton_axis(c), morton_axis(c >> 1), morton_axis(c >> 2), w);
        const bool uni = w[0] == w[1] && w[0] == w[2] && w[0] == w[3] && (w[0] & 0xFFFFu) == (w[0] >> 16);
        lv[lv_off(4) + c] = uni ? (w[0] & 0xFFFFu) : kMixed;
        const unsigned long long m = __ballot(!uni);
        if ((tid & 63u) == 0u) words[word_off(4) + (c >> 6)] = m;
    }
    __syncthreads();
    // levels 3..0, each from the one below: children of cell c are cells 8c .. 8c + 7
    for (int L = 3; L >= 0; L--) {
        const uint32_t n = 1u << (3 * L);
        for (uint32_t c = tid; c < n; c += kGenBlock) {
            const uint4 a = *reinterpret_cast<const uint4 *>(&lv[lv_off(L + 1) + 8u * c]);
            const uint4 d = *reinterpret_cast<const uint4 *>(&lv[lv_off(L + 1) + 8u * c + 4u]);
            const bool mixed = a.x == kMixed || a.y != a.x || a.z != a.x || a.w != a.x || d.x != a.x || d.y != a.x || d.z != a.x ||
                               d.w != a.x;
            lv[lv_off(L) + c] = mixed ? kMixed : a.x;
            const unsigned long long m = __ballot(mixed);   // (lanes past n are inactive: their bits are 0)
            if ((c & 63u) == 0u) words[word_off(L) + (c >> 6)] = m;
        }
        __syncthreads();
    }
    // breadth-first ranks: exclusive scan of the words' popcounts (64 + 11 words, on wave 0)
    if (tid < 64u) {
        const uint32_t a = (uint32_t)__popcll(words[tid]), e = tid < kWords - 64u ? (uint32_t)__popcll(words[64u + tid]) : 0u;
        uint32_t sa = a, se = e;
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t ya = __shfl_up(sa, d), ye = __shfl_up(se, d);
            if (tid >= d) { sa += ya; se += ye; }
        }
        const uint32_t A = __shfl(sa, 63);
        prefix[tid] = sa - a;
        if (tid < kWords - 64u) prefix[64u + tid] = A + se - e;
        if (tid == kWords - 64u - 1u) prefix[kWords] = A + se;
    }
    __syncthreads();
    const uint32_t M = prefix[kWords];
    if (M > kGenMaxMixed) {   // build_svo_bottom_up refuses it (an allocation past node 32767)
        if (tid == 0u) P.counts[b] = 0u;
        return;
    }
    if (tid == 0u) P.counts[b] = 1u + 8u * M;
    uint16_t *slot = P.stage + (size_t)b * kGenSlot;   // node i at slot[7 + i]; a mixed cell of rank r writes slot[8 (r + 1) ..][8]
    if (tid == 0u) slot[7] = (uint16_t)node_word(words, prefix, 0, 0, lv[0]);
    for (uint32_t L = 0; L < 4u; L++) {
        const uint32_t n = 1u << (3 * L);
        for (uint32_t c = tid; c < n; c += kGenBlock) {
            if (lv[lv_off(L) + c] != kMixed) continue;
            const uint32_t r = mixed_rank(words, prefix, L, c);
            uint32_t o[4];
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t k = 8u * c + 2u * j;
                o[j] = node_word(words, prefix, L + 1, k, lv[lv_off(L + 1) + k]) |
                       (node_word(words, prefix, L + 1, k + 1u, lv[lv_off(L + 1) + k + 1u]) << 16);
            }
            if (r < kGenMaxMixed) *reinterpret_cast<uint4 *>(slot + 8u * (r + 1u)) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
    for (uint32_t it = 0; it < 16u; it++) {
        const uint32_t c = it * kGenBlock + tid;
        if (lv[lv_off(4) + c] != kMixed) continue;
        const uint32_t r = mixed_rank(words, prefix, 4, c);
        uint32_t w[4];
        cell_voxels<kGen>(dense, hgt, trees, y0, morton_axis(c), morton_axis(c >> 1), morton_axis(c >> 2), w);
        if (r < kGenMaxMixed)
            *reinterpret_cast<uint4 *>(slot + 8u * (r + 1u)) = make_uint4(w[0] & 0x7FFF7FFFu, w[1] & 0x7FFF7FFFu, w[2] & 0x7FFF7FFFu,
                                                                          w[3] & 0x7FFF7FFFu);
    }
}

// offs[i] = counts[0] + .. + counts[i - 1], i = 0 .. n (n <= kGenBatch), one workgroup
__global__ __launch_bounds__(1024) void gen_scan_kernel(const uint32_t *counts, uint32_t n, uint64_t *offs) {
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x, per = (n + 1023u) / 1024u;
    const uint32_t lo = min(t * per, n), hi = min(lo + per, n);
    uint64_t s = 0;
    for (uint32_t i = lo; i < hi; i++) s += counts[i];
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint64_t y = t >= d ? part[t - d] : 0ull;
        __syncthreads();
        part[t] += y;
        __syncthreads();
    }
    uint64_t run = part[t] - s;
    for (uint32_t i = lo; i < hi; i++) {
        offs[i] = run;
        run += counts[i];
    }
    if (t == 1023u) offs[n] = part[1023];
}

// chunk b's nodes: stage slot b -> out[offs[b] ..)
__global__ __launch_bounds__(kGenBlock) void gen_gather_kernel(const uint16_t *stage, const uint32_t *counts, const uint64_t *offs,
                                                              uint16_t *out) {
    const uint32_t b = blockIdx.x;
    const uint32_t cnt = min(counts[b], kGenSlot - 7u);
    const uint16_t *src = stage + (size_t)b * kGenSlot + 7u;
    uint16_t *dst = out + offs[b];
    for (uint32_t i = threadIdx.x; i < cnt; i += kGenBlock) dst[i] = src[i];
}

}  // namespace

}  // namespace vrt

// One call: the chunks in batches of kGenBatch on c->stream.  Per batch: inputs up, the builder, the scan, the offsets down
// (the one wait), then — while everything so far fits in cap_nodes — the gather into d_gen_out.  The nodes come down once, at
// the end, and only if all of them fit: on VRT_ERR_OOM `nodes` is untouched and every offset is written.
// With `fill` (vrt_ctx.h gen_build_device_blocks) a batch's blocks are not copied up: fill leaves them in d_gen_dense.
static int gen_run(vrt_ctx *c, bool gen, uint32_t seed, const int32_t *pos, const uint16_t *dense, uint32_t n, uint16_t *nodes,
                   uint64_t cap_nodes, uint64_t *offsets, const char *what, vrt::GenFillFn fill = nullptr, void *fill_arg = nullptr) {
    using namespace vrt;
    if (!offsets) return fail(c, VRT_ERR_INVALID_ARG, "%s: offsets is null", what);
    offsets[0] = 0;
    if (n == 0u) return VRT_OK;
    if (gen ? !pos : (!dense && !fill)) return fail(c, VRT_ERR_INVALID_ARG, "%s: null input", what);
    if (gen)
        for (uint64_t i = 0; i < 3ull * n; i++)
            if (pos[i] <= -kCoordLimit || pos[i] >= kCoordLimit)
                return fail(c, VRT_ERR_INVALID_ARG, "%s: chunk %llu has a coordinate %d outside (-2^26, 2^26)", what,
                            (unsigned long long)(i / 3), (int)pos[i]);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->d_gen_stage.once((size_t)kGenBatch * kGenSlot));
    HIP_TRY(c, c->d_gen_counts.once(kGenBatch));
    HIP_TRY(c, c->d_gen_offs.once(kGenBatch + 1));
    HIP_TRY(c, c->d_gen_pos.once((size_t)kGenBatch * 3));
    if (!gen) HIP_TRY(c, c->d_gen_dense.once((size_t)kGenBatch * 32768u));
    hipStream_t st = c->stream;
    std::vector<uint64_t> h_offs(kGenBatch + 1);
    uint64_t total = 0;
    uint32_t refused = 0;
    bool fits = true;
    for (uint32_t b0 = 0; b0 < n; b0 += kGenBatch) {
        const uint32_t nb = std::min(kGenBatch, n - b0);
        GenParams P;
        P.pos = c->d_gen_pos;
        P.dense = c->d_gen_dense;
        P.stage = c->d_gen_stage;
        P.counts = c->d_gen_counts;
        P.seed = seed;
        if (gen) {
            HIP_TRY(c, hipMemcpyAsync(c->d_gen_pos, pos + 3ull * b0, (size_t)nb * 3 * sizeof(int32_t), hipMemcpyHostToDevice, st));
            gen_chunks_kernel<true><<<dim3(nb), dim3(kGenBlock), 0, st>>>(P);
        } else {
            if (fill) {
                if (const int rc = fill(c, fill_arg, b0, nb)) return rc;
            } else {
                HIP_TRY(c, hipMemcpyAsync(c->d_gen_dense, dense + 32768ull * b0, (size_t)nb * 32768u * sizeof(uint16_t), hipMemcpyHostToDevice, st));
            }
            gen_chunks_kernel<false><<<dim3(nb), dim3(kGenBlock), 0, st>>>(P);
        }
        HIP_TRY(c, hipGetLastError());
        gen_scan_kernel<<<dim3(1), dim3(1024), 0, st>>>(c->d_gen_counts, nb, c->d_gen_offs);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(h_offs.data(), c->d_gen_offs, (size_t)(nb + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        for (uint32_t i = 0; i < nb; i++) {
            offsets[b0 + i + 1] = total + h_offs[i + 1];
            refused += h_offs[i + 1] == h_offs[i];
        }
        const uint64_t bt = h_offs[nb];
        if (fits && total + bt <= cap_nodes) {
            if (total + bt > c->d_gen_out.cap()) {   // grow, keeping the nodes gathered so far
                vrt_ctx::Buf<uint16_t> p;
                HIP_TRY(c, p.once(std::max<uint64_t>(total + bt, 2 * c->d_gen_out.cap())));
                if (total) HIP_TRY(c, hipMemcpyAsync(p, c->d_gen_out, (size_t)total * sizeof(uint16_t), hipMemcpyDeviceToDevice, st));
                HIP_TRY(c, hipStreamSynchronize(st));
                c->d_gen_out = std::move(p);
            }
            gen_gather_kernel<<<dim3(nb), dim3(kGenBlock), 0, st>>>(c->d_gen_stage, c->d_gen_counts, c->d_gen_offs, c->d_gen_out + total);
            HIP_TRY(c, hipGetLastError());
        } else {
            fits = false;
        }
        total += bt;
    }
    if (!fits)
        return fail(c, VRT_ERR_OOM, "%s: the chunks need %llu nodes, cap_nodes is %llu (offsets[n] holds the need)", what,
                    (unsigned long long)total, (unsigned long long)cap_nodes);
    if (total) {
        if (!nodes) return fail(c, VRT_ERR_INVALID_ARG, "%s: nodes is null", what);
        HIP_TRY(c, hipMemcpyAsync(nodes, c->d_gen_out, (size_t)total * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
    }
    if (refused)
        return fail(c, VRT_ERR_OUT_OF_RANGE, "%s: %u chunk(s) need more than 32767 nodes (4096 mixed cells or more): their ranges are empty",
                    what, refused);
    return VRT_OK;
}

namespace vrt {
int gen_build_device_blocks(vrt_ctx *c, GenFillFn fill, void *fill_arg, uint32_t n, uint16_t *nodes, uint64_t cap_nodes, uint64_t *offsets,
                            const char *what) {
    return gen_run(c, false, 0u, nullptr, nullptr, n, nodes, cap_nodes, offsets, what, fill, fill_arg);
}
}  // namespace vrt

extern "C" {

int vrt_generate_chunks(vrt_ctx *c, uint32_t seed, const int32_t *chunk_pos, uint32_t n, uint16_t *nodes, uint64_t cap_nodes,
                        uint64_t *offsets) {
    GRP_ROOT(c, vrt_generate_chunks(d, seed, chunk_pos, n, nodes, cap_nodes, offsets));
    if (!c) return VRT_ERR_INVALID_ARG;
    return gen_run(c, true, seed, chunk_pos, nullptr, n, nodes, cap_nodes, offsets, "vrt_generate_chunks");
}

int vrt_build_chunks(vrt_ctx *c, const uint16_t *dense, uint32_t n, uint16_t *nodes, uint64_t cap_nodes, uint64_t *offsets) {
    GRP_ROOT(c, vrt_build_chunks(d, dense, n, nodes, cap_nodes, offsets));
    if (!c) return VRT_ERR_INVALID_ARG;
    return gen_run(c, false, 0u, nullptr, dense, n, nodes, cap_nodes, offsets, "vrt_build_chunks");
}

}  // extern "C"
