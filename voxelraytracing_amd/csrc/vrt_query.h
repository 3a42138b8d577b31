// vrt_query.h — what the world queries (vrt_cast.hip: vrt_cast_rays, vrt_clip.hip: vrt_clip_moves) share: the world as a
// kernel sees it, the voxel at a position, and the host-pointer form of a batch.  A voxel is asked of the derived tables the default march keeps (vrt_accel.hip: the
// cell grid, then the brick of a split cell — at most two loads) after its chunk's chunk_roots entry: the grid takes a root of 0
// for "walk from node 0", the reference for "no chunk".  A world too large for the tables is walked from chunk_roots through the
// node pool, as find_node does.
#pragma once
#include "vrt_ctx.h"

namespace vrt {

namespace {

struct QueryWorld {   // what query_world fills; each kernel's parameters add its queries, its results and their number
    const uint16_t *nodes;
    uint32_t n_nodes;
    const uint32_t *roots;
    uint32_t n_roots;
    const uint32_t *grid;     // null: walk the octree
    const uint16_t *bricks;
    uint32_t brick_entries;
    int32_t min[3];
    uint32_t S;               // world.size_in_chunks
};

constexpr uint32_t kCastBlock = 256;

__device__ __forceinline__ uint32_t cast_node(const QueryWorld &P, uint32_t idx) {
    return idx < P.n_nodes ? (uint32_t)P.nodes[idx] : 0u;   // past the end: an air leaf, as in the march
}

// The voxel at world-local (x, y, z) — every coordinate below 32 S — and lo = the size of the leaf it lies in, minus 1.
__device__ __forceinline__ uint32_t cast_voxel(const QueryWorld &P, uint32_t x, uint32_t y, uint32_t z, uint32_t &lo) {
    const uint32_t S = P.S;
    const uint32_t ch = (x >> 5) + S * ((y >> 5) + S * (z >> 5));
    const uint32_t root = ch < P.n_roots ? P.roots[ch] : 0u;
    if (root == 0u) {   // no chunk (ChunkAlloc reserves node 0): get_voxel is Err(NoChunk), nothing collides in its 32^3
        lo = 31u;
        return 0u;
    }
    if (P.grid) {
        const uint32_t G1 = S * 8u + 1u;
        const uint32_t e = P.grid[((z >> 2) * G1 + (y >> 2)) * G1 + (x >> 2)];
        if (e >= kAirLeaf) { lo = e & 31u; return 0u; }
        if (is_split_entry(e)) {
            const uint32_t i = (e & 0x7FFFFFFFu) + ((x & 3u) | ((y & 3u) << 2) | ((z & 3u) << 4));
            const uint32_t b = i < P.brick_entries ? (uint32_t)P.bricks[i] : 0u;
            lo = b & 1u;
            return b >> 1;
        }
        lo = e & 31u;
        return e >> 16;
    }
    // find_node (ray_tracer.wgsl:76-125 / Svo::find_node): child addresses are relative to the chunk's root
    uint32_t node = cast_node(P, root), depth = 0u;
    while ((node & 0x8000u) && depth < 5u) {
        const uint32_t sh = 4u - depth;
        const uint32_t sel = ((x >> sh) & 1u) | (((y >> sh) & 1u) << 1) | (((z >> sh) & 1u) << 2);
        node = cast_node(P, root + (node & 0x7FFFu) + sel);
        depth += 1u;
    }
    lo = (32u >> depth) - 1u;
    return node & 0x7FFFu;
}

}  // namespace

}  // namespace vrt

// The world the queries see: the tables as of every write enqueued so far (brought up to date on c->stream, as the next frame
// would — which then finds nothing left to do), or the octree itself.  Orders c->stream behind the uploads so far and fills the
// P; the caller launches on c->stream and then calls publish_upload.
static int query_world(vrt_ctx *c, vrt::QueryWorld &P) {
    int rc = validate_frame(c);
    if (rc) return rc;
    hipStream_t st = c->stream;
    rc = ensure_accel_world(c);   // the whole-world build when one is due (the next vrt_render would make it)
    if (rc) return rc;
    rc = frame_waits_for_uploads(c, st, 0u);   // (on c->stream: the node pool and chunk_roots uploads so far)
    if (rc) return rc;
    memset(&P, 0, sizeof P);
    P.nodes = c->d_nodes;
    P.n_nodes = c->max_nodes;
    P.roots = c->d_roots;
    P.n_roots = c->n_roots;
    P.min[0] = c->world.min[0];
    P.min[1] = c->world.min[1];
    P.min[2] = c->world.min[2];
    P.S = c->world.size_in_chunks;
    vrt_ctx::Tables &T = c->tabs[0];
    if (c->accel_ok && !c->accel_dirty && c->accel_S == P.S && T.live) {
        // tabs[0] may have been brought up to date last on another frame stream, and frames in flight may read it: the chunks
        // still dirty are rebuilt here behind all of them
        if (T.update_pending && T.ev_updated) HIP_TRY(c, hipStreamWaitEvent(st, T.ev_updated, 0));
        if (!T.dirty_chunks.empty()) {
            rc = order_after_frames(c, st);
            if (rc) return rc;
            rc = update_tables(c, 0u, st);
            if (rc) return rc;
        }
        if (T.dirty_chunks.empty()) {
            P.grid = T.d_grid;
            P.bricks = T.d_bricks;
            P.brick_entries = T.brick_cap() * 64u;
        }
    }
    return VRT_OK;
}

// The host-pointer form of a batch of n queries: grows the staging buffer (the previous host batch has finished: each one waits
// for its results), copies the queries in on c->stream, enqueues, copies the results out and waits for them.
static int query_batch_host(vrt_ctx *c, const void *q, size_t q_bytes, void *out, size_t out_bytes, uint32_t n,
                            int (*enqueue)(vrt_ctx *, const void *, uint32_t, void *)) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, c->d_query.grow(q_bytes + out_bytes));
    HIP_TRY(c, c->ev_query.ensure());
    uint8_t *dq = c->d_query, *dout = dq + q_bytes;   // (both record sizes are multiples of 4)
    HIP_TRY(c, hipMemcpyAsync(dq, q, q_bytes, hipMemcpyHostToDevice, c->stream));
    const int rc = enqueue(c, dq, n, dout);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(out, dout, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_query, c->stream));
    HIP_TRY(c, hipEventSynchronize(c->ev_query));
    return VRT_OK;
}
