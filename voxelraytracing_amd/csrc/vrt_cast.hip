// vrt_cast.hip — vrt_cast_rays: the client's voxel pick (clientdesktop/src/main.rs:320-325, common::math::cast_ray of
// common/src/math.rs:153-226 over ClientWorld::get_voxel) as a batch, one ray per lane, bit for bit.
//
// The DDA is the reference's text in strict binary32 (the translation unit is built with -ffp-contract=off, correctly rounded
// divide and square root, denormals kept: Makefile).  A voxel is asked of the derived tables the default march keeps
// (vrt_accel.hip: the cell grid, then the brick of a split cell — at most two loads) after its chunk's chunk_roots entry: the
// grid takes a root of 0 for "walk from node 0", the reference for "no chunk".  A world too large for the tables is walked
// from chunk_roots through the node pool, as find_node does.  Every air leaf a ray finds is kept as an aligned cube in
// registers: the steps inside it load nothing.
#include "vrt_ctx.h"

namespace vrt {

namespace {

struct CastParams {
    const vrt_ray_query *q;
    vrt_ray_hit *out;
    uint32_t n;
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

__device__ __forceinline__ uint32_t cast_node(const CastParams &P, uint32_t idx) {
    return idx < P.n_nodes ? (uint32_t)P.nodes[idx] : 0u;   // past the end: an air leaf, as in the march
}

// The voxel at world-local (x, y, z) — every coordinate below 32 S — and lo = the size of the leaf it lies in, minus 1.
__device__ __forceinline__ uint32_t cast_voxel(const CastParams &P, uint32_t x, uint32_t y, uint32_t z, uint32_t &lo) {
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

__global__ __launch_bounds__(kCastBlock) void cast_rays_kernel(CastParams P) {
    const uint32_t i = blockIdx.x * kCastBlock + threadIdx.x;
    if (i >= P.n) return;
    const vrt_ray_query q = P.q[i];
    vrt_ray_hit r;
    r.pos[0] = r.pos[1] = r.pos[2] = 0;
    r.face[0] = r.face[1] = r.face[2] = 0;
    r.dist = 0.0f;
    r.status = VRT_RAY_MISS;
    const float max_dist = q.max_dist;
    // rejected (include/vrt.h): the reference would loop forever (max_dist = inf) or leave the exact integers of f32 / i32
    if (max_dist > 1048576.0f || !(fabsf(q.start[0]) < 16777216.0f) || !(fabsf(q.start[1]) < 16777216.0f) ||
        !(fabsf(q.start[2]) < 16777216.0f)) {
        r.status = VRT_RAY_REJECTED;
        P.out[i] = r;
        return;
    }
    const float sx0 = q.start[0], sy0 = q.start[1], sz0 = q.start[2];
    const float dx = q.dir[0], dy = q.dir[1], dz = q.dir[2];
    // math.rs:163-167, in the order written: ((1 + (b/a)*(b/a)) + (c/a)*(c/a)), correctly rounded / and sqrt
    const float usx = sqrtf(1.0f + (dy / dx) * (dy / dx) + (dz / dx) * (dz / dx));
    const float usy = sqrtf(1.0f + (dx / dy) * (dx / dy) + (dz / dy) * (dz / dy));
    const float usz = sqrtf(1.0f + (dx / dz) * (dx / dz) + (dy / dz) * (dy / dz));
    int32_t mx = (int32_t)floorf(sx0), my = (int32_t)floorf(sy0), mz = (int32_t)floorf(sz0);
    const int32_t stx = dx < 0.0f ? -1 : 1, sty = dy < 0.0f ? -1 : 1, stz = dz < 0.0f ? -1 : 1;
    float lx = dx < 0.0f ? (sx0 - (float)mx) * usx : ((float)(mx + 1) - sx0) * usx;
    float ly = dy < 0.0f ? (sy0 - (float)my) * usy : ((float)(my + 1) - sy0) * usy;
    float lz = dz < 0.0f ? (sz0 - (float)mz) * usz : ((float)(mz + 1) - sz0) * usz;
    // x and z move only in their own branch, which needs their len below the others': a len that starts NaN or +inf (it only
    // grows) keeps its axis where it is for the whole ray
    const bool x_frozen = !(lx < INFINITY), z_frozen = !(lz < INFINITY);
    const uint32_t W = P.S * 32u;
    // the air leaf the last lookup found: voxels v with (v & ~c_lo) == c_base are air (no voxel coordinate is 0xFFFFFFFF)
    uint32_t cbx = 0xFFFFFFFFu, cby = 0xFFFFFFFFu, cbz = 0xFFFFFFFFu, c_lo = 0u;
    float dist = 0.0f;
    while (dist < max_dist) {
        const int32_t px = mx, py = my, pz = mz;
        if (lx < ly && lx < lz) {
            mx += stx;
            dist = lx;
            lx += usx;
        } else if (lz < lx && lz < ly) {
            mz += stz;
            dist = lz;
            lz += usz;
        } else {
            my += sty;
            dist = ly;
            ly += usy;
        }
        // world-local coordinates: inside <=> below W as unsigned (|map| < 2^24 + 3 * 2^21, far from wrapping onto [0, W))
        const uint32_t ux = (uint32_t)mx - (uint32_t)P.min[0], uy = (uint32_t)my - (uint32_t)P.min[1], uz = (uint32_t)mz - (uint32_t)P.min[2];
        if (ux < W && uy < W && uz < W) {
            const uint32_t nm = ~c_lo;
            if ((ux & nm) == cbx && (uy & nm) == cby && (uz & nm) == cbz) continue;   // inside the air leaf already known
            uint32_t lo;
            const uint32_t v = cast_voxel(P, ux, uy, uz, lo);
            if (v != 0u) {
                r.pos[0] = mx; r.pos[1] = my; r.pos[2] = mz;
                r.face[0] = px - mx; r.face[1] = py - my; r.face[2] = pz - mz;
                r.dist = dist == dist ? dist : __uint_as_float(0x7FC00000u);   // (one NaN for every platform: include/vrt.h)
                r.status = VRT_RAY_HIT;
                break;
            }
            c_lo = lo;
            cbx = ux & ~lo; cby = uy & ~lo; cbz = uz & ~lo;
            continue;
        }
        // Outside the world: an early miss where no later step can bring the ray back.  An axis moves only by its own step
        // (its sign fixed for the ray), so once the voxel is beyond the world on an axis whose step leads away from it — or
        // on x / z, whose len is NaN or inf and which never move — every voxel still to come is outside, none collides, and
        // the reference's loop ends in None whatever it does meanwhile (the NaN / inf branches included: only `dist` and the
        // positions change there, and the result of a miss carries neither).
        const bool bx = (int64_t)mx < (int64_t)P.min[0], by = (int64_t)my < (int64_t)P.min[1], bz = (int64_t)mz < (int64_t)P.min[2];
        const bool gone = (ux >= W && ((bx && (stx < 0 || x_frozen)) || (!bx && (stx > 0 || x_frozen)))) ||
                          (uy >= W && ((by && sty < 0) || (!by && sty > 0))) ||
                          (uz >= W && ((bz && (stz < 0 || z_frozen)) || (!bz && (stz > 0 || z_frozen))));
        if (gone) break;
    }
    P.out[i] = r;
}

}  // namespace

}  // namespace vrt

// The world the casts see: the tables as of every write enqueued so far (brought up to date on c->stream, as the next frame
// would — which then finds nothing left to do), or the octree itself.
static int cast_enqueue(vrt_ctx *c, const void *q, uint32_t n, void *out) {
    int rc = validate_frame(c);
    if (rc) return rc;
    hipStream_t st = c->stream;
    rc = ensure_accel_world(c);   // the whole-world build when one is due (the next vrt_render would make it)
    if (rc) return rc;
    rc = frame_waits_for_uploads(c, st, 0u);   // (on c->stream: the node pool and chunk_roots uploads so far)
    if (rc) return rc;
    vrt::CastParams P;
    memset(&P, 0, sizeof P);
    P.q = static_cast<const vrt_ray_query *>(q);
    P.out = static_cast<vrt_ray_hit *>(out);
    P.n = n;
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
            P.brick_entries = T.brick_cap * 64u;
        }
    }
    const uint32_t blocks = (uint32_t)(((uint64_t)n + vrt::kCastBlock - 1u) / vrt::kCastBlock);
    hipLaunchKernelGGL(vrt::cast_rays_kernel, dim3(blocks), dim3(vrt::kCastBlock), 0, st, P);
    HIP_TRY(c, hipGetLastError());
    // Everything after this call is ordered behind it as behind an upload on c->stream: frames on the other streams wait for it
    // before their own table updates, and the next node-pool or chunk_roots upload waits for it (flush_staged) before it
    // overwrites what the cast reads.
    return publish_upload(c);
}

extern "C" {

int vrt_cast_rays_device(vrt_ctx *c, const void *q, uint32_t n, void *out) {
    GRP_ROOT(c, vrt_cast_rays_device(d, q, n, out));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (n == 0u) return VRT_OK;
    if (!q || !out) return fail(c, VRT_ERR_INVALID_ARG, "vrt_cast_rays_device: null argument");
    if (((uintptr_t)q & 3u) || ((uintptr_t)out & 3u)) return fail(c, VRT_ERR_INVALID_ARG, "vrt_cast_rays_device: pointers must be 4-byte aligned");
    HIP_TRY(c, hipSetDevice(c->device));
    return cast_enqueue(c, q, n, out);
}

int vrt_cast_rays(vrt_ctx *c, const vrt_ray_query *q, uint32_t n, vrt_ray_hit *out) {
    GRP_ROOT(c, vrt_cast_rays(d, q, n, out));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (n == 0u) return VRT_OK;
    if (!q || !out) return fail(c, VRT_ERR_INVALID_ARG, "vrt_cast_rays: null argument");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)n * sizeof(vrt_ray_query);
    if (c->cast_cap < n) {   // (the previous host cast has finished: each one waits for its results)
        (void)hipFree(c->d_cast);
        c->d_cast = nullptr;
        c->cast_cap = 0;
        HIP_TRY(c, hipMalloc(&c->d_cast, 2 * bytes));
        c->cast_cap = n;
    }
    if (!c->ev_cast) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_cast, hipEventDisableTiming));
    uint8_t *dq = static_cast<uint8_t *>(c->d_cast), *dout = dq + (size_t)c->cast_cap * sizeof(vrt_ray_query);
    HIP_TRY(c, hipMemcpyAsync(dq, q, bytes, hipMemcpyHostToDevice, c->stream));
    const int rc = cast_enqueue(c, dq, n, dout);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(out, dout, (size_t)n * sizeof(vrt_ray_hit), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_cast, c->stream));
    HIP_TRY(c, hipEventSynchronize(c->ev_cast));
    return VRT_OK;
}

}  // extern "C"
