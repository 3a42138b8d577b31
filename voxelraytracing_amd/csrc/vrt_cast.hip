// vrt_cast.hip — vrt_cast_rays: the client's voxel pick (clientdesktop/src/main.rs:320-325, common::math::cast_ray of
// common/src/math.rs:153-226 over ClientWorld::get_voxel) as a batch, one ray per lane, bit for bit.
//
// The DDA is the reference's text in strict binary32 (the translation unit is built with -ffp-contract=off, correctly rounded
// divide and square root, denormals kept: Makefile).  A voxel is asked as vrt_query.h says (the derived tables, or the octree
// of a world too large for them).  Every air leaf a ray finds is kept as an aligned cube in registers: the steps inside it
// load nothing.
#include "vrt_query.h"

namespace vrt {

namespace {

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

// One launch on c->stream against the world of vrt_query.h's query_world.
static int cast_enqueue(vrt_ctx *c, const void *q, uint32_t n, void *out) {
    vrt::CastParams P;
    const int rc = query_world(c, P);
    if (rc) return rc;
    hipStream_t st = c->stream;
    P.q = static_cast<const vrt_ray_query *>(q);
    P.out = static_cast<vrt_ray_hit *>(out);
    P.n = n;
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
