// vrt_cast.hip — vrt_cast_rays: the client's voxel pick (clientdesktop/src/main.rs:320-325, common::math::cast_ray of
// common/src/math.rs:153-226 over ClientWorld::get_voxel) as a batch, one ray per lane, bit for bit.
//
// The DDA — the rejections, the set-up, one step, the hit record, the early miss — is both/cast_dda.h's, the text the host
// mirror compiles too (the translation unit is built with -ffp-contract=off, correctly rounded divide and square root,
// denormals kept: Makefile); the loop around them is the kernel's own.  A voxel is asked as vrt_query.h says (the derived tables, or the octree
// of a world too large for them).  Every air leaf a ray finds is kept as an aligned cube in registers: the steps inside it
// load nothing.
#include "vrt_query.h"
#include "both/cast_dda.h"

namespace vrt {

namespace {

struct CastParams {
    QueryWorld W;
    const vrt_ray_query *q;
    vrt_ray_hit *out;
    uint32_t n;
};

__global__ __launch_bounds__(kCastBlock) void cast_rays_kernel(CastParams P) {
    const uint32_t i = blockIdx.x * kCastBlock + threadIdx.x;
    if (i >= P.n) return;
    const vrt_ray_query q = P.q[i];
    vrt_ray_hit r;
    r.pos[0] = r.pos[1] = r.pos[2] = 0;
    r.face[0] = r.face[1] = r.face[2] = 0;
    r.dist = 0.0f;
    r.status = VRT_RAY_MISS;
    if (cast_rejected(q.start, q.max_dist)) {
        r.status = VRT_RAY_REJECTED;
        P.out[i] = r;
        return;
    }
    const uint32_t W = P.W.S * 32u;
    // the air leaf the last lookup found: voxels v with (v & ~c_lo) == c_base are air (no voxel coordinate is 0xFFFFFFFF)
    uint32_t cbx = 0xFFFFFFFFu, cby = 0xFFFFFFFFu, cbz = 0xFFFFFFFFu, c_lo = 0u;
    CastDda d = cast_setup(q.start, q.dir);
    const float max_dist = q.max_dist;
    float dist = 0.0f;
    while (dist < max_dist) {
        const int32_t px = d.mx, py = d.my, pz = d.mz;
        dist = cast_step(d);
        // world-local coordinates: inside <=> below W as unsigned (cast_dda.h)
        const uint32_t ux = (uint32_t)d.mx - (uint32_t)P.W.min[0], uy = (uint32_t)d.my - (uint32_t)P.W.min[1], uz = (uint32_t)d.mz - (uint32_t)P.W.min[2];
        if (ux < W && uy < W && uz < W) {
            const uint32_t nm = ~c_lo;
            if ((ux & nm) == cbx && (uy & nm) == cby && (uz & nm) == cbz) continue;   // inside the air leaf already known
            uint32_t lo;
            if (cast_voxel(P.W, ux, uy, uz, lo) != 0u) {
                cast_hit(r, d, px, py, pz, dist);
                r.status = VRT_RAY_HIT;
                break;
            }
            c_lo = lo;
            cbx = ux & ~lo; cby = uy & ~lo; cbz = uz & ~lo;
            continue;
        }
        if (cast_gone(d, P.W.min, W)) break;
    }
    P.out[i] = r;
}

}  // namespace

}  // namespace vrt

// One launch on c->stream against the world of vrt_query.h's query_world.
static int cast_enqueue(vrt_ctx *c, const void *q, uint32_t n, void *out) {
    vrt::CastParams P;
    const int rc = query_world(c, P.W);
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
    return query_batch_host(c, q, (size_t)n * sizeof(vrt_ray_query), out, (size_t)n * sizeof(vrt_ray_hit), n, cast_enqueue);
}

}  // extern "C"
