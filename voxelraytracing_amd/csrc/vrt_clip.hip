// vrt_clip.hip — vrt_clip_moves: the client's collisions (clientdesktop/src/main.rs:316-319; clip_aabb_movement of
// client/src/player.rs:202-244 over ClientWorld::get_collisions_w, client/src/world.rs:369-391, and the Aabb family of
// common/src/math.rs:18-126) as a batch, one box per lane, bit for bit.
//
// The Aabb arithmetic (expand, the overlap tests, the clip of one axis, EPSILON, the rejections) is both/aabb_clip.h's, the text
// the host mirror's Aabb compiles too: only f32 add, subtract and compare occur, in the reference's order (the translation unit
// is built with -ffp-contract=off: Makefile).
// The loop over the world boxes is sequential by specification (include/vrt.h: its answer depends on the order on arbitrary
// lists), so a lane walks its own range in gather order — x, then y, then z — and clips as it goes; the list is
// never stored.  Voxels are vrt_query.h's cast_voxel.  The last leaf found is kept as an aligned cube in registers together
// with whether it is solid: the voxels of the range inside it load nothing, and the rest of a leaf that is not solid is
// stepped over along z (nothing is gathered there, so the order of what is gathered stands).
#include "vrt_query.h"
#include "both/aabb_clip.h"
#include "both/material.h"

namespace vrt {

namespace {

struct ClipParams {
    QueryWorld W;
    const vrt_box_query *q;
    vrt_box_move *out;
    uint32_t n;
    const vrt_material *mats;
};

struct ClipBox {
    float fx, fy, fz, tx, ty, tz;   // Aabb.from, Aabb.to
};

// voxelpack.get(v).is_solid() as the material table holds it: both/material.h's, which the column queries ask too
__device__ __forceinline__ bool clip_solid(const ClipParams &P, uint32_t v) { return material_solid(P.mats, v); }

// world(&bbox.expand(mv)) and the loop over it (player.rs:208-215 / :226-233): (ax, ay, az) enter as mv and leave clipped,
// count = the boxes gathered.  False: the range holds more than VRT_BOX_MAX_VOXELS voxels (asked of the first pass only).
__device__ __forceinline__ bool clip_pass(const ClipParams &P, const ClipBox &b, float mvx, float mvy, float mvz, bool solid0,
                                          bool capped, float &ax, float &ay, float &az, uint32_t &count) {
    float efx = b.fx, efy = b.fy, efz = b.fz, etx = b.tx, ety = b.ty, etz = b.tz;
    aabb_expand(efx, etx, mvx);
    aabb_expand(efy, ety, mvy);
    aabb_expand(efz, etz, mvz);
    // get_collisions_w, world.rs:372-377 (every value is below 2^24 in magnitude: the casts are exact)
    const int32_t x0 = (int32_t)floorf(efx), y0 = (int32_t)floorf(efy), z0 = (int32_t)floorf(efz);
    const int32_t x1 = (int32_t)ceilf(etx), y1 = (int32_t)ceilf(ety), z1 = (int32_t)ceilf(etz);
    count = 0u;
    const int32_t nx = x1 - x0, ny = y1 - y0, nz = z1 - z0;
    if (nx <= 0 || ny <= 0 || nz <= 0) return true;   // an empty or inverted range: no boxes
    if (capped && clip_range_over(nx, ny, nz, VRT_BOX_MAX_VOXELS)) return false;
    const uint32_t W = P.W.S * 32u;
    // the leaf the last lookup found: voxels v with (v & ~c_lo) == c_base lie in it (no voxel coordinate is 0xFFFFFFFF)
    uint32_t cbx = 0xFFFFFFFFu, cby = 0xFFFFFFFFu, cbz = 0xFFFFFFFFu, c_lo = 0u;
    bool c_solid = false;
    // `for x in from.x..to.x { for y { for z {` as one loop: lanes whose ranges differ stay together whichever loop each is in
    int32_t x = x0, y = y0, z = z0;
    for (;;) {
        // world-local coordinates: inside <=> below W as unsigned (|x| < 2^24 + 2, far from wrapping onto [0, W))
        const uint32_t ux = (uint32_t)x - (uint32_t)P.W.min[0], uy = (uint32_t)y - (uint32_t)P.W.min[1], uz = (uint32_t)z - (uint32_t)P.W.min[2];
        bool solid = solid0;   // outside the world get_voxel is Err: Voxel::EMPTY, looked up like any other voxel
        int32_t z_next = z + 1;
        if (ux < W && uy < W && uz < W) {
            const uint32_t nm = ~c_lo;
            if (!((ux & nm) == cbx && (uy & nm) == cby && (uz & nm) == cbz)) {
                uint32_t lo;
                const uint32_t v = cast_voxel(P.W, ux, uy, uz, lo);
                c_lo = lo;
                cbx = ux & ~lo; cby = uy & ~lo; cbz = uz & ~lo;
                c_solid = clip_solid(P, v);
            }
            solid = c_solid;
            if (!solid) z_next = z + (int32_t)(c_lo - (uz & c_lo)) + 1;   // the leaf's last voxel along z, and one on
        }
        if (solid) {
            count += 1u;
            // Aabb::new(pos.as_vec3(), pos.as_vec3() + 1.0), then clip_y_collide, clip_x_collide, clip_z_collide (math.rs:50-115)
            // of it (self) against the unmoved bbox (c)
            const float wfx = (float)x, wfy = (float)y, wfz = (float)z;
            const float wtx = wfx + 1.0f, wty = wfy + 1.0f, wtz = wfz + 1.0f;
            const bool ox = aabb_overlap(wfx, wtx, b.fx, b.tx), oy = aabb_overlap(wfy, wty, b.fy, b.ty), oz = aabb_overlap(wfz, wtz, b.fz, b.tz);
            if (ox && oz) ay = clip_axis(ay, wfy, wty, b.fy, b.ty);
            if (oy && oz) ax = clip_axis(ax, wfx, wtx, b.fx, b.tx);
            if (ox && oy) az = clip_axis(az, wfz, wtz, b.fz, b.tz);
        }
        z = z_next;
        if (z >= z1) {
            z = z0;
            y += 1;
            if (y >= y1) {
                y = y0;
                x += 1;
                if (x >= x1) break;
            }
        }
    }
    return true;
}

__global__ __launch_bounds__(kCastBlock) void clip_moves_kernel(ClipParams P) {
    const uint32_t i = blockIdx.x * kCastBlock + threadIdx.x;
    if (i >= P.n) return;
    const vrt_box_query q = P.q[i];
    vrt_box_move r;
    r.mv[0] = r.mv[1] = r.mv[2] = 0.0f;
    r.status = VRT_BOX_REJECTED;
    r.flags = 0u;
    r.boxes[0] = r.boxes[1] = 0u;
    r._reserved = 0u;
    // rejected (include/vrt.h): clip_in_range
    bool ok = true;
    for (int a = 0; a < 3; a++) ok = ok && clip_in_range(q.from[a]) && clip_in_range(q.to[a]) && clip_in_range(q.mv[a]);
    if (!ok) {
        P.out[i] = r;
        return;
    }
    const bool solid0 = clip_solid(P, 0u);
    const float mvx = q.mv[0], mvy = q.mv[1], mvz = q.mv[2];
    const ClipBox b{q.from[0], q.from[1], q.from[2], q.to[0], q.to[1], q.to[2]};
    float ax = mvx, ay = mvy, az = mvz;
    uint32_t n0 = 0u, n1 = 0u;
    if (!clip_pass(P, b, mvx, mvy, mvz, solid0, true, ax, ay, az, n0)) {
        P.out[i] = r;
        return;
    }
    // eq = mv_clipped.cmpeq(mv), player.rs:216 (-0 == 0)
    uint32_t flags = (ax != mvx ? VRT_BOX_CLIPPED_X : 0u) | (ay != mvy ? VRT_BOX_CLIPPED_Y : 0u) | (az != mvz ? VRT_BOX_CLIPPED_Z : 0u);
    if ((q.flags & VRT_BOX_AUTOJUMP) && (flags & (VRT_BOX_CLIPPED_X | VRT_BOX_CLIPPED_Z))) {
        // bbox.translate(vec3(0.0, 1.1, 0.0)), player.rs:224: the additions of 0.0 are the reference's (-0 becomes 0)
        const ClipBox b2{b.fx + 0.0f, b.fy + 1.1f, b.fz + 0.0f, b.tx + 0.0f, b.ty + 1.1f, b.tz + 0.0f};
        float jx = mvx, jy = mvy, jz = mvz;
        (void)clip_pass(P, b2, mvx, mvy, mvz, solid0, false, jx, jy, jz, n1);
        jy = 0.0f;
        if (fabsf(jx) > fabsf(ax) || fabsf(jy) > fabsf(ay) || fabsf(jz) > fabsf(az)) {
            ay += 1.0f;
            ax = jx;
            az = jz;
            flags |= VRT_BOX_STEPPED_UP;
        }
    }
    r.mv[0] = ax; r.mv[1] = ay; r.mv[2] = az;
    r.status = VRT_BOX_MOVED;
    r.flags = flags;
    r.boxes[0] = n0; r.boxes[1] = n1;
    P.out[i] = r;
}

}  // namespace

}  // namespace vrt

// One launch on c->stream against the world of vrt_query.h's query_world and the device's material table: vrt_write_materials
// copies on c->stream, so the kernel reads every write so far.
static int clip_enqueue(vrt_ctx *c, const void *q, uint32_t n, void *out) {
    vrt::ClipParams P;
    const int rc = query_world(c, P.W);
    if (rc) return rc;
    hipStream_t st = c->stream;
    P.n = n;
    P.q = static_cast<const vrt_box_query *>(q);
    P.out = static_cast<vrt_box_move *>(out);
    P.mats = c->d_mats;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + vrt::kCastBlock - 1u) / vrt::kCastBlock);
    hipLaunchKernelGGL(vrt::clip_moves_kernel, dim3(blocks), dim3(vrt::kCastBlock), 0, st, P);
    HIP_TRY(c, hipGetLastError());
    // ordered as a cast is (vrt_cast.hip): frames on the other streams and the next node-pool or chunk_roots upload wait for it
    return publish_upload(c);
}

extern "C" {

int vrt_clip_moves_device(vrt_ctx *c, const void *q, uint32_t n, void *out) {
    GRP_ROOT(c, vrt_clip_moves_device(d, q, n, out));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (n == 0u) return VRT_OK;
    if (!q || !out) return fail(c, VRT_ERR_INVALID_ARG, "vrt_clip_moves_device: null argument");
    if (((uintptr_t)q & 3u) || ((uintptr_t)out & 3u)) return fail(c, VRT_ERR_INVALID_ARG, "vrt_clip_moves_device: pointers must be 4-byte aligned");
    HIP_TRY(c, hipSetDevice(c->device));
    return clip_enqueue(c, q, n, out);
}

int vrt_clip_moves(vrt_ctx *c, const vrt_box_query *q, uint32_t n, vrt_box_move *out) {
    GRP_ROOT(c, vrt_clip_moves(d, q, n, out));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (n == 0u) return VRT_OK;
    if (!q || !out) return fail(c, VRT_ERR_INVALID_ARG, "vrt_clip_moves: null argument");
    return query_batch_host(c, q, (size_t)n * sizeof(vrt_box_query), out, (size_t)n * sizeof(vrt_box_move), n, clip_enqueue);
}

}  // extern "C"
