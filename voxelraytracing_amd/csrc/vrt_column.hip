// vrt_column.hip — vrt_get_voxels, vrt_column_tops, vrt_read_top_map: the client's get_voxel (client/src/world.rs:352-357) and
// highest_vox_at (world.rs:359-366) as batches, one position or one column per lane, and the whole world from above.
//
// Which voxels count, where a scan starts and the records are both/column_top.h's, the text the host mirror compiles too; the
// loop over y is the kernel's own.  The host mirror's visits every voxel of a column, as the reference does.  Here a voxel is
// asked as vrt_query.h says (the derived tables, or the octree of a world too large for them), and the answer comes with the
// size of the leaf it lies in: a leaf is one voxel throughout, so when that voxel does not count — air, a liquid under
// VRT_COLUMN_SOLID, the 32^3 of a missing chunk — nothing of the leaf does, and the scan goes on below it.  The solid set is 256
// bits made of the context's material table (vrt_write_materials keeps the table on the host as well), passed in the kernel's
// parameters and read there only for a voxel that is not air.
#include "vrt_query.h"
#include "both/column_top.h"

namespace vrt {

namespace {

struct VoxelParams {
    QueryWorld W;
    const int32_t *pos;
    vrt_voxel_at *out;
    uint32_t n;
};

struct ColumnParams {
    QueryWorld W;
    uint32_t solid[8];
    const vrt_column_query *q;
    vrt_column_top *out;
    uint32_t n;
};

struct TopMapParams {
    QueryWorld W;
    uint32_t solid[8];
    vrt_top_entry *map;
    uint32_t flags;
};

constexpr uint32_t kMapX = 32, kMapZ = 8;   // a workgroup's columns: each wave takes two rows of 32 along x
static_assert(kMapX * kMapZ == kCastBlock, "one column per lane");

// The scan of column (ux, uz), world-local, downwards from uy: true with uy and v at the highest voxel that counts
__device__ __forceinline__ bool column_scan(const QueryWorld &W, const uint32_t *solid, uint32_t flags, uint32_t ux, uint32_t uz,
                                            uint32_t &uy, uint32_t &v) {
    for (;;) {
        uint32_t lo;
        v = cast_voxel(W, ux, uy, uz, lo);
        if (column_counts(v, flags, solid)) return true;
        const uint32_t base = uy & ~lo;   // the lowest y of the leaf: nothing of it counts
        if (base == 0u) return false;
        uy = base - 1u;
    }
}

__global__ __launch_bounds__(kCastBlock) void get_voxels_kernel(VoxelParams P) {
    const uint32_t i = blockIdx.x * kCastBlock + threadIdx.x;
    if (i >= P.n) return;
    const int32_t *p = P.pos + (size_t)i * 3u;
    const uint32_t W = P.W.S * 32u;
    // world-local coordinates: inside <=> below W as unsigned (cast_dda.h)
    const uint32_t ux = (uint32_t)p[0] - (uint32_t)P.W.min[0], uy = (uint32_t)p[1] - (uint32_t)P.W.min[1], uz = (uint32_t)p[2] - (uint32_t)P.W.min[2];
    vrt_voxel_at r;
    r.voxel = 0u;
    r.status = (uint16_t)VRT_VOXEL_OUT_OF_BOUNDS;
    if (ux < W && uy < W && uz < W) {
        const uint32_t S = P.W.S;
        const uint32_t ch = (ux >> 5) + S * ((uy >> 5) + S * (uz >> 5));
        const uint32_t root = ch < P.W.n_roots ? P.W.roots[ch] : 0u;
        r.status = (uint16_t)VRT_VOXEL_NO_CHUNK;
        if (root != 0u) {
            uint32_t lo;
            r.voxel = (uint16_t)cast_voxel(P.W, ux, uy, uz, lo);
            r.status = (uint16_t)VRT_VOXEL_OK;
        }
    }
    P.out[i] = r;
}

__global__ __launch_bounds__(kCastBlock) void column_tops_kernel(ColumnParams P) {
    const uint32_t i = blockIdx.x * kCastBlock + threadIdx.x;
    if (i >= P.n) return;
    const vrt_column_query q = P.q[i];
    const uint32_t W = P.W.S * 32u;
    const uint32_t ux = (uint32_t)q.x - (uint32_t)P.W.min[0], uz = (uint32_t)q.z - (uint32_t)P.W.min[2];
    vrt_column_top r;
    uint32_t uy, v;
    if (!(ux < W && uz < W))
        column_outside(r);
    else if (column_start(q.flags, q.from_y, P.W.min[1], W, uy) && column_scan(P.W, P.solid, q.flags, ux, uz, uy, v))
        column_found(r, P.W.min[1], uy, v);
    else
        column_none(r, P.W.min[1]);
    P.out[i] = r;
}

// One column per lane, lanes along x: the four columns of a depth-3 cell read one grid word, a row of a wave stores 256
// contiguous bytes.  The world's side is a multiple of 32, so every lane has a column.
__global__ __launch_bounds__(kCastBlock) void top_map_kernel(TopMapParams P) {
    const uint32_t W = P.W.S * 32u;
    const uint32_t ux = blockIdx.x * kMapX + (threadIdx.x & (kMapX - 1u)), uz = blockIdx.y * kMapZ + threadIdx.x / kMapX;
    vrt_column_top r;
    uint32_t uy = W - 1u, v;
    if (column_scan(P.W, P.solid, P.flags, ux, uz, uy, v))
        column_found(r, P.W.min[1], uy, v);
    else
        column_none(r, P.W.min[1]);
    vrt_top_entry e;
    e.y = r.y;
    e.voxel = r.voxel;
    P.map[(size_t)uz * W + ux] = e;
}

}  // namespace

}  // namespace vrt

static uint32_t query_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + vrt::kCastBlock - 1u) / vrt::kCastBlock); }

// One launch each on c->stream against the world of vrt_query.h's query_world, ordered as a cast is (vrt_cast.hip): frames on
// the other streams and the next node-pool or chunk_roots upload wait for it.
static int voxels_enqueue(vrt_ctx *c, const void *pos, uint32_t n, void *out) {
    vrt::VoxelParams P;
    const int rc = query_world(c, P.W);
    if (rc) return rc;
    P.pos = static_cast<const int32_t *>(pos);
    P.out = static_cast<vrt_voxel_at *>(out);
    P.n = n;
    hipLaunchKernelGGL(vrt::get_voxels_kernel, dim3(query_blocks(n)), dim3(vrt::kCastBlock), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return publish_upload(c);
}

// ... the solid set from the host's copy of the material table: every vrt_write_materials so far, which is what a kernel
// enqueued now would read of the device's
static int columns_enqueue(vrt_ctx *c, const void *q, uint32_t n, void *out) {
    vrt::ColumnParams P;
    const int rc = query_world(c, P.W);
    if (rc) return rc;
    vrt::solid_set(c->h_mats, P.solid);
    P.q = static_cast<const vrt_column_query *>(q);
    P.out = static_cast<vrt_column_top *>(out);
    P.n = n;
    hipLaunchKernelGGL(vrt::column_tops_kernel, dim3(query_blocks(n)), dim3(vrt::kCastBlock), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return publish_upload(c);
}

static int top_map_enqueue(vrt_ctx *c, uint32_t flags, void *map) {
    vrt::TopMapParams P;
    const int rc = query_world(c, P.W);
    if (rc) return rc;
    vrt::solid_set(c->h_mats, P.solid);
    P.map = static_cast<vrt_top_entry *>(map);
    P.flags = flags;
    const uint32_t W = P.W.S * 32u;
    hipLaunchKernelGGL(vrt::top_map_kernel, dim3(W / vrt::kMapX, W / vrt::kMapZ), dim3(vrt::kCastBlock), 0, c->stream, P);
    HIP_TRY(c, hipGetLastError());
    return publish_upload(c);
}

extern "C" {

int vrt_get_voxels_device(vrt_ctx *c, const void *pos, uint32_t n, void *out) {
    GRP_ROOT(c, vrt_get_voxels_device(d, pos, n, out));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (n == 0u) return VRT_OK;
    if (!pos || !out) return fail(c, VRT_ERR_INVALID_ARG, "vrt_get_voxels_device: null argument");
    if (((uintptr_t)pos & 3u) || ((uintptr_t)out & 3u)) return fail(c, VRT_ERR_INVALID_ARG, "vrt_get_voxels_device: pointers must be 4-byte aligned");
    HIP_TRY(c, hipSetDevice(c->device));
    return voxels_enqueue(c, pos, n, out);
}

int vrt_get_voxels(vrt_ctx *c, const int32_t *pos, uint32_t n, vrt_voxel_at *out) {
    GRP_ROOT(c, vrt_get_voxels(d, pos, n, out));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (n == 0u) return VRT_OK;
    if (!pos || !out) return fail(c, VRT_ERR_INVALID_ARG, "vrt_get_voxels: null argument");
    return query_batch_host(c, pos, (size_t)n * 3u * sizeof(int32_t), out, (size_t)n * sizeof(vrt_voxel_at), n, voxels_enqueue);
}

int vrt_column_tops_device(vrt_ctx *c, const void *q, uint32_t n, void *out) {
    GRP_ROOT(c, vrt_column_tops_device(d, q, n, out));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (n == 0u) return VRT_OK;
    if (!q || !out) return fail(c, VRT_ERR_INVALID_ARG, "vrt_column_tops_device: null argument");
    if (((uintptr_t)q & 3u) || ((uintptr_t)out & 3u)) return fail(c, VRT_ERR_INVALID_ARG, "vrt_column_tops_device: pointers must be 4-byte aligned");
    HIP_TRY(c, hipSetDevice(c->device));
    return columns_enqueue(c, q, n, out);
}

int vrt_column_tops(vrt_ctx *c, const vrt_column_query *q, uint32_t n, vrt_column_top *out) {
    GRP_ROOT(c, vrt_column_tops(d, q, n, out));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (n == 0u) return VRT_OK;
    if (!q || !out) return fail(c, VRT_ERR_INVALID_ARG, "vrt_column_tops: null argument");
    return query_batch_host(c, q, (size_t)n * sizeof(vrt_column_query), out, (size_t)n * sizeof(vrt_column_top), n, columns_enqueue);
}

int vrt_top_map_device(vrt_ctx *c, uint32_t flags, void *map) {
    GRP_ROOT(c, vrt_top_map_device(d, flags, map));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (!map) return fail(c, VRT_ERR_INVALID_ARG, "vrt_top_map_device: null argument");
    if (flags & ~VRT_COLUMN_SOLID) return fail(c, VRT_ERR_INVALID_ARG, "vrt_top_map_device: flags %#x (0 or VRT_COLUMN_SOLID)", flags);
    if ((uintptr_t)map & 7u) return fail(c, VRT_ERR_INVALID_ARG, "vrt_top_map_device: the map must be 8-byte aligned");
    HIP_TRY(c, hipSetDevice(c->device));
    return top_map_enqueue(c, flags, map);
}

// The host form: the map is made in the queries' staging buffer (the previous host batch has finished: each one waits for its
// results) and copied out
int vrt_read_top_map(vrt_ctx *c, uint32_t flags, vrt_top_entry *map) {
    GRP_ROOT(c, vrt_read_top_map(d, flags, map));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (!map) return fail(c, VRT_ERR_INVALID_ARG, "vrt_read_top_map: null argument");
    if (flags & ~VRT_COLUMN_SOLID) return fail(c, VRT_ERR_INVALID_ARG, "vrt_read_top_map: flags %#x (0 or VRT_COLUMN_SOLID)", flags);
    int rc = validate_frame(c);   // (the world's size is known from here on)
    if (rc) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t W = (size_t)c->world.size_in_chunks * 32u, bytes = W * W * sizeof(vrt_top_entry);
    HIP_TRY(c, c->d_query.grow(bytes));
    HIP_TRY(c, c->ev_query.ensure());
    uint8_t *dmap = c->d_query;
    rc = top_map_enqueue(c, flags, dmap);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(map, dmap, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_query, c->stream));
    HIP_TRY(c, hipEventSynchronize(c->ev_query));
    return VRT_OK;
}

}  // extern "C"
