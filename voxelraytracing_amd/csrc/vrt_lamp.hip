// vrt_lamp.hip — the lamp list of vrt_set_lamp_light (include/vrt.h): every face of an emissive, solid unit voxel that looks at a
// passable one, in the contract's order — depth-3 cell (x fastest over the whole world), voxel u inside the cell, face f — derived
// on the GPU from a table set's cell grid and brick pool (vrt_accel.hip), chunk_roots, the liquid set and the emission table.
//
// Three launches on the stream of the frame that needs the list, nothing read back:
//   lamp_count_kernel   a thread per cell counts its faces; a workgroup of 256 consecutive cells leaves their sum
//   lamp_scan_kernel    one workgroup: the exclusive scan of the sums in 64 bits (a world can hold more than 2^32 faces; the bases
//                       saturate, and a base at or beyond the cap writes nothing), the list's length and the world's total
//   lamp_write_kernel   the workgroups that have faces count again, scan their 256 cells in LDS and write the entries below the cap
// A cell is looked at twice rather than its count kept: 4 bytes per cell are 67 MB for a 32^3-chunk world, and all but a few cells
// are done after one load (air, or a leaf of a material that gives off nothing) — by construction; how many cells of a world
// take the long path has not been counted.  The kernels are thin: 256 threads, 26 (count) and 34 (write) VGPRs, 1 KiB of LDS, no
// scratch, so registers and LDS do not limit the waves per SIMD; that the grid load per cell is what bounds them is the
// expectation, not a measurement (profiles/lamp_cost.txt has what a whole rebuild takes).  The whole list is rebuilt when
// the frame's table set, the emission table or the liquid set changed since its last build; each frame set has its own, so a build
// is ordered behind that set's previous frame by the stream alone.
#include <cmath>
#include <cstring>

#include "vrt_ctx.h"

namespace vrt {

namespace {

struct LampWorld {
    const uint32_t *grid;     // [8S][8S+1][8S+1]
    const uint16_t *bricks;
    uint32_t brick_entries;
    const uint32_t *roots;
    uint32_t n_roots, S;
    const float *emission;    // 256 floats, on the device
    uint32_t liquid[8];
};

__device__ __forceinline__ bool lamp_liquid(const LampWorld &W, uint32_t voxel) {
    const uint32_t v = min(voxel, 255u);
    return (W.liquid[v >> 5] >> (v & 31u)) & 1u;
}
__device__ __forceinline__ bool lamp_voxel(const LampWorld &W, uint32_t voxel) {
    return voxel != 0u && !lamp_liquid(W, voxel) && W.emission[min(voxel, 255u)] != 0.0f;
}
// the voxel of a cell's entry at u = (x&3) | (y&3) << 2 | (z&3) << 4
__device__ __forceinline__ uint32_t voxel_of_entry(const LampWorld &W, uint32_t e, uint32_t u) {
    if (e >= kAirLeaf) return 0u;
    if (is_split_entry(e)) {
        const uint32_t i = (e & 0x7FFFFFFFu) + u;
        return i < W.brick_entries ? (uint32_t)W.bricks[i] >> 1 : 0u;
    }
    return e >> 16;
}
// may light leave through the unit voxel at (x, y, z)?  Outside the world box, a chunk without a root, air, a liquid.
__device__ __forceinline__ bool lamp_passable(const LampWorld &W, int x, int y, int z) {
    const int size = (int)(W.S * 32u);
    if (x < 0 || y < 0 || z < 0 || x >= size || y >= size || z >= size) return true;
    const uint32_t ch = ((uint32_t)x >> 5) + W.S * (((uint32_t)y >> 5) + W.S * ((uint32_t)z >> 5));
    if ((ch < W.n_roots ? W.roots[ch] : 0u) == 0u) return true;
    const uint32_t G1 = W.S * 8u + 1u;
    const uint32_t e = W.grid[(((uint32_t)z >> 2) * (size_t)G1 + ((uint32_t)y >> 2)) * G1 + ((uint32_t)x >> 2)];
    const uint32_t v = voxel_of_entry(W, e, ((uint32_t)x & 3u) | (((uint32_t)y & 3u) << 2) | (((uint32_t)z & 3u) << 4));
    return v == 0u || lamp_liquid(W, v);
}

// The lamp faces of cell `cell` (x fastest over the world's (8S)^3 cells) in list order: emit(x, y, z, voxel, face) for each.
template <typename Emit>
__device__ __forceinline__ void for_each_lamp_face(const LampWorld &W, uint32_t cell, const Emit &emit) {
    const uint32_t G = W.S * 8u, G1 = G + 1u;
    const uint32_t gx = cell % G, gy = (cell / G) % G, gz = cell / (G * G);
    const uint32_t e = W.grid[((size_t)gz * G1 + gy) * G1 + gx];
    if (e >= kAirLeaf) return;
    const bool split = is_split_entry(e);
    if (!split && !lamp_voxel(W, e >> 16)) return;   // a leaf that gives off nothing (a border entry is 0: voxel 0)
    for (uint32_t u = 0; u < 64u; u++) {
        const uint32_t v = voxel_of_entry(W, e, u);
        if (split && !lamp_voxel(W, v)) continue;
        const uint32_t lx = u & 3u, ly = (u >> 2) & 3u, lz = u >> 4;
        const int x = (int)(gx * 4u + lx), y = (int)(gy * 4u + ly), z = (int)(gz * 4u + lz);
        for (uint32_t f = 0; f < 6u; f++) {
            const uint32_t a = f >> 1;
            const int d = (f & 1u) ? 1 : -1;
            // (inside a leaf cell the neighbour is the same solid voxel)
            const uint32_t l = a == 0u ? lx : (a == 1u ? ly : lz);
            if (!split && ((f & 1u) ? l < 3u : l > 0u)) continue;
            if (lamp_passable(W, x + (a == 0u ? d : 0), y + (a == 1u ? d : 0), z + (a == 2u ? d : 0))) emit((uint32_t)x, (uint32_t)y, (uint32_t)z, v, f);
        }
    }
}

constexpr uint32_t kLampBlock = 256;

__global__ void __launch_bounds__(kLampBlock) lamp_count_kernel(LampWorld W, uint32_t n_cells, uint32_t *sums) {
    __shared__ uint32_t s_sum;
    if (threadIdx.x == 0) s_sum = 0u;
    __syncthreads();
    const uint32_t cell = blockIdx.x * kLampBlock + threadIdx.x;
    uint32_t n = 0;
    if (cell < n_cells) for_each_lamp_face(W, cell, [&](uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) { n++; });
    if (n) atomicAdd(&s_sum, n);
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = s_sum;
}

// info: [0] listed, [1] 0, [2..3] the total in 64 bits
__global__ void __launch_bounds__(1024) lamp_scan_kernel(const uint32_t *sums, uint32_t *bases, uint32_t n, uint32_t cap, uint32_t *info) {
    __shared__ unsigned long long s_part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t lo = min(t * per, n), hi = min(lo + per, n);
    unsigned long long sum = 0;
    for (uint32_t i = lo; i < hi; i++) sum += sums[i];
    s_part[t] = sum;
    __syncthreads();
    for (uint32_t o = 1; o < 1024u; o <<= 1) {   // Hillis-Steele inclusive scan of the partials
        const unsigned long long v = t >= o ? s_part[t - o] : 0ull;
        __syncthreads();
        s_part[t] += v;
        __syncthreads();
    }
    unsigned long long run = s_part[t] - sum;
    for (uint32_t i = lo; i < hi; i++) {
        bases[i] = run < 0xFFFFFFFFull ? (uint32_t)run : 0xFFFFFFFFu;
        run += sums[i];
    }
    if (t == 1023u) {
        const unsigned long long total = s_part[1023];
        info[0] = total < cap ? (uint32_t)total : cap;
        info[1] = 0u;
        info[2] = (uint32_t)total;
        info[3] = (uint32_t)(total >> 32);
    }
}

__global__ void __launch_bounds__(kLampBlock) lamp_write_kernel(LampWorld W, uint32_t n_cells, const uint32_t *sums, const uint32_t *bases, uint32_t cap,
                                                                uint4 *list) {
    __shared__ uint32_t s_scan[kLampBlock];
    const uint32_t base = bases[blockIdx.x];
    if (sums[blockIdx.x] == 0u || base >= cap) return;   // (the same for the whole workgroup)
    const uint32_t t = threadIdx.x, cell = blockIdx.x * kLampBlock + t;
    uint32_t n = 0;
    if (cell < n_cells) for_each_lamp_face(W, cell, [&](uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) { n++; });
    s_scan[t] = n;
    __syncthreads();
    for (uint32_t o = 1; o < kLampBlock; o <<= 1) {
        const uint32_t v = t >= o ? s_scan[t - o] : 0u;
        __syncthreads();
        s_scan[t] += v;
        __syncthreads();
    }
    if (!n) return;
    // (base < cap <= 2^24, VRT_LAMP_CAP's most, and a workgroup holds at most 256 * 384 faces: no wrap)
    uint32_t at = base + s_scan[t] - n;
    for_each_lamp_face(W, cell, [&](uint32_t x, uint32_t y, uint32_t z, uint32_t v, uint32_t f) {
        if (at < cap) list[at] = make_uint4(x | (y << 16), z | (v << 16), f, 0u);
        at++;
    });
}

}  // namespace

}  // namespace vrt

int lamp_list_for_frame(vrt_ctx *c, uint32_t slot, uint32_t tab, hipStream_t st, vrt::LampLaunch &M) {
    const vrt_ctx::Tables &T = c->tabs[tab];
    vrt_ctx::LampList &L = c->lamps[slot];
    // (vrt_render refuses a lamp-lit frame of a world without tables before it enqueues anything, and update_tables has made this set
    // live and brought it up to date: what is asked here again cannot fail behind them — a guard against reading tables that are
    // not there, not a second way to refuse a frame)
    if (!c->accel_ok || c->accel_dirty || !T.live || !T.dirty_chunks.empty() || c->accel_S != c->world.size_in_chunks)
        return fail(c, VRT_ERR_STATE, "vrt_render: a lamp-lit frame (vrt_set_lamp_light) needs the derived tables, which this world does not keep");
    const uint32_t S = c->accel_S;
    const bool fresh = L.valid && L.tab == tab && L.tab_gen == T.gen && L.S == S && L.d_list.cap() == c->lamp_cap &&
                       memcmp(L.emission, c->h_emission, sizeof L.emission) == 0 && memcmp(L.liquid, c->liquid_mask, sizeof L.liquid) == 0;
    if (!fresh) {
        const uint64_t cells64 = (uint64_t)S * 8u * S * 8u * S * 8u;   // (S <= kAccelMaxS: below 2^32)
        const uint32_t n_cells = (uint32_t)cells64, n_blocks = (n_cells + vrt::kLampBlock - 1u) / vrt::kLampBlock;
        L.valid = false;
        HIP_TRY(c, L.d_list.exactly(c->lamp_cap));
        HIP_TRY(c, L.d_sums.grow(n_blocks));
        HIP_TRY(c, L.d_bases.grow(n_blocks));
        HIP_TRY(c, L.d_info.once(4));
        HIP_TRY(c, L.e0.ensure(hipEventDefault));
        HIP_TRY(c, L.e1.ensure(hipEventDefault));
        vrt::LampWorld W;
        W.grid = T.d_grid;
        W.bricks = T.d_bricks;
        W.brick_entries = T.brick_cap() * 64u;
        W.roots = c->d_roots;
        W.n_roots = c->n_roots;
        W.S = S;
        W.emission = vrt::emission_table(c->d_mats);
        memcpy(W.liquid, c->liquid_mask, sizeof W.liquid);
        c->walkers_in_flight = true;   // (the build reads chunk_roots: an upload of them waits for this stream)
        HIP_TRY(c, hipEventRecord(L.e0, st));
        hipLaunchKernelGGL(vrt::lamp_count_kernel, dim3(n_blocks), dim3(vrt::kLampBlock), 0, st, W, n_cells, L.d_sums.get());
        hipLaunchKernelGGL(vrt::lamp_scan_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t *)L.d_sums.get(), L.d_bases.get(), n_blocks, c->lamp_cap,
                           L.d_info.get());
        hipLaunchKernelGGL(vrt::lamp_write_kernel, dim3(n_blocks), dim3(vrt::kLampBlock), 0, st, W, n_cells, (const uint32_t *)L.d_sums.get(),
                           (const uint32_t *)L.d_bases.get(), c->lamp_cap, L.d_list.get());
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(L.e1, st));
        L.tab = tab;
        L.tab_gen = T.gen;
        L.S = S;
        memcpy(L.emission, c->h_emission, sizeof L.emission);
        memcpy(L.liquid, c->liquid_mask, sizeof L.liquid);
        L.builds += 1;
        L.timed = false;
        L.valid = true;
    }
    M.list = L.d_list;
    M.n = L.d_info;
    c->lamp_last = (int)slot;
    return VRT_OK;
}

int vrt_set_lamp_light(vrt_ctx *c, const vrt_lamp_light *opts) {
    if (!c) return VRT_ERR_INVALID_ARG;
    vrt_lamp_light o;
    memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    if (!(o.strength >= 0.0f) || std::isinf(o.strength) || !(o.max_geometry >= 0.0f) || std::isinf(o.max_geometry))
        return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_lamp_light: strength %g, max_geometry %g (each 0 or a finite positive number)", (double)o.strength,
                    (double)o.max_geometry);
    if (o.flags || o._reserved) return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_lamp_light: flags and _reserved must be 0");
    GRP_EACH(c, vrt_set_lamp_light(d, opts));
    if (o.strength == 0.0f) memset(&o, 0, sizeof o);   // (off is 16 zero bytes; max_geometry is not read then)
    if (o.max_geometry == 0.0f) o.max_geometry = 0.0f;   // (-0 as +0)
    if (memcmp(&c->lamp, &o, sizeof o) != 0) c->accum_restart = true;
    c->lamp = o;
    return VRT_OK;
}

// the list the last lamp-lit frame used, once the frames in flight and the context's stream are over: its info words
static int lamp_list_settled(vrt_ctx *c, const char *who, vrt_ctx::LampList **list, uint32_t info[4]) {
    if (c->lamp_last < 0 || !c->lamps[c->lamp_last].valid) return fail(c, VRT_ERR_STATE, "%s: no lamp-lit frame has been rendered", who);
    HIP_TRY(c, hipSetDevice(c->device));
    vrt_ctx::LampList &L = c->lamps[c->lamp_last];
    QUIESCE(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(info, L.d_info, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *list = &L;
    return VRT_OK;
}

int vrt_get_lamp_info(vrt_ctx *c, vrt_lamp_info *out) {
    GRP_ROOT(c, vrt_get_lamp_info(d, out));
    if (!c || !out) return c ? fail(c, VRT_ERR_INVALID_ARG, "vrt_get_lamp_info: null argument") : VRT_ERR_INVALID_ARG;
    vrt_ctx::LampList *L = nullptr;
    uint32_t info[4];
    VRT_TRY(lamp_list_settled(c, "vrt_get_lamp_info", &L, info));
    if (!L->timed) {
        HIP_TRY(c, hipEventElapsedTime(&L->last_ms, L->e0, L->e1));
        L->timed = true;
    }
    memset(out, 0, sizeof *out);
    out->listed = info[0];
    out->cap = c->lamp_cap;
    out->faces = (uint64_t)info[2] | ((uint64_t)info[3] << 32);
    out->builds = L->builds;
    out->last_build_ms = L->last_ms;
    return VRT_OK;
}

int vrt_read_lamps(vrt_ctx *c, vrt_lamp *out, uint32_t cap, uint32_t *n) {
    GRP_ROOT(c, vrt_read_lamps(d, out, cap, n));
    if (!c || (!out && cap)) return c ? fail(c, VRT_ERR_INVALID_ARG, "vrt_read_lamps: null argument") : VRT_ERR_INVALID_ARG;
    vrt_ctx::LampList *L = nullptr;
    uint32_t info[4];
    VRT_TRY(lamp_list_settled(c, "vrt_read_lamps", &L, info));
    static_assert(sizeof(vrt_lamp) == sizeof(uint4), "a list entry is a vrt_lamp");
    const uint32_t m = info[0] < cap ? info[0] : cap;
    if (m) HIP_TRY(c, hipMemcpy(out, L->d_list, (size_t)m * sizeof(vrt_lamp), hipMemcpyDeviceToHost));
    if (n) *n = info[0];
    return VRT_OK;
}
