// vrt_denoise.hip — vrt_set_denoise: the edge-stopped à-trous filter (Dammertz et al. 2010) a path-traced frame goes through
// while the view moves and every frame is a fresh 1-spp image (include/vrt.h states the filter exactly).
//
// A primary hit lies on an axis-aligned voxel face, and the frame's texel already carries the voxel id and the face: two
// pixels see the same surface exactly when they agree on those (the key) and on the integer coordinate of the face's plane
// (the guide word).  The face-shaded material colour is one value over such a set, so averaging radiance inside it is
// averaging irradiance: no albedo to divide out, no depth or normal buffer, no float threshold on geometry.
//
// Behind the frame's last path launch, on the frame's own stream:
//   denoise_guide_kernel      the primary rays once more (create_ray + march<> of vrt_march.h, nothing shaded) for the one
//                             thing the texel does not hold, the plane coordinate: 4 bytes a pixel
//   denoise_pass_lds_kernel   spacings 1 and 2: a 32 x 32 tile and its halo staged through LDS, every texel read from memory
//                             about once (1.27 x / 1.56 x with the halo); the 25 taps are LDS reads
//   denoise_pass_kernel       spacings 4, 8, 16: the taps of neighbouring pixels no longer share texels within a tile, so each
//                             lane reads its own — the guide word first (4 bytes), the 16-byte texel only where it agrees
// The passes go back and forth between the frame's output and one scratch frame; a frame of an odd number of passes is traced
// INTO the scratch frame, so the last pass always lands in the output and nothing is copied.  The pixel's arithmetic is
// both/denoise_math.h's, the text libvrt_host.so's vrth_denoise compiles too.
#include "vrt_ctx.h"
#include "vrt_march.h"
#include "vrt_water.h"
#include "both/denoise_math.h"

namespace vrt {

namespace {

static_assert(kDnMaxPasses == 5u, "a kernel per tap spacing: 1, 2 (LDS), 4, 8, 16");
static_assert(kDnKeyMask == (VRT_ID_VOXEL_MASK | VRT_ID_HIT | VRT_ID_NX | VRT_ID_NY | VRT_ID_NZ | VRT_ID_WATER), "both/denoise_math.h restates the id bits");

// One wave = one 8 x 8 tile, as in the frame's own primary launch; the id word composed as path_primary_kernel composes it (id_word, vrt_path_common.h).
template <int MARCH>
__global__ void __launch_bounds__(256) denoise_guide_kernel(FrameParams P, uint32_t *guide) {
    __shared__ uint32_t smem[24];
    uint32_t *s_liquid = smem;
    stage_lds(P, nullptr, s_liquid, false);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= P.tiles_total) return;
    uint32_t px, py;
    tile_pixel(P, tile, lane, px, py);
    V3 origin, dir;
    create_ray(P, (int)px, (int)py, origin, dir);
    const MarchResult R = march<MARCH, false, false, true>(P, nullptr, s_liquid, origin, dir);
    uint32_t id = 0u;
    if (R.hit) id |= VRT_ID_HIT;
    if (R.norm.x != 0.0f) id |= VRT_ID_NX;
    if (R.norm.y != 0.0f) id |= VRT_ID_NY;
    if (R.norm.z != 0.0f) id |= VRT_ID_NZ;
    guide[py * P.width + px] = denoise_filterable(id) ? denoise_guide(R.pos.x, R.pos.y, R.pos.z, id) : 0u;
}

// ... of a frame with vrt_set_water_optics on: the primary ray marched as path_water_primary_kernel marches it — with the empty
// liquid set when the camera is not in a liquid, so that the guide of a pixel that sees a lake is the water face's plane, as its
// id word is the water voxel's
template <int MARCH>
__global__ void __launch_bounds__(256) denoise_guide_water_kernel(FrameParams P, FrameParams D, uint32_t *guide) {
    __shared__ uint32_t smem[32];
    uint32_t *s_liquid = smem, *s_dry = smem + 24;
    if (threadIdx.x < 8) s_dry[threadIdx.x] = 0u;
    stage_lds(P, nullptr, s_liquid, false);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= P.tiles_total) return;
    uint32_t px, py;
    tile_pixel(P, tile, lane, px, py);
    V3 origin, dir;
    create_ray(P, (int)px, (int)py, origin, dir);
    const bool wet = __builtin_amdgcn_readfirstlane((uint32_t)is_liquid(s_liquid, water_voxel_at(P, origin))) != 0u;
    MarchResult R;
    if (wet) R = march<MARCH, false, false, true>(P, nullptr, s_liquid, origin, dir);
    else R = march<MARCH, false, false, true>(D, nullptr, s_dry, origin, dir);
    uint32_t id = 0u;
    if (R.hit) id |= VRT_ID_HIT;
    if (R.norm.x != 0.0f) id |= VRT_ID_NX;
    if (R.norm.y != 0.0f) id |= VRT_ID_NY;
    if (R.norm.z != 0.0f) id |= VRT_ID_NZ;
    guide[py * P.width + px] = denoise_filterable(id) ? denoise_guide(R.pos.x, R.pos.y, R.pos.z, id) : 0u;
}

struct DenoisePass {
    const Texel *__restrict__ in;
    Texel *__restrict__ out;
    const uint32_t *__restrict__ guide;
    uint32_t stride;   // texels per row of the frame (its width)
    int wt, ht;        // the traced area
    int s;             // tap spacing
    uint32_t stop;     // sigma_color != 0
    float sg2;         // denoise_sigma2
};

__device__ __forceinline__ DnColor texel_color(uint4 t) { return DnColor{__uint_as_float(t.x), __uint_as_float(t.y), __uint_as_float(t.z)}; }
__device__ __forceinline__ uint4 with_color(uint4 t, DnColor c) {
    return make_uint4(__float_as_uint(c.r), __float_as_uint(c.g), __float_as_uint(c.b), t.w);
}

constexpr int kDnTile = 32;   // the LDS kernel's tile: 32 x 32 pixels, four rows of eight per lane's column

// Spacing S = 1, 2.  A texel outside the traced area is staged as zeros: its key has no VRT_ID_HIT, so no filterable pixel takes it.
template <int S>
__global__ void __launch_bounds__(256) denoise_pass_lds_kernel(DenoisePass D) {
    constexpr int R = 2 * S, LW = kDnTile + 2 * R, LN = LW * LW;
    __shared__ uint4 s_tex[LN];          // S = 2: 40 x 40 x 16 B = 25 KiB
    __shared__ uint32_t s_guide[LN];
    const int x0 = (int)blockIdx.x * kDnTile, y0 = (int)blockIdx.y * kDnTile;
    for (int i = (int)threadIdx.x; i < LN; i += 256) {
        const int ly = i / LW, lx = i - ly * LW;
        const int qx = x0 - R + lx, qy = y0 - R + ly;
        uint4 t = make_uint4(0u, 0u, 0u, 0u);
        uint32_t g = 0u;
        if (qx >= 0 && qy >= 0 && qx < D.wt && qy < D.ht) {
            const size_t q = (size_t)qy * D.stride + (uint32_t)qx;
            t = D.in[q];
            g = D.guide[q];
        }
        s_tex[i] = t;
        s_guide[i] = g;
    }
    __syncthreads();
    const int tx = (int)(threadIdx.x & 31u), ty = (int)(threadIdx.x >> 5);
    const int x = x0 + tx;
    if (x >= D.wt) return;
#pragma unroll 1
    for (int k = 0; k < kDnTile / 8; k++) {
        const int y = y0 + ty + 8 * k;
        if (y >= D.ht) break;
        const int ci = (ty + 8 * k + R) * LW + tx + R;
        uint4 t = s_tex[ci];
        if (denoise_filterable(t.w)) {
            const uint32_t key = denoise_key(t.w), g = s_guide[ci];
            auto fetch = [&](int qx, int qy, DnColor &c) {
                const int i = (qy - y0 + R) * LW + (qx - x0 + R);
                if (s_guide[i] != g) return false;
                const uint4 q = s_tex[i];
                if (denoise_key(q.w) != key) return false;
                c = texel_color(q);
                return true;
            };
            t = with_color(t, denoise_pixel(fetch, x, y, S, texel_color(t), D.stop != 0u, D.sg2));
        }
        D.out[(size_t)y * D.stride + (uint32_t)x] = t;
    }
}

// Spacing S = 4, 8, 16 (one kernel each: a kernel trace then tells the passes apart): a wave is 64 pixels of a row, a kibibyte of texels.
template <int S>
__global__ void __launch_bounds__(256) denoise_pass_kernel(DenoisePass D) {
    const int x = (int)(blockIdx.x * 64u + (threadIdx.x & 63u)), y = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (x >= D.wt || y >= D.ht) return;
    const size_t p = (size_t)y * D.stride + (uint32_t)x;
    uint4 t = D.in[p];
    if (denoise_filterable(t.w)) {
        const uint32_t key = denoise_key(t.w), g = D.guide[p];
        auto fetch = [&](int qx, int qy, DnColor &c) {
            if (qx < 0 || qy < 0 || qx >= D.wt || qy >= D.ht) return false;
            const size_t qi = (size_t)qy * D.stride + (uint32_t)qx;
            if (D.guide[qi] != g) return false;
            const uint4 q = D.in[qi];
            if (denoise_key(q.w) != key) return false;
            c = texel_color(q);
            return true;
        };
        t = with_color(t, denoise_pixel(fetch, x, y, S, texel_color(t), D.stop != 0u, D.sg2));
    }
    D.out[p] = t;
}

void launch_denoise_guide(const FrameParams &P, bool literal, bool water, uint32_t *guide, hipStream_t st) {
    const dim3 grid((P.tiles_total + 3u) / 4u), block(256);
    if (water) {   // vrt_set_water_optics
        const FrameParams D = dry_params(P);
        if (literal) hipLaunchKernelGGL(denoise_guide_water_kernel<1>, grid, block, 0, st, P, D, guide);
        else if (P.grid) hipLaunchKernelGGL(denoise_guide_water_kernel<0>, grid, block, 0, st, P, D, guide);
        else hipLaunchKernelGGL(denoise_guide_water_kernel<2>, grid, block, 0, st, P, D, guide);
        return;
    }
    if (literal) hipLaunchKernelGGL(denoise_guide_kernel<1>, grid, block, 0, st, P, guide);
    else if (P.grid) hipLaunchKernelGGL(denoise_guide_kernel<0>, grid, block, 0, st, P, guide);
    else hipLaunchKernelGGL(denoise_guide_kernel<2>, grid, block, 0, st, P, guide);
}

void launch_denoise_pass(const DenoisePass &D, hipStream_t st) {
    if (D.s <= 2) {
        const dim3 grid((uint32_t)(D.wt + kDnTile - 1) / kDnTile, (uint32_t)(D.ht + kDnTile - 1) / kDnTile), block(256);
        if (D.s == 1) hipLaunchKernelGGL(denoise_pass_lds_kernel<1>, grid, block, 0, st, D);
        else hipLaunchKernelGGL(denoise_pass_lds_kernel<2>, grid, block, 0, st, D);
        return;
    }
    const dim3 grid((uint32_t)(D.wt + 63) / 64u, (uint32_t)(D.ht + 3) / 4u), block(256);
    if (D.s == 4) hipLaunchKernelGGL(denoise_pass_kernel<4>, grid, block, 0, st, D);
    else if (D.s == 8) hipLaunchKernelGGL(denoise_pass_kernel<8>, grid, block, 0, st, D);
    else hipLaunchKernelGGL(denoise_pass_kernel<16>, grid, block, 0, st, D);
}

// Pass i over a frame of width x height texels, from `in` to `out`: what a frame (denoise_after_frame) and vrt_selftest_denoise
// both launch
DenoisePass denoise_pass_of(const Texel *in, Texel *out, const uint32_t *guide, uint32_t width, uint32_t height, uint32_t i, float sigma_color) {
    DenoisePass D;
    D.in = in;
    D.out = out;
    D.guide = guide;
    D.stride = width;
    D.wt = (int)(width & ~7u);
    D.ht = (int)(height & ~7u);
    D.s = 1 << i;
    D.stop = sigma_color != 0.0f ? 1u : 0u;
    D.sg2 = denoise_sigma2(sigma_color, i);
    return D;
}

}  // namespace

}  // namespace vrt

// Before a path frame is enqueued: the frame set's scratch frame and guide words (made by its first denoised frame), and
// where the frame is traced — into the scratch frame when the number of passes is odd, so that the last pass lands in frame_out.
int denoise_before_frame(vrt_ctx *c, uint32_t slot, vrt::Texel *frame_out, vrt::Texel **trace_into) {
    *trace_into = frame_out;
    if (!c->denoise.passes || !c->tiles_total) return VRT_OK;
    const size_t n = (size_t)c->width * c->height;
    VRT_TRY(frame_buf(c, c->sz.dn_scratch[slot], n));
    VRT_TRY(frame_buf(c, c->sz.dn_guide[slot], n));   // (beyond the traced area: 0)
    if (c->denoise.passes & 1u) *trace_into = c->sz.dn_scratch[slot];
    return VRT_OK;
}

// Behind the frame's last path launch on its stream: the guide words, then the passes; then, for a timed frame, its closing
// event once more (launch_path_frame recorded it behind the trace), so that the frame's time holds the filter.
int denoise_after_frame(vrt_ctx *c, const vrt::FrameParams &P, const vrt::FramePlan &plan, uint32_t slot, hipStream_t st, vrt::Texel *frame_out,
                        hipEvent_t closing) {
    const uint32_t passes = c->denoise.passes;
    if (!passes || !c->tiles_total) return VRT_OK;
    vrt::launch_denoise_guide(P, plan.literal, c->water.flags != 0u && c->settings.max_ray_bounces > 0u, c->sz.dn_guide[slot], st);
    HIP_TRY(c, hipGetLastError());
    vrt::Texel *a = (passes & 1u) ? c->sz.dn_scratch[slot] : frame_out, *b = (passes & 1u) ? frame_out : c->sz.dn_scratch[slot];
    for (uint32_t i = 0; i < passes; i++) {
        vrt::launch_denoise_pass(vrt::denoise_pass_of(a, b, c->sz.dn_guide[slot], c->width, c->height, i, c->denoise.sigma_color), st);
        HIP_TRY(c, hipGetLastError());
        std::swap(a, b);
    }
    c->sz.dn_last_guide = c->sz.dn_guide[slot];
    if (closing) HIP_TRY(c, hipEventRecord(closing, st));
    return VRT_OK;
}

extern "C" {

int vrt_set_denoise(vrt_ctx *c, const vrt_denoise_opts *opts) {
    if (!c) return VRT_ERR_INVALID_ARG;
    vrt_denoise_opts o;
    memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    if (o.passes > vrt::kDnMaxPasses) return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_denoise: passes %u (0 = off, 1..%u)", o.passes, vrt::kDnMaxPasses);
    if (!(o.sigma_color >= 0.0f) || std::isinf(o.sigma_color))
        return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_denoise: sigma_color %g (0 = no colour stop, or a finite positive number)", (double)o.sigma_color);
    if (o.flags || o._reserved) return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_denoise: flags and _reserved must be 0");
    if (o.passes) {
        if (c->grp) return fail(c, VRT_ERR_STATE, "vrt_set_denoise: not on a multi-device context (a device holds tiles, not neighbouring pixels)");
        if (c->shard_count > 1u || c->tile_major || c->compact)
            return fail(c, VRT_ERR_STATE, "vrt_set_denoise: not on a sharded or tile-major context (its buffer holds tiles, not neighbouring pixels)");
    }
    if (c->grp) return VRT_OK;   // (off, which a multi-device context always is)
    if (!o.passes) memset(&o, 0, sizeof o);
    c->denoise = o;
    return VRT_OK;
}

int vrt_read_guide(vrt_ctx *c, uint32_t *guide) {
    GRP_REFUSE(c, "vrt_read_guide");
    if (!c || !guide) return fail(c, VRT_ERR_INVALID_ARG, "vrt_read_guide: null argument");
    if (!c->sz.dn_last_guide) return fail(c, VRT_ERR_STATE, "vrt_read_guide: no frame has been denoised yet (vrt_set_denoise, then a VRT_MODE_PATH frame)");
    HIP_TRY(c, hipSetDevice(c->device));
    QUIESCE(c);
    HIP_TRY(c, hipMemcpyAsync(guide, c->sz.dn_last_guide, (size_t)c->width * c->height * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return VRT_OK;
}

// The passes of a frame — denoise_pass_of and launch_denoise_pass, as denoise_after_frame calls them — over a frame of the
// caller's choosing: the arrays packed into texels on the host, two copies of that frame on the device (vrth_denoise starts both of
// its buffers from the input too: a pass never stores to a pixel beyond the traced area), buffers and a stream of its own, no context.
int vrt_selftest_denoise(int32_t device, const float *rgb, const uint32_t *ids, const uint32_t *guide, uint32_t w, uint32_t h, const vrt_denoise_opts *opts,
                         float *rgb_out, uint32_t *ids_out) {
    if (!rgb || !ids || !guide || !opts || !rgb_out || !w || !h) return VRT_ERR_INVALID_ARG;
    if (opts->passes > vrt::kDnMaxPasses || !(opts->sigma_color >= 0.0f) || std::isinf(opts->sigma_color) || opts->flags || opts->_reserved)
        return VRT_ERR_INVALID_ARG;
    const uint64_t n64 = (uint64_t)w * h;
    if (n64 > (1ull << 24)) return VRT_ERR_OUT_OF_RANGE;
    const size_t n = (size_t)n64;
    const uint32_t passes = (w & ~7u) && (h & ~7u) ? opts->passes : 0u;   // (no traced area: nothing to launch)
    std::vector<vrt::Texel> host;
    try {
        host.resize(n);
    } catch (const std::bad_alloc &) {
        return VRT_ERR_OOM;
    }
    for (size_t p = 0; p < n; p++) {
        uint32_t c[3];
        memcpy(c, rgb + p * 3, sizeof c);   // (bits: a NaN keeps its payload)
        host[p] = make_uint4(c[0], c[1], c[2], ids[p]);
    }
    if (hipSetDevice(device) != hipSuccess) return VRT_ERR_DEVICE;
    vrt::Texel *d_a = nullptr, *d_b = nullptr;
    uint32_t *d_guide = nullptr;
    hipStream_t st = nullptr;
    int rc = VRT_OK;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { st = nullptr; rc = VRT_ERR_DEVICE; }
    if (rc == VRT_OK && (hipMalloc(&d_a, n * sizeof(vrt::Texel)) != hipSuccess || hipMalloc(&d_b, n * sizeof(vrt::Texel)) != hipSuccess ||
                         hipMalloc(&d_guide, n * sizeof(uint32_t)) != hipSuccess)) rc = VRT_ERR_OOM;
    if (rc == VRT_OK && (hipMemcpyAsync(d_a, host.data(), n * sizeof(vrt::Texel), hipMemcpyHostToDevice, st) != hipSuccess ||
                         hipMemcpyAsync(d_b, host.data(), n * sizeof(vrt::Texel), hipMemcpyHostToDevice, st) != hipSuccess ||
                         hipMemcpyAsync(d_guide, guide, n * sizeof(uint32_t), hipMemcpyHostToDevice, st) != hipSuccess)) rc = VRT_ERR_DEVICE;
    vrt::Texel *a = d_a, *b = d_b;
    for (uint32_t i = 0; rc == VRT_OK && i < passes; i++) {
        vrt::launch_denoise_pass(vrt::denoise_pass_of(a, b, d_guide, w, h, i, opts->sigma_color), st);
        if (hipGetLastError() != hipSuccess) rc = VRT_ERR_DEVICE;
        std::swap(a, b);
    }
    // (a: the buffer the last pass wrote; the input when there was none)
    if (rc == VRT_OK && hipMemcpyAsync(host.data(), a, n * sizeof(vrt::Texel), hipMemcpyDeviceToHost, st) != hipSuccess) rc = VRT_ERR_DEVICE;
    if (st && hipStreamSynchronize(st) != hipSuccess && rc == VRT_OK) rc = VRT_ERR_DEVICE;
    (void)hipFree(d_guide);
    (void)hipFree(d_b);
    (void)hipFree(d_a);
    if (st) (void)hipStreamDestroy(st);
    if (rc != VRT_OK) return rc;
    for (size_t p = 0; p < n; p++) {
        const uint32_t c[3] = {host[p].x, host[p].y, host[p].z};
        memcpy(rgb_out + p * 3, c, sizeof c);
        if (ids_out) ids_out[p] = host[p].w;
    }
    return VRT_OK;
}

}  // extern "C"
