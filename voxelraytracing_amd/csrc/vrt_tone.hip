// vrt_tone.hip — vrt_set_tone_map: the exposure and tone curve a path-traced frame is presented through (include/vrt.h states
// both exactly), and the metering of VRT_TONE_AUTO.
//
// The map itself is the blit's (vrt_kernels.hip: present_tone_kernel, present_plain_tone_kernel — the unmapped blits with
// another quantiser).  Here is what finds the exposure, behind the frame's last launch on the frame's own stream:
//   tone_histogram_kernel   the frame's 16-byte texels once, coalesced: the luminance bin of every pixel of the traced area,
//                           counted in a 256-bin histogram of the workgroup in LDS, then the bins that are not 0 added to the
//                           frame set's with one atomic each.  Integer counts: the result does not depend on any order.
//   tone_finish_kernel      one wave: the bins' prefix sums and the rank's bin, then on one lane the float steps of
//                           both/tone_math.h in the contract's order; writes E and the frame's vrt_tone_info, copies the bins to
//                           where vrt_read_tone_histogram finds them and zeroes them for the frame set's next frame.
// Every frame set has its own block of words (vrt_device.h: kTone*), because vrt_present* of the last frame reads that set's E
// on the device; the adapted exposure chains from block to block in the order of the vrt_render calls, so frame n + 1's
// one-thread step waits for frame n's (ev_tone) when the two ran on different streams.  Nothing comes back to the host on the
// render or present path.
#include "vrt_ctx.h"
#include "both/tone_math.h"

namespace vrt {

namespace {

static_assert(sizeof(vrt_tone_map) == 48 && sizeof(vrt_tone_info) == 40, "include/vrt.h");
static_assert(VRT_TONE_LINEAR == kToneLinear && VRT_TONE_REINHARD == kToneReinhard && VRT_TONE_FILMIC == kToneFilmic && VRT_TONE_AUTO == kToneAuto &&
              VRT_TONE_GAMMA2 == kToneGamma2, "both/tone_math.h restates the constants");
static_assert(kToneHistogram == kToneBins && kToneExposure == 2u * kToneBins && kToneInfo % 2u == 0u && kToneInfo + sizeof(vrt_tone_info) / 4u == kToneWords,
              "the tone block's layout");

constexpr uint32_t kToneRows = 8u;   // rows of 256 pixels a workgroup loads at a time

// A workgroup: 256 columns x `rows` rows (a multiple of kToneRows) of the traced area (wt x ht, of a frame `stride` texels wide);
// a wave reads a kibibyte of one row at a time.  The fewer workgroups, the fewer adds to the frame set's 256 words, which all
// meet in eight cache lines: the host sizes the grid to about vrt_ctx::tone_blocks of them.
__global__ void __launch_bounds__(256) tone_histogram_kernel(const Texel *__restrict__ frame, uint32_t stride, uint32_t wt, uint32_t ht, uint32_t rows,
                                                             uint32_t *bins) {
    __shared__ uint32_t s_bins[kToneBins];
    s_bins[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    const uint32_t y_end = min(ht, (blockIdx.y + 1u) * rows);
    for (uint32_t y0 = blockIdx.y * rows; x < wt && y0 < y_end; y0 += kToneRows) {
        // every row's load first (a row beyond the area: zeros, which no bin counts), then the bins
        Texel t[kToneRows];
#pragma unroll
        for (uint32_t k = 0; k < kToneRows; k++) t[k] = y0 + k < y_end ? frame[(size_t)(y0 + k) * stride + x] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (uint32_t k = 0; k < kToneRows; k++) {
            const int b = tone_bin(tone_luminance(__uint_as_float(t[k].x), __uint_as_float(t[k].y), __uint_as_float(t[k].z)));
            // Lanes that add to one LDS word take turns.  The wave's 64 neighbouring pixels of a row often share one bin (the sky,
            // a lit wall): then one lane adds the wave's count (the count stays exact: the same integer sum)
            const int b0 = __builtin_amdgcn_readfirstlane(b);
            if (__all(b == b0)) {
                const uint32_t lanes = (uint32_t)__popcll(__ballot(1));
                if (b0 >= 0 && (threadIdx.x & 63u) ==(uint32_t)__ffsll((long long)__ballot(1)) - 1u) atomicAdd(&s_bins[b0], lanes);
            } else if (b >= 0) {
                atomicAdd(&s_bins[b], 1u);
            }
        }
    }
    __syncthreads();
    const uint32_t n = s_bins[threadIdx.x];
    if (n) atomicAdd(&bins[threadIdx.x], n);
}

struct ToneFinish {
    uint32_t *block;       // the frame set's tone block
    const float *prev;     // the exposure word of the metered frame before this one (may be this block's own); null: none
    ToneMeter m;
    uint32_t traced;       // pixels of the traced area
    uint32_t frames;       // metered frames since the adaptation started, this one included
};

// One wave; lane l holds bins 4 l .. 4 l + 3.  (The bins' sum is at most 2^28 pixels: 32 bits hold every prefix sum.)
__global__ void __launch_bounds__(64) tone_finish_kernel(ToneFinish F) {
    const uint32_t lane = threadIdx.x;
    uint32_t *const counting = F.block + kToneCounting, *const hist = F.block + kToneHistogram;
    const uint4 q = reinterpret_cast<const uint4 *>(counting)[lane];
    const uint32_t own = q.x + q.y + q.z + q.w;
    uint32_t incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += up;
    }
    const uint64_t n = __shfl(incl, 63, 64);
    const uint64_t rank = n ? tone_rank(n, F.m.percentile) : 0u;
    // the lowest lane whose inclusive prefix sum exceeds the rank holds the rank's bin (n == 0: lane 0 does the step)
    const unsigned long long holds = __ballot(n != 0u && (uint64_t)incl > rank);
    const uint32_t owner = n ? (uint32_t)__ffsll((long long)holds) - 1u : 0u;
    reinterpret_cast<uint4 *>(hist)[lane] = q;
    reinterpret_cast<uint4 *>(counting)[lane] = make_uint4(0u, 0u, 0u, 0u);
    if (lane != owner) return;
    const uint32_t c[4] = {q.x, q.y, q.z, q.w};
    uint32_t b = 4u * lane, before = incl - own, in_bin = 0u;
    if (n) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (in_bin) continue;                       // (found)
            if ((uint64_t)before + c[k] > rank) { b = 4u * lane + (uint32_t)k; in_bin = c[k]; }
            else before += c[k];
        }
    }
    const bool has_prev = F.prev != nullptr;
    const float prev = has_prev ? *F.prev : 0.0f;
    const ToneMetered r = tone_finish(F.m, n, rank, b, before, in_bin, has_prev, prev);
    vrt_tone_info info;
    info.exposure = r.exposure;
    info.target = r.target;
    info.luminance = r.luminance;
    info.bin = r.bin;
    info.counted = n;
    info.skipped = (uint64_t)F.traced - n;
    info.frames = F.frames;
    info._reserved = 0u;
    reinterpret_cast<float *>(F.block)[kToneExposure] = r.exposure;
    *reinterpret_cast<vrt_tone_info *>(F.block + kToneInfo) = info;
}

}  // namespace

}  // namespace vrt

void tone_restart(vrt_ctx *c) {
    c->tone_prev = -1;
    c->tone_frames = 0u;
    c->tone_info_slot = c->tone_hist_slot = -1;
}

int tone_after_frame(vrt_ctx *c, uint32_t slot, hipStream_t st, const vrt::Texel *frame_out, hipEvent_t closing, const float **E) {
    *E = nullptr;
    const vrt_tone_map &o = c->tone;
    if (o.curve == VRT_TONE_OFF) return VRT_OK;
    if (!(o.flags & VRT_TONE_AUTO)) {
        c->tone_info_slot = (int)slot;
        c->tone_info_metered = false;
        c->tone_info_exposure = o.exposure;
        return VRT_OK;
    }
    auto &block = c->d_tone[slot];
    if (!block) {   // (zero from its allocation on: the bins being counted, and an exposure nobody has read)
        HIP_TRY(c, block.once(vrt::kToneWords));
        HIP_TRY(c, hipMemsetAsync(block, 0, vrt::kToneWords * sizeof(uint32_t), st));
    }
    HIP_TRY(c, c->ev_tone.ensure());
    const uint32_t wt = c->width & ~7u, ht = c->height & ~7u;
    if (wt && ht) {
        const uint32_t gx = (wt + 255u) / 256u, gy_want = std::max(1u, c->tone_blocks / gx);
        const uint32_t rows = ((ht + gy_want - 1u) / gy_want + vrt::kToneRows - 1u) / vrt::kToneRows * vrt::kToneRows;
        hipLaunchKernelGGL(vrt::tone_histogram_kernel, dim3(gx, (ht + rows - 1u) / rows), dim3(256), 0, st, frame_out, c->width, wt, ht, rows,
                           block.get() + vrt::kToneCounting);
        HIP_TRY(c, hipGetLastError());
    }
    // the metered frame before this one may still be on its way on another stream: its E is this step's E_prev
    if (c->tone_ev_stream && c->tone_ev_stream != st) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_tone, 0));
    vrt::ToneFinish F;
    F.block = block;
    F.prev = c->tone_prev >= 0 ? reinterpret_cast<const float *>(c->d_tone[c->tone_prev].get()) + vrt::kToneExposure : nullptr;
    F.m = vrt::ToneMeter{o.exposure, o.key, o.adapt, o.min_auto, o.max_auto, o.percentile};
    F.traced = wt * ht;
    F.frames = c->tone_frames + 1u;
    hipLaunchKernelGGL(vrt::tone_finish_kernel, dim3(1), dim3(64), 0, st, F);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(c->ev_tone, st));
    c->tone_ev_stream = st;
    c->tone_prev = (int)slot;
    c->tone_frames += 1u;
    c->tone_info_slot = c->tone_hist_slot = (int)slot;
    c->tone_info_metered = true;
    *E = reinterpret_cast<const float *>(block.get()) + vrt::kToneExposure;
    if (closing) HIP_TRY(c, hipEventRecord(closing, st));   // (a timed frame's time holds the metering, as it holds the denoiser)
    return VRT_OK;
}

// What the calls that read a frame set's tone block wait for: every frame in flight
static int tone_read(vrt_ctx *c, uint32_t slot, uint32_t word, void *dst, size_t bytes) {
    HIP_TRY(c, hipSetDevice(c->device));
    QUIESCE(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(dst, c->d_tone[slot].get() + word, bytes, hipMemcpyDeviceToHost));
    return VRT_OK;
}

extern "C" {

int vrt_set_tone_map(vrt_ctx *c, const vrt_tone_map *opts) {
    if (!c) return VRT_ERR_INVALID_ARG;
    vrt_tone_map o;
    memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    if (!vrt::tone_setting_ok(o))
        return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_tone_map: curve %u, flags 0x%x, exposure %g, white %g, key %g, adapt %g, min_auto %g, max_auto %g, percentile %u "
                    "(include/vrt.h: every float finite and >= 0; exposure > 0 with a curve; key > 0 and adapt in (0, 1] with VRT_TONE_AUTO; percentile <= 1000; "
                    "_reserved 0)", o.curve, o.flags, (double)o.exposure, (double)o.white, (double)o.key, (double)o.adapt, (double)o.min_auto, (double)o.max_auto,
                    o.percentile);
    if (o.curve != VRT_TONE_OFF) {
        if (c->grp) return fail(c, VRT_ERR_STATE, "vrt_set_tone_map: not on a multi-device context (its frame is assembled from messages)");
        if (c->shard_count > 1u || c->tile_major || c->compact)
            return fail(c, VRT_ERR_STATE, "vrt_set_tone_map: not on a sharded or tile-major context (it cannot present its buffer)");
    }
    if (c->grp) return VRT_OK;   // (off, which a multi-device context always is)
    if (o.curve == VRT_TONE_OFF) memset(&o, 0, sizeof o);
    if (memcmp(&c->tone, &o, sizeof o) != 0) {   // the adaptation starts again; what the last frame metered stays readable
        c->tone_prev = -1;
        c->tone_frames = 0u;
    }
    c->tone = o;
    return VRT_OK;
}

int vrt_get_tone_info(vrt_ctx *c, vrt_tone_info *out) {
    GRP_REFUSE(c, "vrt_get_tone_info");
    if (!c || !out) return fail(c, VRT_ERR_INVALID_ARG, "vrt_get_tone_info: null argument");
    if (c->tone_info_slot < 0) return fail(c, VRT_ERR_STATE, "vrt_get_tone_info: no frame has been mapped yet (vrt_set_tone_map, then a VRT_MODE_PATH frame)");
    memset(out, 0, sizeof *out);
    if (!c->tone_info_metered) {
        out->exposure = c->tone_info_exposure;
        out->frames = c->tone_frames;
        return vrt_synchronize(c);
    }
    return tone_read(c, (uint32_t)c->tone_info_slot, vrt::kToneInfo, out, sizeof *out);
}

int vrt_read_tone_histogram(vrt_ctx *c, uint32_t bins[256]) {
    GRP_REFUSE(c, "vrt_read_tone_histogram");
    if (!c || !bins) return fail(c, VRT_ERR_INVALID_ARG, "vrt_read_tone_histogram: null argument");
    if (c->tone_hist_slot < 0)
        return fail(c, VRT_ERR_STATE, "vrt_read_tone_histogram: no frame has been metered yet (vrt_set_tone_map with VRT_TONE_AUTO, then a VRT_MODE_PATH frame)");
    return tone_read(c, (uint32_t)c->tone_hist_slot, vrt::kToneHistogram, bins, vrt::kToneBins * sizeof(uint32_t));
}

}  // extern "C"
