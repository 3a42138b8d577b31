// vrt_frames.hip — GpuResources::new / PixelShader::encode_pass (clientdesktop/src/graphics/mod.rs:155-195,
// shader.rs:371-379; callers main.rs:211-223, 426-454): contexts, the per-frame uniforms, frames in flight, vrt_render,
// read-backs and statistics.  Device memory layout: DESIGN.md section 4.
#include "vrt_ctx.h"
#include "both/refract_math.h"  // (vrt_set_water_refraction: max_span's default and limit)

thread_local std::string g_create_err;

int fail(vrt_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    else g_create_err = buf;
    return code;
}

// Wait for the frame that may still be running on the second stream.
vrt_host_prof g_host_prof;

int quiesce(vrt_ctx *c) {
    if (c->alt_pending) {
        for (hipStream_t st : c->extra_stream)
            if (st) HIP_TRY(c, hipStreamSynchronize(st));
        c->alt_pending = false;
    }
    if (c->own_pending) {
        HIP_TRY(c, hipStreamSynchronize(c->own_stream));
        c->own_pending = false;
    }
    c->shared_readers_in_flight = false;
    return VRT_OK;
}

// The reference dispatches tex_size / 8 workgroups per axis (main.rs:452) over a result texture of any size
// (main.rs:257-262: 1080 rows, the window's aspect): the columns and rows beyond the last whole 8x8 tile are never stored to
// and keep the fresh texture's zeros.  Buffers that are read as whole frames start out zero for such a size.
bool ragged_output(const vrt_ctx *c) { return ((c->width | c->height) & 7u) != 0u; }
hipError_t zero_now(vrt_ctx *c, void *p, size_t bytes) {
    const hipError_t e = hipMemsetAsync(p, 0, bytes, c->stream);
    return e != hipSuccess ? e : hipStreamSynchronize(c->stream);   // (done before a launch on any other stream can follow)
}

static void layout_tiles(vrt_ctx *c) {
    c->tiles_x = c->width / 8u;
    c->tiles_total = c->tiles_x * (c->height / 8u);
    // tiles are dealt out in periods of P = w0 + N - 1: w0 to rank 0, then one to each of ranks 1..N-1
    const uint32_t P = c->shard_w0 + c->shard_count - 1u;
    c->shard_period = P;
    c->shard_run = c->shard_rank == 0 ? c->shard_w0 : 1u;
    c->shard_first = c->shard_rank == 0 ? 0u : c->shard_w0 + c->shard_rank - 1u;
    const uint32_t full = c->tiles_total / P, rem = c->tiles_total % P;
    c->tiles_padded = (c->tiles_total + P - 1u) / P;
    c->tiles_local = full * c->shard_run + (rem > c->shard_first ? (rem - c->shard_first < c->shard_run ? rem - c->shard_first : c->shard_run) : 0u);
    const uint32_t tm_tiles = c->tiles_local > c->tiles_padded ? c->tiles_local : c->tiles_padded;
    c->slots = c->tile_major ? tm_tiles * 64u : c->width * c->height;
}

static int alloc_output(vrt_ctx *c) {
    c->sz = vrt_ctx::Sized{};   // everything of the old size goes (the callers have waited for the frames in flight)
    c->accum_restart = true;
    tone_restart(c);
    layout_tiles(c);
    const size_t n = frame_slots(c);
    HIP_TRY(c, c->sz.own_out.once(n));
    // hit buffer: kHitSegments segments, each able to hold every record its workgroups can produce
    const uint32_t nblocks = (c->tiles_local + 3u) / 4u;
    c->hit_seg_cap = ((nblocks + vrt::kHitSegments - 1u) / vrt::kHitSegments) * 256u;
    if (c->hit_seg_cap == 0) c->hit_seg_cap = 256u;
    HIP_TRY(c, c->sz.d_hits.once((size_t)vrt::kHitSegments * c->hit_seg_cap));  // >= nblocks * 256
    c->n_blocks = nblocks;
    // launched-ray counts: one per primary workgroup (two-launch variants) or one per tile (the one-launch kernel)
    const size_t ncnt = c->tiles_local ? c->tiles_local : 1;
    HIP_TRY(c, c->sz.d_blk_counts.once(ncnt));
    HIP_TRY(c, hipMemsetAsync(c->sz.d_blk_counts, 0, ncnt * sizeof(uint32_t), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->sz.own_out, 0, n * sizeof(vrt::Texel), c->stream));
    // (c->stream may be the caller's: a VRT_RENDER_OWN_STREAMS frame on own_stream is not ordered behind these memsets, and
    // result sizes that are not whole tiles rely on the zeros)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // the extra (stream, output, counts) sets of frames in flight are created when first used (vrt_render)
    c->d_out = c->sz.own_out;  // a resize drops any caller-bound output (its size no longer matches)
    c->last.out = c->sz.own_out; c->last.blk = c->sz.d_blk_counts;
    c->last.fused = false; c->last.has_texels = true;
    c->rendered = false;
    return VRT_OK;
}

int validate_frame(vrt_ctx *c) {
    const uint32_t S = c->world.size_in_chunks;
    if (S == 0 || (uint64_t)S * S * S > c->n_roots)
        return fail(c, VRT_ERR_STATE, "world.size_in_chunks %u does not fit the %u-entry chunk_roots buffer "
                    "(call vrt_resize_world first, main.rs:441-445)", S, c->n_roots);
    if (c->world.size != S * 32u)
        return fail(c, VRT_ERR_STATE, "world.size %u != size_in_chunks*32 (%u)", c->world.size, S * 32u);
    return VRT_OK;
}

// Frame-uniform pieces of create_ray_from_screen (ray_tracer.wgsl:160-161): one IEEE divide per column and row
// instead of two per pixel.  Same operations in the same order as the shader text, in binary32.
int ensure_ndc(vrt_ctx *c) {
    if (c->d_ndc && c->ndc_w == c->width && c->ndc_h == c->height &&
        memcmp(c->ndc_proj, c->cam.proj_size, sizeof c->ndc_proj) == 0)
        return VRT_OK;
    if (!c->d_ndc || c->ndc_w + c->ndc_h < c->width + c->height) {   // (against the size last filled, not the capacity)
        QUIESCE(c);
        c->d_ndc.release();
        HIP_TRY(c, c->d_ndc.once((size_t)c->width + c->height));
    }
    std::vector<float> t((size_t)c->width + c->height);
    volatile float px = c->cam.proj_size[0], py = c->cam.proj_size[1];
    for (uint32_t i = 0; i < c->width; i++) { volatile float q = ((float)(int)i * 2.0f) / px; t[i] = q - 1.0f; }
    for (uint32_t i = 0; i < c->height; i++) { volatile float q = ((float)(int)i * 2.0f) / py; t[c->width + i] = q - 1.0f; }
    VRT_TRY(stage_upload(c, c->d_ndc, t.data(), t.size() * sizeof(float)));
    c->ndc_w = c->width;
    c->ndc_h = c->height;
    memcpy(c->ndc_proj, c->cam.proj_size, sizeof c->ndc_proj);
    return VRT_OK;
}

// A primary ray's origin (:169) and what ray_world asks of it before the first step — finite? on a voxel plane (the nudge, :188-190)? outside
// the world (:285)? — in the operations of create_ray / march_grid (vrt_march.h), once per frame instead of once per lane.
static void cam_origin_facts(const vrt_ctx *c, float origin[3], uint32_t *facts) {
    volatile float o[3];
    for (int k = 0; k < 3; k++) {
        volatile float wm = (float)c->world.min[k];
        o[k] = c->cam.pos[k] - wm;
        origin[k] = o[k];
    }
    uint32_t f = 0u;
    if (!(std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]))) f |= vrt::kCamNotFinite;
    bool on_plane = false, outside = false;
    volatile float world_max = 0.0f + (float)c->world.size;
    for (int k = 0; k < 3; k++) {
        volatile float fl = floorf(o[k]);
        volatile float frac = o[k] - fl;
        if (frac < 0.001f) on_plane = true;
        if (o[k] <= 0.0f || o[k] >= world_max) outside = true;
    }
    if (on_plane) f |= vrt::kCamOnPlane;
    if (outside) f |= vrt::kCamOutside;
    *facts = f;
}

// ray_sky's sun_dir for a ray starting at the camera (ray_tracer.wgsl:149, origin = cam.pos - world.min :169).
static void cam_sun_dir(const vrt_ctx *c, float out[3]) {
    volatile float d[3];
    for (int k = 0; k < 3; k++) {
        volatile float wm = (float)c->world.min[k];
        volatile float origin = c->cam.pos[k] - wm;
        volatile float a = c->settings.sun_pos[k] - wm;
        d[k] = a - origin;
    }
    volatile float xx = d[0] * d[0], yy = d[1] * d[1], zz = d[2] * d[2];
    volatile float s = xx + yy;
    volatile float dot = s + zz;
    volatile float len = sqrtf(dot);
    for (int k = 0; k < 3; k++) { volatile float q = d[k] / len; out[k] = q; }
}

// Fold the event triples of all frames rendered since the last call into acc_ms (synchronises).
static int fold_events(vrt_ctx *c, float last[3]) {
    if (c->ev_used == 0) return VRT_OK;
    QUIESCE(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < c->ev_used; i++) {
        auto &t = c->ev_pool[i];
        float a = 0, b = 0, tot = 0;
        switch (c->ev_kind[i]) {
            case kEvOneKernel:
                HIP_TRY(c, hipEventElapsedTime(&a, t[0], t[1]));
                tot = a;
                break;
            case kEvTwoKernels:
                HIP_TRY(c, hipEventElapsedTime(&a, t[0], t[1]));
                HIP_TRY(c, hipEventElapsedTime(&b, t[2], t[3]));
                HIP_TRY(c, hipEventElapsedTime(&tot, t[0], t[3]));
                break;
            case kEvRecorded:
                HIP_TRY(c, hipEventElapsedTime(&a, t[0], t[1]));
                HIP_TRY(c, hipEventElapsedTime(&b, t[1], t[3]));
                HIP_TRY(c, hipEventElapsedTime(&tot, t[0], t[3]));
                break;
            default:
                continue;  // an empty shard: nothing was launched
        }
        c->acc_ms[0] += a; c->acc_ms[1] += b; c->acc_ms[2] += tot;
        c->acc_frames += 1;
        if (last) { last[0] = a; last[1] = b; last[2] = tot; }
    }
    c->ev_used = 0;
    return VRT_OK;
}

// The frame's uniforms and scene pointers (everything of FrameParams that does not depend on where a frame is written).
void fill_uniforms(const vrt_ctx *c, vrt::FrameParams &P) {
    P.n_nodes = c->max_nodes;
    // only the S^3 entries the frame's WorldData describes are addressable (find_node :120-123)
    P.n_roots = c->world.size_in_chunks * c->world.size_in_chunks * c->world.size_in_chunks;
    P.width = c->width;
    P.height = c->height;
    P.tiles_x = c->tiles_x;
    // tile / tiles_x as a multiply-high: exact while tile * tiles_x < 2^32 (error of the rounded-up reciprocal x tile < 1)
    P.tiles_x_magic = (c->tiles_x > 1u && (uint64_t)c->tiles_total * c->tiles_x < (1ull << 32)) ? (uint32_t)(((1ull << 32) + c->tiles_x - 1u) / c->tiles_x) : 0u;
    P.tiles_total = c->tiles_total;
    P.shard_first = c->shard_first;
    P.shard_run = c->shard_run;
    P.shard_period = c->shard_period;
    P.tiles_local = c->tiles_local;
    P.tile_major = c->tile_major ? 1u : 0u;
    P.compact = c->compact ? 1u : 0u;
    P.cam = c->cam;
    P.settings = c->settings;
    P.world = c->world;
    const vrt_settings &s = c->settings;
    P.finite_settings = std::isfinite(s.sun_intensity) && std::isfinite(s.sky_color[0]) && std::isfinite(s.sky_color[1]) &&
                        std::isfinite(s.sky_color[2]) && std::isfinite(s.sun_pos[0]) && std::isfinite(s.sun_pos[1]) &&
                        std::isfinite(s.sun_pos[2]);
    memcpy(P.liquid, c->liquid_mask, sizeof P.liquid);
    P.liquid_is_range = c->liquid_is_range ? 1u : 0u;
    P.liquid_lo = c->liquid_lo;
    P.liquid_span = c->liquid_span;

    P.shadow_below = vrt::kAirLeaf;   // (no sun marks: vrt_render hands them to the frames that take them)
    P.lit_trips = 0u;

    P.ndc_x = c->d_ndc;
    P.ndc_y = c->d_ndc + c->width;
    cam_sun_dir(c, P.cam_sun_dir);
    cam_origin_facts(c, P.cam_origin, &P.cam_origin_facts);
    for (int k = 0; k < 3; k++) {
        volatile float wm = (float)c->world.min[k];
        volatile float a = c->settings.sun_pos[k] - wm;
        P.sun_local[k] = a;
    }
    {
        volatile float wmax = 0.0f + (float)c->world.size;
        P.world_max = wmax;
    }

}

// Where one frame runs and what it writes: the caller's stream and the current output, or — frames in flight — one of
// the context's own (stream, output, launched-ray counts, path buffers, cursors) sets.
struct FrameSet {
    uint32_t slot = 0;   // 0: the context's own set, k: extra set k - 1
    hipStream_t st;
    vrt::Texel *out;
    uint32_t *blk;
    vrt_ctx::Buf<uint4> *path_buf;
    unsigned long long *counters;
};

// A pipelined frame (vrt_frame_plan.h) takes the next of the context's sets in turn; any other waits for the frames in flight
// and runs alone on c->stream.
static int pick_frame_set(vrt_ctx *c, const vrt::FramePlan &plan, FrameSet &f) {
    const bool bound = c->d_out != c->sz.own_out;
    f = FrameSet{0u, c->stream, c->d_out, c->sz.d_blk_counts, &c->sz.d_path, c->d_counters};
    if (!plan.pipelined) {
        QUIESCE(c);
        return VRT_OK;
    }
    if (c->flip) {
        const uint32_t k = c->flip - 1u;
        f.slot = k + 1u;
        if (plan.path) {
            HIP_TRY(c, c->extra_counters[k].once(kCounterWords));
            f.counters = c->extra_counters[k];
            f.path_buf = &c->sz.extra_path[k];
        }
        HIP_TRY(c, c->extra_stream[k].ensure());
        if (!bound) VRT_TRY(frame_buf(c, c->sz.extra_out[k], frame_slots(c)));   // texels no workgroup covers stay zero (main.rs:452)
        HIP_TRY(c, c->sz.extra_blk[k].once(c->tiles_local ? c->tiles_local : 1));
        f.st = c->extra_stream[k];
        f.blk = c->sz.extra_blk[k];
        if (!bound) f.out = c->sz.extra_out[k];  // a bound output is the caller's buffer for this very frame
        c->alt_pending = true;
        VRT_TRY(frame_waits_for_uploads(c, f.st, k + 1u));
    } else if (c->stream != c->own_stream) {
        f.st = c->own_stream;
        c->own_pending = true;
        VRT_TRY(frame_waits_for_uploads(c, f.st, 0u));
    }
    c->flip = (c->flip + 1u) % c->in_flight;
    return VRT_OK;
}

// The next free event quadruple of the pool (folding the pool into the accumulated times when it is full), as raw handles.
static int next_events(vrt_ctx *c, std::array<hipEvent_t, 4> &ev, uint8_t **kind) {
    if (c->ev_used == c->ev_pool.size()) {
        // (512 frames of events: creating one costs the host a few microseconds, so a context is at full speed once it has
        // rendered that many frames between two vrt_get_stats calls; folding costs one drain per 512 frames)
        if (c->ev_pool.size() >= 512) {
            VRT_TRY(fold_events(c, nullptr));
        } else {
            std::array<vrt_ctx::Event, 4> t;   // (joins the pool whole or not at all)
            for (auto &e : t) HIP_TRY(c, e.ensure(hipEventDefault));
            c->ev_pool.push_back(std::move(t));
            c->ev_kind.push_back(kEvNone);
        }
    }
    *kind = &c->ev_kind[c->ev_used];
    **kind = kEvNone;
    const auto &t = c->ev_pool[c->ev_used++];
    ev = {t[0], t[1], t[2], t[3]};
    return VRT_OK;
}

// VRT_RENDER_ACCUMULATE: is the frame allowed, and how many samples does the sum hold before it (0: it starts again)?
// Checked before anything is enqueued.
int accum_frame_start(vrt_ctx *c, const vrt_render_opts &o, uint32_t *from) {
    *from = 0;
    if (!(o.flags & VRT_RENDER_ACCUMULATE)) return VRT_OK;
    if (o.mode != VRT_MODE_PATH) return fail(c, VRT_ERR_INVALID_ARG, "vrt_render: VRT_RENDER_ACCUMULATE is for VRT_MODE_PATH frames (mode %u)", o.mode);
    const uint32_t spp = o.spp ? o.spp : 1u;
    const uint32_t n = (c->accum_restart || o.seed != c->accum_seed) ? 0u : c->accum_n;
    if ((uint64_t)n + spp > (1ull << 24))
        return fail(c, VRT_ERR_OUT_OF_RANGE, "vrt_render: %u accumulated + %u samples > 2^24 (past it the count is not exact in f32)", n, spp);
    *from = n;
    return VRT_OK;
}

// Wavefront path trace: the launches vrt_frame_plan.h's plan_path decided on, enqueued in for_each_path_step's order.
static_assert(vrt::kPlanHitSegments == vrt::kHitSegments, "the plan sizes the path buffers");
static int launch_path_frame(vrt_ctx *c, vrt::FrameParams &P, const FrameSet &f, uint32_t tab, const vrt::PathPlan &plan, std::array<hipEvent_t, 4> &ev,
                             uint8_t &ev_kind) {
    // two sets of three record planes; grows only, and hipFree waits for whatever still uses the old one
    HIP_TRY(c, f.path_buf->grow(6 * plan.cap));
    if (plan.needs_acc_planes) VRT_TRY(frame_buf(c, c->sz.path_acc[f.slot], (size_t)plan.samples * c->slots));   // (grows with the samples of a chain)
    if (plan.needs_accum_sum) {   // (dropped by a resize, with the accumulation: the first frame stores the sum whole)
        VRT_TRY(frame_buf(c, c->sz.d_accum, frame_slots(c)));
        HIP_TRY(c, c->ev_accum.ensure());
    }
    // what a frame's kernels read from the launch instead of being built per combination: the coat's coin, the pass-through draw
    const uint32_t lobes = (plan.polish ? vrt::kSunLobePolish : 0u) | (plan.translucent ? vrt::kSunLobeTranslucent : 0u);
    // The record buffer of a light's rays (the sun's, the lamps'), the frame set's own: three planes of plan.cap records and two
    // cursor sets, zero when the frame starts; the fields every such launch struct has
    auto light_rays = [&](vrt_ctx::Buf<uint4> &recs, vrt_ctx::Buf<uint32_t> &counts, auto &launch, uint32_t *(&seg)[2]) -> int {
        constexpr size_t kSegWords = (size_t)vrt::kHitSegments * vrt::kSegStride;
        HIP_TRY(c, recs.grow(3 * plan.cap));
        HIP_TRY(c, counts.once(2 * kSegWords));
        seg[0] = counts;
        seg[1] = seg[0] + kSegWords;
        HIP_TRY(c, hipMemsetAsync(seg[0], 0, 2 * kSegWords * sizeof(uint32_t), f.st));
        launch.recs = recs;
        launch.cap = (uint32_t)plan.cap;
        launch.seg_cap = plan.seg_cap;
        launch.lobes = lobes;
        return VRT_OK;
    };
    vrt::SunLaunch S{};
    uint32_t *sun_seg[2] = {nullptr, nullptr};
    if (plan.sun) {   // vrt_set_sun_light
        VRT_TRY(light_rays(c->sz.sun_recs[f.slot], c->sz.sun_counts[f.slot], S, sun_seg));
        S.k = c->settings.sun_intensity * c->sun.strength;   // (one binary32 product: the contract's k)
    }
    vrt::LampLaunch M{};
    uint32_t *lamp_seg[2] = {nullptr, nullptr};
    if (plan.lamp) {   // vrt_set_lamp_light: the frame set's lamp list, brought up to date on its stream, and its lamp-ray buffer
        VRT_TRY(lamp_list_for_frame(c, f.slot, tab, f.st, M));
        VRT_TRY(light_rays(c->sz.lamp_recs[f.slot], c->sz.lamp_counts[f.slot], M, lamp_seg));
        M.strength = c->lamp.strength;
        M.max_geometry = c->lamp.max_geometry;
        M.sun = plan.sun ? 1u : 0u;
    }
    // vrt_set_water_optics: the setting as the kernels of vrt_path_water.h take it
    const vrt::WaterLaunch W{{c->water.absorb[0], c->water.absorb[1], c->water.absorb[2]}, c->water.reflectance, lobes, plan.sun ? 1u : 0u};
    // vrt_set_water_refraction: the setting as the kernels of vrt_path_refract.h take it (a water frame's launches go to them).  Off:
    // X is built all the same and nothing reads it — no launch below takes it unless `refracts`
    const bool refracts = c->refraction.ior != 0.0f;
    const vrt::RefractLaunch X{c->refraction.ior, refracts ? 1.0f / c->refraction.ior : 0.0f, c->refraction.max_span, 0u};
    // vrt_set_haze: the setting as the kernels of vrt_path_haze.h take it.  Off: H is built all the same and nothing reads it
    const vrt::HazeLaunch H{plan.haze ? 1.0f / c->haze.density : 0.0f, {c->haze.albedo[0], c->haze.albedo[1], c->haze.albedo[2]}, lobes, plan.sun ? 1u : 0u};
    // vrt_set_camera_sampling: the setting as the primary kernels of vrt_path_lens.h take it
    const vrt::LensLaunch L{c->lens.pixel_spread, c->lens.aperture, c->lens.focus_distance, lobes};
    vrt::Texel *const frame_out = P.out, *const acc = c->sz.path_acc[f.slot];
    P.hit_seg_cap = plan.seg_cap;
    P.acc = plan.planes ? acc : nullptr;
    P.acc_slots = c->slots;
    P.chain = 1u;
    if (plan.planes) P.out = acc;   // what the bounce launches accumulate into, through slots that carry the plane
    constexpr uint32_t kSegWords = vrt::kHitSegments * vrt::kSegStride;
    uint32_t *const seg[3] = {P.seg_counts, P.seg_counts + kSegWords, P.seg_counts + 2 * kSegWords};
    uint4 *const buf[2] = {*f.path_buf, *f.path_buf + 3 * plan.cap};
    P.path_cap = (uint32_t)plan.cap;
    P.in_cap = (uint32_t)plan.cap;
    P.in_seg_cap = plan.seg_cap;
    P.spp = plan.spp;
    P.seed = plan.seed;
    P.sample_base = plan.sample_base;
    const bool timed = ev[0] != nullptr;
    if (timed) HIP_TRY(c, hipEventRecord(ev[0], f.st));
    if (plan.zero_output) HIP_TRY(c, hipMemsetAsync(f.out, 0, (size_t)c->slots * sizeof(vrt::Texel), f.st));
    // Only the steps that read and write the context's sum are ordered behind the previous accumulating frame's (it may be in
    // flight on another frame set's stream); this frame's launches before them overlap it
    bool sum_waited = false, first_marked = false;
    auto enqueue = [&](const vrt::PathStep &s) -> int {
        using namespace vrt;
        if (s.kind == kStepSunRays || s.kind == kStepLampRays) {   // (its trace launch's parameters, and the cursor set that launch appended to)
        } else if (traces_paths(s.kind)) {   // a launch of the trace
            P.sample = s.sample;
            P.chain = s.chain;
            P.seg_counts = seg[s.launch % 3u];
            P.seg_in = seg[(s.launch + 2u) % 3u];
            P.seg_clear = seg[(s.launch + 1u) % 3u];
            P.path_out = buf[s.launch & 1u];
            P.path_in = buf[(s.launch + 1u) & 1u];
            P.last_bounce = s.last_bounce;
            S.counts = sun_seg[s.launch & 1u];
            S.clear = sun_seg[(s.launch + 1u) & 1u];
            M.counts = lamp_seg[s.launch & 1u];
            M.clear = lamp_seg[(s.launch + 1u) & 1u];
        } else if (plan.finish_into_accum && !sum_waited) {
            if (c->accum_ev_recorded) HIP_TRY(c, hipStreamWaitEvent(f.st, c->ev_accum, 0));
            sum_waited = true;
        }
        switch (s.kind) {
            case kStepPrimary:
                if (plan.lens) launch_path_primary_lens(P, L, plan.kstats, plan.literal, f.st);
                else launch_path_primary(P, plan.kstats, plan.literal, plan.emit, plan.polish, plan.translucent, f.st);
                break;
            case kStepLaneBounce: launch_path_bounce(P, plan.kstats, plan.literal, plan.emit, plan.polish, plan.translucent, f.st); break;
            case kStepCellsBounce: launch_path_bounce_cells(P, plan.refill, s.segments, plan.pool_batches, plan.emit, plan.polish, plan.translucent, f.st); break;
            case kStepSunlitPrimary:
                if (plan.lens) launch_path_primary_lens_sunlit(P, L, S, plan.kstats, plan.literal, f.st);
                else launch_path_primary_sunlit(P, S, plan.kstats, plan.literal, f.st);
                break;
            case kStepSunlitBounce: launch_path_bounce_sunlit(P, S, plan.kstats, plan.literal, f.st); break;
            case kStepSunRays: launch_path_sun(P, S, plan.kstats, plan.literal, plan.sun_cells, f.st); break;
            case kStepLampPrimary: launch_path_primary_lamp(P, L, S, M, plan.lens, plan.kstats, plan.literal, f.st); break;
            case kStepLampBounce: launch_path_bounce_lamp(P, S, M, plan.kstats, plan.literal, f.st); break;
            case kStepLampRays: launch_path_lamp_rays(P, M, plan.kstats, plan.literal, f.st); break;
            case kStepWaterPrimary:
                if (refracts) launch_path_primary_refract(P, W, S, X, plan.kstats, plan.literal, f.st);
                else launch_path_primary_water(P, W, S, plan.kstats, plan.literal, f.st);
                break;
            case kStepWaterBounce:
                if (refracts) launch_path_bounce_refract(P, W, S, X, plan.kstats, plan.literal, f.st);
                else launch_path_bounce_water(P, W, S, plan.kstats, plan.literal, f.st);
                break;
            case kStepHazePrimary: launch_path_primary_haze(P, H, S, plan.kstats, plan.literal, f.st); break;
            case kStepHazeBounce: launch_path_bounce_haze(P, H, S, plan.kstats, plan.literal, f.st); break;
            case kStepChainFinish:
                launch_path_chain_finish(plan.finish_into_accum ? c->sz.d_accum.get() : frame_out, frame_out, acc, c->slots, s.chain, s.first, s.last, s.count, f.st);
                break;
            case kStepResolve:
                launch_path_accum_resolve(frame_out, plan.finish_into_accum ? c->sz.d_accum.get() : acc, c->slots, s.first, s.last, s.count, f.st);
                break;
            case kStepFinalDivide: launch_path_finish(frame_out, c->slots, s.count, f.st); break;
        }
        HIP_TRY(c, hipGetLastError());
        if (!first_marked && timed) HIP_TRY(c, hipEventRecord(ev[1], f.st));   // (behind the frame's first launch)
        first_marked = true;
        return VRT_OK;
    };
    int rc = VRT_OK;
    vrt::for_each_path_step(plan, [&](const vrt::PathStep &s) { if (!rc) rc = enqueue(s); });
    P.out = frame_out;
    VRT_TRY(rc);
    if (!first_marked && timed) HIP_TRY(c, hipEventRecord(ev[1], f.st));   // (a frame without a launch)
    if (sum_waited) {
        HIP_TRY(c, hipEventRecord(c->ev_accum, f.st));
        c->accum_ev_recorded = true;
    }
    if (timed) {
        HIP_TRY(c, hipEventRecord(ev[3], f.st));
        ev_kind = kEvRecorded;
    }
    return VRT_OK;
}

// Primary (+ shadow) rays: one launch (plan.one_launch) or two.
static int launch_march_frame(vrt_ctx *c, const vrt::FrameParams &P, const FrameSet &f, const vrt::FramePlan &plan, std::array<hipEvent_t, 4> &ev,
                              uint8_t &ev_kind) {
    if (!c->tiles_local) return VRT_OK;  // an empty shard
    if (plan.shadow && plan.one_launch) vrt::launch_primary_shadow_fused(P, plan.march, plan.kstats, f.st, ev[0], ev[1]);
    else vrt::launch_primary(P, plan.march, plan.kstats, plan.shadow, f.st, ev[0], ev[1]);
    HIP_TRY(c, hipGetLastError());
    if (ev[0]) ev_kind = kEvOneKernel;
    if (!plan.one_launch) {
        vrt::launch_shadow(P, plan.march, plan.kstats, f.st, ev[2], ev[3]);
        HIP_TRY(c, hipGetLastError());
        if (ev[0]) ev_kind = kEvTwoKernels;
    }
    return VRT_OK;
}


extern "C" {

int vrt_create(const vrt_config *cfg, vrt_ctx **out) {
    if (!cfg || !out) return fail(nullptr, VRT_ERR_INVALID_ARG, "vrt_create: null argument");
    *out = nullptr;
    if (cfg->n_devices > 1u) return grp_create(cfg, out);
    // (2^17 nodes of headroom: a chunk rebuild stages up to a chunk's 32 767 + 24 nodes behind a root in one run of 16-byte loads,
    // whose byte offsets must not wrap — vrt_accel.hip)
    if (cfg->max_nodes < 2 || cfg->max_nodes > 0x7FFE0000u)
        return fail(nullptr, VRT_ERR_INVALID_ARG, "max_nodes must be in [2, 2^31 - 2^17] (the pool is addressed through a 32-bit byte offset)");
    if (cfg->width == 0 || cfg->height == 0)
        return fail(nullptr, VRT_ERR_INVALID_ARG, "output %ux%u: dimensions must be non-zero", cfg->width, cfg->height);
    if ((uint64_t)cfg->width * cfg->height > (1ull << 28))
        return fail(nullptr, VRT_ERR_INVALID_ARG, "output too large");
    const uint32_t sc = cfg->shard_count ? cfg->shard_count : 1u;
    if (cfg->shard_rank >= sc) return fail(nullptr, VRT_ERR_INVALID_ARG, "shard_rank %u >= shard_count %u", cfg->shard_rank, sc);
    if (cfg->shard_root_weight > 4096u) return fail(nullptr, VRT_ERR_INVALID_ARG, "shard_root_weight %u out of range", cfg->shard_root_weight);
    if ((cfg->flags & VRT_FLAG_ROW_MAJOR) && (cfg->flags & VRT_FLAG_TILE_MAJOR))
        return fail(nullptr, VRT_ERR_INVALID_ARG, "VRT_FLAG_ROW_MAJOR and VRT_FLAG_TILE_MAJOR exclude each other");
    if ((cfg->flags & VRT_FLAG_COMPACT) && ((cfg->flags & VRT_FLAG_ROW_MAJOR) || (sc == 1u && !(cfg->flags & VRT_FLAG_TILE_MAJOR))))
        return fail(nullptr, VRT_ERR_INVALID_ARG, "VRT_FLAG_COMPACT is for tile-major shard buffers");

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(nullptr, VRT_ERR_DEVICE, "no HIP device available (%s)", hipGetErrorString(e));
    int dev = cfg->device;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    }
    if (dev >= ndev) return fail(nullptr, VRT_ERR_INVALID_ARG, "device %d out of range (%d devices)", dev, ndev);

    vrt_ctx *c = new (std::nothrow) vrt_ctx();
    if (!c) return fail(nullptr, VRT_ERR_OOM, "host allocation failed");
    c->device = dev;
    c->shard_rank = cfg->shard_rank;
    c->shard_count = sc;
    c->shard_w0 = cfg->shard_root_weight ? cfg->shard_root_weight : 1u;
    c->tile_major = (sc > 1u && !(cfg->flags & VRT_FLAG_ROW_MAJOR)) || (cfg->flags & VRT_FLAG_TILE_MAJOR);
    c->compact = (cfg->flags & VRT_FLAG_COMPACT) != 0;
    c->width = cfg->width;
    c->height = cfg->height;
    c->max_nodes = cfg->max_nodes & ~1u;  // NodeBuffer::new forces an even size (shader.rs:10-12)
    c->accel_max_s = kAccelMaxS;
    if (const char *e = getenv("VRT_ACCEL_MAX_S")) {
        const long v = strtol(e, nullptr, 10);
        if (v >= 0 && v < (long)kAccelMaxS) c->accel_max_s = (uint32_t)v;
    }
    c->march_direct_max_s = kMarchDirectMaxS;
    if (const char *e = getenv("VRT_MARCH_DIRECT_MAX_S")) {
        const long v = strtol(e, nullptr, 10);
        if (v >= 0 && v <= (long)kMarchDirectMaxS) c->march_direct_max_s = (uint32_t)v;
    }
    if (const char *e = getenv("VRT_TILE_ORDER")) c->tile_lpt = e[0] != '0';
    if (const char *e = getenv("VRT_SUN_MARKS")) c->sun_marks = e[0] != '0';
    if (const char *e = getenv("VRT_LIT_VOXELS")) c->lit_voxels = e[0] != '0';
    if (const char *e = getenv("VRT_LIT_VOXEL_LAYERS")) { const long v = atol(e); if (v >= 0 && v <= 4096) c->lit_voxel_layers = (int)v; }
    if (const char *e = getenv("VRT_DARK_MARKS")) c->dark_marks = e[0] != '0';
    if (const char *e = getenv("VRT_DARK_VOXEL_LAYERS")) { const long v = atol(e); if (v >= 0 && v <= 4096) c->dark_voxel_layers = (int)v; }
    if (const char *e = getenv("VRT_DARK_DEPTH")) { const long v = atol(e); if (v >= 0 && v <= 4096) c->dark_depth = (int)v; }
    if (const char *e = getenv("VRT_LIT_SLAB")) { const long v = atol(e); if (v >= 1 && v <= 4096) c->lit_slab = (uint32_t)v; }
    // (0: screen order while the view moves — profiles/r05_tile_order_moving.txt)
    if (const char *e = getenv("VRT_TILE_ORDER_MOVING")) c->tile_lpt_moving = e[0] != '0' ? 1u : 0u;
    c->mov_any_size = getenv("VRT_TILE_ORDER_MOVING") != nullptr;   // (asked for by name: also for frames larger than kMovingTilesMax)
    if (const char *e = getenv("VRT_TILE_ORDER_RADIUS")) { const int v = atoi(e); if (v >= 1 && v <= 6) c->mov_radius = (uint32_t)v; }
    if (const char *e = getenv("VRT_PATH_POOL")) c->path_pool = e[0] != '0';
    if (const char *e = getenv("VRT_LAMP_CAP")) { const long v = atol(e); if (v >= 1 && v <= (1l << 24)) c->lamp_cap = (uint32_t)v; }   // (tests: a list that is cut off)
    if (const char *e = getenv("VRT_TONE_BLOCKS")) { const long v = atol(e); if (v >= 1 && v <= 65536) c->tone_blocks = (uint32_t)v; }   // (docs/KERNELS.md: the sweep)
    if (const char *e = getenv("VRT_PATH_CELLS")) c->path_cells = e[0] != '0';
    if (const char *e = getenv("VRT_PATH_POOL_REFILL")) c->path_refill = (uint32_t)atoi(e);
    if (const char *e = getenv("VRT_PATH_POOL_K")) { const int v = atoi(e); if (v == 4 || v == 5) c->path_pool_batches = (uint32_t)v; }
    if (const char *e = getenv("VRT_PATH_SAMPLES_PER_CHAIN")) { const int v = atoi(e); if (v >= 1 && v <= 16) c->path_samples = (uint32_t)v; }
    if (const char *e = getenv("VRT_TIMING_EVERY")) { const long v = strtol(e, nullptr, 10); if (v >= 1 && v <= 1000000) c->timing_every = (uint32_t)v; }
    memset(c->h_mats, 0, sizeof c->h_mats);
    memset(c->h_emission, 0, sizeof c->h_emission);
    memset(c->h_polish, 0, sizeof c->h_polish);
    memset(c->h_translucency, 0, sizeof c->h_translucency);
    memset(&c->cam, 0, sizeof c->cam);
    memset(&c->settings, 0, sizeof c->settings);
    memset(&c->world, 0, sizeof c->world);
    memset(&c->stats, 0, sizeof c->stats);

    auto body = [&]() -> int {
        HIP_TRY(c, hipSetDevice(dev));
        HIP_TRY(c, c->own_stream.ensure());
        c->stream = c->own_stream;
        HIP_TRY(c, c->d_nodes.once(c->max_nodes));
        // fresh buffer = zeros = every node an air leaf (client/src/world.rs:273-274)
        HIP_TRY(c, hipMemsetAsync(c->d_nodes, 0, (size_t)c->max_nodes * sizeof(uint16_t), c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));   // (uploads run on their own stream)
        // the upload path's fixtures now, not at the first edit (a mapped pinned allocation is tens of milliseconds)
        HIP_TRY(c, c->up_stream.ensure());
        HIP_TRY(c, c->ev_pool_upload.ensure());
        HIP_TRY(c, c->h_ring.ensure(vrt_ctx::kRingSegBytes * vrt_ctx::kRingSegs));
        HIP_TRY(c, hipHostGetDevicePointer((void **)&c->d_ring, c->h_ring, 0));
        static_assert(sizeof c->h_mats == vrt::kMaterials * sizeof(vrt_material), "the emission table follows the 256 materials");
        static_assert(vrt_ctx::kMatsAlloc * sizeof(vrt_material) == sizeof c->h_mats + sizeof c->h_emission + sizeof c->h_polish + sizeof c->h_translucency + sizeof(vrt_material),
                      "whole materials");
        // + the emission table (vrt::emission_table) + the polish table (vrt::polish_table) + the translucency table and the coat word
        HIP_TRY(c, c->d_mats.once(vrt_ctx::kMatsAlloc));
        HIP_TRY(c, hipMemsetAsync(c->d_mats, 0, vrt_ctx::kMatsAlloc * sizeof(vrt_material), c->stream));
        HIP_TRY(c, c->d_counters.once(kCounterWords));
        HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, kCounterBytes, c->stream));
        VRT_TRY(alloc_roots(c, cfg->world_size_chunks));
        VRT_TRY(alloc_output(c));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return VRT_OK;
    };
    const int rc = body();
    if (rc != VRT_OK) {
        g_create_err = c->err;
        vrt_destroy(c);
        return rc;
    }
    *out = c;
    return VRT_OK;
}

void vrt_destroy(vrt_ctx *c) {
    if (!c) return;
    if (c->grp) { grp_destroy(c); return; }
    (void)hipSetDevice(c->device);
    // nothing is destroyed or freed under work that still uses it: every stream the context owns or was given, once
    auto drain = [](hipStream_t st) { if (st) (void)hipStreamSynchronize(st); };
    if (c->stream != c->own_stream) drain(c->stream);
    drain(c->own_stream);
    drain(c->up_stream);
    for (hipStream_t st : c->extra_stream) drain(st);
    delete c;   // the buffers, events, streams and the ring go with it: behind the waits above, the context's device current
}

const char *vrt_last_error(const vrt_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int vrt_set_camera(vrt_ctx *c, const vrt_cam_data *cam) {
    GRP_EACH(c, vrt_set_camera(d, cam));
    if (!c || !cam) return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_camera: null argument");
    if (memcmp(&c->cam, cam, sizeof *cam) != 0) { c->view_gen++; c->cam_gen++; c->accum_restart = true; }
    c->cam = *cam;
    return VRT_OK;
}

int vrt_set_settings(vrt_ctx *c, const vrt_settings *s) {
    GRP_EACH(c, vrt_set_settings(d, s));
    if (!c || !s) return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_settings: null argument");
    if (memcmp(&c->settings, s, sizeof *s) != 0) { c->view_gen++; c->accum_restart = true; }
    c->settings = *s;
    return VRT_OK;
}

int vrt_set_world(vrt_ctx *c, const vrt_world_data *w) {
    GRP_EACH(c, vrt_set_world(d, w));
    if (!c || !w) return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_world: null argument");
    if (memcmp(&c->world, w, sizeof *w) != 0) { c->view_gen++; c->accum_restart = true; }
    c->world = *w;
    return VRT_OK;
}

int vrt_resize_output(vrt_ctx *c, uint32_t width, uint32_t height) {
    if (c && c->grp) return grp_resize_output(c, width, height);
    if (!c) return VRT_ERR_INVALID_ARG;
    if (width == 0 || height == 0 || (uint64_t)width * height > (1ull << 28))
        return fail(c, VRT_ERR_INVALID_ARG, "output %ux%u: dimensions must be non-zero, at most 2^28 pixels", width, height);
    HIP_TRY(c, hipSetDevice(c->device));
    QUIESCE(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->width = width;
    c->height = height;
    return alloc_output(c);
}

int vrt_render(vrt_ctx *c, const vrt_render_opts *opts) {
    if (c && c->grp) return grp_render(c, opts);
    if (!c) return VRT_ERR_INVALID_ARG;
    VRT_PROF(3, "vrt_render (one context)");
    struct IssueClock {   // vrt_get_issue_profile: the calling thread's time in here, whichever way the call leaves
        vrt_ctx *c;
        std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        ~IssueClock() {
            c->prof_render_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            c->prof_frames += 1u;
        }
    } issue_clock{c};
    vrt_render_opts o{};
    if (opts) o = *opts;
    if (o.mode > VRT_MODE_PATH) return fail(c, VRT_ERR_INVALID_ARG, "vrt_render: mode %u not supported", o.mode);
    if (o.mode == VRT_MODE_PATH && o.variant != 0) return fail(c, VRT_ERR_INVALID_ARG, "vrt_render: the path trace has one kernel variant");
    if (o.stats > 2u) return fail(c, VRT_ERR_INVALID_ARG, "vrt_render: stats %u (0, 1 = count steps, 2 = clock probe)", o.stats);
    if (o.stats == 2u && (o.mode != VRT_MODE_PRIMARY_SHADOW || (o.variant != 0u)))
        return fail(c, VRT_ERR_INVALID_ARG, "vrt_render: the clock probe (stats = 2) is a build of the default primary + shadow kernel");
    if (!vrt::variant_supported(o.variant)) return fail(c, VRT_ERR_INVALID_ARG, "vrt_render: unknown kernel variant %u", o.variant);
    const bool accum = (o.flags & VRT_RENDER_ACCUMULATE) != 0u;
    uint32_t accum_from = 0;
    VRT_TRY(accum_frame_start(c, o, &accum_from));
    {
        VRT_PROF(7, "  validate + hipSetDevice");
        VRT_TRY(validate_frame(c));
        HIP_TRY(c, hipSetDevice(c->device));
    }
    if (c->compact && (o.mode == VRT_MODE_PATH || !vrt::one_launch_march(o.variant, c->compact) || c->settings.show_step_count == 1u))
        return fail(c, VRT_ERR_STATE, "vrt_render: a VRT_FLAG_COMPACT context renders primary(+shadow) frames with the default march "
                    "only (no path trace, step-count view, literal or two-launch variants)");
    if (o.stats == 1u) VRT_TRY(frame_buf(c, c->sz.d_steps, frame_slots(c)));
    if (o.stats == 2u && !c->d_clock) {
        HIP_TRY(c, c->d_clock.once(2));
        HIP_TRY(c, hipMemsetAsync(c->d_clock, 0, 2 * sizeof(unsigned long long), c->stream));
        VRT_TRY(publish_upload(c));
    }
    {
        VRT_PROF(8, "  ensure_ndc");
        VRT_TRY(ensure_ndc(c));
    }

    // ---- plan: what kind of frame this is (vrt_frame_plan.h), decided before anything of it is enqueued ----
    vrt::FrameFacts F;
    F.mode = o.mode; F.variant = o.variant; F.stats = o.stats; F.flags = o.flags;
    F.compact = c->compact; F.show_step_count = c->settings.show_step_count == 1u; F.air_liquid = c->h_mats[0].is_liquid == 1u;
    if (F.air_liquid && c->compact)
        return fail(c, VRT_ERR_STATE, "vrt_render: materials[0].is_liquid == 1 (air flagged liquid) is traced by the literal march only");
    // vrt_set_lamp_light: a lamp-lit path frame reads the derived tables for its lamp list, whatever it marches with
    const bool lamp_lit = o.mode == VRT_MODE_PATH && c->lamp.strength != 0.0f && c->settings.max_ray_bounces > 0u;
    // vrt_set_water_optics: a water frame's kernels have no lamp term and no lens (include/vrt.h); refused before anything is enqueued
    const bool water_frame = o.mode == VRT_MODE_PATH && c->water.flags != 0u && c->settings.max_ray_bounces > 0u;
    if (water_frame && c->lamp.strength != 0.0f)
        return fail(c, VRT_ERR_STATE, "vrt_render: water optics (vrt_set_water_optics) and lamp light (vrt_set_lamp_light) do not compose yet");
    if (water_frame && (c->lens.pixel_spread != 0.0f || c->lens.aperture != 0.0f))
        return fail(c, VRT_ERR_STATE, "vrt_render: water optics (vrt_set_water_optics) and camera sampling (vrt_set_camera_sampling) do not compose yet");
    // vrt_set_haze: a haze frame's kernels have no water, no lamp term and no lens (include/vrt.h); refused in the same way
    const bool haze_frame = o.mode == VRT_MODE_PATH && c->haze.density != 0.0f && c->settings.max_ray_bounces > 0u;
    if (haze_frame && c->water.flags != 0u)
        return fail(c, VRT_ERR_STATE, "vrt_render: haze (vrt_set_haze) and water optics (vrt_set_water_optics) do not compose yet");
    if (haze_frame && c->lamp.strength != 0.0f)
        return fail(c, VRT_ERR_STATE, "vrt_render: haze (vrt_set_haze) and lamp light (vrt_set_lamp_light) do not compose yet");
    if (haze_frame && (c->lens.pixel_spread != 0.0f || c->lens.aperture != 0.0f))
        return fail(c, VRT_ERR_STATE, "vrt_render: haze (vrt_set_haze) and camera sampling (vrt_set_camera_sampling) do not compose yet");
    if (vrt::asks_for_tables(F) || lamp_lit) {
        VRT_PROF(9, "  ensure_accel_world");
        VRT_TRY(ensure_accel_world(c));
    }
    if (lamp_lit && (!c->accel_ok || c->accel_dirty || c->accel_S != c->world.size_in_chunks))   // (before anything of the frame is enqueued)
        return fail(c, VRT_ERR_STATE, "vrt_render: a lamp-lit frame (vrt_set_lamp_light) needs the derived tables, which this world does not keep");
    F.accel_ok = c->accel_ok; F.in_flight = c->in_flight; F.tiles_local = c->tiles_local;
    F.caller_stream = c->stream != c->own_stream; F.output_bound = c->d_out != c->sz.own_out; F.present_fusable = presentation_fusable(c);
    const vrt::FramePlan plan = vrt::plan_frame(F);

    // ---- enqueue.  What is in flight is announced ahead of the launches it speaks of (own_pending, alt_pending, shared_readers_in_flight,
    // walkers_in_flight) and stays announced if the call fails further down: that costs a wait, the opposite a race.  No part of the record. ----
    FrameSet f;
    {
        VRT_PROF(10, "  pick_frame_set (+ its upload waits)");
        VRT_TRY(pick_frame_set(c, plan, f));
    }
    if (c->wait_before_frame) {
        HIP_TRY(c, hipStreamWaitEvent(f.st, c->wait_before_frame, 0));
        c->wait_before_frame = nullptr;
    }

    // this frame's table set, brought up to date on its own stream (which waits for the uploads so far first)
    constexpr uint32_t kQuietFrames = 64;
    if (c->tables_split && ++c->quiet_frames > kQuietFrames && c->tabs[0].dirty_chunks.empty()) {
        c->tables_split = false;   // no edit for a while: everybody reads tabs[0] again; the other sets go stale
        for (uint32_t k = 1; k < vrt_ctx::kMaxInFlight; k++) c->tabs[k].live = false;
    }
    const uint32_t tab = c->tables_split ? f.slot : 0u;
    const vrt_ctx::Tables &T = c->tabs[tab];
    const bool edit_in_front = !T.dirty_chunks.empty();   // this frame brings an edited chunk's tables up to date first
    // a frame of another frame set that reads the shared set: an edit's update of tabs[0] must wait for it (update_tables)
    const bool reads_tables = plan.tables || lamp_lit;
    const bool shares = reads_tables && tab == 0u && f.slot != 0u;
    {
        VRT_PROF(11, "  frame_waits_for_uploads + update_tables");
        VRT_TRY(frame_waits_for_uploads(c, f.st, f.slot));   // (a frame on c->stream too: the node pool's uploads have their own stream)
        if (reads_tables) VRT_TRY(update_tables(c, tab, f.st));
    }
    if (shares) {   // the shared set from another frame set's stream: behind its last update
        if (c->tabs[0].update_pending && f.st != c->stream) HIP_TRY(c, hipStreamWaitEvent(f.st, c->tabs[0].ev_updated, 0));
        c->shared_readers_in_flight = true;
    }

    vrt::FrameParams P;
    memset(&P, 0, sizeof P);
    P.nodes = c->d_nodes;
    P.roots = c->d_roots;
    P.mats = c->d_mats;
    if (plan.tables && c->accel_S == c->world.size_in_chunks && !c->accel_dirty && T.live && T.dirty_chunks.empty()) {
        P.grid = T.d_grid;
        P.bricks = T.d_bricks;
        P.grid_dim = c->accel_S * 8u;
        P.grid_bytes = (uint32_t)(grid_entries(c->accel_S) * sizeof(uint32_t));  // [8S][8S+1][8S+1]: the zero border
        P.brick_bytes = (uint32_t)((size_t)T.brick_cap() * 64u * sizeof(uint16_t));
        if (T.d_mblk) {
            P.cdir = T.d_cdir;
            P.cdir_bytes = (uint32_t)(chunk_dir_entries(c->accel_S) * sizeof(uint32_t));
            P.mblk = T.d_mblk;
            // (a direct world: exactly its lines — a position beyond the last slab must be out of range, it reads as zeros)
            P.mblk_bytes = (uint32_t)(c->march_direct ? direct_cell_entries(c->accel_S) * sizeof(uint4) : (size_t)T.mblk_cap() * 512u * sizeof(uint4));
            P.march_direct = c->march_direct ? 1u : 0u;
        }
    }
    // what reads the node pool and chunk_roots: uploads then wait for the frames in flight
    // (a water frame's kernels read chunk_roots for the voxel a segment starts in: vrt_water.h)
    if (!P.grid || plan.walks_octree || water_frame) c->walkers_in_flight = true;
    P.out = f.out;
    P.hits = c->sz.d_hits;
    P.blk_counts = f.blk;
    P.counters = f.counters;
    P.seg_counts = reinterpret_cast<uint32_t *>(f.counters + vrt::kCtrCount);
    P.hit_seg_cap = c->hit_seg_cap;
    P.steps = o.stats == 1u ? c->sz.d_steps : nullptr;
    P.clock = o.stats == 2u ? c->d_clock : nullptr;
    fill_uniforms(c, P);
    // the shadow rays of the one-launch frame stop at lit cells: this set's sun marks, made now if the tables or the sun changed
    if (P.grid && plan.shadow && plan.variant == 0u && !plan.kstats) VRT_TRY(sun_marks_for_frame(c, tab, f.st, shares, P));
    if (plan.fuse_present) {
        VRT_TRY(screen_buffer_for_frame(c, f.slot, f.st, c->width, c->height));
        P.screen = reinterpret_cast<uint32_t *>(c->d_screen[f.slot].get());
        P.screen_only = (c->pres_flags & VRT_PRESENT_SKIP_TEXELS) ? 1u : 0u;
        memcpy(P.present_box, c->pres_box, sizeof P.present_box);
        P.crosshair = c->pres_ch;
    }

    // an untimed frame: the launches carry no events (vrt_stats' kernel times average the timed ones)
    std::array<hipEvent_t, 4> ev{nullptr, nullptr, nullptr, nullptr};
    uint8_t no_kind = kEvNone, *ev_kind = &no_kind;
    if (!(c->timing_every > 1u && (c->frame_no++ % c->timing_every) != 0u && !plan.kstats && !(o.flags & VRT_RENDER_TIMED))) {
        VRT_PROF(12, "  next_events");
        VRT_TRY(next_events(c, ev, &ev_kind));
    }
    // The frame is about to be enqueued on its stream: say so again.  pick_frame_set announced it, but what ran since may
    // have waited for the frames in flight and cleared the announcement with them — next_events folds the event pool every
    // 512 timed frames and drains for it.  Without this the frame was in flight unannounced: vrt_read_output right behind it
    // copied the slot's previous frame (tools/soak_edits.py seed 7, check 1161: once in 180 000 frames), and an upload
    // would not have waited for it.
    if (f.st != c->stream) {
        if (f.st == c->own_stream) c->own_pending = true;
        else c->alt_pending = true;
    }
    // (the same drain clears shared_readers_in_flight: without this an edit right behind the fold frame let the next slot-0
    // frame rebuild chunks of tabs[0] in place while this frame still read them)
    if (shares) c->shared_readers_in_flight = true;
    // the order this frame's tiles are launched in, and whether it notes its trips for an order to come (vrt_order.hip)
    TileOrderPlan order_plan;
    VRT_TRY(tile_order_before_frame(c, P, f.st, plan, edit_in_front, order_plan));
    // the counters feed stats frames and the path trace's segment cursors; a plain primary(+shadow) frame reads none
    if (plan.kstats || plan.path) HIP_TRY(c, hipMemsetAsync(f.counters, 0, kCounterBytes, f.st));
    vrt_tone_map frame_tone{};          // (a primary frame is never mapped)
    const float *tone_E = nullptr;
    {
        VRT_PROF(13, "  the launch(es)");
        int rc;
        if (plan.path) {
            // vrt_set_denoise: a frame of an odd number of passes is traced into its scratch frame (the last pass lands in f.out)
            FrameSet ft = f;
            VRT_TRY(denoise_before_frame(c, f.slot, f.out, &ft.out));
            P.out = ft.out;
            vrt::PathFacts PF;
            PF.spp = o.spp ? o.spp : 1u; PF.seed = o.seed; PF.bounces = c->settings.max_ray_bounces;
            PF.kstats = plan.kstats; PF.literal = plan.literal;
            PF.has_grid = P.grid != nullptr; PF.has_cells = P.mblk != nullptr; PF.march_direct = P.march_direct != 0u;
            PF.accum = accum; PF.accum_from = accum_from; PF.emissive = c->n_emissive != 0u; PF.polished = c->n_polished != 0u; PF.translucent = c->n_translucent != 0u;
            PF.sun = c->sun.strength != 0.0f;
            PF.lamp = c->lamp.strength != 0.0f;
            PF.water = c->water.flags != 0u;
            PF.haze = c->haze.density != 0.0f;
            PF.camera_sampling = c->lens.pixel_spread != 0.0f || c->lens.aperture != 0.0f;
            PF.path_samples = c->path_samples; PF.path_pool = c->path_pool; PF.path_cells = c->path_cells;
            PF.path_pool_batches = c->path_pool_batches; PF.path_refill = c->path_refill;
            PF.in_flight = c->in_flight; PF.hit_seg_cap = c->hit_seg_cap;
            rc = launch_path_frame(c, P, ft, tab, vrt::plan_path(PF), ev, *ev_kind);
            // (a timed frame's closing event is recorded again behind the filter: vrt_stats and VRT_RENDER_TIMED time it with its passes)
            if (!rc) rc = denoise_after_frame(c, P, plan, f.slot, f.st, f.out, ev[3]);
            // vrt_set_tone_map: the colours the frame's texels now hold are metered (VRT_TONE_AUTO), and the setting is the frame's
            if (!rc) rc = tone_after_frame(c, f.slot, f.st, f.out, ev[3], &tone_E);
            frame_tone = c->tone;
        }
        else rc = launch_march_frame(c, P, f, plan, ev, *ev_kind);
        if (rc) {
            if (accum) c->accum_restart = true;   // (what the sum holds is not known)
            return rc;
        }
    }
    if (accum) {
        c->accum_n = accum_from + (o.spp ? o.spp : 1u);
        c->accum_seed = o.seed;
        c->accum_restart = false;
    }
    VRT_TRY(tile_order_after_frame(c, P, f.st, order_plan));   // (the sort behind the frame that noted its trips)

    // ---- record: the frame is enqueued; from here on the read-backs, the presentation and the statistics speak of it ----
    c->last = vrt_ctx::LastFrame{f.out, f.blk, plan.counts_per_tile ? c->tiles_local : c->n_blocks, f.st, f.slot, tab, o.mode, o.spp ? o.spp : 1u,
                                 plan.fuse_present, !(plan.fuse_present && P.screen_only), o.stats == 1u, frame_tone, tone_E};
    c->rendered = true;
    c->flushed_at_call = false;   // (the next frame's first staged range may go out at its call again: vrt_uploads.hip)
    c->timing_pending = true;
    return VRT_OK;
}

int vrt_set_sun_light(vrt_ctx *c, const vrt_sun_light *opts) {
    if (!c) return VRT_ERR_INVALID_ARG;
    vrt_sun_light o;
    memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    if (!(o.strength >= 0.0f) || std::isinf(o.strength))
        return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_sun_light: strength %g (0 = off, or a finite positive number)", (double)o.strength);
    if (o.flags || o._reserved[0] || o._reserved[1]) return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_sun_light: flags and _reserved must be 0");
    GRP_EACH(c, vrt_set_sun_light(d, opts));
    if (o.strength == 0.0f) memset(&o, 0, sizeof o);   // (-0: off is 16 zero bytes)
    if (memcmp(&c->sun, &o, sizeof o) != 0) c->accum_restart = true;
    c->sun = o;
    return VRT_OK;
}

int vrt_set_water_optics(vrt_ctx *c, const vrt_water_optics *opts) {
    if (!c) return VRT_ERR_INVALID_ARG;
    vrt_water_optics o;
    memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    if (o.flags & ~VRT_WATER_ON) return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_water_optics: flags %#x (0 or VRT_WATER_ON)", o.flags);
    if (o._reserved[0] || o._reserved[1] || o._reserved[2]) return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_water_optics: _reserved must be 0");
    for (float a : o.absorb)   // (checked whatever the flags say)
        if (!(a >= 0.0f) || std::isinf(a))
            return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_water_optics: absorb %g %g %g (each finite and >= 0)", (double)o.absorb[0], (double)o.absorb[1],
                        (double)o.absorb[2]);
    if (!(o.reflectance >= 0.0f && o.reflectance <= 1.0f))
        return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_water_optics: reflectance %g (in [0, 1])", (double)o.reflectance);
    GRP_EACH(c, vrt_set_water_optics(d, opts));
    // what is kept: off is 32 zero bytes, -0 is +0
    if (!o.flags) memset(&o, 0, sizeof o);
    for (float &a : o.absorb) if (a == 0.0f) a = 0.0f;
    if (o.reflectance == 0.0f) o.reflectance = 0.0f;
    if (memcmp(&c->water, &o, sizeof o) != 0) c->accum_restart = true;
    c->water = o;
    return VRT_OK;
}

int vrt_set_haze(vrt_ctx *c, const vrt_haze *opts) {
    if (!c) return VRT_ERR_INVALID_ARG;
    vrt_haze o;
    memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    if (!(o.density == 0.0f || (o.density >= 0x1p-20f && o.density <= 64.0f)))
        return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_haze: density %g (0 = off, or in [2^-20, 64])", (double)o.density);
    for (float a : o.albedo)   // (checked whatever the density is)
        if (!(a >= 0.0f && a <= 1.0f))
            return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_haze: albedo %g %g %g (each in [0, 1])", (double)o.albedo[0], (double)o.albedo[1], (double)o.albedo[2]);
    if (o.flags || o._reserved[0] || o._reserved[1] || o._reserved[2]) return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_haze: flags and _reserved must be 0");
    GRP_EACH(c, vrt_set_haze(d, opts));
    // what is kept: off is 32 zero bytes, -0 is +0
    if (o.density == 0.0f) memset(&o, 0, sizeof o);
    for (float &a : o.albedo) if (a == 0.0f) a = 0.0f;
    if (memcmp(&c->haze, &o, sizeof o) != 0) c->accum_restart = true;
    c->haze = o;
    return VRT_OK;
}

int vrt_set_water_refraction(vrt_ctx *c, const vrt_water_refraction *opts) {
    if (!c) return VRT_ERR_INVALID_ARG;
    vrt_water_refraction o;
    memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    if (!(o.ior == 0.0f || (o.ior >= 1.0f && o.ior <= 4.0f)))
        return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_water_refraction: ior %g (0 = off, or in [1, 4])", (double)o.ior);
    if (o.max_span > vrt::kRefractSpanMax)
        return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_water_refraction: max_span %u (0 = %u; at most %u)", o.max_span, vrt::kRefractSpanDefault,
                    vrt::kRefractSpanMax);
    if (o.flags || o._reserved) return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_water_refraction: flags and _reserved must be 0");
    GRP_EACH(c, vrt_set_water_refraction(d, opts));
    // what is kept: off is 16 zero bytes, max_span 0 is 64
    if (o.ior == 0.0f) memset(&o, 0, sizeof o);
    else if (o.max_span == 0u) o.max_span = vrt::kRefractSpanDefault;
    if (memcmp(&c->refraction, &o, sizeof o) != 0) c->accum_restart = true;
    c->refraction = o;
    return VRT_OK;
}

int vrt_set_camera_sampling(vrt_ctx *c, const vrt_camera_sampling *opts) {
    if (!c) return VRT_ERR_INVALID_ARG;
    vrt_camera_sampling o;
    memset(&o, 0, sizeof o);
    if (opts) o = *opts;
    const float f[3] = {o.pixel_spread, o.aperture, o.focus_distance};
    for (float x : f)
        if (!(x >= 0.0f) || std::isinf(x))
            return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_camera_sampling: pixel_spread %g, aperture %g, focus_distance %g (each 0 or a finite positive number)",
                        (double)o.pixel_spread, (double)o.aperture, (double)o.focus_distance);
    if (o.pixel_spread > 8.0f) return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_camera_sampling: pixel_spread %g (at most 8 pixels)", (double)o.pixel_spread);
    if (o.aperture != 0.0f && o.focus_distance == 0.0f) return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_camera_sampling: an aperture needs a focus_distance");
    if (o.flags) return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_camera_sampling: flags must be 0");
    GRP_EACH(c, vrt_set_camera_sampling(d, opts));
    // what is kept: -0 as +0, and no focus distance without a lens (it is not read, so it is not compared; off is 16 zero bytes)
    if (o.pixel_spread == 0.0f) o.pixel_spread = 0.0f;
    if (o.aperture == 0.0f) o.aperture = o.focus_distance = 0.0f;
    if (memcmp(&c->lens, &o, sizeof o) != 0) c->accum_restart = true;
    c->lens = o;
    return VRT_OK;
}

int vrt_reset_accumulation(vrt_ctx *c) {
    GRP_EACH(c, vrt_reset_accumulation(d));
    if (!c) return VRT_ERR_INVALID_ARG;
    c->accum_restart = true;
    return VRT_OK;
}

int vrt_get_accumulation(vrt_ctx *c, uint32_t *samples, uint32_t *seed) {
    GRP_ROOT(c, vrt_get_accumulation(d, samples, seed));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (samples) *samples = c->accum_n;
    if (seed) *seed = c->accum_seed;
    return VRT_OK;
}

int vrt_synchronize(vrt_ctx *c) {
    if (c && c->grp) return grp_synchronize(c);
    if (!c) return VRT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    QUIESCE(c);
    VRT_TRY(flush_staged(c));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->up_stream) HIP_TRY(c, hipStreamSynchronize(c->up_stream));
    c->walkers_in_flight = false;   // nothing is in flight any more
    for (auto &T : c->tabs) T.update_pending = false;
    return VRT_OK;
}

int vrt_read_output(vrt_ctx *c, float *rgb, uint32_t *ids, uint8_t *rgba8) {
    if (c && c->grp) { const int rc_ = grp_synchronize(c); if (rc_) return rc_; }
    GRP_ROOT(c, vrt_read_output(d, rgb, ids, rgba8));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (!c->rendered) return fail(c, VRT_ERR_STATE, "vrt_read_output: nothing rendered yet");
    if (c->compact) return fail(c, VRT_ERR_STATE, "vrt_read_output: a VRT_FLAG_COMPACT context holds 8-byte records, not texels (vrt_assemble_compact shades them)");
    if (!c->last.has_texels) return fail(c, VRT_ERR_STATE, "vrt_read_output: the last frame stored its window pixels only (vrt_set_presentation with VRT_PRESENT_SKIP_TEXELS)");
    HIP_TRY(c, hipSetDevice(c->device));
    QUIESCE(c);
    const size_t npix = (size_t)c->width * c->height;
    if (rgba8) {
        if (c->tile_major) return fail(c, VRT_ERR_STATE, "vrt_read_output: rgba8 readback needs the row-major (unsharded) layout");
        HIP_TRY(c, c->sz.d_rgba8.once(npix * 4));
        vrt::launch_quantize(c->last.out, c->sz.d_rgba8, c->width, c->height, c->stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(rgba8, c->sz.d_rgba8, npix * 4, hipMemcpyDeviceToHost, c->stream));
    }
    std::vector<vrt::Texel> t;
    if (rgb || ids) {
        t.resize(c->slots);
        HIP_TRY(c, hipMemcpyAsync(t.data(), c->last.out, t.size() * sizeof(vrt::Texel), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!rgb && !ids) return VRT_OK;
    auto put = [&](size_t dst, const vrt::Texel &x) {
        if (rgb) { memcpy(rgb + dst * 3, &x, 12); }
        if (ids) ids[dst] = x.w;
    };
    if (!c->tile_major) {
        for (size_t i = 0; i < npix; i++) put(i, t[i]);
        return VRT_OK;
    }
    // sharded: de-interleave this context's tiles; foreign tiles read as zero
    if (rgb) memset(rgb, 0, npix * 3 * sizeof(float));
    if (ids) memset(ids, 0, npix * sizeof(uint32_t));
    for (uint32_t tl = 0; tl < c->tiles_local; tl++) {
        const uint32_t tile = vrt::shard_tile(tl, c->shard_first, c->shard_run, c->shard_period);
        const uint32_t tx = (tile % c->tiles_x) * 8u, ty = (tile / c->tiles_x) * 8u;
        for (uint32_t p = 0; p < 64; p++) put((size_t)(ty + (p >> 3)) * c->width + tx + (p & 7u), t[(size_t)tl * 64 + p]);
    }
    return VRT_OK;
}

int vrt_read_steps(vrt_ctx *c, uint32_t *steps) {
    GRP_REFUSE(c, "vrt_read_steps");
    if (!c || !steps) return fail(c, VRT_ERR_INVALID_ARG, "vrt_read_steps: null argument");
    if (!c->rendered || !c->last.stats || !c->sz.d_steps)
        return fail(c, VRT_ERR_STATE, "vrt_read_steps: the last frame was not rendered with opts.stats = 1");
    if (c->tile_major) return fail(c, VRT_ERR_STATE, "vrt_read_steps: needs the row-major (unsharded) layout");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(steps, c->sz.d_steps, (size_t)c->width * c->height * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return VRT_OK;
}

int vrt_get_stats(vrt_ctx *c, vrt_stats *out) {
    if (c && c->grp) return grp_get_stats(c, out);
    if (!c || !out) return fail(c, VRT_ERR_INVALID_ARG, "vrt_get_stats: null argument");
    if (!c->rendered) return fail(c, VRT_ERR_STATE, "vrt_get_stats: nothing rendered yet");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->timing_pending) {
        float last[3] = {0, 0, 0};
        VRT_TRY(fold_events(c, last));
        std::vector<unsigned long long> hbuf(kCounterBytes / sizeof(unsigned long long));
        HIP_TRY(c, hipMemcpyAsync(hbuf.data(), c->d_counters, kCounterBytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        unsigned long long *h = hbuf.data();
        unsigned long long launched = 0;
        if (c->last.mode == VRT_MODE_PRIMARY_SHADOW && c->last.n_counts) {
            std::vector<uint32_t> bc(c->last.n_counts);
            HIP_TRY(c, hipMemcpyAsync(bc.data(), c->last.blk, bc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            for (uint32_t v : bc) launched += v;
        }
        vrt_stats s;
        memset(&s, 0, sizeof s);
        s.primary_rays = (uint64_t)c->tiles_local * 64u * (c->last.mode == VRT_MODE_PATH ? c->last.spp : 1u);
        s.secondary_rays = c->last.mode == VRT_MODE_PRIMARY_SHADOW ? launched : 0;
        if (c->last.mode == VRT_MODE_PATH && c->last.stats) s.secondary_rays = h[vrt::kCtrSecondary];
        if (c->last.stats) {
            s.hits = h[vrt::kCtrHits];
            s.steps = h[vrt::kCtrSteps];
            s.node_visits = h[vrt::kCtrVisits];
            s.primary_steps = h[vrt::kCtrPrimarySteps];
            s.primary_node_visits = h[vrt::kCtrPrimaryVisits];
        }
        if (c->d_clock) {  // clock-probe frames since the last call
            unsigned long long clk[2] = {0, 0};
            HIP_TRY(c, hipMemcpyAsync(clk, c->d_clock, sizeof clk, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemsetAsync(c->d_clock, 0, sizeof clk, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            s.clock_shader_ticks = clk[0];
            s.clock_ref_ticks = clk[1];
        }
        s.ms_primary = last[0]; s.ms_secondary = last[1]; s.ms_total = last[2];
        s.frames = c->acc_frames;
        s.sum_ms_primary = c->acc_ms[0]; s.sum_ms_secondary = c->acc_ms[1]; s.sum_ms_total = c->acc_ms[2];
        c->acc_frames = 0;
        c->acc_ms[0] = c->acc_ms[1] = c->acc_ms[2] = 0;
        c->stats = s;
        c->timing_pending = false;
    }
    *out = c->stats;
    return VRT_OK;
}

int vrt_get_issue_profile(vrt_ctx *c, vrt_issue_profile *out) {
    if (!c || !out) return fail(c, VRT_ERR_INVALID_ARG, "vrt_get_issue_profile: null argument");
    if (c->grp) return grp_get_issue_profile(c, out);
    memset(out, 0, sizeof *out);
    out->devices = 1u;
    out->frames = c->prof_frames;
    if (c->prof_frames) out->render_us = c->prof_render_us / (double)c->prof_frames;
    c->prof_render_us = 0.0;
    c->prof_frames = 0u;
    return VRT_OK;
}

int vrt_set_frames_in_flight(vrt_ctx *c, uint32_t n) {
    if (c && c->grp) return grp_set_frames_in_flight(c, n);
    if (!c) return VRT_ERR_INVALID_ARG;
    if (n < 1u || n > vrt_ctx::kMaxInFlight) return fail(c, VRT_ERR_INVALID_ARG, "vrt_set_frames_in_flight: 1..%u", vrt_ctx::kMaxInFlight);
    HIP_TRY(c, hipSetDevice(c->device));
    QUIESCE(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->in_flight = n;
    c->flip = 0;
    // the table sets of frame slots that no longer render go stale: nobody brings them up to date, so their dirty lists
    // would only grow (and, full, force whole-world builds on a context whose active sets are fine)
    for (uint32_t k = n; k < vrt_ctx::kMaxInFlight; k++) {
        auto &T = c->tabs[k];
        for (uint32_t ch : T.dirty_chunks) T.chunk_is_dirty[ch] = 0;
        T.dirty_chunks.clear();
        T.live = false;
    }
    return VRT_OK;
}

int vrt_set_stream(vrt_ctx *c, void *hip_stream) {
    GRP_REFUSE(c, "vrt_set_stream");
    if (!c) return VRT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    QUIESCE(c);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream.get();
    return VRT_OK;
}

int vrt_bind_output(vrt_ctx *c, void *texels) {
    GRP_REFUSE(c, "vrt_bind_output");
    if (!c) return VRT_ERR_INVALID_ARG;
    if (texels && ((uintptr_t)texels % 16u)) return fail(c, VRT_ERR_INVALID_ARG, "vrt_bind_output: texels must be 16-byte aligned");
    // stream-ordered: launches capture the pointer, so frames already enqueued keep writing where they were
    // told to and the next vrt_render uses the new buffer (lets a host ping-pong two gather messages)
    c->d_out = texels ? (vrt::Texel *)texels : c->sz.own_out;
    c->last.out = c->d_out;
    c->rendered = false;
    return VRT_OK;
}

int vrt_device_output(vrt_ctx *c, void **texels, uint64_t *bytes) {
    GRP_ROOT(c, vrt_device_output(d, texels, bytes));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (texels) *texels = c->d_out == c->sz.own_out ? c->last.out : c->d_out;  // own buffers: the one holding the last frame
    if (bytes) *bytes = (uint64_t)c->slots * (c->compact ? 8u : sizeof(vrt::Texel));
    return VRT_OK;
}

int vrt_shard_info(vrt_ctx *c, uint32_t *tiles_local, uint32_t *tiles_padded, uint32_t *tiles_total) {
    GRP_ROOT(c, vrt_shard_info(d, tiles_local, tiles_padded, tiles_total));
    if (!c) return VRT_ERR_INVALID_ARG;
    if (tiles_local) *tiles_local = c->tiles_local;
    if (tiles_padded) *tiles_padded = c->tiles_padded;
    if (tiles_total) *tiles_total = c->tiles_total;
    return VRT_OK;
}

}  // extern "C"
