#pragma once
// vrt_ctx.h — what the translation units of the backend (the C ABI of include/vrt.h over the gfx950 kernels) share:
// the context, the kernels' launchers, and the helpers that cross a file boundary.
//   vrt_frames.hip   contexts, uniforms, frame sets, vrt_render, read-backs, stats
//   vrt_uploads.hip  uploads without draining, which chunks a write touched, the derived tables
//   vrt_lit.hip      the sun marks of a table set: their kernels, the frame's hook, the read-backs
//   vrt_present.hip  the presentation blit and the gather root's assembly
//   vrt_group.hip    one context over several devices
//   vrt_cast.hip, vrt_clip.hip   the world queries (vrt_cast_rays, vrt_clip_moves) over vrt_query.h: the world as a kernel
//                    sees it and the host-pointer batch
//   vrt_gen.hip      the chunk source (vrt_generate_chunks, vrt_build_chunks)
//   vrt_edit.hip     shapes onto chunks that exist (vrt_edit_chunks), in front of vrt_gen.hip's builder
//   vrt_denoise.hip  the path trace's denoiser (vrt_set_denoise, vrt_read_guide) and its kernels
//   vrt_tone.hip     exposure and tone mapping of presented path frames (vrt_set_tone_map): the metering kernels and the read-backs
//   both/            not of this seam: the arithmetic those three kernels share with the host mirror (both/both.h)
//
// Replaces the reference's wgpu seam: GpuResources / Buffers / NodeBuffer / SimpleBuffer /
// ArrayBuffer / PixelShader (clientdesktop/src/graphics/{mod.rs,shader.rs}).  Device memory layout
// (DESIGN.md §HBM layout): the node pool is kept byte-identical to the host pool (little-endian u16 =
// the reference's packed u32 pairs), chunk_roots is a dense u32[S^3], materials 256 x 32 B, output one
// 16-byte texel {r,g,b f32, id u32} per pixel slot, hit buffer 16 B per local pixel.
// Ownership: every device allocation of a context is a vrt_ctx::Buf (vrt_devbuf.h), every event, stream and pinned allocation a
// vrt_ctx::Event / Stream / Pinned (vrt_handle.h, made where first used: ensure()); all go with the context, and so do a group's
// with the group.  Raw pointers and handles are aliases or the caller's: stream, last.stream, wait_before_frame, screen_stream[],
// d_ring.  What depends on the output size is vrt_ctx::Sized: a resize assigns it an empty value.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "vrt_devbuf.h"
#include "vrt_frame_plan.h"
#include "vrt_handle.h"
#include "vrt_device.h"

namespace vrt {
struct HipAlloc {   // vrt_devbuf.h's allocator over the HIP runtime
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void *p) { (void)hipFree(p); }
};
// vrt_handle.h's policies over the HIP runtime: an event (untimed unless asked: hipEventDefault for the ones that are read as
// times), a non-blocking stream, mapped pinned host memory
struct HipEvent {
    using T = hipEvent_t;
    static hipError_t create(T *e, unsigned flags = hipEventDisableTiming) { return hipEventCreateWithFlags(e, flags); }
    static void destroy(T e) { (void)hipEventDestroy(e); }
};
struct HipStream {
    using T = hipStream_t;
    static hipError_t create(T *s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
    static void destroy(T s) { (void)hipStreamDestroy(s); }
};
struct HipPinned {
    using T = uint8_t *;
    static hipError_t create(T *p, size_t bytes) { return hipHostMalloc((void **)p, bytes, hipHostMallocMapped); }
    static void destroy(T p) { (void)hipHostFree(p); }
};
bool variant_supported(uint32_t variant);
void launch_primary(const FrameParams &P, uint32_t variant, bool stats, bool shadow, hipStream_t st, hipEvent_t e0, hipEvent_t e1);
void launch_shadow(const FrameParams &P, uint32_t variant, bool stats, hipStream_t st, hipEvent_t e0, hipEvent_t e1);
void launch_primary_shadow_fused(const FrameParams &P, uint32_t march, bool stats, hipStream_t st, hipEvent_t e0, hipEvent_t e1);
// emit: the kernels that add the light of emissive hits (vrt_write_emission; the table is the 256 floats after P.mats)
// polish: the kernels that also flip the coat's coin on every hit (vrt_write_polish; the table behind the emission table) — given with emit
// translucent: the kernels that first draw whether the path passes through (vrt_write_translucency; the table behind the polish
// table) — given with emit; they take the coat's draw under the word behind the tables, so polish chooses nothing among them
void launch_path_primary(const FrameParams &P, bool stats, bool literal, bool emit, bool polish, bool translucent, hipStream_t st);
void launch_path_bounce(const FrameParams &P, bool stats, bool literal, bool emit, bool polish, bool translucent, hipStream_t st);
void launch_path_bounce_cells(const FrameParams &P, uint32_t refill_at, uint32_t segments, uint32_t pool_batches, bool emit, bool polish, bool translucent,
                              hipStream_t st);
// vrt_set_sun_light (vrt_path_sun.h): a sun-lit frame's trace launches — they append a sun ray's record for every hit that sees the
// sun — and the launch behind each that marches the records (cells: with the occlusion-only march over the march cells)
void launch_path_primary_sunlit(const FrameParams &P, const SunLaunch &S, bool stats, bool literal, hipStream_t st);
void launch_path_bounce_sunlit(const FrameParams &P, const SunLaunch &S, bool stats, bool literal, hipStream_t st);
void launch_path_sun(const FrameParams &P, const SunLaunch &S, bool stats, bool literal, bool cells, hipStream_t st);
// vrt_set_camera_sampling (vrt_path_lens.h): bounce 0 of a frame with the setting on, plain and sun-lit
void launch_path_primary_lens(const FrameParams &P, const LensLaunch &L, bool stats, bool literal, hipStream_t st);
void launch_path_primary_lens_sunlit(const FrameParams &P, const LensLaunch &L, const SunLaunch &S, bool stats, bool literal, hipStream_t st);
// vrt_set_lamp_light (vrt_path_lamp.h): a lamp-lit frame's trace launches — one pair that carries the sun term too (M.sun) and, the
// primary one, camera sampling (sampled: L is read) — and the launch behind each that marches the lamp rays it appended
void launch_path_primary_lamp(const FrameParams &P, const LensLaunch &L, const SunLaunch &S, const LampLaunch &M, bool sampled, bool stats, bool literal,
                              hipStream_t st);
void launch_path_bounce_lamp(const FrameParams &P, const SunLaunch &S, const LampLaunch &M, bool stats, bool literal, hipStream_t st);
void launch_path_lamp_rays(const FrameParams &P, const LampLaunch &M, bool stats, bool literal, hipStream_t st);
// vrt_set_water_optics (vrt_path_water.h): a water frame's trace launches (S: with buffers when the frame is sun-lit too)
void launch_path_primary_water(const FrameParams &P, const WaterLaunch &W, const SunLaunch &S, bool stats, bool literal, hipStream_t st);
void launch_path_bounce_water(const FrameParams &P, const WaterLaunch &W, const SunLaunch &S, bool stats, bool literal, hipStream_t st);
// vrt_set_water_refraction (vrt_path_refract.h): the same two launches where the context's ior is not 0
void launch_path_primary_refract(const FrameParams &P, const WaterLaunch &W, const SunLaunch &S, const RefractLaunch &X, bool stats, bool literal,
                                 hipStream_t st);
void launch_path_bounce_refract(const FrameParams &P, const WaterLaunch &W, const SunLaunch &S, const RefractLaunch &X, bool stats, bool literal,
                                hipStream_t st);
// vrt_set_haze (vrt_path_haze.h): a haze frame's trace launches (S: with buffers when the frame is sun-lit too)
void launch_path_primary_haze(const FrameParams &P, const HazeLaunch &H, const SunLaunch &S, bool stats, bool literal, hipStream_t st);
void launch_path_bounce_haze(const FrameParams &P, const HazeLaunch &H, const SunLaunch &S, bool stats, bool literal, hipStream_t st);
void launch_path_finish(Texel *out, uint32_t n, uint32_t spp, hipStream_t st);
void launch_tile_order(const uint32_t *cost, uint32_t n, uint32_t shift, uint32_t *scratch, uint32_t *order, hipStream_t st);
bool launch_tile_order_blocks(const uint32_t *cost, uint32_t tiles_x, uint32_t tiles_y, uint32_t shift, uint32_t radius, uint32_t *order, hipStream_t st, uint32_t threads);
void launch_path_chain_finish(Texel *sum, Texel *mean, const Texel *acc, uint32_t n, uint32_t chain, bool first, bool last, uint32_t count,
                              hipStream_t st);
void launch_path_accum_resolve(Texel *out, Texel *sum, uint32_t n, bool first, bool last, uint32_t count, hipStream_t st);
void launch_quantize(const Texel *out, uint8_t *rgba8, uint32_t w, uint32_t h, hipStream_t st);
void launch_assemble(const Texel *gathered, Texel *dst, uint32_t width, uint32_t tiles_x, uint32_t tiles_total,
                     uint32_t root_weight, uint32_t period, bool skip_root, uint64_t rank_stride, hipStream_t st);
// tone: a mapped frame's blit (vrt_set_tone_map) — the kernels that put the exposure and the curve in front of every texel's
// quantisation; null: the blit as it is without the setting
void launch_present(const Texel *out, uint32_t w, uint32_t h, uint32_t screen_w, uint32_t screen_h, const vrt_crosshair &ch,
                    uint8_t *rgba8, bool one_to_one, const uint32_t box[4], hipStream_t st, const ToneBlit *tone = nullptr);
void launch_assemble_shade(const FrameParams &P, const void *gathered, Texel *dst, uint32_t root_weight, uint32_t period,
                           uint64_t rank_stride, hipStream_t st);
// vrt_accel.hip's table builders over the node pool and a table set (vrt_device.h PoolView / TableView; vrt_ctx::Tables::view);
// liquid: the 256-bit is_liquid mask the march cells are built with
void launch_accel_cells(const PoolView &pool, const TableView &tv, uint32_t *totals, uint32_t *chunk_needs, hipStream_t st);
void launch_accel_bricks(const PoolView &pool, const TableView &tv, const uint32_t liquid[8], hipStream_t st);
void launch_accel_chunks(const PoolView &pool, const TableView &tv, const uint32_t liquid[8], const uint32_t *chunks, const uint32_t *extents,
                         const uint32_t *chunk_roots_host, uint32_t n, hipStream_t st, hipEvent_t done);
void launch_upload_words(void *dst, const void *pinned_src, uint32_t n_words, hipStream_t st);
void launch_upload_batch(void *dst0, void *dst1, const void *pinned_ring, const UploadBatch &batch, uint32_t n_pieces, hipStream_t st);
}  // namespace vrt

// Host-time profile of the frame path (VRT_HOST_PROF=1: printed at process exit): where the calling thread's microseconds per
// frame go, section by section (profiles/r04_group_host_profile.txt).  Off, a section costs one test of a flag.
#include <chrono>
struct vrt_host_prof {
    bool on = getenv("VRT_HOST_PROF") != nullptr;
    double us[24] = {};
    unsigned long long n[24] = {};
    const char *name[24] = {};
    ~vrt_host_prof() {
        if (!on) return;
        for (int i = 0; i < 24; i++)
            if (n[i]) fprintf(stderr, "host-prof %-34s %9llu calls %8.2f us each\n", name[i] ? name[i] : "?", n[i], us[i] / (double)n[i]);
    }
};
extern __attribute__((visibility("hidden"))) vrt_host_prof g_host_prof;
struct vrt_prof_scope {
    int i;
    std::chrono::steady_clock::time_point t0;
    vrt_prof_scope(int i_, const char *name) : i(i_) {
        if (g_host_prof.on) { g_host_prof.name[i] = name; t0 = std::chrono::steady_clock::now(); }
    }
    ~vrt_prof_scope() {
        if (!g_host_prof.on) return;
        g_host_prof.us[i] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        g_host_prof.n[i] += 1;
    }
};
#define VRT_PROF(i, name) vrt_prof_scope prof_scope_##i(i, name)

static_assert(sizeof(vrt_material) == 32, "Material layout (mod.rs:20-28)");
static_assert(sizeof(vrt_cam_data) == 160, "CamData layout (mod.rs:82-91)");
static_assert(sizeof(vrt_world_data) == 32, "WorldData layout (mod.rs:113-120)");
static_assert(sizeof(vrt_settings) == 48, "Settings layout (mod.rs:132-143)");
static_assert(sizeof(vrt_crosshair) == 32, "Crosshair layout (mod.rs:63-70)");
static_assert(sizeof(vrt::Texel) == 16, "texel");

struct vrt_group;

static constexpr size_t kSegBytes = (size_t)vrt::kHitSegments * vrt::kSegStride * sizeof(uint32_t);
// three sets of segment cursors: launch g of a path frame appends to set g % 3, reads set (g - 1) % 3 and clears set
// (g + 1) % 3 for its successor, so no memset sits between two launches
static constexpr size_t kCounterBytes = vrt::kCtrCount * sizeof(unsigned long long) + 3 * kSegBytes;   // + the path trace's 3 cursor sets
static constexpr size_t kCounterWords = kCounterBytes / sizeof(unsigned long long);
static_assert(kCounterWords * sizeof(unsigned long long) == kCounterBytes, "the counters are allocated as 64-bit words");

struct vrt_ctx {
    template <typename T> using Buf = vrt::DevBuf<T, vrt::HipAlloc>;
    using Event = vrt::Handle<vrt::HipEvent>;
    using Stream = vrt::Handle<vrt::HipStream>;
    using Pinned = vrt::Handle<vrt::HipPinned>;
    vrt_group *grp = nullptr;   // a multi-device context (vrt_config.n_devices > 1): everything else below is unused, see vrt_group
    hipEvent_t wait_before_frame = nullptr;  // set by a multi-device context: the next frame's stream waits for it first (its message slot is free)
    int device = 0;
    Stream own_stream;
    // Two frames in flight (what a swapchain gives the reference): consecutive plain frames alternate between the
    // context's two streams, each with its own output buffer, so one frame's tail overlaps the next one's ramp-up
    // instead of the in-order queue's ~5 us hand-over.  Everything else on the context waits for both (quiesce()).
    static constexpr uint32_t kMaxInFlight = 4;
    Stream extra_stream[kMaxInFlight - 1];   // each made by the first frame that runs on it
    Buf<unsigned long long> extra_counters[kMaxInFlight - 1];   // path mode: its own segment cursors
    uint32_t in_flight = 2;        // vrt_set_frames_in_flight
    bool alt_pending = false;      // frames may still be running on the extra streams
    bool own_pending = false;      // ... or on own_stream while the caller's stream is the context's stream (VRT_RENDER_OWN_STREAMS)
    uint32_t flip = 0;             // which (stream, output, counts) set the next pipelined frame takes
    hipStream_t stream = nullptr;
    // four hipEvents per frame rendered since the last vrt_get_stats.  Primary(+shadow) frames: {begin, end} of the first
    // kernel and {begin, end} of the second, stamped by the dispatches themselves (hipExtLaunchKernel), so the stream
    // carries no marker packets between frames.  Path frames: [0], [1], [3] recorded around the launches.
    std::vector<std::array<Event, 4>> ev_pool;   // (timing enabled)
    std::vector<uint8_t> ev_kind;  // EvKind
    size_t ev_used = 0;
    double acc_ms[3] = {0, 0, 0};
    uint32_t acc_frames = 0;

    uint32_t max_nodes = 0;  // even
    uint32_t world_size = 0;
    uint32_t n_roots = 0;
    uint32_t width = 0, height = 0;
    uint32_t shard_rank = 0, shard_count = 1, shard_w0 = 1;
    uint32_t shard_first = 0, shard_run = 1, shard_period = 1;  // vrt_device.h shard_tile()
    bool whole_frame_owner = false;  // device_ids[0] of a multi-device context: its row-major buffer holds the assembled frame
    bool compact = false;     // VRT_FLAG_COMPACT: 8-byte records instead of texels (a sharded, tile-major context whose tiles cross a link)
    bool tile_major = false;  // output layout [t_local][64]: always when sharded, on request (VRT_FLAG_TILE_MAJOR) otherwise
    uint32_t tiles_x = 0, tiles_total = 0, tiles_local = 0, tiles_padded = 0;
    uint32_t slots = 0;  // pixel slots in the output buffer

    Buf<uint16_t> d_nodes;
    Buf<uint32_t> d_roots;
    Buf<vrt_material> d_mats;       // the 256 materials, then the 256 floats of the emission table (vrt::emission_table), then the 256 entries of the polish table (vrt::polish_table), the 256 of the translucency table (vrt::translucency_table) and the coat word (vrt::coat_word): kMatsAlloc
    vrt::Texel *d_out = nullptr;    // where frames are written: sz.own_out or caller-bound memory
    // What the last frame was, for the calls that read it back or present it.  vrt_render assigns it whole once the frame is
    // enqueued: a call that returns an error leaves the record of the frame before it.  alloc_output, vrt_bind_output and the
    // presentation blit change single fields.
    struct LastFrame {
        vrt::Texel *out = nullptr;     // the buffer holding the frame
        uint32_t *blk = nullptr, n_counts = 0;   // its launched-ray counts, and how many of them a primary + shadow frame wrote
        hipStream_t stream = nullptr;  // the stream it was enqueued on
        uint32_t slot = 0, tab = 0, mode = 0, spp = 1;   // its frame set and its table set
        // it stored the window's image itself (vrt_set_presentation), and texels at all (not with VRT_PRESENT_SKIP_TEXELS); opts.stats == 1
        bool fused = false, has_texels = true, stats = false;
        // vrt_set_tone_map as it stood at the frame's vrt_render (curve 0: not a mapped frame), and where the blit reads the
        // frame's E: the frame set's word on the device (a metered frame) or, null, tone.exposure
        vrt_tone_map tone{};
        const float *tone_E = nullptr;
    } last;
    // What a resize drops (alloc_output assigns an empty Sized, then makes own_out, d_hits and d_blk_counts again): every buffer
    // sized by the output, made on first use, and what is only true of their contents.
    struct Sized {
        Buf<vrt::Texel> own_out;
        Buf<uint4> d_hits;
        Buf<uint32_t> d_blk_counts;  // hit records per primary workgroup
        Buf<uint4> d_path;  // path mode: 2 buffers x 3 planes x (kHitSegments * hit_seg_cap) records, lazily allocated, grows only
        Buf<uint32_t> d_steps;
        Buf<uint8_t> d_rgba8;
        // the frame sets beyond the first: output, counts and path buffers
        Buf<vrt::Texel> extra_out[kMaxInFlight - 1];
        Buf<uint32_t> extra_blk[kMaxInFlight - 1];
        Buf<uint4> extra_path[kMaxInFlight - 1];
        Buf<vrt::Texel> path_acc[kMaxInFlight];        // the samples' accumulation planes of a launch chain, per frame set
        // vrt_set_sun_light: per frame set, made by its first sun-lit frame — 3 planes x (kHitSegments * hit_seg_cap) sun-ray
        // records, and two sets of segment cursors (trace launch g appends to set g & 1 and clears the other for its successor)
        Buf<uint4> sun_recs[kMaxInFlight];
        Buf<uint32_t> sun_counts[kMaxInFlight];
        // vrt_set_lamp_light: the same again for the lamp rays, made by the frame set's first lamp-lit frame
        Buf<uint4> lamp_recs[kMaxInFlight];
        Buf<uint32_t> lamp_counts[kMaxInFlight];
        Buf<uint32_t> d_tile_cost, d_tile_order, d_tile_scratch;   // vrt_order.hip, made together
        bool tile_order_valid = false;
        Buf<vrt::Texel> d_accum;     // VRT_RENDER_ACCUMULATE: the running sum
        Buf<vrt::Texel> dn_scratch[kMaxInFlight];   // vrt_set_denoise: per frame set, made by its first denoised frame
        Buf<uint32_t> dn_guide[kMaxInFlight];
        uint32_t *dn_last_guide = nullptr;          // the guide of the last denoised frame (one of dn_guide)
    } sz;
    uint32_t n_blocks = 0;
    Buf<unsigned long long> d_counters;  // [kCtrCount] stats, then the hit-segment counters
    uint32_t hit_seg_cap = 0;       // records per hit segment: what the kernels are given (d_hits holds kHitSegments of them)
    Buf<unsigned long long> d_clock;  // clock-probe frames: {s_memtime ticks, s_memrealtime ticks}, summed until vrt_get_stats
    // vrt_present's targets: one per frame set, written on the stream of the frame that is presented (vrt_present.hip); bytes
    Buf<uint8_t> d_screen[4];
    hipStream_t screen_stream[4] = {nullptr, nullptr, nullptr, nullptr};   // the stream of the buffer's last blit

    // derived lookup tables of the grid march (vrt_accel.hip), brought up to date lazily when their inputs changed: the whole
    // world (accel_dirty) or only the chunks a write touched.  One set per frame set in use (tabs[0] always; tabs[k] once
    // frame set k has rendered): a frame in flight reads its own set, so bringing the next frame's set up to date does not
    // have to wait for it — each set keeps its own list of the chunks dirtied since *it* was last brought up to date.
    struct Tables {
        Buf<uint32_t> d_grid;         // [8S][8S+1][8S+1] with the zero border
        Buf<uint16_t> d_bricks;
        uint32_t brick_cap() const { return (uint32_t)(d_bricks.cap() / 64u); }   // in 64-word bricks, as the kernels take it
        // the march cells (vrt_accel.hip): a chunk directory [S][S+1][S+1] and 8-KiB blocks of 512 cells (0: outside the world,
        // 1: shared by the chunks that are one air leaf, the rest: one chunk each; the tail takes chunks that stop being air)
        Buf<uint32_t> d_cdir;
        Buf<uint4> d_mblk;
        uint32_t mblk_cap() const { return (uint32_t)(d_mblk.cap() / 512u); }     // in 512-cell blocks, as the kernels take it
        Buf<uint32_t> d_mblk_tail;
        Buf<uint32_t> d_chunk_bricks, d_chunk_bases, d_chunk_caps, d_brick_tail;
        // what vrt_accel.hip's builders take of the set as it is allocated now; direct: a world without the chunk directory
        vrt::TableView view(bool direct) const {
            return {d_grid, d_bricks, brick_cap(), d_chunk_bricks, d_chunk_bases, d_chunk_caps, d_brick_tail, direct ? nullptr : d_cdir.get(), d_mblk, d_mblk_tail, mblk_cap()};
        }
        bool live = false;           // a copy of tabs[0] as of the last whole-world build, plus its own chunk updates since
        std::vector<uint32_t> dirty_chunks;     // chunk slots whose nodes or root changed since this set was last brought up to date
        std::vector<uint8_t> chunk_is_dirty;    // ... as flags, [n_roots]
        std::vector<uint8_t> chunk_may_have_moved;  // rebuilt alone since the last whole-world build: may sit in the pool's tail
        uint32_t chunks_moved = 0;
        uint32_t chunk_builds = 0;              // chunks this set has rebuilt alone (vrt_accel_info reports the most advanced set's)
        uint64_t gen = 0;                       // what the set's device tables hold: a new value of c->tables_gen with every build, copy and chunk update (the lamp lists' key)
        // the sun marks in d_grid's air leaves and the shadow pool (vrt_lit.hip, which alone writes this record but for take_from)
        struct SunMarks {
            // What marks are made for: they hold while the set's tables are the ones they were made from (gen), the sun stands where
            // it stood and the smallest marked leaf is the same.  (The sun is compared bit for bit: -0.0f is another sun than 0.0f.)
            struct Key {
                uint64_t gen = 0;
                float sun[3] = {0.f, 0.f, 0.f};
                uint32_t min_lo = 0;
                uint32_t liquid[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // the liquid ids the dark marks' blockers were judged by (all 0 while the dark marks are off)
                bool same(const Key &o) const {
                    return gen == o.gen && memcmp(sun, o.sun, sizeof sun) == 0 && min_lo == o.min_lo && memcmp(liquid, o.liquid, sizeof liquid) == 0;
                }
            } made, want;                       // what the marks in the grid were made for; what the frames ask for:
            uint32_t want_frames = 0;           // the pass runs once kLitSettleFrames frames in a row have asked for the same marks
            bool valid = false;                 // the grid holds marks, made for `made`
            // the voxel marks (vrt_lit.hip: accel_lit_voxels_kernel): the shadow pool — d_bricks entry for entry, a lit air voxel of a
            // split cell holding vrt::kLitVoxel — made behind the lit pass that made the cell marks and held exactly as long as they
            // are; a copy of the set does not take it along.  Allocated by the set's first pass that builds voxel marks
            Buf<uint16_t> d_pool;
            Buf<uint32_t> d_clash;              // one word: the world holds kLitVoxel in a brick (the pool is then a plain copy)
            bool voxels_valid = false;
            uint64_t pool_gen = ~0ull;          // the tables the pool was last written from (vrt_read_lit_voxels reads it back, marks or none)
            // the flag comes back to the host behind the pass, without a wait: a frame that finds the pass over reads it, and where it is set
            // goes back to the plain bricks; the tables it was set for get no voxel pass again (a moved sun: the world still holds the id)
            Pinned h_clash;
            bool clash_pending = false;
            uint64_t clash_gen = ~0ull;
            uint32_t voxel_layers = 0;          // K the pool was made with
            // the dark marks (vrt_lit.hip: accel_dark_kernel): bit 21 of the grid's air leaves, made behind the lit passes and held
            // exactly as long as the cell marks are; a copy of the set carries them in its grid.  d_floors: a byte per grid entry,
            // which of the cell's four voxel layers across the sun's axis are closed (the pass's scratch; no frame reads it)
            Buf<uint8_t> d_floors;
            bool dark_valid = false;
            uint32_t dark_voxel_layers = 0;     // K_d the pool's dark voxel marks were made with (accel_dark_voxels_kernel); 0: it holds none
            Event ev;                           // behind the set's last lit pass: a frame on another stream that reads the marks waits for it
            bool pending = false;               // ... recorded and not yet known to be over
            hipStream_t stream = nullptr;       // the stream the pass ran on (frames on it are ordered behind it as they are)
            Event ev_guard;                     // what the context's stream held when a pass on another stream was enqueued
            // do the marks in the grid hold for the set's tables as they are now (T.gen), whatever the sun?
            bool holds(uint64_t gen) const { return valid && made.gen == gen; }
            // is the shadow pool one of `entries` entries, and the one written from these tables by the pass whose marks hold?
            bool pool_fits(size_t entries) const { return d_pool && d_pool.cap() == entries; }
            bool pool_is_of(uint64_t gen, size_t entries) const { return pool_gen == gen && holds(gen) && pool_fits(entries); }
            // What a copy of a table set (of `gen`; the original's: A of a_gen) takes along: the grid's copy carries A's cell marks,
            // which hold for the copy if they held for the original; whoever reads the copy is ordered behind the copy; the shadow
            // pool stays behind (a copy is made for edits, whose chunk updates drop every mark)
            void take_from(const SunMarks &A, uint64_t a_gen, uint64_t gen) {
                valid = A.holds(a_gen);
                made = A.made; made.gen = gen;
                pending = voxels_valid = false;
                dark_valid = valid && A.dark_valid;
            }
        } lit;
        Event ev_updated;                       // behind this set's last chunk update (a reader of the node pool and chunk_roots)
        bool update_pending = false;            // ... recorded and not yet known to be over
    };
    Tables tabs[kMaxInFlight];
    uint64_t tables_gen = 0;
    // The sets are split — every frame set its own — only while edits arrive: two copies of the tables are twice the lines
    // in every XCD's 4 MB L2 (measured: + 1.0 % on the C2 frame period).  After kQuietFrames frames without a dirtied chunk
    // every frame set reads tabs[0] again; the next edit splits them (one wait for the frames in flight, then copies).
    bool tables_split = false;
    uint32_t quiet_frames = 0;
    bool shared_readers_in_flight = false;   // a frame on another frame set is reading tabs[0] (cleared with the frames in flight)
    Buf<uint32_t> d_brick_total;
    Buf<uint32_t> d_chunk_needs;         // whole-world build scratch: which chunks need a block of march cells
    bool march_direct = false;           // the march cells of the whole world, no chunk directory (worlds up to march_direct_max_s)
    uint32_t march_direct_max_s = 0;     // kMarchDirectMaxS, or VRT_MARCH_DIRECT_MAX_S (tests: the directory on a small world)
    uint32_t n_bricks = 0;        // bricks inside the chunks' regions after the last whole-world build
    uint32_t accel_S = 0;         // world size the tables were built for
    bool accel_dirty = true;
    bool accel_ok = false;        // false: world too large for the tables, variant 0 runs as variant 2
    uint32_t accel_max_s = 0;     // kAccelMaxS, or less through VRT_ACCEL_MAX_S (tests of the fallback)
    // Every 8th plain frame carries the dispatch-stamped timing events (VRT_TIMING_EVERY=N changes it): a launch with events
    // costs the host 13 us, one without 4 us (tools/host_cost.py) — nothing on one device, the frame period of a
    // multi-device context that issues to eight from one thread.
    uint32_t timing_every = 8, frame_no = 0;
    bool path_pool = true;         // VRT_PATH_POOL=0 / VRT_PATH_CELLS=0: bounce launches with lane = path (the round-1 structure) instead of the
    bool path_cells = true;        // pool kernel over the march cells (tests: the two structures hold each other's frames)
    uint32_t path_samples = 8;     // VRT_PATH_SAMPLES_PER_CHAIN: samples a launch chain traces at once when spp > 1 (1: one, as round 1 did)
    uint32_t path_pool_batches = 0;   // VRT_PATH_POOL_K = 4 | 5: the bounce waves' pools; 0: 5 for small worlds with two frames in flight, else 4
    uint32_t path_refill = 0;      // VRT_PATH_POOL_REFILL: idle lanes that send a bounce wave back to its pool (0: the default, 16)
    uint32_t accel_builds = 0;
    bool sun_marks = true;         // VRT_SUN_MARKS=0: shadow rays never stop at lit cells (the A/B of profiles/DECISIONS.md)
    uint32_t lit_slab = 0;         // VRT_LIT_SLAB: layers a launch of the lit pass tests a cell's corridor over (1: layer by layer; 0: by grid size, vrt_lit.hip)
    uint32_t lit_passes = 0;       // lit passes launched (vrt_get_sun_marks)
    bool lit_voxels = true;        // VRT_LIT_VOXELS=0: the cell marks alone (the A/B of profiles/lit_voxels_ab.txt); VRT_SUN_MARKS=0 switches both off
    int lit_voxel_layers = -1;     // VRT_LIT_VOXEL_LAYERS: voxel layers a voxel's walk may take (0: no voxel marks; -1: by grid size, vrt_lit.hip)
    uint32_t lit_voxel_passes = 0; // voxel-mark passes launched (vrt_read_lit_voxels)
    uint32_t lit_last_voxel_layers = 0, lit_last_voxel_trips = 0;   // of the last one-launch shadow frame: 0 = it read the plain bricks
    uint32_t lit_last_min_leaf = 0, lit_last_trips = 0;   // of the last one-launch shadow frame: 0 = its marks were off
    bool dark_marks = true;        // VRT_DARK_MARKS=0: no dark pass, shadow rays never stop at dark cells (the A/B of profiles/dark_marks_ab.txt)
    int dark_depth = -1;           // VRT_DARK_DEPTH: layers the dark pass walks a corridor over (0: no dark marks; -1: by grid size, vrt_lit.hip)
    uint32_t dark_passes = 0;      // dark passes launched
    int dark_voxel_layers = -1;    // VRT_DARK_VOXEL_LAYERS: voxel layers a dark voxel's walk may take (0: no dark voxel marks; -1: by grid size, vrt_lit.hip)
    uint32_t dark_voxel_passes = 0;        // dark voxel passes launched (vrt_read_dark_voxels)
    uint32_t dark_last_voxel_layers = 0;   // of the last one-launch shadow frame: 0 = its pool held no dark voxel marks, or it read the plain bricks
    bool dark_last_used = false;   // the last one-launch shadow frame's shadow rays stopped at dark cells (vrt_get_dark_marks)
    // longest tiles first (vrt_kernels.hip: tile_order_*), for a context that renders one frame at a time
    // (vrt_set_frames_in_flight(1)) and whose view is at rest: the second plain frame of an unchanged view (camera, settings,
    // world, materials) notes its tiles' march-loop trips, right behind it on the stream four small launches turn them into the
    // order the following frames of that view launch their tiles in.  The order is only worth anything for the very view it
    // was made from (a launch's tail is a handful of tiles with grazing rays, and which tiles those are changes with a hundredth
    // of a voxel of camera travel; measured): any change of the view goes back to screen order.  With two
    // frames in flight the other frame already fills a launch's tail and the order buys nothing.
    bool tile_lpt = true;               // VRT_TILE_ORDER=0: screen order always
    uint32_t view_gen = 0;              // counts the changes of anything a tile's trips depend on
    uint32_t frame_view_gen = ~0u;      // ... as of the last frame rendered
    uint32_t order_view_gen = ~0u;      // ... as of the frame the order was made from
    // ... and while the view MOVES (1, the default): a frame notes its trips, ONE launch behind it sorts blocks of 4 x 4 tiles by
    // their trips dilated over `mov_radius` blocks (vrt_kernels.hip: launch_tile_order_blocks, ~ 17 us), and the order is KEPT for
    // the frames that follow while their camera stays within what the dilation covers (vrt_order.hip, hold_limits: ~ 8 of the bench's orbit steps)
    // and nothing but the camera has changed; the frame that comes near the edge of that notes its trips for the next order.  A
    // view that moves too fast for its orders to be used stops asking for them (mov_backoff).  One frame at a time, orbit:
    // 112.8 -> 109.1 us per frame (profiles/r05_tile_order_moving.txt).  0 (VRT_TILE_ORDER_MOVING=0): screen order while the
    // view moves.
    uint32_t tile_lpt_moving = 1;
    uint32_t order_uses = 0;            // frames that used the dilated order in d_tile_order
    uint32_t mov_backoff = 0, mov_skip = 0;   // moving frames that go without asking for an order (doubles while orders go unused)
    bool mov_any_size = false;          // VRT_TILE_ORDER_MOVING set by name: also frames of more than kMovingTilesMax tiles
    uint32_t mov_radius = 5;            // VRT_TILE_ORDER_RADIUS: blocks the order is dilated over
    // vrt_present*: whether a window of (one_w x one_h) over a texture of the same size samples every texel at its centre
    uint32_t one_w = 0, one_h = 0;
    bool one_to_one = false;
    // vrt_set_presentation: the declared crosshair / window / flags; whether frames of (pres_for_w x pres_for_h) can store their own
    // window pixels (found once per size and declaration) and the crosshair's box; which frame sets' screen buffers hold the
    // image their last frame stored itself (whether the last frame stored one, and texels at all: last.fused, last.has_texels)
    bool pres_on = false;
    vrt_crosshair pres_ch{};
    uint32_t pres_w = 0, pres_h = 0, pres_flags = 0;
    uint32_t pres_for_w = 0, pres_for_h = 0, pres_box[4] = {0, 0, 0, 0};
    bool pres_fusable = false;
    uint32_t ordered_frames = 0;        // frames launched in an order (vrt_accel_info.ordered_frames)
    bool order_dilated = false;         // the order in d_tile_order is a dilated one
    uint32_t cam_gen = 0, order_cam_gen = 0;   // counts the changes of the camera (each is a change of the view too)
    vrt_cam_data order_cam{};           // the camera of the frame the order was made from
    bool tile_order_stale = false;      // a chunk was edited since the order was made: still used, made again by the next frame without an edit in front of it
    uint32_t frame_mode = ~0u;          // vrt_mode of the last frame rendered (a change of mode is a change of view)
    float accel_last_ms = 0.f;
    uint64_t roots_tag = 0;         // vrt_write_chunk_roots_tagged: the caller's tag of the table as last written (0: none)
    uint32_t roots_tag_offset = 0, roots_tag_n = 0;
    std::vector<uint32_t> h_roots;  // what chunk_roots holds, to recognise the reference's per-frame rewrite of the same table
    std::vector<std::pair<uint32_t, uint32_t>> roots_index;  // (root, chunk slot) sorted by root, roots != 0: which chunk owns a node
    bool roots_index_stale = true;

    // uploads are staged through pinned memory (copy-at-call semantics without waiting for the device) and ordered with
    // the frames in flight by events, not by draining them
    Pinned h_ring;                // the pinned ring ...
    uint8_t *d_ring = nullptr;    // ... and where the device sees it
    static constexpr size_t kRingSegBytes = 1u << 20, kRingSegs = 8;
    Event ring_ev[kRingSegs][2];   // behind a segment's last copy on c->stream [0] / the upload stream [1]; null: none yet
    uint32_t ring_seg = 0;
    size_t ring_off = 0;
    // node-pool / chunk_roots uploads staged since the last flush: copied into the ring at call time, launched together — one
    // copy kernel for all of them — before the next thing that reads those buffers (a frame's table update, a whole-world
    // build, a synchronise).  The reference drains every pending GiveChunkData per frame (main.rs:289-295): a launch per
    // range made the frame loop host-bound beyond two uploads per frame (27 us each).
    struct Staged { uint32_t buf, dst_word, n_words; size_t ring_at; };
    std::vector<Staged> staged;
    size_t staged_bytes = 0;
    bool flushed_at_call = false;     // a staged range went out at its vrt_write_* call since the last frame (the device was idle): the next ones wait for the batch
    bool staged_seg[kRingSegs] = {};  // ring segments the staged ranges lie in (their events are recorded at the flush)
    Event ev_frames;                  // scratch: "everything enqueued on that frame stream so far"
    Event ev_upload;                  // the last upload / table rebuild on c->stream
    // Node-pool and chunk_roots uploads have a stream of their own: frame set 0 runs on c->stream, and an upload queued
    // behind a frame there would wait for it.  What reads those two buffers — the table updates, and frames that walk the
    // octree itself (variants 1 / 2, worlds beyond the tables) — is what an upload waits for, nothing else.
    Stream up_stream;
    Event ev_pool_upload;                     // the last upload on up_stream
    uint64_t pool_gen = 0;                    // bumped by every upload on up_stream
    uint64_t seen_pool_gen[kMaxInFlight + 1] = {0, 0, 0, 0, 0};  // [slot] of the frame streams as seen_gen, [kMaxInFlight] c->stream
    bool walkers_in_flight = false;           // a frame that reads the node pool has been enqueued since the last full synchronise
    uint64_t upload_gen = 0;          // bumped by every upload; a frame stream waits for ev_upload when it has not seen it
    uint64_t seen_gen[kMaxInFlight] = {0, 0, 0, 0};  // [0] own_stream, [k] extra_stream[k - 1]

    Buf<float> d_ndc;             // ndc_x[width] then ndc_y[height] (FrameParams), rebuilt when proj_size or the output size change
    uint32_t ndc_w = 0, ndc_h = 0;
    float ndc_proj[2] = {0.f, 0.f};

    // vrt_cast_rays / vrt_clip_moves (vrt_query.h query_batch_host): the device copy of a host batch, queries then results, in
    // bytes; a host batch waits on ev_query for its own results before it returns, so the two kinds share one buffer
    Buf<uint8_t> d_query;
    Event ev_query;

    // vrt_generate_chunks / vrt_build_chunks (vrt_gen.hip): one batch's staging slots, node counts, offsets and inputs (made on
    // first use), and the compacted nodes of a whole call (grown as needed)
    Buf<uint16_t> d_gen_stage;
    Buf<uint32_t> d_gen_counts;
    Buf<uint64_t> d_gen_offs;
    Buf<int32_t> d_gen_pos;
    Buf<uint16_t> d_gen_dense;
    Buf<uint16_t> d_gen_out;
    // vrt_edit_chunks (vrt_edit.hip): one batch's input trees and per-chunk records, the call's shapes and bins (grown as needed)
    Buf<uint16_t> d_edit_nodes;
    Buf<uint8_t> d_edit_chunks;    // kGenBatch records (vrt_edit.hip's EditChunk), in bytes
    Buf<uint8_t> d_edit_changed;   // kGenBatch
    Buf<vrt_shape> d_edit_shapes;
    Buf<uint16_t> d_edit_bins;

    vrt_material h_mats[256];
    static constexpr size_t kMatsAlloc = 256 + 256 * sizeof(float) / sizeof(vrt_material) + 256 * sizeof(vrt_polish) / sizeof(vrt_material) +
                                         256 * sizeof(vrt_translucency) / sizeof(vrt_material) + 1;   // d_mats, in materials (the last one holds the coat word)
    float h_emission[256];    // vrt_write_emission's table (zeros at creation) and how many of its entries are not 0: a frame
    uint32_t n_emissive = 0;  // of a context with none runs the kernels without the emission term
    vrt_polish h_polish[256]; // vrt_write_polish's table (zero bytes at creation) and how many of its entries have a chance that is
    uint32_t n_polished = 0;  // not 0: a frame of a context with none runs the kernels that do not flip the coat's coin
    vrt_translucency h_translucency[256];   // vrt_write_translucency's table (zero bytes at creation) and how many of its entries
    uint32_t n_translucent = 0;             // have a chance that is not 0: a frame of a context with none runs what ran before
    uint32_t coat_word = 0;   // what the word behind the tables holds on the device: n_polished != 0 (vrt_write_polish keeps it)
    uint32_t liquid_mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // bit v <=> h_mats[v].is_liquid == 1 (kept by vrt_write_materials)
    bool liquid_is_range = true;                          // the liquid ids are one range below 255, or none
    uint32_t liquid_lo = 0x80000000u, liquid_span = 0u;   // (none: no 15-bit voxel id is 0x80000000)
    vrt_cam_data cam;
    vrt_settings settings;
    vrt_world_data world;

    // vrt_get_issue_profile: the calling thread's time inside vrt_render since the last call of it
    double prof_render_us = 0.0;
    uint32_t prof_frames = 0;

    // VRT_RENDER_ACCUMULATE: the running sum is sz.d_accum (one texel per slot, never divided; allocated by the first accumulating
    // frame, dropped by alloc_output); the samples in it and their seed, whether the next accumulating frame starts again at 0,
    // and the event behind the last step that wrote the sum (the next frame's first step that touches it waits for it)
    uint32_t accum_n = 0, accum_seed = 0;
    bool accum_restart = true;
    Event ev_accum;
    bool accum_ev_recorded = false;
    // vrt_set_denoise (vrt_denoise.hip): the setting (passes 0: off); the scratch frames the passes go back and forth over and the
    // guide words are sz.dn_scratch / sz.dn_guide
    vrt_denoise_opts denoise{};
    // vrt_set_tone_map (vrt_tone.hip): the setting (48 zero bytes: off).  One word block per frame set, made by its first metered
    // frame (vrt::kTone*: the histogram being counted, the last metered frame's, its E and its vrt_tone_info); the frame set whose
    // block holds the adapted exposure of the metered frame before the next one (-1: the adaptation starts), the metered frames
    // since it started, and the event behind the last one-thread step: the next one, on whatever stream, waits for it
    vrt_tone_map tone{};
    Buf<uint32_t> d_tone[kMaxInFlight];
    int tone_prev = -1;
    uint32_t tone_frames = 0;
    Event ev_tone;
    uint32_t tone_blocks = 512;              // VRT_TONE_BLOCKS: about how many workgroups count a frame's histogram
    hipStream_t tone_ev_stream = nullptr;    // the stream ev_tone was last recorded on (null: never)
    // the last mapped frame (vrt_get_tone_info) and the last metered one (vrt_read_tone_histogram): -1 none yet
    int tone_info_slot = -1, tone_hist_slot = -1;
    bool tone_info_metered = false;          // the last mapped frame was metered: its record is in its set's block
    float tone_info_exposure = 0.0f;         // ... it was not: its E
    vrt_sun_light sun{};      // vrt_set_sun_light: the setting (16 zero bytes: off); the sun-ray buffers are sz.sun_recs / sz.sun_counts
    vrt_water_optics water{}; // vrt_set_water_optics: the setting (32 zero bytes: off)
    vrt_water_refraction refraction{};   // vrt_set_water_refraction: the setting (16 zero bytes: off; max_span never 0 beside an ior)
    vrt_haze haze{};          // vrt_set_haze: the setting (32 zero bytes: off)
    vrt_camera_sampling lens{};   // vrt_set_camera_sampling: the setting (16 zero bytes: off)
    // vrt_set_lamp_light (vrt_lamp.hip): the setting (16 zero bytes: off), the cap (VRT_LAMP_CAP) and one lamp list per frame set,
    // built on that set's stream by the lamp-lit frame that finds it out of date: what it was built from is kept beside it
    vrt_lamp_light lamp{};
    uint32_t lamp_cap = 1u << 20;
    struct LampList {
        Buf<uint4> d_list;                 // lamp_cap entries (include/vrt.h: vrt_lamp)
        Buf<uint32_t> d_sums, d_bases;     // faces per block of 256 cells, and their exclusive scan (saturating)
        Buf<uint32_t> d_info;              // [0] listed = N, [1] 0, [2..3] the world's faces in 64 bits
        bool valid = false;
        uint32_t tab = 0, S = 0;           // the table set and world size ...
        uint64_t tab_gen = 0;              // ... its contents ...
        float emission[256];               // ... the emission table and the liquid set of the last build
        uint32_t liquid[8];
        uint32_t builds = 0;
        Event e0, e1;                      // around the last build (read by vrt_get_lamp_info, never by a frame)
        float last_ms = 0.f;
        bool timed = false;                // last_ms is the last build's
    } lamps[kMaxInFlight];
    int lamp_last = -1;                    // the frame set whose list the last lamp-lit frame used
    bool rendered = false;
    bool timing_pending = false;
    vrt_stats stats;

    std::string err;
};

enum EvKind : uint8_t { kEvNone = 0, kEvOneKernel = 1, kEvTwoKernels = 2, kEvRecorded = 3 };

// Largest world the grid march's tables cover: the cell grid is addressed by a 32-bit byte offset built with signed
// 24-bit multiplies (8S (8S+1)^2 * 4 B < 2^31, (8S+1)^2 * 4 < 2^23), bricks by brick * 128 B < 2^32.
static constexpr uint32_t kAccelMaxS = 100;
// ... the march cells (16 bytes per cell) are addressed the same way: 8S (8S+1)^2 * 16 B < 2^31
static constexpr uint32_t kMarchBlocksMax = 1u << 18;   // 2 GiB of march-cell blocks (byte offsets stay below 2^31)
// Small worlds skip the directory: the cells of the whole world, [4S][4S+1][4S+1] lines of 2 x 2 x 2 cells (one dependent
// load and a divergent branch less per change of chunk: 17.5 against 16.1 Grays/s on C4).  16^3 chunks: 35 MB; larger
// worlds go through the directory (32^3: 23 MB instead of 273).
static constexpr uint32_t kMarchDirectMaxS = 16;
static constexpr uint32_t kAccelMaxBricks = 0x1FE0000u - 1u;   // 0x80000000 | brick * 64 stays below vrt::kAirLeaf
// Chunks that can be rebuilt alone between two whole-world builds: each may move, once, into a 512-brick region
// (64 KiB) at the tail of the brick pool.
static constexpr uint32_t kTailChunks = 128;
// A write that touches more chunks than this is cheaper as a whole-world build.
static constexpr uint32_t kMaxDirtyChunks = 256;

// ---- helpers that cross a translation unit (hidden: the library exports include/vrt.h and nothing else) ----
#define VRT_HIDDEN __attribute__((visibility("hidden")))
extern VRT_HIDDEN thread_local std::string g_create_err;
VRT_HIDDEN int fail(vrt_ctx *ctx, int code, const char *fmt, ...);
// vrt_gen.hip's builder over blocks that are on the device already (vrt_edit.hip): n chunks in batches of 2048; for each batch
// fill(c, arg, b0, nb) enqueues on c->stream whatever leaves chunk b0 + i's block dense[x + 32*(y + 32*z)] in
// c->d_gen_dense + 32768 i (a non-zero return ends the call with it), then the builder, the scan and the gather run and
// nodes / offsets come out as vrt_build_chunks's do.  The stream is drained once per batch, after fill's work and the scan.
namespace vrt {
typedef int (*GenFillFn)(vrt_ctx *c, void *arg, uint32_t b0, uint32_t nb);
VRT_HIDDEN int gen_build_device_blocks(vrt_ctx *c, GenFillFn fill, void *fill_arg, uint32_t n, uint16_t *nodes, uint64_t cap_nodes,
                                       uint64_t *offsets, const char *what);
}
#define HIP_TRY(ctx, expr)                                                                          \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail(ctx, e_ == hipErrorOutOfMemory ? VRT_ERR_OOM : VRT_ERR_DEVICE, "%s: %s", #expr, \
                        hipGetErrorString(e_));                                                     \
    } while (0)

// Multi-device entry points switch the calling thread's current HIP device; the caller gets its own back.
struct DeviceRestore {
    int dev = -1;
    DeviceRestore() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; }
    ~DeviceRestore() { if (dev >= 0) (void)hipSetDevice(dev); }
};

#define VRT_TRY(call)                  \
    do {                               \
        const int rc_ = (call);        \
        if (rc_) return rc_;           \
    } while (0)
VRT_HIDDEN int quiesce(vrt_ctx *c);   // wait for the frames that may still be running on the context's other streams
#define QUIESCE(c) VRT_TRY(quiesce(c))

// vrt_frames.hip
VRT_HIDDEN bool ragged_output(const vrt_ctx *c);
VRT_HIDDEN hipError_t zero_now(vrt_ctx *c, void *p, size_t bytes);
inline size_t frame_slots(const vrt_ctx *c) { return c->slots ? c->slots : 1; }   // what a buffer of one element per pixel slot holds (an empty shard: one)
// A buffer that is read as a whole frame, of at least n elements: zero from its allocation on where the output is not whole tiles
// (ragged_output).  Every caller but the path trace's sample planes asks for the same n until a resize drops the buffer: made once.
template <typename T>
inline int frame_buf(vrt_ctx *c, vrt_ctx::Buf<T> &buf, size_t n) {
    if (n <= buf.cap()) return VRT_OK;
    HIP_TRY(c, buf.grow(n));
    if (ragged_output(c)) HIP_TRY(c, zero_now(c, buf.get(), n * sizeof(T)));
    return VRT_OK;
}
VRT_HIDDEN int validate_frame(vrt_ctx *c);
VRT_HIDDEN int accum_frame_start(vrt_ctx *c, const vrt_render_opts &o, uint32_t *from);
VRT_HIDDEN int ensure_ndc(vrt_ctx *c);
VRT_HIDDEN void fill_uniforms(const vrt_ctx *c, vrt::FrameParams &P);
// vrt_present.hip: whether this frame can store its own window pixels (vrt_set_presentation) and, then, its screen buffer
VRT_HIDDEN bool presentation_fusable(vrt_ctx *c);
VRT_HIDDEN int screen_buffer_for_frame(vrt_ctx *c, uint32_t slot, hipStream_t st, uint32_t screen_w, uint32_t screen_h);
// vrt_order.hip: the order a one-frame-at-a-time context launches its tiles in, around the frame's launch in vrt_render
struct TileOrderPlan { bool sort = false, dilate = false; };
VRT_HIDDEN int tile_order_before_frame(vrt_ctx *c, vrt::FrameParams &P, hipStream_t st, const vrt::FramePlan &plan, bool edit_in_front, TileOrderPlan &order);
VRT_HIDDEN int tile_order_after_frame(vrt_ctx *c, const vrt::FrameParams &P, hipStream_t st, const TileOrderPlan &plan);
// vrt_denoise.hip: around a path frame's launches in vrt_render (vrt_set_denoise)
VRT_HIDDEN int denoise_before_frame(vrt_ctx *c, uint32_t slot, vrt::Texel *frame_out, vrt::Texel **trace_into);
VRT_HIDDEN int denoise_after_frame(vrt_ctx *c, const vrt::FrameParams &P, const vrt::FramePlan &plan, uint32_t slot, hipStream_t st, vrt::Texel *frame_out,
                                   hipEvent_t closing);
// vrt_tone.hip: behind a path frame's last launch (the denoiser's passes included) in vrt_render (vrt_set_tone_map with
// VRT_TONE_AUTO): the histogram and the one-thread step; *E: where the frame's blit reads its exposure (null: the setting's own).
// tone_restart: the adaptation starts again and the last mapped / metered frame is forgotten (a resize)
VRT_HIDDEN int tone_after_frame(vrt_ctx *c, uint32_t slot, hipStream_t st, const vrt::Texel *frame_out, hipEvent_t closing, const float **E);
VRT_HIDDEN void tone_restart(vrt_ctx *c);
// vrt_uploads.hip
VRT_HIDDEN int alloc_roots(vrt_ctx *c, uint32_t world_size);
VRT_HIDDEN int flush_staged(vrt_ctx *c);
VRT_HIDDEN int order_after_frames(vrt_ctx *c, hipStream_t target);
VRT_HIDDEN int order_after_frames(vrt_ctx *c);
VRT_HIDDEN int publish_upload(vrt_ctx *c);
VRT_HIDDEN int wait_for_pool_uploads(vrt_ctx *c, hipStream_t st, uint32_t slot);
VRT_HIDDEN int frame_waits_for_uploads(vrt_ctx *c, hipStream_t st, uint32_t slot);
VRT_HIDDEN int stage_upload(vrt_ctx *c, void *dst, const void *src, size_t bytes, bool pool = false);
VRT_HIDDEN void mark_all_dirty(vrt_ctx *c);
VRT_HIDDEN int ensure_accel_world(vrt_ctx *c);
VRT_HIDDEN int update_tables(vrt_ctx *c, uint32_t k, hipStream_t st);
// wait for the frames in flight; the frame being enqueued has been announced on its stream already (alt_pending / own_pending) and stays so
VRT_HIDDEN int quiesce_before_frame(vrt_ctx *c);
VRT_HIDDEN size_t grid_entries(uint32_t S);   // the cell grid with its zero border: [8S][8S+1][8S+1]
VRT_HIDDEN size_t chunk_dir_entries(uint32_t S);
VRT_HIDDEN size_t direct_cell_entries(uint32_t S);
// the G^3 cells (G = 8 accel_S) of a device grid of the context, without the border, on c->stream; waits for the copy
VRT_HIDDEN int read_grid_cells(vrt_ctx *c, const uint32_t *d_grid, uint32_t *cells);
// vrt_lit.hip: the sun marks of table set `tab` for the sun at P.sun_local, made on `st` if the set does not hold them; fills what the
// frame's shadow rays are given (P.shadow_below, lit_trips, shadow_bricks, lit_voxel_trips: left as they are — kAirLeaf, 0, null, 0 —
// when this world and sun get no marks or c->sun_marks is off) and c->lit_last_*, what the read-backs report of the frame.
// `shares`: the frame is of another frame set than the table set's own (tabs[0] read from a second stream)
VRT_HIDDEN int sun_marks_for_frame(vrt_ctx *c, uint32_t tab, hipStream_t st, bool shares, vrt::FrameParams &P);
// vrt_lamp.hip: the frame set's lamp list, rebuilt on `st` if what it was built from has changed (the frame's tables are up to date
// on `st` and it waits for the uploads so far); fills M.list and M.n
VRT_HIDDEN int lamp_list_for_frame(vrt_ctx *c, uint32_t slot, uint32_t tab, hipStream_t st, vrt::LampLaunch &M);

// ---- one context over several devices (vrt_config.n_devices > 1): vrt_group.hip ----
// ---------------------------------------------------------------------------------------------------------------------
// One context over several devices (vrt_config.n_devices > 1).
//
// The reference is one process on one thread driving one GpuResources (main.rs:398-455); this keeps that shape for a
// node with several GPUs.  A group is N ordinary contexts, one per entry of device_ids: device 0's is a row-major shard
// root, the others are tile-major shard contexts that write 8-byte records (or texels, VRT_FLAG_TEXEL_MESSAGES).  Every
// upload is replicated (each context stages its own copy); a frame is
//     for r >= 1:  [device r] wait until device 0 has consumed message slot k -> render into device 0's memory
//                             (peer stores over xGMI, hipDeviceEnablePeerAccess) -> record done[r][k]
//     device 0:    render its own tiles straight into frame buffer k (its in-flight stream X) -> on X: wait for every
//                  done[r][k] -> shade / scatter the messages into the frame -> record consumed[k]
// all enqueued from the calling thread without waiting for anything: two message slots and device 0's two frame buffers
// give the same two frames in flight a single device has.  No collective library, no second process.
// ---------------------------------------------------------------------------------------------------------------------
// One issuing thread per device other than the root: the caller stays one thread (the reference's shape), but issuing a
// frame to N devices from it alone costs N x (launch + event record + waits) and makes eight devices host-bound
// (DESIGN.md §7).  A worker sleeps on a condition variable between frames' bursts and spins briefly first, so a frame
// loop finds it awake; every API call joins the workers before it returns — nothing of a context is ever touched by
// two threads at once.
struct GrpWorker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::atomic<uint64_t> posted{0}, finished{0};
    std::function<int()> job;
    int rc = 0;
    bool quit = false;
    double last_job_us = 0.0;   // how long the last job took this thread (read by the caller after join())

    void run() {
        uint64_t seen = 0;
        for (;;) {
            for (int spin = 0; spin < 20000 && posted.load(std::memory_order_acquire) == seen; spin++) __builtin_ia32_pause();
            if (posted.load(std::memory_order_acquire) == seen) {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return quit || posted.load(std::memory_order_acquire) != seen; });
                if (quit) return;
            }
            seen = posted.load(std::memory_order_acquire);
            const auto t0 = std::chrono::steady_clock::now();
            rc = job();
            last_job_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            finished.store(seen, std::memory_order_release);
        }
    }
    void post(std::function<int()> f) {
        job = std::move(f);
        {
            std::lock_guard<std::mutex> lk(m);
            posted.fetch_add(1, std::memory_order_release);
        }
        cv.notify_one();
    }
    int join() {
        const uint64_t want = posted.load(std::memory_order_acquire);
        while (finished.load(std::memory_order_acquire) != want) __builtin_ia32_pause();
        return rc;
    }
    void stop() {
        {
            std::lock_guard<std::mutex> lk(m);
            quit = true;
        }
        cv.notify_one();
        if (th.joinable()) th.join();
    }
};

struct vrt_group {
    std::vector<vrt_ctx *> dev;      // dev[0] = the root
    std::vector<std::unique_ptr<GrpWorker>> workers;   // [r - 1] issues for dev[r]; empty: the calling thread issues for all (VRT_GROUP_THREADS=0)
    bool texels = false;             // VRT_FLAG_TEXEL_MESSAGES
    bool poison = false;             // VRT_FLAG_POISON_MESSAGES
    // [r] device r cannot store into device 0's memory (peer access refused), or VRT_FLAG_STAGED_MESSAGES: it renders into
    // stage[r][slot], a buffer of its own, and copies the message over afterwards (hipMemcpyPeerAsync, its own stream)
    std::vector<uint8_t> staged;
    static constexpr uint32_t kSlots = 2;
    std::vector<std::array<vrt_ctx::Buf<uint8_t>, kSlots>> stage;   // [r][slot], on device r
    vrt_ctx::Buf<uint8_t> recv[kSlots];                    // on device 0: [n_devices][tiles_padded * 64] records or texels
    size_t rank_stride = 0;                                // bytes between two devices' messages
    vrt_ctx::Event consumed[kSlots];                       // device 0 has assembled the frame of this slot
    bool consumed_used[kSlots] = {false, false};
    std::vector<std::array<vrt_ctx::Event, kSlots>> done;  // [r][slot]: device r's message is complete
    uint32_t slot = 0, in_flight = 2;
    bool last_was_stats = false;
    // The stream device 0's share of the current frame was enqueued on, published by the calling thread once its own vrt_render has
    // returned: every issuing thread then makes that stream wait for ITS message itself (one hipStreamWaitEvent each, in parallel)
    // instead of the caller making N - 1 of them in turn behind the join — they were ~ 6 us each, the part of the caller's frame that
    // grew with N (profiles/r06_bench_modes_rehearsal.txt: 10 / 20 / 48 us at N = 2 / 4 / 8).  nullptr: not yet; kNoFrameStream: the
    // root's render failed, nobody waits for anything.
    std::atomic<hipStream_t> frame_stream{nullptr};
    static inline hipStream_t no_frame_stream() { return reinterpret_cast<hipStream_t>(static_cast<uintptr_t>(1)); }
    // vrt_get_issue_profile: sums over the frames since its last call
    struct { uint32_t frames = 0; double render = 0, root = 0, shard_sum = 0, shard_max = 0, join = 0, tail = 0, waits = 0; } prof;
};

VRT_HIDDEN int grp_create(const vrt_config *cfg, vrt_ctx **out);
VRT_HIDDEN void grp_destroy(vrt_ctx *c);
VRT_HIDDEN int grp_render(vrt_ctx *c, const vrt_render_opts *opts);
VRT_HIDDEN int grp_synchronize(vrt_ctx *c);
VRT_HIDDEN int grp_get_stats(vrt_ctx *c, vrt_stats *out);
VRT_HIDDEN int grp_get_issue_profile(vrt_ctx *c, vrt_issue_profile *out);
VRT_HIDDEN int grp_resize_output(vrt_ctx *c, uint32_t w, uint32_t h);
VRT_HIDDEN int grp_set_frames_in_flight(vrt_ctx *c, uint32_t n);
inline vrt_ctx *grp_root(vrt_ctx *c) { return c->grp->dev[0]; }
template <typename F>
inline int grp_each(vrt_ctx *c, F f) {
    DeviceRestore restore;
    for (vrt_ctx *d : c->grp->dev) {
        const int rc = f(d);
        if (rc) { c->err = d->err; return rc; }
    }
    return VRT_OK;
}
#define GRP_EACH(c, call)                                                   \
    do {                                                                    \
        if ((c) && (c)->grp) return grp_each((c), [&](vrt_ctx *d) { return call; }); \
    } while (0)
#define GRP_ROOT(c, call)                                                   \
    do {                                                                    \
        if ((c) && (c)->grp) { DeviceRestore restore_; vrt_ctx *d = grp_root(c); const int rc_ = call; if (rc_) (c)->err = d->err; return rc_; } \
    } while (0)
#define GRP_REFUSE(c, what)                                                 \
    do {                                                                    \
        if ((c) && (c)->grp) return fail((c), VRT_ERR_STATE, what ": not on a multi-device context (it owns its streams and message buffers)"); \
    } while (0)
