#pragma once
// vrt_frame_plan.h — what kind of frame a vrt_render call asks for, decided once (vrt_frames.hip: vrt_render plans the frame,
// enqueues it, records it), and — for a path-traced frame — which launches it is made of (plan_path, for_each_path_step:
// launch_path_frame enqueues them).  Pure functions over plain values, no context pointer, no HIP header:
// tools/check_frame_plan.cpp holds them to the predicates and the loop they replaced over every combination of the facts.  A new
// kernel route is a line in plan_frame or plan_path.
#include <cstddef>
#include <cstdint>

#include "../../include/vrt.h"

namespace vrt {

struct FrameFacts {   // what the decisions depend on, copied out of the options and the context
    uint32_t mode = 0, variant = 0, stats = 0, flags = 0;   // vrt_render_opts (variant: as requested)
    bool compact = false;           // VRT_FLAG_COMPACT: the context's pixel slots are 8-byte records
    bool show_step_count = false;   // settings.show_step_count == 1: the step-count debug view (F2 in the reference, main.rs:368-370)
    bool air_liquid = false;        // materials[0].is_liquid == 1
    bool accel_ok = false;          // the world fits the derived tables (as ensure_accel_world left it)
    uint32_t in_flight = 1, tiles_local = 0;   // vrt_set_frames_in_flight; this context's tiles (0: an empty shard)
    bool caller_stream = false;     // vrt_set_stream: the context's stream is not its own
    bool output_bound = false;      // vrt_bind_output: frames are written to the caller's memory
    bool present_fusable = false;   // vrt_set_presentation: frames of this size can store their own window pixels
};

struct FramePlan {   // what the rest of the call reads: each field is explained where plan_frame sets it
    uint32_t mode = 0, variant = 0, march = 0;
    bool shadow = false, path = false, kstats = false, literal = false, tables = false, one_launch = false, may_pipeline = false,
         pipelined = false, fuse_present = false, walks_octree = false, counts_per_tile = false, orderable = false;
};

// Primary + shadow in one launch: the default march, and — on a context whose pixel slots are 8-byte records — the octree walk
// it falls back to when the world is too large for the derived tables (the two-launch kernels store and re-read 16-byte
// texels, which such a buffer has no room for).
inline bool one_launch_march(uint32_t variant, bool compact) { return variant == 0u || (variant == 2u && compact); }

// Whether the requested frame asks for the derived tables at all: ensure_accel_world runs for those, ahead of plan_frame.
// The fast marches never ask whether *air* is liquid (ray_tracer.wgsl:226 asks for every voxel, voxel 0 included): a material
// table that flags voxel 0 as liquid — nothing the reference's data packs do — is traced by the literal march, variant 1.
inline bool asks_for_tables(const FrameFacts &F) { return !F.air_liquid && (F.variant == 0u || F.variant == 3u || F.mode == VRT_MODE_PATH); }

inline FramePlan plan_frame(const FrameFacts &F) {
    FramePlan p;
    p.mode = F.mode;   // as asked (the tile order and the record of the last frame note it)
    p.shadow = F.mode == VRT_MODE_PRIMARY_SHADOW;
    p.path = F.mode == VRT_MODE_PATH;
    p.literal = F.air_liquid;
    // the frame reads the derived tables: it asks for them and the world fits them.  (Asked of the variant before or after the
    // fallback below this is the same: the fallback is taken only where accel_ok is false.)
    p.tables = asks_for_tables(F) && F.accel_ok;
    // the kernel variant after every fallback: 0 the grid march over the tables, primary + shadow in one launch; 1 the literal
    // octree walk; 2 the ancestor-cache octree walk (a world too large for the tables); 3 the grid march in two launches
    p.variant = F.air_liquid ? 1u : (!p.tables && (F.variant == 0u || F.variant == 3u)) ? 2u : F.variant;
    p.march = p.variant == 3u ? 0u : p.variant;   // what the launchers take
    // per-lane iteration counts exist in the STATS kernels only; the step-count debug view needs them, so it runs those kernels too
    p.kstats = F.stats == 1u || F.show_step_count;
    // one launch finishes the frame's pixels (through store_pixel): every primary-only frame, and primary + shadow of such a march
    p.counts_per_tile = p.shadow && one_launch_march(p.variant, F.compact);   // (launched-ray counts: else one per primary workgroup)
    p.one_launch = F.mode == VRT_MODE_PRIMARY || p.counts_per_tile;
    // Two (or more) frames in flight: plain frames — one launch, or the path trace's chain of launches — alternate between the
    // context's frame sets; anything else (stats, the two-launch variants, a caller's stream or bound buffer without
    // VRT_RENDER_OWN_STREAMS) waits for them and runs alone on the context's stream.  VRT_RENDER_OWN_STREAMS: the caller set a
    // stream and / or bound an output but lets this frame run on the context's own streams (nothing on the caller's stream consumes
    // it before a synchronise; frames in flight are bound to different buffers) — the gather root's own tiles in bench.py
    p.may_pipeline = p.one_launch || p.path;
    p.pipelined = F.in_flight > 1u && p.may_pipeline && !p.kstats &&
                  ((F.flags & VRT_RENDER_OWN_STREAMS) != 0u || (!F.caller_stream && !F.output_bound));
    // vrt_set_presentation: a one-launch frame whose window samples texel for texel also stores the window's image
    p.fuse_present = p.one_launch && F.tiles_local != 0u && F.present_fusable;
    p.walks_octree = p.variant == 1u || p.variant == 2u;   // reads the node pool and chunk_roots (so does a frame given no tables)
    // longest tiles first (vrt_order.hip): plain frames of the grid march in one launch, as far as the kind of frame decides it
    p.orderable = !p.path && p.variant == 0u && !p.kstats && F.stats == 0u;
    return p;
}

// ---- the path-traced frame (plan.path): a wavefront path trace, per chain of samples one launch per bounce over the compacted
// live-path buffer, then a pass that takes the chain into the frame or a sum ----

constexpr uint32_t kPlanHitSegments = 256;   // vrt::kHitSegments (vrt_device.h; vrt_frames.hip asserts the two equal)

struct PathFacts {   // copied out of the options, the context and the frame's parameters
    uint32_t spp = 1, seed = 0;     // vrt_render_opts (spp: at least 1)
    uint32_t bounces = 0;           // settings.max_ray_bounces
    bool kstats = false, literal = false;   // the FramePlan's
    bool has_grid = false;          // the frame was handed the derived tables (P.grid)
    bool has_cells = false;         // ... and the march cells with them (P.mblk)
    bool march_direct = false;      // the march cells without a chunk directory (what the pool launcher's 320-ray pools ask for)
    bool accum = false;             // VRT_RENDER_ACCUMULATE ...
    uint32_t accum_from = 0;        // ... with this many samples in the context's sum before the frame (accum_frame_start)
    bool emissive = false;          // vrt_write_emission: some material gives off light
    bool polished = false;          // vrt_write_polish: some material's coat has a chance that is not 0
    bool translucent = false;       // vrt_write_translucency: some material lets a path through with a chance that is not 0
    bool sun = false;               // vrt_set_sun_light: the strength is not 0
    bool camera_sampling = false;   // vrt_set_camera_sampling: pixel_spread or aperture is not 0
    bool lamp = false;              // vrt_set_lamp_light: the strength is not 0
    bool water = false;             // vrt_set_water_optics: VRT_WATER_ON (never with lamp or camera_sampling: vrt_render refuses the pair)
    bool haze = false;              // vrt_set_haze: the density is not 0 (never with water, lamp or camera_sampling: vrt_render refuses the pair)
    // the context's switches (vrt_create reads them from the environment)
    uint32_t path_samples = 8;      // VRT_PATH_SAMPLES_PER_CHAIN
    bool path_pool = true, path_cells = true;   // VRT_PATH_POOL, VRT_PATH_CELLS
    uint32_t path_pool_batches = 0, path_refill = 0;   // VRT_PATH_POOL_K, VRT_PATH_POOL_REFILL
    uint32_t in_flight = 1;         // vrt_set_frames_in_flight
    uint32_t hit_seg_cap = 256;     // records per segment of the hit buffer (a multiple of 256)
};

enum PathFinish : uint32_t {   // the pass behind each chain of samples
    kFinishNone,          // one sample per chain adding straight to the frame's texels (divided at the end, if by more than 1)
    kChainIntoFrame,      // path_chain_finish_kernel: the chain's planes join the frame in sample order; the last chain divides
    kChainIntoSum,        // ... join the context's sum; the last chain stores the mean into the frame
    kResolveIntoSum,      // path_accum_resolve_kernel: the texel's one sample joins the context's sum, the last stores the mean
    kResolveIntoOwnSum,   // ... joins the frame set's own sum (its first plane)
};

struct PathPlan {   // each field is explained where plan_path sets it
    uint32_t spp = 1, seed = 0, bounces = 0;
    bool kstats = false, literal = false, emit = false, polish = false, translucent = false, sun = false, sun_cells = false, lens = false, lamp = false, water = false, haze = false;
    uint32_t samples = 1;
    bool planes = false, own_sum = false, cells = false;
    uint32_t seg_cap = 0;
    size_t cap = 0;
    uint32_t pool_batches = 4, refill = 0;
    bool zero_output = false;
    PathFinish finish = kFinishNone;
    bool finish_into_accum = false, divide_at_end = false;
    bool needs_acc_planes = false, needs_accum_sum = false;
    uint32_t sample_base = 0, accum_count = 1;
};

inline PathPlan plan_path(const PathFacts &F) {
    PathPlan p;
    p.spp = F.spp; p.seed = F.seed; p.bounces = F.bounces;
    p.kstats = F.kstats; p.literal = F.literal;   // which build of the lane = path kernels (the launchers take them)
    // Plain frames over the derived tables trace their bounces with what was built for speed; a stats frame, the literal march
    // and a world too large for the tables keep the round-1 structure: one sample per chain, one lane = path launch per bounce
    const bool fast = !F.kstats && !F.literal && F.has_grid;
    // Several samples per launch chain (plain frames, spp > 1): every launch of the chain carries `samples` times the rays —
    // 2.7 rays per lane are not enough to cover a bounce launch's tail — and a frame of 16 spp is 4 x 4
    // launches instead of 16 x 4.  Each sample accumulates into its own plane; the chain's finishing pass adds the planes
    // to the frame in sample order, which is the order one sample per chain adds them in.
    // vrt_set_sun_light: every trace launch of a sun-lit frame is followed by a launch that marches the sun rays it appended
    // (vrt_path_sun.h), and stream order is what puts a segment's sun term between its emission term and the next segment's.  The
    // pool kernel carries all later segments in one launch and cannot be interleaved, and one record per slot per launch is what
    // keeps the sun launch's read-modify-write plain: such a frame is one sample per chain, one lane = path launch per bounce,
    // whatever its world.  What the sun launch marches with: the occlusion-only march over the march cells where a plain frame
    // has them, else the trace's own march
    p.sun = F.sun && F.bounces > 0u;
    p.sun_cells = p.sun && fast && F.has_cells && F.path_cells;
    // vrt_set_lamp_light: the same structure for the same reasons — each trace launch is followed by the launch over the lamp rays it
    // appended (vrt_path_lamp.h), behind the sun launch when the frame is sun-lit too.  Its kernels are one pair that carries both terms
    p.lamp = F.lamp && F.bounces > 0u;
    // vrt_set_water_optics: a water frame's kernels choose each segment's liquid set (vrt_path_water.h); the pool kernel's march cells
    // have the table's set baked into their "passes" bits, so such a frame is again one sample per chain, one lane = path launch per
    // bounce, planned as a sun-lit frame is.  Sun-lit too, its sun launches are the sun-lit frame's own (sun_cells included: sun rays
    // pass liquids as they always have)
    p.water = F.water && F.bounces > 0u;
    // vrt_set_haze: a haze frame's kernels draw a distance behind every march and may append a sun ray from a point in the air
    // (vrt_path_haze.h); the pool kernel has neither, so such a frame is once more one sample per chain, one lane = path launch per
    // bounce, planned as a sun-lit frame is.  Sun-lit too, its sun launches are the sun-lit frame's own (sun_cells included)
    p.haze = F.haze && F.bounces > 0u;
    p.samples = (F.spp > 1u && fast && F.bounces > 0u && !p.sun && !p.lamp && !p.water && !p.haze) ? (F.spp < F.path_samples ? F.spp : F.path_samples) : 1u;
    p.planes = p.samples > 1u;
    // vrt_write_emission: a sample's light is then several terms (emissive hits, the sky), summed by themselves before they
    // join the frame.  The planes do that, and so does a one-sample chain whose texel holds that sample alone: an accumulating
    // frame's (path_accum_resolve_kernel takes it into the sum behind every sample) and — own_sum — an emissive frame's of
    // several samples, which takes the same pass into a sum of its own (the frame set's first plane).  Without emission a
    // sample is one term, added straight to the texel, and a 1-spp frame's texel is its one sample either way.
    // vrt_write_polish: a polished frame's kernels carry the emission term (a zero entry adds nothing), so it is planned with
    // everything an emissive frame is planned with; polish is what the launchers switch on
    // vrt_write_translucency: the same again.  The translucent kernels are one family, whether the frame is polished or not
    // (they take the coat's draw under a word the uploads keep on the device), so translucent is what the launchers look at first
    // vrt_set_sun_light: and again — a sample is then several terms (the sun terms, the sky).  Its kernels are one pair, which reads
    // from its launch whether there is a coat or a pass-through draw
    p.emit = F.emissive || F.polished || F.translucent || p.sun || p.lamp || p.water || p.haze;
    p.polish = F.polished;
    p.translucent = F.translucent;
    // vrt_set_camera_sampling: the frame's kStepPrimary / kStepSunlitPrimary launches are the kernels of vrt_path_lens.h, which give
    // every sample a primary ray of its own; the chains, the launches behind bounce 0 and the finishing passes are what they are
    p.lens = F.camera_sampling && F.bounces > 0u;
    p.own_sum = p.emit && !p.planes && !F.accum && F.spp > 1u && F.bounces > 0u;
    // a segment of the path buffers holds what its workgroups can produce for every sample of a chain; a buffer, every segment
    p.seg_cap = F.hit_seg_cap * p.samples;
    p.cap = (size_t)kPlanHitSegments * p.seg_cap;
    // Bounce launches over the march cells: every later segment of a chain in ONE launch of the pool kernel (vrt_path.hip);
    // worlds without march cells, or with the pool switched off: one lane = path launch per bounce.
    p.cells = fast && F.bounces > 1u && F.path_pool && F.has_cells && F.path_cells && !p.sun && !p.lamp && !p.water && !p.haze;
    // the pool's batches of 64 rays per wave: 5 with two frames in flight (the launcher grants them to direct worlds only), else 4
    p.pool_batches = F.path_pool_batches ? F.path_pool_batches : (F.in_flight > 1u ? 5u : 4u);
    p.refill = F.path_refill;
    p.zero_output = F.bounces == 0u;   // no segment is traced: the frame is zeros, and nothing below is launched
    // an accumulating frame's samples continue the sum's: they seed as sample_base + s, and the mean is over accum_count
    p.sample_base = F.accum ? F.accum_from : 0u;
    p.accum_count = p.sample_base + F.spp;   // (<= 2^24: accum_frame_start)
    p.finish = p.zero_output ? kFinishNone
             : p.planes      ? (F.accum ? kChainIntoSum : kChainIntoFrame)
             : F.accum       ? kResolveIntoSum   // one sample per chain: bit-exact only one sample at a time
             : p.own_sum     ? kResolveIntoOwnSum
                             : kFinishNone;
    p.finish_into_accum = p.finish == kChainIntoSum || p.finish == kResolveIntoSum;   // ordered behind the previous accumulating frame
    p.divide_at_end = !p.zero_output && p.finish == kFinishNone && F.spp > 1u;   // path_finish_kernel: rgb /= spp behind the last sample
    p.needs_acc_planes = p.planes || p.own_sum;   // the frame set's planes: `samples` frames of texels
    p.needs_accum_sum = F.accum;   // the context's sum (and the event behind its last writer), whether or not this frame reaches it
    return p;
}

// (the first five trace a segment of the paths — the launches PathStep::launch counts — and come first: traces_paths asks for them;
// kStepSunlitPrimary / kStepSunlitBounce are a sun-lit frame's, each followed by a kStepSunRays with its launch number;
// kStepLampPrimary / kStepLampBounce, appended behind the others, are a lamp-lit frame's, sun-lit or not: each is followed by a
// kStepSunRays, if the frame is sun-lit too, and then by a kStepLampRays; kStepWaterPrimary / kStepWaterBounce, behind those again,
// are a water frame's, each followed by a kStepSunRays if the frame is sun-lit too; kStepHazePrimary / kStepHazeBounce, last, are a
// haze frame's, followed in the same way)
enum PathStepKind : uint32_t { kStepPrimary, kStepLaneBounce, kStepCellsBounce, kStepSunlitPrimary, kStepSunlitBounce, kStepSunRays,
                               kStepChainFinish, kStepResolve, kStepFinalDivide, kStepLampPrimary, kStepLampBounce, kStepLampRays,
                               kStepWaterPrimary, kStepWaterBounce, kStepHazePrimary, kStepHazeBounce };
inline bool traces_paths(PathStepKind k) { return k <= kStepSunlitBounce || k == kStepLampPrimary || k == kStepLampBounce || k == kStepWaterPrimary ||
                                                      k == kStepWaterBounce || k == kStepHazePrimary || k == kStepHazeBounce; }

struct PathStep {   // one launch of the frame
    PathStepKind kind;
    uint32_t sample, chain;   // the chain traces samples [sample, sample + chain) of every pixel
    // the launch's number within the frame, counting the trace's launches: it appends to cursor set launch % 3, reads set
    // (launch + 2) % 3 and clears (launch + 1) % 3 for the next; it writes path buffer launch & 1 and reads the other
    uint32_t launch;
    uint32_t segments;        // bounce segments the launch traces (the pool kernel: all that are left of the chain)
    bool last_bounce;         // paths that hit in this launch end
    bool first, last;         // a finishing pass: the chain holds the sum's first sample / the frame's last
    uint32_t count;           // ... and what the last divides by
};

// The frame's launches in stream order.  All three cursor sets are zero when the frame starts (vrt_render cleared them).
template <class F>
void for_each_path_step(const PathPlan &p, F &&f) {
    uint32_t g = 0;
    for (uint32_t smp = 0; smp < p.spp && p.bounces > 0u; smp += p.samples) {
        const uint32_t chain = p.spp - smp < p.samples ? p.spp - smp : p.samples;
        for (uint32_t b = 0; b < p.bounces; b++, g++) {
            PathStep s{b == 0u ? kStepPrimary : p.cells ? kStepCellsBounce : kStepLaneBounce, smp, chain, g, 1u, b + 1u == p.bounces, false, false, 0u};
            if (s.kind == kStepCellsBounce) {   // the waves carry their own survivors from one segment to the next
                s.segments = p.bounces - b;
                s.last_bounce = true;
                b += s.segments - 1u;
            }
            if (p.sun) s.kind = b == 0u ? kStepSunlitPrimary : kStepSunlitBounce;
            if (p.lamp) s.kind = b == 0u ? kStepLampPrimary : kStepLampBounce;
            if (p.water) s.kind = b == 0u ? kStepWaterPrimary : kStepWaterBounce;
            if (p.haze) s.kind = b == 0u ? kStepHazePrimary : kStepHazeBounce;
            f(s);
            if (p.sun) {   // the records that launch appended: cursor set launch & 1 of the sun buffer
                s.kind = kStepSunRays;
                f(s);
            }
            if (p.lamp) {   // ... and of the lamp buffer
                s.kind = kStepLampRays;
                f(s);
            }
        }
        if (p.finish != kFinishNone)
            f(PathStep{p.finish == kChainIntoFrame || p.finish == kChainIntoSum ? kStepChainFinish : kStepResolve, smp, chain, g, 0u, false,
                       p.sample_base + smp == 0u, smp + chain >= p.spp, p.accum_count});
    }
    if (p.divide_at_end) f(PathStep{kStepFinalDivide, 0u, 0u, g, 0u, false, false, true, p.spp});
}

}  // namespace vrt
