#pragma once
// vrt_frame_plan.h — what kind of frame a vrt_render call asks for, decided once (vrt_frames.hip: vrt_render plans the frame,
// enqueues it, records it).  Pure functions over plain values, no context pointer, no HIP header: tools/check_frame_plan.cpp holds
// them to the predicates they replaced over every combination of the facts.  A new kernel route is a line in plan_frame.
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

}  // namespace vrt
